"""The fused K | V projection + key pack (fresco_attn_fwd_kvproj) with a RANGE of key tiles per workgroup, and its use on
every layer call that runs the cross-frame pass.

Kernel level: ops.attention_kvproj against the two-launch path (fresco_linear with x_rows, then kv_pack inside ops.attention) and
against an fp32 torch evaluation, at key counts around every edge of the tiling: one partial tile, the exact 64-key tile
edge, the first tile of a second range, a range shorter than the others, a last range that is short AND ends in a partial
tile.  T, the tiles per workgroup, is read from the kernel source so that the edges move with it.
Processor level: the modes with the temporal pass (cf_temporal, full) take the fused pack by default and agree with the
unfused processor and with the oracle; misaligned weight views take the unfused path.

Bars: those of test_gpu_attention.py::test_fused_kv_projection_pack -- both paths within 1e-3 (+ 1e-3 relative) of the fp32
reference, fused against two-launch < 1e-3 (their fp16 K / V can differ in the last place), and the fused path's error no
more than twice the two-launch path's + 1e-4."""
import copy
import math
import os
import re

import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiles(k_in):
    src = open(os.path.join(ROOT, "fresco_amd", "csrc", "attn.hip")).read()
    m = re.search(r"TILES = KIN == 320 \? (\d+) : (\d+);", src)
    return int(m.group(1 if k_in == 320 else 2))


LAYERS = {"L3": (8, 40, 320), "L2": (8, 80, 640)}  # heads, head dim, K_in
B, LQ, GROUPS, X_ROWS = 4, 128, 2, 4 * 320
_inputs = {}


def _layer_inputs(layer):
    """seeded q, hidden rows and weights of one layer, made once and never written to"""
    if layer not in _inputs:
        H, D, K = LAYERS[layer]
        g = synth.gen(71 + K)
        # (weights in the range of nn.Linear's init, which the synthetic attention layers use)
        wk = ((2 * torch.rand(H * D, K, generator=g) - 1) / math.sqrt(K)).half()
        wv = ((2 * torch.rand(H * D, K, generator=g) - 1) / math.sqrt(K)).half()
        q = torch.randn(B, LQ, H * D, generator=g).half()
        x = torch.randn(X_ROWS, K, generator=g).half()
        _inputs[layer] = tuple(t.to(DEV) for t in (q, x, wk, wv))
    return _inputs[layer]


def _m_values(layer):
    T = _tiles(LAYERS[layer][2])
    return [1, 63, 64, 65, 64 * T - 1, 64 * T, 64 * T + 1, 128 * T + 17]


def _err(out, ref, what):
    err = (out.float() - ref).abs()
    assert bool((err <= 1e-3 + 1e-3 * ref.abs()).all()), "%s: max err %.3e" % (what, float(err.max()))
    return float(err.max())


@pytest.mark.parametrize("mi", range(8))
@pytest.mark.parametrize("layer", ["L3", "L2"])
def test_kvproj_tile_ranges(layer, mi):
    import fresco_amd.ops as ops
    H, D, K = LAYERS[layer]
    M = _m_values(layer)[mi]
    assert M <= X_ROWS
    q, x, wk, wv = _layer_inputs(layer)
    g = synth.gen(1000 * mi + K)
    # each group's keys: M different rows from anywhere in the hidden tensor (both halves), in random order
    rows = torch.cat([torch.randperm(X_ROWS, generator=g)[:M] for _ in range(GROUPS)]).to(torch.int32).to(DEV)
    scale = 1.0 / math.sqrt(D)
    fused = ops.attention_kvproj(q, x, rows, wk, wv, H, scale, n_groups=GROUPS, M=M)
    again = ops.attention_kvproj(q, x, rows, wk, wv, H, scale, n_groups=GROUPS, M=M)
    assert torch.equal(fused, again)
    k2, v2 = ops.linear(x, [wk, wv], x_rows=rows)
    two = ops.attention(q, k2.view(GROUPS, M, H * D), v2.view(GROUPS, M, H * D), H, scale, n_groups=GROUPS, M=M, group_rows=M)
    # fp32 evaluation of the same attention (TF32 off: plain fp32 products)
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        xs = x.float()[rows.long()].view(GROUPS, M, K)
        kf, vf = xs @ wk.float().T, xs @ wv.float().T
        grp = torch.arange(B, device=DEV) // (B // GROUPS)  # batch entries of the first half read group 0's keys
        qh = q.float().view(B, LQ, H, D).transpose(1, 2)
        kh = kf[grp].view(B, M, H, D).transpose(1, 2)
        vh = vf[grp].view(B, M, H, D).transpose(1, 2)
        ref = (torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).transpose(1, 2).reshape(B, LQ, H * D)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = prev
    e_f = _err(fused, ref, "fused %s M=%d" % (layer, M))
    e_u = _err(two, ref, "two-launch %s M=%d" % (layer, M))
    d = float((fused.float() - two.float()).abs().max())
    print("kvproj tiles %s M=%d: err vs fp32 %.2e (two-launch %.2e), fused vs two-launch %.2e" % (layer, M, e_f, e_u, d))
    assert d < 1e-3
    assert e_f <= 2.0 * e_u + 1e-4


def _case(layer, masked):
    case = synth.make_attention_case(4, 256, layer, seed=25)
    if not masked:
        case = dict(case)
        case["cf_mask"] = torch.zeros_like(case["cf_mask"])
        case["cf_mask"][0] = True
    return case


def _run(case, mode, masked, fused, attn=None):
    import fresco_amd
    import fresco_amd.ops as ops
    ctrl = synth.controller_for(case, mode, DEV)
    if not masked:
        ctrl.attn_mask = None
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl)
    proc.fuse_kv_pack = fused
    if attn is None:
        attn = copy.deepcopy(case["attn"]).to(DEV).half()
    real = ops.attention_kvproj
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    ops.attention_kvproj = counted
    try:
        with torch.no_grad():
            out = proc(attn, case["hidden"].to(DEV).half())
    finally:
        ops.attention_kvproj = real
    return out, len(calls)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("mode", ["cf_temporal", "full"])
@pytest.mark.parametrize("layer", ["L3", "L2"])
def test_processor_fused_pack_with_temporal_pass(layer, mode, masked):
    case = _case(layer, masked)
    out_f, n_f = _run(case, mode, masked, True)
    out_u, n_u = _run(case, mode, masked, False)
    assert n_f == 1 and n_u == 0  # the default processor takes the fused pack on these calls
    ref32 = synth.oracle_attention(case, mode, round_dtype=None)
    e_f = _err(out_f.cpu(), ref32, "fused %s %s" % (layer, mode))
    e_u = _err(out_u.cpu(), ref32, "unfused %s %s" % (layer, mode))
    d = float((out_f.float() - out_u.float()).abs().max())
    print("processor %s %s masked=%s: err vs fp32 oracle %.2e (unfused %.2e), fused vs unfused %.2e"
          % (layer, mode, masked, e_f, e_u, d))
    assert d < 1e-3
    assert e_f < 2.0 * e_u + 1e-4


def test_misaligned_weight_views_take_the_unfused_path():
    """to_k / to_v as contiguous views 4 elements (8 bytes) into a flat buffer: not 16-byte aligned, so neither the fused
    pack nor fresco_linear may read them; the call still runs and matches the aligned one."""
    case = _case("L3", True)
    out_a, n_a = _run(case, "cf_temporal", True, True)
    attn = copy.deepcopy(case["attn"]).to(DEV).half()
    for name in ("to_k", "to_v"):
        m = getattr(attn, name)
        flat = torch.empty(m.weight.numel() + 8, dtype=torch.float16, device=DEV)
        view = flat[4:4 + m.weight.numel()].view_as(m.weight)
        view.copy_(m.weight.detach())
        m.weight = torch.nn.Parameter(view, requires_grad=False)
        assert m.weight.data_ptr() % 16 == 8 and m.weight.is_contiguous()
    out_m, n_m = _run(case, "cf_temporal", True, True, attn=attn)
    assert n_a == 1 and n_m == 0
    ref32 = synth.oracle_attention(case, "cf_temporal", round_dtype=None)
    _err(out_m.cpu(), ref32, "misaligned weights")
    assert float((out_m.float() - out_a.float()).abs().max()) < 1e-3
