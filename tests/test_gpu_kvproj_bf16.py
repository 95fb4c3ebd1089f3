"""The fused K | V projection + key pack in bf16 (fresco_attn_fwd_kvproj with FRESCO_BF16) and its use by the processor
under FRESCOAttnProcessor2_0.fuse_kv_pack_bf16.

Kernel level: ops.attention_kvproj on bf16 tensors at key counts around every edge of the tiling (as
test_gpu_kvproj_tiles.py, T read from the kernel source), against an fp64 attention over K, V = fp64 (x W^T) rounded to
bf16 -- the storage rounding the oracle applies with round_dtype=torch.bfloat16 -- with the two-launch bf16 path
(ops.linear with a row table, then ops.attention) as the yardstick.  With t = max |err| / (rms(ref) + |ref|):
    t_fused <= 2^-6 (the bf16 processor bar), t_two <= 2^-6, t_fused <= 2 t_two + 2^-10
(the two paths round K and V along different accumulation chains; 2^-10 is half a bf16 ulp of relative slack).
Value range: w_v scaled by 2^18 (exact in bf16) scales the output by 2^18 and nothing overflows.
Processor level: with the flag on the cross-frame pass takes the fused pack exactly once, in bf16, with no warning, within
2^-6 of the bf16 oracle and 2 t_unfused + 2^-10 of the default processor; the default processor never calls it; misaligned
weight views take the unfused path."""
import copy
import math
import os
import re
import warnings

import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2.0 ** -6
SLACK = 2.0 ** -10


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
        wk = ((2 * torch.rand(H * D, K, generator=g) - 1) / math.sqrt(K)).to(BF)
        wv = ((2 * torch.rand(H * D, K, generator=g) - 1) / math.sqrt(K)).to(BF)
        q = torch.randn(B, LQ, H * D, generator=g).to(BF)
        x = torch.randn(X_ROWS, K, generator=g).to(BF)
        _inputs[layer] = tuple(t.to(DEV) for t in (q, x, wk, wv))
    return _inputs[layer]


def _m_values(layer):
    T = _tiles(LAYERS[layer][2])
    return [1, 63, 64, 65, 64 * T - 1, 64 * T, 64 * T + 1, 128 * T + 17]


def _rms(x):
    return float(x.double().pow(2).mean().sqrt())


def _t(out, ref):
    out = out.double().cpu()
    ref = ref.double().cpu()
    return float(((out - ref).abs() / (_rms(ref) + ref.abs())).max())


def _rows(layer, mi, M):
    g = synth.gen(1000 * mi + LAYERS[layer][2])
    # each group's keys: M different rows from anywhere in the hidden tensor (both halves), in random order
    return torch.cat([torch.randperm(X_ROWS, generator=g)[:M] for _ in range(GROUPS)]).to(torch.int32).to(DEV)


def _ref64(q, x, wk, wv, rows, H, D, M, scale):
    """fp64 attention over K, V = fp64 (x W^T) rounded to bf16, on the bf16 x and W"""
    K = x.shape[1]
    xs = x.double()[rows.long()].view(GROUPS, M, K)
    kf = (xs @ wk.double().T).to(BF).double()
    vf = (xs @ wv.double().T).to(BF).double()
    grp = torch.arange(B, device=q.device) // (B // GROUPS)  # batch entries of the first half read group 0's keys
    qh = q.double().view(B, LQ, H, D).transpose(1, 2)
    kh = kf[grp].view(B, M, H, D).transpose(1, 2)
    vh = vf[grp].view(B, M, H, D).transpose(1, 2)
    return (torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).transpose(1, 2).reshape(B, LQ, H * D)


@pytest.mark.parametrize("mi", range(8))
@pytest.mark.parametrize("layer", ["L3", "L2"])
def test_kvproj_bf16_tile_ranges(layer, mi):
    import fresco_amd.ops as ops
    H, D, K = LAYERS[layer]
    M = _m_values(layer)[mi]
    assert M <= X_ROWS
    q, x, wk, wv = _layer_inputs(layer)
    rows = _rows(layer, mi, M)
    scale = 1.0 / math.sqrt(D)
    fused = ops.attention_kvproj(q, x, rows, wk, wv, H, scale, n_groups=GROUPS, M=M)
    again = ops.attention_kvproj(q, x, rows, wk, wv, H, scale, n_groups=GROUPS, M=M)
    assert fused.dtype == BF
    assert torch.equal(fused, again)
    k2, v2 = ops.linear(x, [wk, wv], x_rows=rows)
    two = ops.attention(q, k2.view(GROUPS, M, H * D), v2.view(GROUPS, M, H * D), H, scale, n_groups=GROUPS, M=M, group_rows=M)
    ref = _ref64(q, x, wk, wv, rows, H, D, M, scale)
    t_f, t_u = _t(fused, ref), _t(two, ref)
    print("kvproj bf16 tiles %s M=%d: t_fused = %.4f x 2^-6, t_two = %.4f x 2^-6, bound 2 t_two + 2^-10 = %.4f x 2^-6"
          % (layer, M, t_f * 64, t_u * 64, (2 * t_u + SLACK) * 64))
    assert t_f <= BAR, t_f
    assert t_u <= BAR, t_u
    assert t_f <= 2.0 * t_u + SLACK, (t_f, t_u)


def _ordered(t):
    """bf16 -> integers whose difference counts representable values in between"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("layer", ["L3", "L2"])
def test_kvproj_bf16_value_range(layer):
    """w_v scaled by 2^18, exact in bf16: V leaves fp16's range, every fp32 sum scales exactly, and the output is the
    unscaled one times 2^18"""
    import fresco_amd.ops as ops
    H, D, K = LAYERS[layer]
    M = 64 * _tiles(K) + 1
    q, x, wk, wv = _layer_inputs(layer)
    rows = _rows(layer, 6, M)
    scale = 1.0 / math.sqrt(D)
    big = (wv.float() * 2.0 ** 18).to(BF)
    assert torch.equal(big.float(), wv.float() * 2.0 ** 18)
    vmax = float((x.float()[rows.long()] @ big.float().T).abs().max())
    assert vmax > 65504.0, vmax
    base = ops.attention_kvproj(q, x, rows, wk, wv, H, scale, n_groups=GROUPS, M=M)
    out = ops.attention_kvproj(q, x, rows, wk, big, H, scale, n_groups=GROUPS, M=M)
    assert out.dtype == BF and bool(torch.isfinite(out).all())
    back = (out.float() * 2.0 ** -18).to(BF)
    d = int((_ordered(back) - _ordered(base)).abs().max())
    print("kvproj bf16 range %s: max |V| = %.3e, ulp distance of out / 2^18 from the unscaled run = %d" % (layer, vmax, d))
    assert d <= 1, d


# ---- processor ----------------------------------------------------------------------------------------------------------
CASES = {"L3": (3, 128, "L3"), "L2": (3, 256, "L2")}  # HW = 256 in both
_cases, _refs = {}, {}


def _case(layer, masked):
    if (layer, masked) not in _cases:
        N, R, lay = CASES[layer]
        case = synth.make_attention_case(N, R, lay, seed=3, dtype=BF)
        assert case["HW"] == 256
        if not masked:
            case = dict(case)
            case["cf_mask"] = torch.zeros_like(case["cf_mask"])
            case["cf_mask"][0] = True
        _cases[(layer, masked)] = case
    return _cases[(layer, masked)]


def _oracle(layer, masked, mode):
    key = (layer, masked, mode)
    if key not in _refs:
        _refs[key] = synth.oracle_attention(_case(layer, masked), mode, round_dtype=BF)
    return _refs[key]


def _run(case, mode, masked, flag, attn=None):
    """one layer call; -> (out, [dtypes of attention_kvproj's floating operands per call], [(weights, row table?) per
    ops.linear call], RuntimeWarnings)"""
    import fresco_amd
    import fresco_amd.ops as ops
    ctrl = synth.controller_for(case, mode, DEV, dtype=BF)
    if not masked:
        ctrl.attn_mask = None
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl)
    if flag is not None:
        proc.fuse_kv_pack_bf16 = flag
    if attn is None:
        attn = copy.deepcopy(case["attn"]).to(DEV).to(BF)
    real_kv, real_lin = ops.attention_kvproj, ops.linear
    kv_calls, lin_calls = [], []

    def kv_counted(*a, **kw):
        kv_calls.append([t.dtype for t in a if torch.is_tensor(t) and t.is_floating_point()])
        return real_kv(*a, **kw)

    def lin_counted(x, weights, *a, **kw):
        lin_calls.append((1 if torch.is_tensor(weights) else len(weights), kw.get("x_rows") is not None))
        return real_lin(x, weights, *a, **kw)

    ops.attention_kvproj, ops.linear = kv_counted, lin_counted
    try:
        with warnings.catch_warnings(record=True) as rec, torch.no_grad():
            warnings.simplefilter("always")
            out = proc(attn, case["hidden"].to(DEV))
    finally:
        ops.attention_kvproj, ops.linear = real_kv, real_lin
    return out, kv_calls, lin_calls, [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]


def test_fused_pack_bf16_is_off_by_default():
    import fresco_amd
    assert fresco_amd.FRESCOAttnProcessor2_0.fuse_kv_pack_bf16 is False
    assert fresco_amd.FRESCOAttnProcessor2_0.native_bf16 is True


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("mode", ["cf", "cf_temporal", "full"])
@pytest.mark.parametrize("layer", ["L3", "L2"])
def test_processor_fused_pack_bf16(layer, mode, masked):
    case = _case(layer, masked)
    out_f, kv_f, lin_f, warn_f = _run(case, mode, masked, True)
    out_u, kv_u, lin_u, warn_u = _run(case, mode, masked, None)  # the default processor
    assert len(kv_f) == 1 and kv_f[0] and all(dt == BF for dt in kv_f[0]), kv_f
    assert kv_u == []  # the default stays the two-launch bf16 path
    assert not warn_f and not warn_u, (warn_f, warn_u)
    assert out_f.dtype == BF and out_u.dtype == BF
    # V is projected inside the pack and nowhere else: no three-weight launch, no gathered launch
    assert not any(nw == 3 or rows for nw, rows in lin_f), lin_f
    if mode in ("cf_temporal", "full"):  # q | k in full: the temporal pass reads K of every row
        assert any(nw == 2 and not rows for nw, rows in lin_f), lin_f
    ref = _oracle(layer, masked, mode)
    t_f, t_u = _t(out_f, ref), _t(out_u, ref)
    print("processor bf16 %s %s masked=%s: t_fused = %.4f x 2^-6, t_unfused = %.4f x 2^-6"
          % (layer, mode, masked, t_f * 64, t_u * 64))
    assert t_f <= BAR, t_f
    assert t_f <= 2.0 * t_u + SLACK, (t_f, t_u)


def test_misaligned_bf16_weight_views_take_the_unfused_path():
    """to_k / to_v as contiguous views 4 elements (8 bytes) into a flat buffer: not 16-byte aligned, so neither the fused
    pack nor fresco_linear may read them; the call still runs and matches the aligned one."""
    case = _case("L3", True)
    out_a, kv_a, _, _ = _run(case, "cf_temporal", True, True)
    attn = copy.deepcopy(case["attn"]).to(DEV).to(BF)
    for name in ("to_k", "to_v"):
        m = getattr(attn, name)
        flat = torch.empty(m.weight.numel() + 8, dtype=BF, device=DEV)
        view = flat[4:4 + m.weight.numel()].view_as(m.weight)
        view.copy_(m.weight.detach())
        m.weight = torch.nn.Parameter(view, requires_grad=False)
        assert m.weight.data_ptr() % 16 == 8 and m.weight.is_contiguous()
    out_m, kv_m, _, _ = _run(case, "cf_temporal", True, True, attn=attn)
    assert len(kv_a) == 1 and kv_m == []
    a = out_a.double().cpu()
    frac = float(((out_m.double().cpu() - a).abs() / (2.0 ** -7 * (_rms(a) + a.abs()))).max())
    print("misaligned bf16 weights: worst |misaligned - aligned| / (2^-7 (rms + |ref|)) = %.3f" % frac)
    assert frac <= 1.0, frac
    assert _t(out_m, _oracle("L3", True, "cf_temporal")) <= BAR
