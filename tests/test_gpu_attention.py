"""GPU parity of the attention kernels and the processor against the CPU oracle / reference goldens.
Every call goes through the C ABI of libfresco_hip.so (fresco_amd.ops -> ctypes)."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import closed_form as cf
import synth
from oracle import fresco_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
# fp16 storage of P / outputs: |err| <~ 2^-11 relative per element; parity bar of BASELINE.json's north star: 1e-3
# absolute on O(1) outputs (+ 1e-3 relative where |ref| exceeds 1: the fp16 output grid)
ATOL, RTOL = 1e-3, 1e-3


def _check(out, ref, atol=ATOL, rtol=RTOL, what=""):
    out = out.float().cpu()
    err = (out - ref).abs()
    bound = atol + rtol * ref.abs()
    assert bool((err <= bound).all()), "%s: max err %.3e (ref max %.3e)" % (what, float(err.max()), float(ref.abs().max()))
    return float(err.max())


def _dense_ref(q, k, v, heads, scale, groups_of_b, diag_bias=0.0):
    """q (B,Lq,C), k/v (G,M,C) fp32; batch b uses group groups_of_b[b]."""
    outs = []
    for b in range(q.shape[0]):
        g = groups_of_b[b]
        o = O.dense_attention(O._heads(q[b:b + 1], heads), O._heads(k[g:g + 1], heads), O._heads(v[g:g + 1], heads),
                              scale, diag_bias)
        outs.append(O._merge(o))
    return torch.cat(outs, 0)


@pytest.mark.parametrize("D", [8, 16, 32, 40, 64, 80, 96, 128])
@pytest.mark.parametrize("Lq,M", [(64, 64), (200, 333), (128, 1)])
def test_attention_plain(D, Lq, M):
    import fresco_amd.ops as ops
    g = synth.gen(D * 1000 + Lq)
    B, H = 3, 8 if D <= 40 else 4
    C = H * D
    q = torch.randn(B, Lq, C, generator=g).half()
    k = torch.randn(B, M, C, generator=g).half()
    v = torch.randn(B, M, C, generator=g).half()
    scale = 1.0 / math.sqrt(D)
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale)
    ref = _dense_ref(q.float(), k.float(), v.float(), H, scale, list(range(B)))
    _check(out, ref, what="plain D=%d" % D)


@pytest.mark.parametrize("D,H", [(40, 8), (80, 8)])
def test_attention_grouped_rows_and_bias(D, H):
    """cross-frame grouping (kv_rows gather, shared group) and the spatial pass (diag bias, scale 0.2)."""
    import fresco_amd.ops as ops
    g = synth.gen(7 + D)
    chunk, N, HW = 2, 3, 96
    B, C = chunk * N, H * D
    q = torch.randn(B, HW, C, generator=g).half()
    k = torch.randn(B, HW, C, generator=g).half()
    v = torch.randn(B, HW, C, generator=g).half()
    mask = torch.rand(N, HW, generator=g) < 0.3
    mask[0] = True
    rows = mask.reshape(-1).nonzero().squeeze(1).to(torch.int32)
    scale = 1.0 / math.sqrt(D)
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale, kv_rows=rows.to(DEV), n_groups=chunk,
                        M=int(rows.numel()), group_rows=N * HW)
    kc = O.compact_cross_frame(k.float(), mask, N, chunk)
    vc = O.compact_cross_frame(v.float(), mask, N, chunk)
    ref = _dense_ref(q.float(), kc, vc, H, scale, [b // N for b in range(B)])
    _check(out, ref, what="grouped")
    # frame-0-only fallback (no matching mask): kv_rows None, M = HW
    out0 = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale, n_groups=chunk, M=HW, group_rows=N * HW)
    k0 = k.float().reshape(chunk, N, HW, C)[:, 0]
    v0 = v.float().reshape(chunk, N, HW, C)[:, 0]
    _check(out0, _dense_ref(q.float(), k0, v0, H, scale, [b // N for b in range(B)]), what="frame0")
    # spatial-guided form: per-batch keys, logit scale 0.2/sqrt(D), diagonal bias
    outb = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, 0.2 * scale, diag_bias=1.5)
    refb = _dense_ref(q.float(), k.float(), v.float(), H, 0.2 * scale, list(range(B)), diag_bias=1.5)
    _check(outb, refb, what="diag bias")


@pytest.mark.parametrize("B,Lq,M", [(2, 1024, 300), (1, 700, 1500)])
def test_attention_underfilled_grid_takes_small_workgroups(B, Lq, M):
    """D = 40 launches whose 512-row workgroups would not fill the chip (the shape of a frame shard in a multi-GPU run)
    switch to 256-row workgroups (one query block per wave): same arithmetic, other instantiation."""
    import fresco_amd.ops as ops
    g = synth.gen(B * 1000 + Lq)
    H, D = 8, 40
    C = H * D
    q = torch.randn(B, Lq, C, generator=g).half()
    k = torch.randn(B, M, C, generator=g).half()
    v = torch.randn(B, M, C, generator=g).half()
    scale = 1.0 / math.sqrt(D)
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale)
    _check(out, _dense_ref(q.float(), k.float(), v.float(), H, scale, list(range(B))), what="small workgroups")


def test_attention_forced_rescale():
    """One key dominates late in the sequence: exercises the running-max rescale of every tile."""
    import fresco_amd.ops as ops
    g = synth.gen(11)
    B, H, D, L = 1, 8, 40, 320
    C = H * D
    q = torch.randn(B, L, C, generator=g).half()
    k = torch.randn(B, L, C, generator=g).half()
    v = torch.randn(B, L, C, generator=g).half()
    k[0, 70] = (q[0, 5].float() * 4).half()   # spike in tile 1
    k[0, 300] = (q[0, 5].float() * 8).half()  # bigger spike in tile 4
    scale = 1.0 / math.sqrt(D)
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale)
    _check(out, _dense_ref(q.float(), k.float(), v.float(), H, scale, [0]), what="rescale")


@pytest.mark.parametrize("D", [40, 80])
@pytest.mark.parametrize("qgain", [1.0, 2.2, 6.0, 30.0])
def test_attention_logit_ranges(D, qgain):
    """The flash kernel picks, per wave, between the path without a running-max search (when |c q| max|k|
    proves every exponent fits fp16) and the search + deferred-rescale path.  qgain moves the logits from
    'always provably safe' over 'mixed per wave' to 'never safe, near one-hot softmax'; a slow ramp along the
    keys makes the running max creep upwards tile after tile."""
    import fresco_amd.ops as ops
    g = synth.gen(int(D * 10 + qgain))
    B, H, Lq, M = 2, 8, 256, 700
    C = H * D
    q = (torch.randn(B, Lq, C, generator=g) * qgain * torch.linspace(0.3, 1.5, Lq).view(1, Lq, 1)).half()
    k = (torch.randn(B, M, C, generator=g) * torch.linspace(0.5, 1.6, M).view(1, M, 1)).half()
    v = torch.randn(B, M, C, generator=g).half()
    scale = 1.0 / math.sqrt(D)
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale)
    ref = _dense_ref(q.float(), k.float(), v.float(), H, scale, list(range(B)))
    assert bool(torch.isfinite(out).all())
    # the 1e-3 contract also in the large-logit regime (tools/fold_margin.py: the kernel's arithmetic, emulated on the CPU,
    # stays within 0.65 of this bar on exactly these inputs, folded or exact scale; fp16 output rounding adds <= 0.25)
    _check(out, ref, what="qgain %g D=%d" % (qgain, D))


@pytest.mark.parametrize("D", [40, 80])
def test_attention_fold_limit_structured(D):
    """The folded exponent scale is taken up to a logit bound of 24 on an EMPIRICAL margin (attn_cfg.h, tools/fold_margin.py:
    N(0,1) and query-aligned keys).  Structured activations at that limit: a few dominant channels carry most of |q|, |k|,
    and k is correlated with q (the keys of a query's own neighbourhood), so many logits sit near the Cauchy-Schwarz
    bound with the same sign -- the case a Gaussian test does not reach.  Bounds c |q| max|k| of 16 ... 24."""
    import fresco_amd.ops as ops
    g = synth.gen(900 + D)
    B, H, Lq, M = 2, 8, 256, 640
    C = H * D
    prof = torch.ones(D)
    prof[:3] = 6.0                                  # three dominant channels per head
    prof = prof / prof.norm() * math.sqrt(D)
    base = torch.randn(B, 1, H, D, generator=g)     # a direction shared by queries and keys of a batch element
    qd = (0.8 * base + 0.6 * torch.randn(B, Lq, H, D, generator=g)) * prof
    kd = (0.8 * base + 0.6 * torch.randn(B, M, H, D, generator=g)) * prof
    scale = 1.0 / math.sqrt(D)
    c = scale * math.log2(math.e)
    # scale q so that the largest per-wave bound c |q| max|k| lands just under the fold limit
    bound = c * qd.norm(dim=-1).max() * kd.norm(dim=-1).max()
    qd = qd * (23.5 / float(bound))
    q, k = qd.reshape(B, Lq, C).half(), kd.reshape(B, M, C).half()
    v = torch.randn(B, M, C, generator=g).half()
    out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale)
    ref = _dense_ref(q.float(), k.float(), v.float(), H, scale, list(range(B)))
    e = _check(out, ref, what="structured fold limit D=%d" % D)
    print("fold limit, structured q / k, D=%d: max err %.2e" % (D, e if e is not None else float("nan")))


@pytest.mark.parametrize("D,H,N,HW", [
    (8, 8, 4, 150), (40, 8, 8, 150), (80, 8, 5, 150), (40, 8, 16, 150),   # one MFMA tile: 4, 2, 3 (15 of 16 slots), 1 trajectories
    (40, 8, 3, 151), (16, 5, 7, 149), (64, 3, 12, 90), (32, 8, 1, 100),  # ragged last block, odd head counts, N = 1
    (40, 8, 20, 70), (80, 8, 32, 40), (40, 8, 17, 64),                    # two key tiles (second one partial)
    (40, 8, 40, 33), (8, 8, 70, 20)])                                     # long clips: vector-ALU path
def test_temporal_attention(D, H, N, HW):
    import fresco_amd.ops as ops
    g = synth.gen(3 * D + N)
    chunk = 2
    C, B = H * D, chunk * N
    q = torch.randn(B, HW, C, generator=g).half()
    k = torch.randn(B, HW, C, generator=g).half()
    v = torch.randn(B, HW, C, generator=g).half()
    fwd = torch.stack([torch.randperm(HW, generator=g) for _ in range(N)], 0)
    tm = torch.rand(HW, N, N, generator=g) < 0.6
    tm = tm | tm.transpose(1, 2) | torch.eye(N, dtype=torch.bool)
    scale = 0.2 / math.sqrt(D)
    out = ops.temporal_attention(q.to(DEV), k.to(DEV), v.to(DEV), fwd.to(DEV).unsqueeze(1),
                                 tm.to(DEV).unsqueeze(1), H, scale, chunk)
    ref = O.temporal_attention(q.float(), k.float(), v.float(), fwd, tm, H, scale, chunk)
    _check(out, ref, what="temporal")


MODES = ["plain", "full", "cf_temporal", "cf", "temporal"]


def _run_processor(case, mode, device=DEV):
    import fresco_amd
    ctrl = synth.controller_for(case, mode, device)
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl if mode != "plain" else fresco_amd.AttentionControl())
    attn = copy.deepcopy(case["attn"]).to(device).half()  # the case keeps its CPU fp32 module for the oracle
    with torch.no_grad():
        return proc(attn, case["hidden"].to(device).half())


@pytest.mark.parametrize("mode", MODES)
def test_processor_reference_golden_kat7(golden, mode):
    """Appendix-B KAT 7 inputs (closed form), outputs of the UNMODIFIED reference (fp32, CPU) as golden.
    The HIP path runs the same inputs in fp16: tolerance = fp16 storage of q/k/v/P/out."""
    d = cf.base_case()
    C, heads, HW, B = 64, 8, 64, 8
    W = cf.attn_weights(C)
    fm, bm, tm = O.mapping_ind(d["bwd"], d["bo"], d["imgs"], scale=8.0)
    case = dict(attn=synth.FakeAttn(C, heads, W), hidden=cf.attn_hidden(B, HW, C, 0.0),
                ref=cf.attn_hidden(B, HW, C, 0.4), fwd_map=fm, bwd_map=bm, tmask=tm,
                cf_mask=O.cross_frame_masks(d["bo"], scales=(8.0,))[0], N=4, HW=HW, C=C, heads=heads)
    out = _run_processor(case, mode)
    ref = torch.from_numpy(golden["proc_" + mode])
    # outputs are O(1..5) sums of 64 fp16-rounded terms
    _check(out, ref, atol=1e-3, rtol=2e-3, what="KAT7 " + mode)


@pytest.mark.parametrize("heads", [2, 1])
@pytest.mark.parametrize("mode", ["full", "cf_temporal", "cf"])
def test_processor_reference_golden_decoder_head_dims(headdim_golden, heads, mode):
    """The KAT-7 inputs widened to C = 80, i.e. head dim 40 (up_blocks.3) with 2 heads and 80 (up_blocks.2) with 1:
    outputs of the UNMODIFIED reference (fp32, CPU; tests/golden/make_proc_headdim_golden.py) as golden for the flash and
    temporal kernels at the head dims the decoder runs (the projections of this width stay the modules' own GEMMs)."""
    d = cf.base_case()
    C, HW, B = 80, 64, 8
    W = cf.attn_weights(C)
    fm, bm, tm = O.mapping_ind(d["bwd"], d["bo"], d["imgs"], scale=8.0)
    case = dict(attn=synth.FakeAttn(C, heads, W), hidden=cf.attn_hidden(B, HW, C, 0.0),
                ref=cf.attn_hidden(B, HW, C, 0.4), fwd_map=fm, bwd_map=bm, tmask=tm,
                cf_mask=O.cross_frame_masks(d["bo"], scales=(8.0,))[0], N=4, HW=HW, C=C, heads=heads)
    out = _run_processor(case, mode)
    ref = torch.from_numpy(headdim_golden["proc_d%d_%s" % (C // heads, mode)])
    _check(out, ref, atol=1e-3, rtol=2e-3, what="D=%d %s" % (C // heads, mode))


@pytest.mark.parametrize("layer", ["L2", "L3"])
@pytest.mark.parametrize("mode", MODES)
def test_processor_vs_oracle_cfg1(layer, mode):
    """BASELINE config 1 shapes (N=4, 256^2): HIP processor vs the oracle mirroring fp16 storage rounding."""
    case = synth.make_attention_case(4, 256, layer, seed=1)
    out = _run_processor(case, mode)
    ref = synth.oracle_attention(case, mode)
    e = _check(out, ref, atol=1e-3, rtol=1e-3, what="%s %s" % (layer, mode))
    # and against the un-rounded fp32 oracle: the stated fp16 tolerance of BASELINE.md (1e-3 abs)
    ref32 = synth.oracle_attention(case, mode, round_dtype=None)
    _check(out, ref32, atol=1e-3, rtol=1e-3, what="%s %s fp32" % (layer, mode))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["full", "cf"])
def test_processor_other_activation_dtypes(mode, dtype):
    """fp32 / bf16 pipelines: the module's own projections run in that dtype, q, k, v are rounded to fp16 for the
    kernels and the result is cast back -- the same HIP path, within the fp16 contract of the fp32 oracle (bf16: the
    oracle sees the bf16-rounded weights and inputs; the tolerance covers bf16 projections, 3 significant digits)."""
    import fresco_amd
    case = synth.make_attention_case(4, 256, "L3", seed=3)
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, synth.controller_for(case, mode, DEV, dtype=dtype))
    attn = copy.deepcopy(case["attn"]).to(DEV).to(dtype)
    with torch.no_grad():
        out = proc(attn, case["hidden"].to(DEV).to(dtype))
    assert out.dtype == dtype
    if dtype == torch.bfloat16:
        case = dict(case)
        case["attn"] = copy.deepcopy(case["attn"]).to(dtype).float()
        case["hidden"] = case["hidden"].to(dtype).float()
        case["ref"] = case["ref"].to(dtype).float()
    ref32 = synth.oracle_attention(case, mode, round_dtype=None)
    tol = 1e-3 if dtype == torch.float32 else 2e-2
    _check(out, ref32, atol=tol, rtol=tol, what="%s %s" % (mode, dtype))


def test_processor_large_mask_blocks():
    """Block occlusions: M ~ (1 + 0.5 (N-1)) HW keys, many broken trajectories."""
    case = synth.make_attention_case(4, 256, "L3", seed=2, occ_mode="blocks")
    for mode in ("cf", "cf_temporal"):
        out = _run_processor(case, mode)
        _check(out, synth.oracle_attention(case, mode), atol=1e-3, rtol=1e-3, what="blocks " + mode)


def test_processor_crossattn_path(golden):
    """encoder_hidden_states given -> plain attention over the 5 text tokens; controller untouched."""
    import fresco_amd
    d = cf.base_case()
    C, heads = 64, 8
    attn = synth.FakeAttn(C, heads, cf.attn_weights(C)).to(DEV).half()
    ctrl = fresco_amd.AttentionControl()
    ctrl.stored_attn["decoder_attn"] = [torch.zeros(8, 64, C, device=DEV, dtype=torch.half)]
    ctrl.enable_intraattn()
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl)
    hs = cf.attn_hidden(8, 64, C, 0.0).to(DEV).half()
    enc = cf.attn_hidden(8, 5, C, 1.3).to(DEV).half()
    with torch.no_grad():
        out = proc(attn, hs, encoder_hidden_states=enc)
    assert ctrl.index == 0  # cross-attention must not advance the store index
    _check(out, torch.from_numpy(golden["proc_crossattn"]), atol=1e-3, rtol=2e-3, what="crossattn")


def test_full_size_properties_cfg2():
    """BASELINE config 2 size (N=8, 512^2, L3: HW=4096, C=320): size-independent properties.
    (1) sampled query rows against the oracle; (2) constant V -> output = that constant;
    (3) permuting the key order leaves the result unchanged up to fp16 rounding."""
    import fresco_amd.ops as ops
    g = synth.gen(5)
    chunk, N, HW, H, D = 2, 8, 4096, 8, 40
    B, C = chunk * N, H * D
    q = torch.randn(B, HW, C, generator=g).half()
    k = torch.randn(B, HW, C, generator=g).half()
    v = torch.randn(B, HW, C, generator=g).half()
    mask = torch.rand(N, HW, generator=g) < 0.1
    mask[0] = True
    rows = mask.reshape(-1).nonzero().squeeze(1).to(torch.int32)
    scale = 1.0 / math.sqrt(D)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    out = ops.attention(qd, kd, vd, H, scale, kv_rows=rows.to(DEV), n_groups=chunk, M=int(rows.numel()),
                        group_rows=N * HW)
    # (1) 48 sampled query rows of 3 batches
    sel = torch.randint(0, HW, (48,), generator=g)
    kc = O.compact_cross_frame(k.float(), mask, N, chunk)
    vc = O.compact_cross_frame(v.float(), mask, N, chunk)
    for b in (0, 7, 13):
        ref = _dense_ref(q[b:b + 1, sel].float(), kc, vc, H, scale, [b // N])
        _check(out[b:b + 1, sel], ref, what="sampled rows b=%d" % b)
    # (2) constant V
    vconst = torch.full_like(vd, 0.625)
    oc = ops.attention(qd, kd, vconst, H, scale, kv_rows=rows.to(DEV), n_groups=chunk, M=int(rows.numel()),
                       group_rows=N * HW)
    assert float((oc.float() - 0.625).abs().max()) < 2e-3
    # (3) key permutation invariance
    perm = rows[torch.randperm(rows.numel(), generator=g)]
    op = ops.attention(qd, kd, vd, H, scale, kv_rows=perm.to(DEV), n_groups=chunk, M=int(rows.numel()),
                       group_rows=N * HW)
    assert float((op.float() - out.float()).abs().max()) < 2e-3
    assert torch.isfinite(out.float()).all()


def test_processor_4d_input_residual_rescale_groupnorm():
    """the generic AttnProcessor branches SD-1.5's attn1 does not take: 4-D (B,C,h,w) hidden states,
    group_norm, residual connection and output rescale (diffusion_hacked.py:183-199, 379-385)"""
    import fresco_amd
    g = synth.gen(21)
    B, C, h, w, heads = 4, 64, 6, 5, 8
    attn = synth.FakeAttn(C, heads)
    attn.group_norm = torch.nn.GroupNorm(8, C)
    attn.residual_connection = True
    attn.rescale_output_factor = 2.0
    with torch.no_grad():
        for p in attn.parameters():
            p.copy_(p.half().float())
    x = torch.randn(B, C, h, w, generator=g).half()
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, fresco_amd.AttentionControl())
    with torch.no_grad():
        attn_dev = copy.deepcopy(attn).to(DEV).half()
        out = proc(attn_dev, x.to(DEV))
        # the group norm in front of the attention is the MODULE's own (PyTorch, fp16 on the GPU), not part of the path under
        # test: the oracle starts from its fp16 output, so that the bar below measures the HIP path alone
        xs16 = x.to(DEV).view(B, C, h * w).transpose(1, 2)
        xn = attn_dev.group_norm(xs16.transpose(1, 2)).transpose(1, 2).float().cpu()
        W = [p.detach().float() for p in attn.weights()]
        core = O.fresco_attention(xn, W[0], W[1], W[2], W[3], attn.to_out[0].bias.detach().float(), heads,
                                  round_dtype=torch.float16)
        ref = (core.transpose(-1, -2).reshape(B, C, h, w) + x.float()) / 2.0
    assert out.shape == (B, C, h, w) and out.dtype == torch.float16
    # (residual add and 1/rescale run in fp16 on values up to ~4: rtol covers that output grid)
    _check(out, ref, atol=1e-3, rtol=2e-3, what="4-D / residual / rescale")


def test_processor_rejects_unsupported_inputs():
    import fresco_amd
    attn = synth.FakeAttn(64, 8).to(DEV)
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, fresco_amd.AttentionControl())
    import fresco_amd.ops as ops
    x32 = torch.zeros(2, 16, 64, device=DEV)
    assert proc(attn, x32).dtype == torch.float32   # fp32 activations: computed in fp16, cast back (documented)
    with pytest.raises(TypeError):                  # the operator itself takes fp16 only
        ops.attention(x32, x32, x32, 8, 1.0)
    with pytest.raises(NotImplementedError):        # a mask that depends on the query
        proc(attn.half(), x32.half(), attention_mask=torch.zeros(2, 16, 16, device=DEV))


@pytest.mark.parametrize("C,heads", [(320, 8), (640, 8)])
@pytest.mark.parametrize("kind", ["additive", "bool"])
def test_processor_attention_mask(C, heads, kind):
    """attention_mask on the plain self-attention path and on the cross-attention path (reference :192-196, 303-305: an
    additive bias handed to SDPA): the processor folds it into an extra contraction dimension of the ordinary kernel.
    Reference: fp32 softmax(q k^T / sqrt(D) + bias) v from the same fp16-rounded projections."""
    import fresco_amd
    g = synth.gen(C + len(kind))
    B, L, Lk = 3, 96, 77
    attn = synth.FakeAttn(C, heads)
    with torch.no_grad():
        for p in attn.parameters():
            p.copy_(p.half().float())
    D = C // heads

    def ref_call(x, enc, bias):
        q = (x.float() @ attn.to_q.weight.T).half().float()
        k = (enc.float() @ attn.to_k.weight.T).half().float()
        v = (enc.float() @ attn.to_v.weight.T).half().float()
        qh, kh, vh = (t.view(t.shape[0], t.shape[1], heads, D).transpose(1, 2) for t in (q, k, v))
        sc = qh @ kh.transpose(-1, -2) / math.sqrt(D) + bias[:, None, None, :]
        o = (torch.softmax(sc, -1) @ vh).transpose(1, 2).reshape(x.shape[0], x.shape[1], C).half().float()
        return o @ attn.to_out[0].weight.T + attn.to_out[0].bias

    proc = fresco_amd.FRESCOAttnProcessor2_0(2, None)
    dev_attn = copy.deepcopy(attn).to(DEV).half()
    for cross in (False, True):
        x = torch.randn(B, L, C, generator=g).half()
        enc = torch.randn(B, Lk, C, generator=g).half() if cross else x
        n = enc.shape[1]
        keep = torch.rand(B, n, generator=g) < 0.7
        keep[:, 0] = True
        if kind == "bool":
            mask, bias = keep, torch.zeros(B, n).masked_fill(~keep, float("-inf"))
        else:  # the reference's own construction (diffusion_hacked.py:569) plus a soft part
            soft = 0.5 * torch.randn(B, n, generator=g)
            bias = (1 - keep.float()) * -10000.0 + soft
            mask = bias
        with torch.no_grad():
            out = proc(dev_attn, x.to(DEV), encoder_hidden_states=enc.to(DEV) if cross else None,
                       attention_mask=mask.to(DEV))
            ref = ref_call(x, enc, bias)
        _check(out, ref, atol=1e-3, rtol=2e-3, what="mask %s cross=%d D=%d" % (kind, cross, D))
    # together with a cross-frame key MASK of this scale the reference cannot use an attention_mask either: rejected
    ctrl = fresco_amd.AttentionControl()
    ctrl.enable_cfattn([torch.ones(1, L, dtype=torch.bool, device=DEV)])
    procf = fresco_amd.FRESCOAttnProcessor2_0(1, ctrl)
    with pytest.raises(ValueError):
        procf(dev_attn, torch.randn(1, L, C).half().to(DEV), attention_mask=torch.zeros(1, L, device=DEV))
    # ... but with controller.attn_mask None every frame attends to frame 0's keys and the mask addresses exactly those
    # (reference :227-247, 303-305: its SDPA accepts it): frame f's output = masked attention of its queries over frame 0's
    # K / V of the same CFG half
    ctrl0 = fresco_amd.AttentionControl()
    ctrl0.use_cfattn = True
    assert ctrl0.attn_mask is None
    proc0 = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl0)
    nf = 3
    x = torch.randn(2 * nf, L, C, generator=g).half()
    keep = torch.rand(2 * nf, L, generator=g) < 0.7
    keep[:, 0] = True
    bias = (1 - keep.float()) * -10000.0 + 0.5 * torch.randn(2 * nf, L, generator=g)
    with torch.no_grad():
        out = proc0(dev_attn, x.to(DEV), attention_mask=bias.to(DEV))
    q = (x.float() @ attn.to_q.weight.T).half().float()
    k = (x.float() @ attn.to_k.weight.T).half().float().view(2, nf, L, C)[:, :1].expand(-1, nf, -1, -1).reshape(2 * nf, L, C)
    v = (x.float() @ attn.to_v.weight.T).half().float().view(2, nf, L, C)[:, :1].expand(-1, nf, -1, -1).reshape(2 * nf, L, C)
    qh, kh, vh = (t.view(2 * nf, L, heads, D).transpose(1, 2) for t in (q, k, v))
    sc = qh @ kh.transpose(-1, -2) / math.sqrt(D) + bias[:, None, None, :]
    o = (torch.softmax(sc, -1) @ vh).transpose(1, 2).reshape(2 * nf, L, C).half().float()
    ref0 = o @ attn.to_out[0].weight.T + attn.to_out[0].bias
    _check(out, ref0, atol=1e-3, rtol=2e-3, what="mask + cross-frame (frame 0 keys) D=%d" % D)


@pytest.mark.parametrize("C,heads", [(256, 8), (512, 8), (320, 8)])
def test_processor_attention_mask_fully_masked_rows(C, heads):
    """Head dims 32 and 64 run the flash kernel's MCOL instantiations (running max clamped to +-6e4 raw units), 40 the
    padded one.  A batch element whose keys are ALL masked (the reference's additive -10000: a uniform softmax, not NaN)
    and one whose whole first 64-key tile is masked must give the reference's result on every head dim."""
    import fresco_amd
    g = synth.gen(C + 7)
    B, L = 3, 160
    D = C // heads
    attn = synth.FakeAttn(C, heads)
    with torch.no_grad():
        for p in attn.parameters():
            p.copy_(p.half().float())
    x = torch.randn(B, L, C, generator=g).half()
    keep = torch.rand(B, L, generator=g) < 0.7
    keep[0, :] = False           # every key masked
    keep[1, :64] = False         # the first key tile masked
    keep[1, 64] = True
    bias = (1 - keep.float()) * -10000.0
    q = (x.float() @ attn.to_q.weight.T).half().float()
    k = (x.float() @ attn.to_k.weight.T).half().float()
    v = (x.float() @ attn.to_v.weight.T).half().float()
    qh, kh, vh = (t.view(B, L, heads, D).transpose(1, 2) for t in (q, k, v))
    sc = qh @ kh.transpose(-1, -2) / math.sqrt(D) + bias[:, None, None, :]
    o = (torch.softmax(sc, -1) @ vh).transpose(1, 2).reshape(B, L, C).half().float()
    ref = (o @ attn.to_out[0].weight.T + attn.to_out[0].bias).detach()
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, None)
    with torch.no_grad():
        out = proc(copy.deepcopy(attn).to(DEV).half(), x.to(DEV), attention_mask=bias.to(DEV))
    assert bool(torch.isfinite(out).all())
    _check(out, ref, atol=1e-3, rtol=2e-3, what="fully masked rows D=%d" % D)



@pytest.mark.parametrize("layer,N,R", [("L3", 4, 256), ("L2", 4, 256), ("L3", 8, 512), ("L2", 8, 512)])
@pytest.mark.parametrize("masked", [True, False])
def test_fused_kv_projection_pack(layer, N, R, masked):
    """Round 6: on cross-frame-only calls the K | V projection of the selected rows runs INSIDE the key pack
    (fresco_attn_fwd_kvproj: K and V never reach HBM).  Against the fp32 oracle at the usual bar, and against the two-launch
    path (fresco_linear with x_rows + kv_pack): the fp16 K / V values may differ in the last place (one accumulation chain in
    natural k order vs two chains in permuted order), so the outputs agree to fp16 rounding, not bit for bit.
    masked=False: controller.attn_mask None -> every frame attends to frame 0's HW keys."""
    import fresco_amd
    case = synth.make_attention_case(N, R, layer, seed=21 + N)
    if not masked:
        case = dict(case)
        case["cf_mask"] = torch.zeros_like(case["cf_mask"])
        case["cf_mask"][0] = True
    outs = {}
    for fused in (True, False):
        ctrl = synth.controller_for(case, "cf", DEV)
        if not masked:
            ctrl.attn_mask = None
        proc = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl)
        proc.fuse_kv_pack = fused
        attn = copy.deepcopy(case["attn"]).to(DEV).half()
        with torch.no_grad():
            outs[fused] = proc(attn, case["hidden"].to(DEV).half())
    ref32 = synth.oracle_attention(case, "cf", round_dtype=None, device=DEV if N > 4 else None)
    e_f = _check(outs[True], ref32, atol=1e-3, rtol=1e-3, what="fused %s" % layer)
    e_u = _check(outs[False], ref32, atol=1e-3, rtol=1e-3, what="two-launch %s" % layer)
    d = float((outs[True].float() - outs[False].float()).abs().max())
    print("fused K|V projection + pack, %s N=%d masked=%s: max err vs fp32 oracle %.2e (two-launch path %.2e), fused vs "
          "two-launch %.2e" % (layer, N, masked, e_f, e_u, d))
    assert d < 1e-3
    assert e_f < 2.0 * e_u + 1e-4  # (no worse than the path it replaces)


def test_fused_kv_projection_pack_is_deterministic_and_sees_weight_updates():
    import fresco_amd
    case = synth.make_attention_case(4, 256, "L3", seed=33)
    ctrl = synth.controller_for(case, "cf", DEV)
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl)
    attn = copy.deepcopy(case["attn"]).to(DEV).half()
    x = case["hidden"].to(DEV).half()
    with torch.no_grad():
        a = proc(attn, x)
        b = proc(attn, x)
        assert torch.equal(a, b)
        attn.to_v.weight.mul_(0.5)       # the kernel reads the live weights: V halves, so does the output (to_out is linear)
        c = proc(attn, x)
    bias = attn.to_out[0].bias.float()
    assert float(((c.float() - bias) - 0.5 * (a.float() - bias)).abs().max()) < 2e-3
