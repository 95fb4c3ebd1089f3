"""GPU parity of the bf16 instantiations of the attention, temporal-attention and projection kernels, through
fresco_amd.ops.

Error bars (rms(x) = root mean square over the tensor):
  attention, temporal : against the fp64 softmax on the bf16 inputs, |err| <= 2^-7 (rms(v) + |ref|): about two bf16 ulps of
                        the output plus the same on the scale of v (P is rounded to bf16, 2^-9 relative, before the PV
                        product).  torch's own bf16 SDPA reaches 0.40 of this bar on the CPU, a CPU model of the kernel
                        (exact bf16 products, P rounded to bf16, row sum of the rounded P) 0.57.
  linear              : against the fp32 matmul of the bf16 operands, |err| <= 2^-8 |ref| + 2^-14 rms(ref): one bf16
                        rounding (2^-9 relative) with a factor two, plus fp32 accumulation-order noise near zero.
Every test prints its worst error as a fraction of the bar."""
import math

import pytest
import torch

import synth
from oracle import fresco_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


def _rms(x):
    return float(x.double().pow(2).mean().sqrt())


def _check_attn(out, ref, v, what):
    assert out.dtype == BF, out.dtype
    out = out.double().cpu()
    assert bool(torch.isfinite(out).all()), what
    bound = 2.0 ** -7 * (_rms(v) + ref.abs())
    frac = float(((out - ref).abs() / bound).max())
    print("%s: worst |err| / bar = %.3f" % (what, frac))
    assert frac <= 1.0, (what, frac)
    return frac


def _ref64(q, k, v, heads, scale, groups_of_b, diag_bias=0.0):
    """fp64 softmax(scale q k^T + diag_bias I) v; q (B,Lq,C), k/v (G,M,C); batch b uses group groups_of_b[b]."""
    q, k, v = q.double(), k.double(), v.double()
    outs = []
    for b in range(q.shape[0]):
        g = groups_of_b[b]
        qh, kh, vh = O._heads(q[b:b + 1], heads), O._heads(k[g:g + 1], heads), O._heads(v[g:g + 1], heads)
        s = qh @ kh.transpose(-1, -2) * scale
        if diag_bias:
            n = min(s.shape[-2], s.shape[-1])
            s[..., range(n), range(n)] += diag_bias
        outs.append(O._merge(torch.softmax(s, -1) @ vh))
    return torch.cat(outs, 0)


def _qkv(g, B, Lq, M, C, kgain=1.0, Bk=None):
    q = torch.randn(B, Lq, C, generator=g).to(BF)
    k = (torch.randn(Bk or B, M, C, generator=g) * kgain).to(BF)
    v = torch.randn(Bk or B, M, C, generator=g).to(BF)
    return q, k, v


def _run(q, k, v, H, scale, **kw):
    import fresco_amd.ops as ops
    return ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale, **kw)


@pytest.mark.parametrize("D", [8, 16, 32, 40, 64, 80, 96, 128])
@pytest.mark.parametrize("Lq,M", [(64, 64), (200, 333), (128, 1)])
def test_bf16_attention_plain(D, Lq, M):
    g = synth.gen(D * 1000 + Lq)
    B, H = 3, 8 if D <= 40 else 4
    q, k, v = _qkv(g, B, Lq, M, H * D)
    scale = 1.0 / math.sqrt(D)
    _check_attn(_run(q, k, v, H, scale), _ref64(q, k, v, H, scale, list(range(B))), v, "plain D=%d (%d,%d)" % (D, Lq, M))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("which", ["d40_one_block", "d80_halves", "d80_halves_small_q", "d80_single"])
def test_bf16_attention_instantiations(which):
    """D = 40 with one query block per wave (a grid that would leave CUs idle at 512 rows per workgroup); D = 80 in the
    <80, 2> instantiation (B H >= CUs) and in the single-block one (B H < CUs).  <80, 2> votes per workgroup between the
    half-tile body and two passes of the single-block body: with N(0,1) q, k (logit bound up to 22 log2 units, the first
    tile's maximum about 4) the no-max-search test fails somewhere in every workgroup and all of them fall back; q * 0.4
    (bound <= 9) keeps every workgroup on the half-tile body."""
    qgain = 1.0
    if which == "d40_one_block":
        B, H, D, Lq, M = 1, 8, 40, 700, 150
    elif which.startswith("d80_halves"):
        H, D, Lq, M = 8, 80, 320, 200
        B = (_cus() + H - 1) // H
        qgain = 0.4 if which.endswith("small_q") else 1.0
    else:
        B, H, D, Lq, M = 2, 8, 80, 320, 200
    g = synth.gen(len(which) + D)
    q, k, v = _qkv(g, B, Lq, M, H * D)
    q = (q.float() * qgain).to(BF)
    scale = 1.0 / math.sqrt(D)
    _check_attn(_run(q, k, v, H, scale), _ref64(q, k, v, H, scale, list(range(B))), v, which)


@pytest.mark.parametrize("D", [40, 80])
def test_bf16_attention_grouping(D):
    """cross-frame grouping (kv_rows gather from a random mask with frame 0 full; frame-0-only form) and the spatial form
    (scale 0.2 / sqrt(D), diagonal bias)."""
    g = synth.gen(7 + D)
    chunk, N, HW, H = 2, 3, 96, 8
    B, C = chunk * N, H * D
    q, k, v = _qkv(g, B, HW, HW, C)
    mask = torch.rand(N, HW, generator=g) < 0.3
    mask[0] = True
    rows = mask.reshape(-1).nonzero().squeeze(1).to(torch.int32)
    scale = 1.0 / math.sqrt(D)
    grp = [b // N for b in range(B)]
    out = _run(q, k, v, H, scale, kv_rows=rows.to(DEV), n_groups=chunk, M=int(rows.numel()), group_rows=N * HW)
    kc = O.compact_cross_frame(k.double(), mask, N, chunk)
    vc = O.compact_cross_frame(v.double(), mask, N, chunk)
    _check_attn(out, _ref64(q, kc, vc, H, scale, grp), vc, "grouped D=%d" % D)
    out0 = _run(q, k, v, H, scale, n_groups=chunk, M=HW, group_rows=N * HW)
    k0 = k.reshape(chunk, N, HW, C)[:, 0]
    v0 = v.reshape(chunk, N, HW, C)[:, 0]
    _check_attn(out0, _ref64(q, k0, v0, H, scale, grp), v0, "frame0 D=%d" % D)
    outb = _run(q, k, v, H, 0.2 * scale, diag_bias=1.5)
    _check_attn(outb, _ref64(q, k, v, H, 0.2 * scale, list(range(B)), diag_bias=1.5), v, "diag bias D=%d" % D)


@pytest.mark.parametrize("D", [40, 80])
def test_bf16_attention_large_logits(D):
    """keys at 6 x N(0,1): |logit| ~ 25.  A scale folded into a re-rounded bf16 Q (what the fp16 kernel does up to this
    logit range) misses the bar by 3 - 4 x here; the bf16 kernels keep Q exact and scale the fp32 scores."""
    g = synth.gen(60 + D)
    B, H, Lq, M = 3, 8, 200, 333
    q, k, v = _qkv(g, B, Lq, M, H * D, kgain=6.0)
    scale = 1.0 / math.sqrt(D)
    _check_attn(_run(q, k, v, H, scale), _ref64(q, k, v, H, scale, list(range(B))), v, "6x keys D=%d" % D)


def test_bf16_attention_forced_rescale():
    """one key dominates late in the sequence: the running-max rescale (m_run on the bf16 grid) on every tile"""
    g = synth.gen(11)
    B, H, D, L = 1, 8, 40, 320
    q, k, v = _qkv(g, B, L, L, H * D)
    k[0, 70] = (q[0, 5].float() * 4).to(BF)
    k[0, 300] = (q[0, 5].float() * 8).to(BF)
    scale = 1.0 / math.sqrt(D)
    _check_attn(_run(q, k, v, H, scale), _ref64(q, k, v, H, scale, [0]), v, "rescale")


@pytest.mark.parametrize("what", ["v_2p18", "v_2m30", "q_2p10_k_2m10"])
@pytest.mark.parametrize("D", [40, 80])
def test_bf16_attention_value_range(what, D):
    """power-of-two factors (exact in bf16): values far beyond fp16's largest / below its smallest normal number, and
    q, k whose product is O(1) while neither fits the fp16 kernel's comfortable range"""
    g = synth.gen(5 + D)
    B, H, Lq, M = 2, 8, 200, 333
    q, k, v = _qkv(g, B, Lq, M, H * D)
    if what == "v_2p18":
        v = (v.float() * 2.0 ** 18).to(BF)
    elif what == "v_2m30":
        v = (v.float() * 2.0 ** -30).to(BF)
    else:
        q, k = (q.float() * 2.0 ** 10).to(BF), (k.float() * 2.0 ** -10).to(BF)
    scale = 1.0 / math.sqrt(D)
    _check_attn(_run(q, k, v, H, scale), _ref64(q, k, v, H, scale, list(range(B))), v, "%s D=%d" % (what, D))


def test_bf16_attention_strided_qkv():
    """q, k, v as column slices of one (B, L, 3C) buffer"""
    g = synth.gen(21)
    B, H, D, L = 2, 8, 40, 200
    C = H * D
    qkv = torch.randn(B, L, 3 * C, generator=g).to(BF)
    dq = qkv.to(DEV)
    import fresco_amd.ops as ops
    scale = 1.0 / math.sqrt(D)
    out = ops.attention(dq[..., :C], dq[..., C:2 * C], dq[..., 2 * C:], H, scale)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    _check_attn(out, _ref64(q, k, v, H, scale, list(range(B))), v, "strided")


@pytest.mark.parametrize("D,H,N,HW", [(40, 8, 8, 150), (80, 8, 5, 150), (40, 8, 3, 151), (40, 8, 20, 70), (40, 8, 40, 33)])
def test_bf16_temporal_attention(D, H, N, HW):
    """one key tile, two key tiles and the vector-ALU path (N > 32); maps and mask as in test_temporal_attention"""
    import fresco_amd.ops as ops
    g = synth.gen(3 * D + N)
    chunk = 2
    C, B = H * D, chunk * N
    q, k, v = _qkv(g, B, HW, HW, C)
    fwd = torch.stack([torch.randperm(HW, generator=g) for _ in range(N)], 0)
    tm = torch.rand(HW, N, N, generator=g) < 0.6
    tm = tm | tm.transpose(1, 2) | torch.eye(N, dtype=torch.bool)
    scale = 0.2 / math.sqrt(D)
    out = ops.temporal_attention(q.to(DEV), k.to(DEV), v.to(DEV), fwd.to(DEV).unsqueeze(1), tm.to(DEV).unsqueeze(1), H,
                                 scale, chunk)
    ref = O.temporal_attention(q.double(), k.double(), v.double(), fwd, tm, H, scale, chunk)
    assert ref.dtype == torch.float64
    _check_attn(out, ref, v, "temporal D=%d N=%d HW=%d" % (D, N, HW))


# ---- linear -------------------------------------------------------------------------------------------------------------
def _check_linear(o, r, what):
    assert o.dtype == BF
    o = o.float().cpu()
    bound = 2.0 ** -8 * r.abs() + 2.0 ** -14 * _rms(r)
    frac = float(((o - r).abs() / bound).max())
    print("%s: worst |err| / bar = %.3f" % (what, frac))
    assert frac <= 1.0, (what, frac)


def _lin_ref(x, W, b):
    y = x.float().reshape(-1, x.shape[-1]) @ W.float().t()
    return y if b is None else y + b.float()


@pytest.mark.parametrize("K,N,nw,M,bias", [(320, 320, 3, 1000, False), (640, 640, 2, 129, True), (320, 320, 1, 64, True)])
def test_bf16_linear_matches_fp32_matmul(K, N, nw, M, bias):
    import fresco_amd.ops as ops
    g = synth.gen(K + N + nw + M)
    x = torch.randn(M, K, generator=g).to(BF)
    W = (torch.randn(nw * N, K, generator=g) / K ** 0.5).to(BF)
    b = torch.randn(nw * N, generator=g).to(BF) if bias else None
    Ws = [w.contiguous().to(DEV) for w in W.chunk(nw, 0)]
    bs = None if b is None else [t.contiguous().to(DEV) for t in b.chunk(nw, 0)]
    outs = ops.linear(x.to(DEV), Ws, bs)
    assert len(outs) == nw
    for j, (o, r) in enumerate(zip(outs, _lin_ref(x, W, b).chunk(nw, 1))):
        assert tuple(o.shape) == (M, N)
        _check_linear(o, r, "linear K=%d nw=%d out %d" % (K, nw, j))


def test_bf16_linear_gathered_rows_and_fused_kv_buffer():
    import fresco_amd.ops as ops
    g = synth.gen(3)
    B, HW, C = 4, 96, 320
    x = torch.randn(B, HW, C, generator=g).to(BF)
    W = (torch.randn(2 * C, C, generator=g) / C ** 0.5).to(BF)
    dx, dW = x.to(DEV), W.to(DEV)
    # a 77-entry table that repeats rows
    rows = torch.randint(0, 40, (77,), generator=g).to(torch.int32)
    assert rows.unique().numel() < 77
    o = ops.linear(dx, [dW[:C].contiguous()], None, x_rows=rows.to(DEV))[0]
    assert tuple(o.shape) == (77, C)
    _check_linear(o, _lin_ref(x.reshape(-1, C)[rows.long()], W[:C], None), "gathered rows")
    # outputs written into the two halves of a fused K|V buffer
    kv = torch.zeros(B, HW, 2 * C, dtype=BF, device=DEV)
    outs = ops.linear(dx, [dW[:C].contiguous(), dW[C:].contiguous()], None, outs=[kv[..., :C], kv[..., C:]])
    assert outs[0].data_ptr() == kv.data_ptr()
    r = _lin_ref(x, W, None)
    _check_linear(kv[..., :C].reshape(-1, C), r[:, :C], "fused K|V buffer, K half")
    _check_linear(kv[..., C:].reshape(-1, C), r[:, C:], "fused K|V buffer, V half")


def test_bf16_mixed_dtypes_raise():
    import fresco_amd.ops as ops
    g = synth.gen(1)
    q, k, v = (t.to(DEV) for t in _qkv(g, 2, 64, 64, 320))
    with pytest.raises(TypeError):
        ops.attention(q, k.half(), v, 8, 0.158)
    with pytest.raises(TypeError):
        ops.attention(q.half(), k, v, 8, 0.158)
    fwd = torch.stack([torch.randperm(64, generator=g) for _ in range(1)], 0).to(DEV).unsqueeze(1)
    tm = torch.ones(64, 1, 1, dtype=torch.bool, device=DEV).unsqueeze(1)
    with pytest.raises(TypeError):
        ops.temporal_attention(q, k, v.half(), fwd, tm, 8, 0.03, 2)
    x = torch.zeros(8, 320, dtype=BF, device=DEV)
    W = torch.zeros(320, 320, dtype=BF, device=DEV)
    with pytest.raises(ValueError):
        ops.linear(x, W.half())
    with pytest.raises(ValueError):
        ops.linear(x.half(), W)
    with pytest.raises(ValueError):
        ops.linear(x, W, [torch.zeros(320, dtype=torch.float16, device=DEV)])
