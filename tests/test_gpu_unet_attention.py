"""The plain attention processor on the GPU: unet_attention (head dim 160) against a float64 softmax on the same fp16 operands,
and UNetAttnProcessor against the float64 records of the restated module (tests/unet_attention_model.py, stand-in weights;
tests/golden/unet_attention_golden.npz holds each record's checksums and the reference arithmetic's noise).

Bars:
  * the kernel: the project's attention bar, |got - ref| <= 1e-3 + 2e-3 |ref| (tests/test_gpu_attention.py), N(0, 1) q, k, v;
    the operands lie inside larger buffers whose other rows and columns are NaN (k, v, q) or a sentinel (out): a pad key that
    reached the maximum, the sum or P.V, or a read or a store outside the tensors, shows as a non-finite value, an error or a
    changed sentinel; a second run gives the same bits and leaves the inputs unchanged;
  * the processor: |got - record| <= 4 x the recorded noise of the reference arithmetic x the record's largest magnitude (the
    margin of DESIGN.md sections 16 - 20), read from the golden file;
  * the shell: UNetTransformer around stand-in modules carrying the processor against the same shell around the fp32 stand-in
    attention, within section 20's module bar plus the attention bar.
Every comparison prints its ratio to the bar; the processor's beside the ratio of the restated module in fp16 on PyTorch's own
kernels.
"""
import os

import numpy as np
import pytest
import torch

import unet_attention_model as M
import unet_transformer_model as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D = 160
GUARD_ROWS, GUARD_COLS = 3, 8          # (8 fp16 columns: the tensors stay 16-byte aligned)
SENTINEL = 7.0
LQS = (1, 31, 32, 33, 64, 100, 256)
LKS = (1, 5, 63, 64, 65, 77, 129, 256, 448)


def _bits(t):
    return t.view(torch.int16)


def _embed(parts, rows, fill):
    """one (GUARD_ROWS + rows + GUARD_ROWS, GUARD_COLS + sum of widths + GUARD_COLS) buffer of `fill`; part i ((B, L, C) fp16) goes
    to rows GUARD_ROWS .. + B L of its column block; -> (buffer, [the (B, L, C) views])"""
    C = parts[0].shape[-1]
    buf = torch.full((rows + 2 * GUARD_ROWS, len(parts) * C + 2 * GUARD_COLS), fill, dtype=torch.float16, device=DEV)
    views = []
    for i, p in enumerate(parts):
        B, L, _ = p.shape
        v = buf[GUARD_ROWS:GUARD_ROWS + B * L, GUARD_COLS + i * C:GUARD_COLS + (i + 1) * C].unflatten(0, (B, L))
        v.copy_(p)
        views.append(v)
    return buf, views


def _reference(q, k, v, H, scale):
    """float64 softmax attention on the GPU from the fp16 operands -> (out (B, Lq, C), scaled logits (B, H, Lq, Lk))"""
    B, Lq, C = q.shape
    split = lambda t: t.double().view(B, -1, H, D).transpose(1, 2)  # noqa: E731
    logits = split(q) @ split(k).transpose(-1, -2) * scale
    out = (torch.softmax(logits, -1) @ split(v)).transpose(1, 2).reshape(B, Lq, C)
    return out, logits


def _run(name, q, k, v, H, layout, ref=None):
    """unet_attention on q, k, v embedded in guarded buffers in the given layout; every check of the module docstring"""
    from fresco_amd import ops
    B, Lq, C = q.shape
    Lk = k.shape[1]
    scale = D ** -0.5
    nan = float("nan")
    if layout == "qkv":       # q | k | v as column slices of one (rows, 3 C) buffer
        bufs = [_embed([q, k, v], B * max(Lq, Lk), nan)]
        (qv, kv, vv), = [b[1] for b in bufs]
    else:                     # q alone; k | v as column slices of a (rows, 2 C) buffer
        bufs = [_embed([q], B * Lq, nan), _embed([k, v], B * Lk, nan)]
        (qv,), (kv, vv) = bufs[0][1], bufs[1][1]
    keep = [b[0].clone() for b in bufs]
    obuf = torch.full((B * Lq + 2 * GUARD_ROWS, C + 2 * GUARD_COLS), SENTINEL, dtype=torch.float16, device=DEV)
    out = obuf[GUARD_ROWS:GUARD_ROWS + B * Lq, GUARD_COLS:GUARD_COLS + C].unflatten(0, (B, Lq))
    got = ops.unet_attention(qv, kv, vv, H, scale, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (B, Lq, C)
    res = got.clone()
    again = ops.unet_attention(qv, kv, vv, H, scale)            # a second run, into a dense tensor of its own: the same bits
    assert again.is_contiguous() and torch.equal(_bits(again), _bits(res)), name
    for (buf, _), kept in zip(bufs, keep):
        assert torch.equal(_bits(buf), _bits(kept)), name       # the inputs (NaN bands included) are unchanged
    out.fill_(SENTINEL)
    assert bool((obuf == SENTINEL).all()), name                 # nothing was stored around the output
    if ref is None:
        ref = _reference(q, k, v, H, scale)[0]
    assert bool(torch.isfinite(res).all()), name
    err = (res.double() - ref).abs()
    bar = 1e-3 + 2e-3 * ref.abs()
    ratio = float((err / bar).max())
    assert ratio <= 1.0, (name, ratio)
    return ratio


def _operands(B, H, Lq, Lk, seed):
    gen = torch.Generator().manual_seed(seed)
    C = H * D
    return tuple(torch.randn(B, L, C, generator=gen).half().to(DEV) for L in (Lq, Lk, Lk))


@pytest.mark.parametrize("Lk", LKS, ids=lambda v: "Lk%d" % v)
def test_kernel_matches_float64_softmax(Lk):
    """one key; a ragged first block; exactly two blocks of 32; a one-key third block; the text; a one-key second tile;
    several tiles -- each with one query, ragged and whole query blocks, and several of them"""
    worst = 0.0
    for Lq in LQS:
        for B, H in ((1, 1), (3, 2)):
            q, k, v = _operands(B, H, Lq, Lk, seed=1000 * Lq + Lk + B)
            ref = _reference(q, k, v, H, D ** -0.5)[0]
            for layout in ("qkv", "kv"):
                worst = max(worst, _run("B%d H%d Lq%d Lk%d %s" % (B, H, Lq, Lk, layout), q, k, v, H, layout, ref))
    print("unet_attention Lk=%d: worst error / bar %.3f over Lq in %s" % (Lk, worst, LQS))


def test_kernel_at_eight_heads():
    q, k, v = _operands(2, 8, 33, 77, seed=5)
    for layout in ("qkv", "kv"):
        print("unet_attention (2, 8, 33, 77) %s: worst error / bar %.3f" % (layout, _run("B2 H8 " + layout, q, k, v, 8, layout)))


def test_kernel_dense_operands_and_default_output():
    """what the processor's cross-attention hands over at head dim 160 when nothing is a slice"""
    from fresco_amd import ops
    q, k, v = _operands(2, 2, 40, 77, seed=9)
    out = ops.unet_attention(q, k, v, 2, D ** -0.5)
    ref = _reference(q, k, v, 2, D ** -0.5)[0]
    assert out.is_contiguous() and bool(((out.double() - ref).abs() <= 1e-3 + 2e-3 * ref.abs()).all())


def test_kernel_large_logits():
    """q scaled so that the scaled logits reach about +-30"""
    q, k, v = _operands(2, 2, 100, 300, seed=11)
    q = (q.float() * 7.0).half()
    ref, logits = _reference(q, k, v, 2, D ** -0.5)
    assert float(logits.max()) > 25.0 and float(logits.min()) < -25.0
    for layout in ("qkv", "kv"):
        print("unet_attention logits in [%.1f, %.1f] %s: worst error / bar %.3f"
              % (float(logits.min()), float(logits.max()), layout, _run("large logits " + layout, q, k, v, 2, layout, ref)))


def _with_common_direction(seed, late_sign):
    """q = N(0, 1) + 0.75 in every component, so a key of +-3 in every component has a scaled logit of about +-28 (+-3) for
    every row, where an N(0, 1) key has one of about N(0, 1.25^2)"""
    B, H, Lq, Lk = 2, 2, 70, 300
    q, k, v = _operands(B, H, Lq, Lk, seed)
    q = (q.float() + 0.75).half()
    k = k.clone()
    if late_sign > 0:
        k[:, 290] = 3.0                       # ONE key of the third tile holds every row's maximum
    else:
        k[:, 128:] = -3.0                     # every key after the first tile lies far below it
    return q, k, v


def test_kernel_late_tile_holds_every_rows_maximum():
    q, k, v = _with_common_direction(13, +1)
    ref, logits = _reference(q, k, v, 2, D ** -0.5)
    assert bool((logits.argmax(-1) == 290).all())
    assert float((logits[..., 290] - logits[..., :128].max(-1).values).min()) > 4.0    # the running maximum must move
    for layout in ("qkv", "kv"):
        print("unet_attention maximum in the third tile %s: worst error / bar %.3f"
              % (layout, _run("late maximum " + layout, q, k, v, 2, layout, ref)))


def test_kernel_keys_after_the_first_tile_lie_far_below_it():
    q, k, v = _with_common_direction(17, -1)
    ref, logits = _reference(q, k, v, 2, D ** -0.5)
    assert float((logits[..., :128].max(-1).values - logits[..., 128:].max(-1).values).min()) > 8.0
    for layout in ("qkv", "kv"):
        print("unet_attention later tiles far below the first %s: worst error / bar %.3f"
              % (layout, _run("low tail " + layout, q, k, v, 2, layout, ref)))


# ---------------------------------------------------------------------------------------------------------------------
# the processor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def records(gold):
    """the float64 record of every case and mode, derived once on the CPU and checked against the golden file's checksums"""
    recs = {}
    for case in M.CASES:
        for mode in M.MODES:
            key = "%s_%s" % (M.case_key(case), mode)
            o = M.record(case, mode)[0]
            sums, sample = M.checksums(o)
            np.testing.assert_allclose(gold[key + "_sums"], sums, rtol=1e-9)
            np.testing.assert_allclose(gold[key + "_thin"], sample, rtol=0, atol=1e-9)
            recs[key] = o
    return recs


def _module(case, mode, processor):
    return M.build_case(case, mode, torch.float16, processor).to(DEV)


def _spy_linears(attn):
    """forward hooks on the module's Linears: the processor must not call them"""
    seen = []
    hooks = [m.register_forward_hook(lambda mod, a, o, _n=n: seen.append(_n))
             for n, m in attn.named_modules() if isinstance(m, torch.nn.Linear)]
    return seen, hooks


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_processor_matches_the_record(case, mode, gold, records):
    from fresco_amd import UNetAttnProcessor, ops
    C, heads, n, L, Tt, TW = case
    key = "%s_%s" % (M.case_key(case), mode)
    x, text = (t.to(DEV) for t in M.inputs(case))
    e = text if mode == "cross" else None
    attn = _module(case, mode, UNetAttnProcessor())
    seen, hooks = _spy_linears(attn)
    calls = []
    real = {nm: getattr(ops, nm) for nm in ("linear", "vae_conv", "attention", "unet_attention")}
    for nm, fn in real.items():
        setattr(ops, nm, lambda *a, _f=fn, _n=nm, **k: calls.append(_n) or _f(*a, **k))
    try:
        got = attn(x, encoder_hidden_states=e)
    finally:
        for nm, fn in real.items():
            setattr(ops, nm, fn)
        for h in hooks:
            h.remove()
    assert got.shape == (n, L, C) and got.dtype == torch.float16 and bool(torch.isfinite(got).all())
    assert seen == []                                                  # no nn.Linear ran
    if C == 1280:     # vae_conv projections around unet_attention
        assert calls == (["vae_conv", "unet_attention", "vae_conv"] if mode == "self"
                         else ["vae_conv", "vae_conv", "unet_attention", "vae_conv"]), calls
    else:             # fresco_linear and fresco_attn_fwd, the text through vae_conv
        assert calls == (["linear", "attention", "linear"] if mode == "self"
                         else ["linear", "vae_conv", "attention", "linear"]), calls
    with torch.no_grad():
        theirs = _module(case, mode, M.RefProcessor())(x, encoder_hidden_states=e)   # PyTorch's own fp16 kernels, for context
    rec = records[key]
    noise, peak = float(gold[key + "_noise"]), float(gold[key + "_peak"])
    bar = 4 * noise * peak
    ratio = float((got.double().cpu() - rec).abs().max() / bar)
    tratio = float((theirs.double().cpu() - rec).abs().max() / bar)
    print("%s |got - record| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16 module: %.3f)"
          % (key, noise, peak, ratio, tratio))
    assert ratio <= 1.0, (key, ratio)
    assert torch.equal(attn(x, encoder_hidden_states=e), got)          # a second call (the text from the cache): the same bits


@pytest.mark.parametrize("case", M.CASES[:2], ids=M.case_key)
def test_self_attention_at_320_and_640_is_the_fresco_processors(case):
    """the same two library calls as FRESCOAttnProcessor2_0 without a controller: reuse, not a copy"""
    from fresco_amd import FRESCOAttnProcessor2_0, UNetAttnProcessor
    x, _ = (t.to(DEV) for t in M.inputs(case))
    attn = _module(case, "self", UNetAttnProcessor())
    mine = attn(x)
    attn.set_processor(FRESCOAttnProcessor2_0(2, None))
    with torch.no_grad():
        assert torch.equal(attn(x), mine)


@pytest.mark.parametrize("case", [M.CASES[0], M.CASES[3]], ids=M.case_key)
def test_text_cache(case):
    from fresco_amd import UNetAttnProcessor, ops
    x, text = (t.to(DEV) for t in M.inputs(case))
    cached, plain = UNetAttnProcessor(), UNetAttnProcessor(cache_text_kv=False)
    attn = _module(case, "cross", cached)
    convs = []
    real = ops.vae_conv
    ops.vae_conv = lambda x_, w, *a, **k: convs.append(int(w.shape[0])) or real(x_, w, *a, **k)
    try:
        first = attn(x, encoder_hidden_states=text)
        n_first = len(convs)
        second = attn(x, encoder_hidden_states=text)
        assert len(convs) - n_first == n_first - 1                     # every launch but the text's
        attn.set_processor(plain)
        assert torch.equal(attn(x, encoder_hidden_states=text), first) and torch.equal(second, first)
        assert len(convs) == 3 * n_first - 1
    finally:
        ops.vae_conv = real
    attn.set_processor(cached)
    text.mul_(2)                                                       # a version bump: the cached processor projects again
    after = attn(x, encoder_hidden_states=text)
    attn.set_processor(UNetAttnProcessor())
    assert torch.equal(attn(x, encoder_hidden_states=text), after) and not torch.equal(after, first)
    attn.set_processor(cached)
    assert torch.equal(attn(x, encoder_hidden_states=text.clone()), after)   # a new tensor at the same values
    cached.clear()
    assert torch.equal(attn(x, encoder_hidden_states=text), after)


def test_residual_connection_and_rescale_output_factor():
    from fresco_amd import UNetAttnProcessor
    case = M.CASES[2]
    x, text = (t.to(DEV) for t in M.inputs(case))
    attn = _module(case, "cross", UNetAttnProcessor())
    base = attn(x, encoder_hidden_states=text)
    attn.residual_connection, attn.rescale_output_factor = True, 2.0
    assert torch.equal(attn(x, encoder_hidden_states=text), (base + x) / 2.0)


@pytest.mark.parametrize("case", [T.CASES[2], T.CASES[0]], ids=T.case_key)
def test_transformer_shell_around_the_processor(case):
    """UNetTransformer around stand-in attention modules carrying UNetAttnProcessor against the same shell around the fp32
    stand-in attention with the same weights: section 20's module bar plus the attention bar"""
    from fresco_amd import UNetAttnProcessor, UNetTransformer
    assert case in ((1280, 8, 2, 4, 4, 5, 64), (320, 8, 2, 8, 12, 7, 64))
    C, heads, n, H, W, Tt, TW = case
    tgold = T.load_golden(GOLDEN)
    noise, peak = float(tgold[T.case_key(case) + "_noise"][1]), float(tgold[T.case_key(case) + "_peak"][1])
    x, text = (t.to(DEV) for t in T.inputs(case))
    mod = T.build(C, heads, TW, torch.float16).to(DEV)
    blk = mod.transformer_blocks[0]
    ref = UNetTransformer.from_module(mod)(x, text).sample
    proc = UNetAttnProcessor()
    for name, cross in (("attn1", None), ("attn2", TW)):
        old = getattr(blk, name)
        own = M.Attention(C, heads, cross, proc).half().to(DEV)
        own.load_state_dict(old.state_dict())
        setattr(blk, name, own)
    got = UNetTransformer.from_module(mod)(x, text).sample
    assert got.shape == (n, C, H, W) and bool(torch.isfinite(got).all())
    bar = 4 * noise * peak + 1e-3 + 2e-3 * ref.double().abs()
    ratio = float(((got.double() - ref.double()).abs() / bar).max())
    print("%s shell around the processor: worst error / (4 x %.2e x %.3g + the attention bar) = %.3f"
          % (T.case_key(case), noise, peak, ratio))
    assert ratio <= 1.0
