"""The UNet transformer on the GPU: the kernels of csrc/unet_tf.hip against float64 on the same operands, the native module
against the float64 records of the restated one (tests/golden/unet_transformer_golden.npz; stand-in weights and stand-in
attention, tests/unet_transformer_model.py), patch_unet_resnets + patch_unet_transformers on a stand-in tree, and one block
around the project's own attention processor.

Bars (e = 2^-24, one fp32 rounding):
  * unet_layernorm: test_gpu_vae.py's norm bar with x := x + r,
    16 e ((|x| + |mean|) rstd |gamma| + |beta|) + 1e-6 + 2^-11 |y|; sum_out is bit-equal to (x.float() + r.float()).half(); a
    second run gives the same bits;
  * unet_geglu: with v, g the exact value and gate and Bv = K e (sum |x| |Wv| + |bv|), Bg likewise (vae_conv's accumulation
    bar),  |gelu(g)| Bv + 1.13 |v| Bg + 1.13 Bv Bg + 16 e |v| max(|g|, 1) + 2^-11 |ref| + 1e-6:  1.13 bounds |gelu'|, and
    16 e |v| |g| covers the fp32 evaluation of 0.5 g (1 + erf(g / sqrt 2)), about 8 roundings, each absolute in |g|, with a
    factor 2;
  * the module: |got - record| <= 4 x the recorded noise of the reference arithmetic for that tensor x its largest magnitude
    (DESIGN.md sections 16, 17 and 19's margin), for the first block's GEGLU output and the module's output.
Every comparison prints its ratio to the bar; the module's beside the ratio of PyTorch's own fp16 kernels on the restated
module.
"""
import math
import os

import numpy as np
import pytest
import torch

import unet_transformer_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = 2.0 ** -24
H11 = 2.0 ** -11


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _check(name, got, ref, bound):
    got, ref, bound = (t.detach().to("cpu", torch.float64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
                       for t in (got, ref, bound))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    print("%s: worst error / bound %.3f" % (name, float((err / bound).max())))
    assert np.isfinite(got).all() and np.all(err <= bound), name


# ---------------------------------------------------------------------------------------------------------------
# unet_layernorm
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 320, 640, 1280, 2560], ids=lambda c: "C%d_pieces%d" % (c, c // 8))
def test_layernorm_matches_float64(C):
    """320: fewer 16-byte pieces than a wave has lanes; 1280: 2.5 per lane; 2560: the widest, five per lane"""
    from fresco_amd import ops
    eps = 1e-5
    gamma, beta = (_randn(C, seed=C + 1) * 0.5 + 1.0).to(DEV), _randn(C, seed=C + 2).to(DEV)
    for rows in (1, 3, 64, 257):
        x, r = _randn(rows, C, seed=C + rows) * 2.0 + 0.5, _randn(rows, C, seed=C + rows + 1) * 1.5
        x[-1] = x[-1] * 0.125 - 6.0        # one row is shifted and scaled: its statistics differ
        x, r = x.half().to(DEV), r.half().to(DEV)
        keep_x, keep_r = x.clone(), r.clone()
        for use_r in (False, True):
            xs = x.double() + (r.double() if use_r else 0.0)
            mean = xs.mean(-1, keepdim=True)
            rstd = 1.0 / torch.sqrt(xs.var(-1, unbiased=False, keepdim=True) + eps)
            ref = (xs - mean) * rstd * gamma.double() + beta.double()
            bar = 16 * E * ((xs.abs() + mean.abs()) * rstd * gamma.double().abs() + beta.double().abs()) + 1e-6 + H11 * ref.abs()
            rounded = (x.float() + r.float()).half() if use_r else x
            for want_sum in (False, True):
                res = ops.unet_layernorm(x, gamma, beta, eps, residual=r if use_r else None, want_sum=want_sum)
                y, total = res if want_sum else (res, None)
                assert y.dtype == torch.float16 and y.shape == x.shape and y.is_contiguous()
                _check("layernorm C=%d rows=%d%s%s" % (C, rows, " + r" if use_r else "", " + sum_out" if want_sum else ""),
                       y, ref, bar)
                if want_sum:
                    assert torch.equal(total, rounded)                      # x + r rounded ONCE
                again = ops.unet_layernorm(x, gamma, beta, eps, residual=r if use_r else None, want_sum=want_sum)
                assert torch.equal(y, again[0] if want_sum else again)
        assert torch.equal(x, keep_x) and torch.equal(r, keep_r)            # the inputs are left unchanged


def test_layernorm_row_strides_and_leading_shapes():
    """x and r as column slices of wider tensors (row strides above C, each its own), and (n, L, C) as the module passes it"""
    from fresco_amd import ops
    C, rows, eps = 320, 67, 1e-5
    gamma, beta = (_randn(C, seed=1) * 0.5 + 1.0).to(DEV), _randn(C, seed=2).to(DEV)
    wide_x, wide_r = (_randn(rows, C + 64, seed=3) * 2.0).half().to(DEV), (_randn(rows, 2 * C, seed=4)).half().to(DEV)
    x, r = wide_x[:, 64:], wide_r[:, C:]
    assert x.stride(0) == C + 64 and r.stride(0) == 2 * C and not x.is_contiguous()
    keep = wide_x.clone()
    y, total = ops.unet_layernorm(x, gamma, beta, eps, residual=r, want_sum=True)
    dense_y, dense_total = ops.unet_layernorm(x.contiguous(), gamma, beta, eps, residual=r.contiguous(), want_sum=True)
    assert torch.equal(y, dense_y) and torch.equal(total, dense_total) and torch.equal(wide_x, keep)
    assert torch.equal(total, (x.float() + r.float()).half())
    xs = x.double() + r.double()
    mean = xs.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(xs.var(-1, unbiased=False, keepdim=True) + eps)
    ref = (xs - mean) * rstd * gamma.double() + beta.double()
    _check("layernorm strided C=320 rows=67", y, ref,
           16 * E * ((xs.abs() + mean.abs()) * rstd * gamma.double().abs() + beta.double().abs()) + 1e-6 + H11 * ref.abs())
    x3 = x.contiguous().view(1, rows, C)
    assert torch.equal(ops.unet_layernorm(x3, gamma, beta, eps, residual=r.contiguous().view(1, rows, C)).view(rows, C), y)
    # a 3-D column slice: 10 rows of 64 at a stride of 192, the leading dimensions nested
    C = 64
    gamma, beta = (_randn(C, seed=5) * 0.5 + 1.0).to(DEV), _randn(C, seed=6).to(DEV)
    wide = (_randn(2, 5, 192, seed=7) * 2.0 + 0.5).half().to(DEV)
    x, keep = wide[..., 64:128], wide.clone()
    assert x.shape == (2, 5, C) and x.stride() == (960, 192, 1) and not x.is_contiguous()
    y = ops.unet_layernorm(x, gamma, beta, eps)
    assert y.shape == (2, 5, C) and y.dtype == torch.float16 and y.is_contiguous() and torch.equal(wide, keep)
    assert torch.equal(y, ops.unet_layernorm(x.contiguous(), gamma, beta, eps))
    xs = x.double()
    mean = xs.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(xs.var(-1, unbiased=False, keepdim=True) + eps)
    ref = (xs - mean) * rstd * gamma.double() + beta.double()
    _check("layernorm 3-D column slice C=64 rows=10 ld=192", y, ref,
           16 * E * ((xs.abs() + mean.abs()) * rstd * gamma.double().abs() + beta.double().abs()) + 1e-6 + H11 * ref.abs())


# ---------------------------------------------------------------------------------------------------------------
# unet_geglu
# ---------------------------------------------------------------------------------------------------------------
def _geglu_case(M_, K, inner, seed):
    """x, diffusers-layout weight and bias; the gate's bias is drawn over [-6, 6] so both tails of the erf are hit"""
    x = (_randn(M_, K, seed=seed) * 1.0).half()
    w = (_randn(2 * inner, K, seed=seed + 1) * K ** -0.5).half()
    b = _randn(2 * inner, seed=seed + 2) * 0.5
    b[inner:] = torch.rand(inner, generator=torch.Generator().manual_seed(seed + 3)) * 12.0 - 6.0
    return x, w, b


def _geglu_ref_and_bar(x, w, b, K, inner):
    xd, wd, bd = x.double().cpu(), w.double().cpu(), b.double().cpu()
    v, g = xd @ wd[:inner].t() + bd[:inner], xd @ wd[inner:].t() + bd[inner:]
    Bv = K * E * (xd.abs() @ wd[:inner].abs().t() + bd[:inner].abs())
    Bg = K * E * (xd.abs() @ wd[inner:].abs().t() + bd[inner:].abs())
    gelu = 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))
    ref = v * gelu
    bar = gelu.abs() * Bv + 1.13 * v.abs() * Bg + 1.13 * Bv * Bg + 16 * E * v.abs() * g.abs().clamp(min=1.0) + H11 * ref.abs() + 1e-6
    return ref, bar, g


def _geglu_against_float64(M_, K, inner):
    from fresco_amd import ops
    from fresco_amd.unet_transformer import pack_geglu_weight
    x, w, b = _geglu_case(M_, K, inner, seed=M_ + K + inner)
    pw, pb = pack_geglu_weight(w, b)
    xg, pw, pb = x.to(DEV), pw.to(DEV), pb.to(DEV)
    out = ops.unet_geglu(xg, pw, pb)
    assert out.shape == (M_, inner) and out.dtype == torch.float16
    ref, bar, g = _geglu_ref_and_bar(x, w, b, K, inner)
    if M_ * inner >= 127 * 32:
        assert float(g.min()) < -4.0 and float(g.max()) > 4.0                # both tails
    _check("geglu M=%d K=%d inner=%d" % (M_, K, inner), out, ref, bar)
    assert torch.equal(out, ops.unet_geglu(xg, pw, pb))                      # a second run: the same bits


@pytest.mark.parametrize("K", [32, 64, 320])
@pytest.mark.parametrize("M_", [1, 127, 128, 129, 300], ids=lambda m: "M%d" % m)
def test_geglu_matches_float64(M_, K):
    """inner 32: one pair block, three waves' channel blocks dead; 64: exactly one tile; 96: a ragged second tile; 160;
    M = 300 x inner = 160 is 3 x 3 = 9 workgroups, more than the 8 XCDs of the deal"""
    for inner in (32, 64, 96, 160):
        _geglu_against_float64(M_, K, inner)


def test_geglu_at_the_unet_width():
    _geglu_against_float64(129, 320, 1280)


def test_geglu_row_stride_and_flat_rows():
    from fresco_amd import ops
    from fresco_amd.unet_transformer import pack_geglu_weight
    K, inner, L = 64, 96, 150
    x, w, b = _geglu_case(2 * L, K, inner, seed=5)
    pw, pb = pack_geglu_weight(w, b)
    xg, pw, pb = x.to(DEV), pw.to(DEV), pb.to(DEV)
    dense = ops.unet_geglu(xg, pw, pb)
    # ldo > inner: the columns beyond inner are left untouched
    buf = torch.full((2 * L, inner + 8), 7.0, dtype=torch.float16, device=DEV)
    got = ops.unet_geglu(xg, pw, pb, out=buf[:, :inner])
    assert got.data_ptr() == buf.data_ptr() and torch.equal(buf[:, :inner], dense)
    assert bool((buf[:, inner:] == 7.0).all())
    # two images' tokens as one flat M: the same bits as each image on its own, and as the (n, L, K) tensor
    x3 = xg.view(2, L, K)
    both = ops.unet_geglu(x3, pw, pb)
    assert both.shape == (2, L, inner) and torch.equal(both.view(2 * L, inner), dense)
    for i in range(2):
        assert torch.equal(ops.unet_geglu(x3[i].contiguous(), pw, pb), both[i])


# ---------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_module_matches_the_record(case, gold):
    from fresco_amd import UNetTransformer
    C, heads, n, H, W, T, TW = case
    key = M.case_key(case)
    mod = M.build(C, heads, TW, torch.float16).to(DEV)   # the restated module in fp16 on the GPU, with the stand-in weights
    native = UNetTransformer.from_module(mod)
    x, text = (t.to(DEV) for t in M.inputs(case))
    x_cl = x.contiguous(memory_format=torch.channels_last)
    taps, ttaps = {}, {}
    res = native(x_cl, text, taps=taps)
    out = res.sample
    with torch.no_grad():
        tout = mod(x, text, taps=ttaps).sample   # PyTorch's own kernels in fp16: printed beside ours for context, nothing asserted
    assert out.shape == (n, C, H, W) and out.dtype == torch.float16
    assert out.is_contiguous(memory_format=torch.channels_last) and out.permute(0, 2, 3, 1).is_contiguous()
    assert taps["geglu"].shape == (n, H * W, 4 * C) and taps["tokens"].shape == (n, H * W, C)
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    ours = {"tap": taps["geglu"].reshape(n, H, W, 4 * C), "out": out.permute(0, 2, 3, 1)}
    theirs = {"tap": ttaps["tap"].reshape(n, H, W, 4 * C), "out": tout.permute(0, 2, 3, 1)}
    worst = []
    for i, t in enumerate(M.TENSORS):
        rec = gold["%s_%s" % (key, t)]
        a, b = M.thin(ours[t].double()), M.thin(theirs[t].double())
        assert a.shape == rec.shape, (t, a.shape, rec.shape)
        bar = 4 * noise[i] * peak[i]
        ratio, tratio = float(np.abs(a - rec).max() / bar), float(np.abs(b - rec).max() / bar)
        print("%s %-3s |got - record| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16 module: %.3f)"
              % (key, t, noise[i], peak[i], ratio, tratio))
        worst.append((ratio, t))
    assert max(worst)[0] <= 1.0, max(worst)
    # the same bits from a contiguous input (converted once), from a second call, as a tuple, and in the plain layout
    assert torch.equal(native(x, text).sample, out)
    as_tuple = native(x_cl, text, return_dict=False)
    assert isinstance(as_tuple, tuple) and len(as_tuple) == 1 and torch.equal(as_tuple[0], out)
    plain = native(x_cl, text, memory_format=torch.contiguous_format).sample
    assert plain.is_contiguous() and plain.shape == out.shape and torch.equal(plain, out)
    assert torch.equal(UNetTransformer.from_module(mod, memory_format=torch.contiguous_format)(x, text).sample, out)


def test_patched_tree_runs_natively(monkeypatch):
    from fresco_amd import (UNetResnet, UNetTransformer, ops, patch_unet_resnets, patch_unet_transformers, unpatch_unet_resnets,
                            unpatch_unet_transformers)
    n, c, H, W, T, TW = 2, 320, 8, 12, 7, 64
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn(n, c, H, W, generator=gen) * 1.5).half()
    x[-1] = x[-1] * 0.5 + 1.0
    temb = torch.randn(n, M.R.TEMB_CHANNELS, generator=gen).half()
    text = torch.randn(n, T, TW, generator=gen).half()
    with torch.no_grad():
        rec = M.build_tree(torch.float64)(x.double(), temb.double(), text.double())                   # the unpatched tree in float64
        r16 = M.build_tree(torch.float32)(x.float(), temb.float(), text.float(), M.round16).double()  # the reference's noise
    peak = float(rec.abs().max())
    noise = float((r16 - rec).abs().max() / peak)
    assert noise > 0
    tree = M.build_tree(torch.float16).to(DEV)
    xd, td, ed = x.to(DEV), temb.to(DEV), text.to(DEV)
    with torch.no_grad():
        own = tree(xd, td, ed)                                                                        # PyTorch's fp16 kernels
    seen = []
    own_r, own_t = M.R.Resnet.forward, M.Transformer.forward
    monkeypatch.setattr(M.R.Resnet, "forward", lambda self, *a, **k: seen.append("resnet") or own_r(self, *a, **k))
    monkeypatch.setattr(M.Transformer, "forward", lambda self, *a, **k: seen.append("transformer") or own_t(self, *a, **k))
    assert patch_unet_resnets(tree) == 1 and patch_unet_transformers(tree) == 1
    try:
        res_native, tf_native = vars(tree.resnets[0])["forward"], vars(tree.attentions[0])["forward"]
        assert isinstance(res_native, UNetResnet) and isinstance(tf_native, UNetTransformer)
        ptrs = {}

        def res_spy(x_, t_, *a, **k):
            o = res_native(x_, t_, *a, **k)
            ptrs["resnet_out"] = o.data_ptr()
            return o

        def tf_spy(h_, *a, **k):
            ptrs["transformer_in"] = h_.data_ptr()
            ptrs["transformer_in_nhwc"] = h_.permute(0, 2, 3, 1).is_contiguous()
            o = tf_native(h_, *a, **k)
            ptrs["transformer_out_nhwc"] = o[0].permute(0, 2, 3, 1).is_contiguous()
            return o
        tree.resnets[0].__dict__["forward"] = res_spy
        tree.attentions[0].__dict__["forward"] = tf_spy
        gn_inputs = []
        gn = ops.unet_groupnorm
        monkeypatch.setattr(ops, "unet_groupnorm", lambda x_, *a, **k: gn_inputs.append(x_.data_ptr()) or gn(x_, *a, **k))
        with torch.no_grad():
            got = tree(xd, td, ed)
        assert seen == []                                      # the modules' own forwards did not run
        # no copy between the resnet and the transformer: the transformer's GroupNorm READS the resnet's output
        assert ptrs["transformer_in"] == ptrs["resnet_out"] and ptrs["transformer_in_nhwc"]
        assert len(gn_inputs) == 3 and gn_inputs[2] == ptrs["resnet_out"]
        assert ptrs["transformer_out_nhwc"]                    # what the consumer permutes and reshapes is NHWC in memory
        bar = 4 * noise * peak
        ratio, tratio = float((got.double().cpu() - rec).abs().max() / bar), float((own.double().cpu() - rec).abs().max() / bar)
        print("patched tree |got - float64| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16 tree: %.3f)"
              % (noise, peak, ratio, tratio))
        assert got.shape == (n, H * W, 64) and ratio <= 1.0
    finally:
        assert unpatch_unet_resnets(tree) == 1 and unpatch_unet_transformers(tree) == 1
    assert not any("forward" in vars(m) for m in tree.modules())
    with torch.no_grad():
        back = tree(xd, td, ed)
    assert seen == ["resnet", "transformer"] and float((back.double() - own.double()).abs().max()) <= 4 * noise * peak


def test_block_around_the_projects_own_attention():
    """synth.FakeAttn modules called through FRESCOAttnProcessor2_0 (no controller) as attn1 / attn2 of one block at 320
    channels, 8 heads (head dim 40), 8 x 8 tokens, a 7-token text: the shell runs around the project's attention and matches
    the same shell around the fp32 stand-in attention with the same weights"""
    import fresco_amd
    import synth
    from fresco_amd import UNetTransformer
    C, heads, n, H, W, T = 320, 8, 2, 8, 8, 7
    case = (C, heads, n, H, W, T, C)                 # FakeAttn's to_k takes C values: the text is C wide
    x, text = (t.to(DEV) for t in M.inputs(case))
    x64, text64 = x.double().cpu(), text.double().cpu()
    with torch.no_grad():
        rec = M.build(C, heads, C, torch.float64)(x64, text64).sample
        r16 = M.build(C, heads, C, torch.float32)(x64.float(), text64.float(), q=M.round16).sample.double()
    peak = float(rec.abs().max())
    noise = float((r16 - rec).abs().max() / peak)
    mod = M.build(C, heads, C, torch.float16).to(DEV)
    blk = mod.transformer_blocks[0]
    standin = {"attn1": blk.attn1, "attn2": blk.attn2}
    calls = {}
    hooks = [a.register_forward_hook(lambda m, args, kwargs, o, _k=k: calls.__setitem__(_k, (args[0], kwargs, o)), with_kwargs=True)
             for k, a in standin.items()]
    ref = UNetTransformer.from_module(mod)(x, text).sample
    for h in hooks:
        h.remove()

    class ProcessorAttn(synth.FakeAttn):
        """diffusers' Attention.forward: the processor is called with the module"""

        def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **kwargs):
            return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states,
                                  attention_mask=attention_mask, **kwargs)
    for k, a in standin.items():
        own = ProcessorAttn(C, heads, [a.to_q.weight, a.to_k.weight, a.to_v.weight, a.to_out[0].weight], a.to_out[0].bias)
        own = own.half().to(DEV)
        own.processor = fresco_amd.FRESCOAttnProcessor2_0(2, None)
        setattr(blk, k, own)
        # the attention itself, on what the stand-in was given: the processor's own tolerance
        y, kwargs, o = calls[k]
        with torch.no_grad():
            mine = own(y, **kwargs)
        assert mine.shape == o.shape and mine.dtype == torch.float16
        _check("block with the processor: %s" % k, mine, o, 1e-3 + 2e-3 * o.double().abs())
    got = UNetTransformer.from_module(mod)(x, text).sample
    assert got.shape == (n, C, H, W) and bool(torch.isfinite(got).all())
    _check("block with the processor: output (module bar 4 x %.2e x %.3g + the attention's)" % (noise, peak), got, ref,
           4 * noise * peak + 1e-3 + 2e-3 * ref.double().abs())
