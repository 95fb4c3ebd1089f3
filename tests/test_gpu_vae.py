"""The VAE decoder on the GPU: the kernels of csrc/vae.hip against float64 on the same operands, and the native decoder end
to end -- every recorded tap, the image and its uint8 form -- against the float64 records of the restated module
(tests/golden/vae_golden.npz; stand-in weights, tests/vae_model.py).

Bars (e = 2^-24, one fp32 rounding):
  * vae_conv: the fp16 operands are exact, so |got - ref| <= K e sum |x| |w| + 2^-11 |ref| + 1e-6 (fp32 output: without the
    2^-11 term): the worst case of K fp32 additions plus one output rounding;
  * GroupNorm [+ SiLU]: test_gpu_midas.py's bound, 16 e ((|x| + |mean|) rstd |gamma| + |beta|) + 1e-6, plus 2^-11 |y| for the
    fp16 result (SiLU's slope is at most 1.1, inside the 16);
  * softmax: 2^-11 p + 8 e, and every row sums to 1 within Lk 2^-12;
  * end to end: |got - record| <= 4 x the recorded noise of the reference arithmetic for that tensor x its largest magnitude
    (DESIGN.md section 16's margin: two fp16-class evaluations in different summation orders); uint8 image: no value 2 or
    more from the record, the share one apart at most twice the reference arithmetic's recorded share plus 0.5 %.
Every comparison prints its ratio to the bar.
"""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_model as M
from conv_ref import check as _check, conv_ref as _conv_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = 2.0 ** -24
H11 = 2.0 ** -11


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------
# vae_conv
# ---------------------------------------------------------------------------------------------------------------
CONV_SHAPES = {
    # name: (n, Hs, Ws, cin, cout, ksize, up2)
    "ragged_tile_two_images": (2, 10, 14, 128, 128, 3, False),
    "K4608": (1, 9, 5, 512, 256, 3, False),
    "shortcut_1x1": (1, 9, 5, 512, 256, 1, False),
    "several_tiles": (1, 24, 40, 256, 512, 3, False),
    "up2": (2, 5, 7, 256, 256, 3, True),
}


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", sorted(CONV_SHAPES))
def test_conv_matches_float64(shape, residual):
    from fresco_amd import _lib, ops
    from fresco_amd.vae import pack_conv_weight
    n, Hs, Ws, cin, cout, k, up2 = CONV_SHAPES[shape]
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    seed = sum(map(ord, shape))
    x = (_randn(n, Hs, Ws, cin, seed=seed) * 1.5).half().to(DEV)
    x[-1] = x[-1] * 0.5 + 1.0  # the last image differs in scale and offset: a border that bleeds would show
    w = (_randn(cout, cin, k, k, seed=seed + 1) * (2.0 / (cin * k * k)) ** 0.5).half().to(DEV)
    bias = _randn(cout, seed=seed + 2).to(DEV)
    res = (_randn(n, H, W, cout, seed=seed + 3) * 2.0).half().to(DEV) if residual else None
    ref, mass = _conv_ref(x, w, up2)
    ref = ref + bias.double() + (res.double() if residual else 0.0)
    K = cin * k * k
    wp = pack_conv_weight(w)
    got = ops.vae_conv(x, wp, bias, n, H, W, cin, cout, k, up2=up2, residual=res)
    assert got.shape == (n, H, W, cout) and got.dtype == torch.float16
    _check("conv %s fp16" % shape, got, ref, K * E * mass + H11 * ref.abs() + 1e-6)
    if not residual:
        got32 = ops.vae_conv(x, wp, bias, n, H, W, cin, cout, k, up2=up2, out_kind=_lib.VAE_OUT_F32)
        assert got32.dtype == torch.float32
        _check("conv %s fp32" % shape, got32, ref, K * E * mass + 1e-6)
        again = ops.vae_conv(x, wp, bias, n, H, W, cin, cout, k, up2=up2, out_kind=_lib.VAE_OUT_F32)
        assert torch.equal(got32, again)


def test_conv_ragged_channels_and_the_nchw_image():
    """conv_out's form: 128 -> 3 channels written as (n, 3, H, W); and conv_in's: 4 real channels padded to 32"""
    from fresco_amd import _lib, ops
    from fresco_amd.vae import pack_conv_weight
    n, H, W = 2, 10, 22
    x = _randn(n, H, W, 128, seed=5).half().to(DEV)
    w = (_randn(3, 128, 3, 3, seed=6) * (1.0 / 1152) ** 0.5).half().to(DEV)
    bias = _randn(3, seed=7).to(DEV)
    ref, mass = _conv_ref(x, w, False)
    ref = ref + bias.double()
    got = ops.vae_conv(x, pack_conv_weight(w), bias, n, H, W, 128, 3, 3, out_kind=_lib.VAE_OUT_F16_NCHW)
    assert got.shape == (n, 3, H, W)
    bound = 1152 * E * mass + H11 * ref.abs() + 1e-6
    _check("conv 128 -> 3 NCHW", got.permute(0, 2, 3, 1), ref, bound)
    nhwc = ops.vae_conv(x, pack_conv_weight(w), bias, n, H, W, 128, 3, 3)
    assert torch.equal(nhwc, got.permute(0, 2, 3, 1))
    z = _randn(n, 4, H, W, seed=8).half().to(DEV)
    wq, bq = (torch.eye(4) + 0.2 * _randn(4, 4, seed=9)).to(DEV), (0.1 * _randn(4, seed=10)).to(DEV)
    xin = ops.vae_input(z, wq, bq)
    assert xin.shape == (n, H, W, 32) and not xin[..., 4:].any()
    pq = torch.einsum("oc,nchw->nhwo", wq.double(), z.double()) + bq.double()
    _check("post_quant_conv", xin[..., :4], pq, 8 * E * (torch.einsum("oc,nchw->nhwo", wq.double().abs(), z.double().abs())
                                                         + bq.double().abs()) + H11 * pq.abs() + 1e-6)
    w_in = (_randn(512, 4, 3, 3, seed=11) * (1.0 / 36) ** 0.5).half().to(DEV)
    b_in = _randn(512, seed=12).to(DEV)
    ref, mass = _conv_ref(xin[..., :4].contiguous(), w_in, False)
    ref = ref + b_in.double()
    got = ops.vae_conv(xin, pack_conv_weight(w_in, cin_pad=32), b_in, n, H, W, 32, 512, 3)
    _check("conv_in 4 (32) -> 512", got, ref, 288 * E * mass + H11 * ref.abs() + 1e-6)


def test_conv_per_image_weights_in_both_attention_arrangements():
    """n 2, L 70, K 512: Q K^T (70 ragged output columns, fp32, row stride 96), V^T = W_v x^T (the weights are the pixel
    operand, a per-row bias, per-image x as the weight matrix) and P V over the key axis padded to 96"""
    from fresco_amd import _lib, ops
    n, L, C, Lp = 2, 70, 512, 96
    q = _randn(n, L, C, seed=1).half().to(DEV)
    k = _randn(n, L, C, seed=2).half().to(DEV)
    k[1] *= 0.5
    scores = torch.full((n * L, Lp), float("nan"), dtype=torch.float32, device=DEV)
    ops.vae_conv(q, k, None, n, L, 1, C, L, 1, out_kind=_lib.VAE_OUT_F32, w_img_stride=L * C, ldo=Lp, out=scores)
    ref = q.double() @ k.double().transpose(1, 2)
    mass = q.double().abs() @ k.double().abs().transpose(1, 2)
    _check("Q K^T", scores.view(n, L, Lp)[..., :L], ref, C * E * mass + 1e-6)
    assert torch.isnan(scores[:, L:]).all()  # nothing is stored beyond cout

    wv = (_randn(C, C, seed=3) * C ** -0.5).half().to(DEV)
    bv = _randn(C, seed=4).to(DEV)
    h = _randn(n, L, C, seed=5).half().to(DEV)
    h[1] += 1.0
    vt = torch.zeros(n, C, Lp, dtype=torch.float16, device=DEV)
    ops.vae_conv(wv, h, bv, n, C, 1, C, L, 1, x_img_stride=0, w_img_stride=L * C, bias_rows=True, ldo=Lp, out=vt)
    ref = (h.double() @ wv.double().t() + bv.double()).transpose(1, 2)
    mass = (h.double().abs() @ wv.double().abs().t()).transpose(1, 2)
    _check("V^T", vt[..., :L], ref, C * E * mass + H11 * ref.abs() + 1e-6)
    assert not vt[..., L:].any()

    p = torch.zeros(n, L, Lp, dtype=torch.float16, device=DEV)
    p[..., :L] = torch.softmax(_randn(n, L, L, seed=6) * 3.0, -1).half().to(DEV)
    o = ops.vae_conv(p, vt, None, n, L, 1, Lp, C, 1, w_img_stride=C * Lp)
    ref = p.double() @ vt.double().transpose(1, 2)
    mass = p.double() @ vt.double().abs().transpose(1, 2)
    _check("P V", o.view(n, L, C), ref, Lp * E * mass + H11 * ref.abs() + 1e-6)


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm + SiLU, softmax
# ---------------------------------------------------------------------------------------------------------------
def _groupnorm_against_float64(n, H, W, C, silu):
    from fresco_amd import ops
    x = _randn(n, H, W, C, seed=C) * 3.0 + 1.5
    x[1] = x[1] * 0.25 - 4.0
    x = x.half()
    gamma, beta = _randn(C, seed=C + 1) * 0.5 + 1.0, _randn(C, seed=C + 2)
    x64 = x.double().permute(0, 3, 1, 2)
    ref = F.group_norm(x64, 32, gamma.double(), beta.double(), 1e-6)
    if silu:
        ref = F.silu(ref)
    ref = ref.permute(0, 2, 3, 1).numpy()
    g = x64.reshape(n, 32, -1)
    mean, rstd = g.mean(2), 1.0 / torch.sqrt(g.var(2, unbiased=False) + 1e-6)
    per_c = lambda t: t.repeat_interleave(C // 32, 1)[:, None, None, :].numpy()  # noqa: E731
    bound = 16 * E * ((np.abs(x.double().numpy()) + np.abs(per_c(mean))) * per_c(rstd) * np.abs(gamma.double().numpy())
                      + np.abs(beta.double().numpy())) + 1e-6 + H11 * np.abs(ref)
    y = ops.vae_groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6, silu=silu)
    assert y.dtype == torch.float16 and y.shape == x.shape
    _check("groupnorm C=%d%s" % (C, " + SiLU" if silu else ""), y, ref, bound)
    assert torch.equal(y, ops.vae_groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6, silu=silu))


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("C", [128, 256, 512], ids=lambda c: "C%d_cpg%d" % (c, c // 32))
def test_groupnorm_silu_matches_float64(C, silu):
    """(2, 18, 30): 540 pixels = three workgroups of the statistics pass, the last one partly filled; image 1 is shifted and
    scaled, so that its statistics differ"""
    _groupnorm_against_float64(2, 18, 30, C, silu)


@pytest.mark.parametrize("C", [128, 512], ids=lambda c: "C%d_cpg%d" % (c, c // 32))
@pytest.mark.parametrize("P", [1, 257])
def test_groupnorm_at_one_pixel_and_a_second_chunk_of_one(C, P):
    """the edges of the statistics pass (csrc/groupnorm_stats.h) on fp16 rows: one pixel per image, and 257 pixels = a full
    chunk and one more pixel"""
    _groupnorm_against_float64(2, 1, P, C, True)


@pytest.mark.parametrize("Lk", [70, 1000, 4096])
def test_softmax_matches_float64(Lk):
    from fresco_amd import ops
    rows, ld = 12, (Lk + 31) // 32 * 32
    scale = 512 ** -0.5
    s = torch.full((rows, ld), float("nan"))
    s[:, :Lk] = _randn(rows, Lk, seed=Lk) * 40.0
    s[1, :Lk] = torch.linspace(-3e4, 3e4, Lk)                  # logits spanning +-3e4 before the scale
    s[2, :Lk] = _randn(Lk, seed=Lk + 1) * 1e4
    s[2, Lk // 2], s[2, Lk - 1] = 3e4, -3e4
    s[3, :Lk] = 7.25                                           # a constant row
    s[4, :Lk] = -3e4
    s[4, Lk - 1] = 3e4                                         # one-hot in effect
    p = ops.vae_softmax(s.to(DEV), Lk, scale, ld_out=ld)
    assert p.shape == (rows, ld) and p.dtype == torch.float16
    assert not p[:, Lk:].any()
    ref = torch.softmax(s[:, :Lk].double() * scale, -1)
    _check("softmax Lk=%d" % Lk, p[:, :Lk], ref, H11 * ref + 8 * E)
    sums = p[:, :Lk].double().sum(-1).cpu()
    print("softmax Lk=%d: worst |row sum - 1| / (Lk 2^-12) %.3f" % (Lk, float((sums - 1).abs().max() / (Lk * 2.0 ** -12))))
    assert ((sums - 1).abs() <= Lk * 2.0 ** -12).all()
    assert torch.equal(p[3, :Lk].cpu(), torch.full((Lk,), 1.0 / Lk, dtype=torch.float32).half())


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def vae16():
    """the restated module in fp16 on the GPU, with the stand-in weights"""
    return M.build(torch.float16).to(DEV)


@pytest.fixture(scope="module")
def decoder(vae16):
    from fresco_amd import VAEDecoder
    return VAEDecoder.from_vae(vae16)


def decoder_against_record(case, gold, vae16, decoder):
    """every tap and the image of decode(latents(case)) against the record `gold`, the uint8 rule where the record holds the
    whole uint8 image, and a second call's bits -> the image (tests/test_gpu_vae_fullsize.py runs its own records through
    this).  vae16 None: without PyTorch's module beside ours"""
    key = M.case_key(case)
    z = M.latents(case).to(DEV)
    taps, ttaps = {}, {}
    img = decoder.decode(z, taps=taps).sample
    with torch.no_grad():
        # PyTorch's own kernels in fp16: printed beside ours for context, nothing asserted on it
        timg = vae16(z, ttaps) if vae16 is not None else torch.full_like(img, float("nan"))
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    worst = []
    for i, t in enumerate(M.TAPS + ("image",)):
        ours = M.thin(taps[t].double()) if t != "image" else M.thin_image(img.double())
        theirs = M.thin(ttaps[t].double()) if t in ttaps else M.thin_image(timg.double()) if t == "image" else np.nan
        rec = gold["%s_%s" % (key, t)]
        assert ours.shape == rec.shape, (t, ours.shape, rec.shape)
        bar = 4 * noise[i] * peak[i]
        ratio, tratio = float(np.abs(ours - rec).max() / bar), float(np.abs(theirs - rec).max() / bar)
        print("%s %-8s |got - record| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16 module: %.3f)"
              % (key, t, noise[i], peak[i], ratio, tratio))
        worst.append((ratio, t))
    assert img.shape == (case[0], 3, 8 * case[1], 8 * case[2]) and img.dtype == torch.float16
    assert all(ratio <= 1.0 for ratio, _ in worst), worst  # (a NaN ratio fails here; max() of the pairs would step over it)
    if key + "_image_u8" in gold:
        u8, rec8 = M.tensor2numpy(img), gold[key + "_image_u8"]
        d = np.abs(u8.astype(int) - rec8.astype(int))
        td = np.abs(M.tensor2numpy(timg).astype(int) - rec8.astype(int))
        share, allowed = float((d == 1).mean()), 2 * float(gold[key + "_u8_share"]) + 0.005
        print("%s uint8 image: largest difference %d, one apart %.3f %% (allowed %.3f %%)   (PyTorch fp16 module: %d, %.3f %%)"
              % (key, d.max(), 100 * share, 100 * allowed, td.max(), 100 * float((td == 1).mean())))
        assert d.max() <= 1 and share <= allowed
    again = decoder.decode(z, return_dict=False)[0]
    assert torch.equal(img, again)
    return img


@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_decoder_matches_the_record(case, gold, vae16, decoder):
    assert M.case_key(case) + "_image_u8" in gold  # these records hold the whole uint8 image: its rule is applied
    decoder_against_record(case, gold, vae16, decoder)


def test_patched_pipe_decodes_natively(vae16, decoder, monkeypatch):
    import fresco_amd
    from fresco_amd import patch_vae_decode, unpatch_vae_decode
    import sys
    step_mod = sys.modules["fresco_amd.step"]  # (the package exports the function under the module's name)
    case = M.CASES[0]
    z = M.latents(case).to(DEV)
    want = decoder.decode(z).sample
    pipe = types.SimpleNamespace(vae=vae16)
    calls = []
    own_forward = vae16.forward
    monkeypatch.setattr(vae16, "forward", lambda *a, **k: calls.append("module") or own_forward(*a, **k))
    try:
        patch_vae_decode(pipe)
        assert torch.equal(pipe.vae.decode(z).sample, want)
        assert torch.equal(pipe.vae.decode(z, return_dict=False)[0], want)
        assert calls == []

        # fresco_amd.step with saliency, flows and occs: decode -> warp -> encode (pipe_FRESCO.py:44-47)
        class Sched:
            alphas_cumprod = torch.cumprod(1.0 - torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2, dim=0)
            one = torch.tensor(1.0)

            def previous_timestep(self, t):
                return t - 50

        class Dist:
            def __init__(self, x):
                self.x = x

            def sample(self):
                return F.avg_pool2d(self.x.float(), 8).to(self.x.dtype)[:, [0, 1, 2, 0]]
        seen = {}
        pipe.scheduler = Sched()
        monkeypatch.setattr(vae16, "config", types.SimpleNamespace(scaling_factor=0.5), raising=False)
        monkeypatch.setattr(vae16, "encode", lambda image: types.SimpleNamespace(latent_dist=Dist(image)), raising=False)
        monkeypatch.setattr(step_mod, "warp_tensor", lambda image, *a, **k: seen.setdefault("image", image))
        sample, eps = z * 0.7, (_randn(*z.shape, seed=3) * 0.1).half().to(DEV)
        prev, x0 = fresco_amd.step(pipe, eps, 701, sample, torch.Generator(DEV).manual_seed(0), flows=[0], occs=[0],
                                   saliency=torch.ones(1))
        pred, _ = step_mod.predict_x0(sample, eps, alpha_prod_t=float(Sched.alphas_cumprod[701]))
        assert torch.equal(seen["image"], decoder.decode(pred / 0.5).sample) and calls == []
        assert torch.equal(x0, 0.5 * Dist(seen["image"]).sample()) and prev.shape == z.shape
    finally:
        unpatch_vae_decode(pipe)
    assert "decode" not in vars(vae16)
    assert pipe.vae.decode(z).sample.shape == want.shape and calls == ["module"]
