"""The VAE encoder on the GPU: the kernels of csrc/vae_enc.hip against float64 on the same operands, and the native encoder
end to end -- every recorded tap and the distribution's parameters -- against the float64 records of the restated module
(tests/golden/vae_encoder_golden.npz; stand-in weights, tests/vae_encoder_model.py).

Bars (e = 2^-24, one fp32 rounding):
  * vaeenc_conv_down: test_gpu_vae.py's convolution bar, |got - ref| <= K e sum |x| |w| + 2^-11 |ref| + 1e-6 with K = 9 cin (the
    fp16 operands are exact: K fp32 additions in the worst case plus one output rounding); the last output row and the last
    output column are also compared alone, so that a wrong pad decision cannot hide in a maximum over the tensor;
  * vaeenc_input: exact;
  * vaeenc_moments: 2^-11 |ref| + 16 e sum |x| |w| + 1e-7;
  * vaeenc_sample: 2^-11 |ref| + 8 e (|mean| + |std noise|) + 1e-7;
  * end to end: |got - record| <= 4 x the recorded noise of the reference arithmetic for that tensor x its largest magnitude
    (DESIGN.md section 16 / 17's margin: two fp16-class evaluations in different summation orders).
Every comparison prints its ratio to the bar.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_encoder_model as EM
import vae_model as M

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
# vaeenc_conv_down
# ---------------------------------------------------------------------------------------------------------------
DOWN_SHAPES = {
    # name: (n, H, W, cin, cout)
    "exact_tiles": (2, 16, 32, 128, 128),
    "odd_sides_ragged_tiles": (1, 17, 25, 512, 512),          # the pad row and column are never read
    "even_sides_ragged_tiles": (1, 18, 34, 256, 256),         # both are read; several channel chunks
    "one_pixel_per_image": (3, 2, 2, 128, 128),
    "ragged_cout": (1, 20, 36, 128, 40),
    # cout & 3 != 0: the one-element-per-store epilogue; one chunk, nine steps; cout below one MFMA block, so one wave column
    # multiplies one block and the other none; 3 x 5 pixels inside one tile, pad row and column both read
    "scalar_store_cout": (1, 6, 10, 32, 6),
}


def _down_ref(x, w):
    """x (n, H, W, cin) fp16, w (cout, cin, 3, 3) fp16 on the GPU -> (float64 result, sum |x| |w|), both (n, H // 2, W // 2,
    cout): F.pad on the right and bottom, im2col at stride 2 (F.unfold) and one float64 product"""
    x64 = F.pad(x.double().permute(0, 3, 1, 2), (0, 1, 0, 1))
    n, H, W = x.shape[:3]
    w64 = w.double().reshape(w.shape[0], -1)
    outs = []
    for xx, ww in ((x64, w64), (x64.abs(), w64.abs())):
        cols = F.unfold(xx, 3, stride=2)
        outs.append((ww @ cols).transpose(1, 2).reshape(n, H // 2, W // 2, -1))
    return outs


@pytest.mark.parametrize("shape", sorted(DOWN_SHAPES))
def test_conv_down_matches_float64(shape):
    from fresco_amd import ops
    from fresco_amd.vae import pack_conv_weight
    n, H, W, cin, cout = DOWN_SHAPES[shape]
    seed = sum(map(ord, shape))
    # x is the head of a longer buffer whose tail holds 100: a pad row or column that is READ instead of taken as zero shows,
    # in the last image too
    buf = torch.full((n * H * W * cin + (W + 2) * cin,), 100.0, dtype=torch.float16, device=DEV)
    x = buf[:n * H * W * cin].view(n, H, W, cin)
    x.copy_((_randn(n, H, W, cin, seed=seed) * 1.5).half())
    x[-1] = x[-1] * 0.5 + 1.0  # the last image differs in scale and offset: an image that bleeds into the one before shows
    w = (_randn(cout, cin, 3, 3, seed=seed + 1) * (2.0 / (cin * 9)) ** 0.5).half().to(DEV)
    bias = _randn(cout, seed=seed + 2).to(DEV)
    ref, mass = _down_ref(x, w)
    ref = ref + bias.double()
    got = ops.vaeenc_conv_down(x, pack_conv_weight(w), bias)
    assert got.shape == (n, H // 2, W // 2, cout) and got.dtype == torch.float16
    bound = 9 * cin * E * mass + H11 * ref.abs() + 1e-6
    _check("conv_down %s" % shape, got, ref, bound)
    _check("conv_down %s, last row" % shape, got[:, -1], ref[:, -1], bound[:, -1])
    _check("conv_down %s, last column" % shape, got[:, :, -1], ref[:, :, -1], bound[:, :, -1])
    again = ops.vaeenc_conv_down(x, pack_conv_weight(w), bias)
    assert torch.equal(got, again)
    assert bool((buf[n * H * W * cin:] == 100.0).all())


@pytest.mark.parametrize("size", [(1, 8, 8), (2, 24, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_input_is_exact(size):
    from fresco_amd import ops
    n, H, W = size
    img = _randn(n, 3, H, W, seed=H).half().to(DEV)
    out = ops.vaeenc_input(img)
    assert out.shape == (n, H, W, 32) and out.dtype == torch.float16
    assert torch.equal(out[..., :3], img.permute(0, 2, 3, 1)) and not out[..., 3:].any()
    out8 = ops.vaeenc_input(img, cpad=8)
    assert out8.shape == (n, H, W, 8) and torch.equal(out8[..., :3], img.permute(0, 2, 3, 1)) and not out8[..., 3:].any()


@pytest.mark.parametrize("size", [(2, 5, 7), (3, 20, 28)], ids=lambda s: "%dx%dx%d" % s)
def test_moments_match_float64(size):
    from fresco_amd import ops
    n, hh, ww = size
    h = (_randn(n, hh, ww, 8, seed=hh) * 3.0).to(DEV)
    h[-1] = h[-1] * 0.25 + 2.0
    wq, bq = (torch.eye(8) + 0.2 * _randn(8, 8, seed=1)).to(DEV), (0.1 * _randn(8, seed=2)).to(DEV)
    got = ops.vaeenc_moments(h, wq, bq)
    assert got.shape == (n, 8, hh, ww) and got.dtype == torch.float16
    ref = torch.einsum("oc,nhwc->nohw", wq.double(), h.double()) + bq.double()[None, :, None, None]
    mass = torch.einsum("oc,nhwc->nohw", wq.double().abs(), h.double().abs())
    _check("moments %dx%dx%d" % size, got, ref, H11 * ref.abs() + 16 * E * mass + 1e-7)
    assert torch.equal(got, ops.vaeenc_moments(h, wq, bq))


@pytest.mark.parametrize("scale", [1.0, 0.18215])
def test_sample_matches_float64_on_both_sides_of_the_clamp(scale):
    from fresco_amd import ops
    n, hh, ww = 2, 9, 13
    params = torch.cat([_randn(n, 4, hh, ww, seed=3) * 2.0, _randn(n, 4, hh, ww, seed=4) * 3.0 - 2.0], 1).half()
    noise = _randn(n, 4, hh, ww, seed=5).half()
    # hand-made elements: logvar below, at and above the clamp's edges.  Below -30: mean 0 and noise 8, so that
    # exp(-15) 8 = 2.4e-6 (clamped) stands against exp(-20) 8 = 1.6e-8; above 20: noise 0.5, so that exp(10) / 2 = 11013
    # (clamped) stands against exp(12.5) / 2, which is not an fp16 number
    for i, (lv, nz, mean) in enumerate(((-40.0, 8.0, 0.0), (-30.0, 8.0, 0.0), (0.0, 1.5, -0.75), (20.0, 0.5, 3.0), (25.0, 0.5, 3.0),
                                        (25.0, -0.5, 0.0))):
        params[i % n, 4 + i % 4, i, 2 * i], noise[i % n, i % 4, i, 2 * i], params[i % n, i % 4, i, 2 * i] = lv, nz, mean
    got = ops.vaeenc_sample(params.to(DEV), noise.to(DEV), scale)
    assert got.shape == noise.shape and got.dtype == torch.float16
    mean, logvar = params[:, :4].double(), params[:, 4:].double().clamp(-30.0, 20.0)
    spread = torch.exp(0.5 * logvar) * noise.double()
    ref = float(np.float32(scale)) * (mean + spread)
    _check("sample scale %g" % scale, got, ref, H11 * ref.abs() + 8 * E * (mean.abs() + spread.abs()) + 1e-7)
    for i in range(6):
        print("  hand-made element %d: got %.6g, float64 %.6g" % (i, float(got[i % n, i % 4, i, 2 * i]), float(ref[i % n, i % 4, i, 2 * i])))
    assert float(got[0, 0, 0, 0]) > 1e-6 * scale and float(got[0, 0, 4, 8]) > 1000 * scale
    assert torch.equal(got, ops.vaeenc_sample(params.to(DEV), noise.to(DEV), scale))


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return EM.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def vae16():
    """the restated module (both halves) in fp16 on the GPU, with the stand-in weights"""
    return EM.build(torch.float16).to(DEV)


@pytest.fixture(scope="module")
def encoder(vae16):
    from fresco_amd import VAEEncoder
    return VAEEncoder.from_vae(vae16)


def encoder_against_record(case, gold, vae16, encoder):
    """every tap and the parameters of encode(images(case)) against the record `gold`, and a second call's bits -> the
    parameters (tests/test_gpu_vae_encoder_fullsize.py runs its own records through this)"""
    key = EM.case_key(case)
    x = EM.images(case).to(DEV)
    taps, ttaps = {}, {}
    dist = encoder.encode(x, taps=taps).latent_dist
    with torch.no_grad():
        tparams = vae16.encode_forward(x, ttaps)  # PyTorch's own kernels in fp16: printed beside ours for context, nothing asserted
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    worst = []
    for i, t in enumerate(EM.TAPS + ("parameters",)):
        ours = EM.thin(taps[t].double()) if t != "parameters" else dist.parameters.double().cpu().numpy()
        theirs = EM.thin(ttaps[t].double()) if t != "parameters" else tparams.double().cpu().numpy()
        rec = gold["%s_%s" % (key, t)]
        assert ours.shape == rec.shape, (t, ours.shape, rec.shape)
        bar = 4 * noise[i] * peak[i]
        ratio, tratio = float(np.abs(ours - rec).max() / bar), float(np.abs(theirs - rec).max() / bar)
        print("%s %-10s |got - record| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16 module: %.3f)"
              % (key, t, noise[i], peak[i], ratio, tratio))
        worst.append((ratio, t))
    n, H, W = case
    assert dist.parameters.shape == (n, 8, H // 8, W // 8) and dist.parameters.dtype == torch.float16
    assert all(ratio <= 1.0 for ratio, _ in worst), worst  # (a NaN ratio fails here; max() of the pairs would step over it)
    again = encoder.encode(x, return_dict=False)[0]
    assert torch.equal(dist.parameters, again.parameters)
    return dist.parameters


@pytest.mark.parametrize("case", EM.CASES, ids=EM.case_key)
def test_encoder_matches_the_record(case, gold, vae16, encoder):
    encoder_against_record(case, gold, vae16, encoder)


def test_latent_dist_is_the_modules_distribution(encoder):
    from fresco_amd import ops
    case = EM.CASES[0]
    dist = encoder.encode(EM.images(case).to(DEV)).latent_dist
    p = dist.parameters
    shape = (case[0], 4, case[1] // 8, case[2] // 8)
    assert torch.equal(dist.mode(), p[:, :4]) and torch.equal(dist.mean, p[:, :4]) and tuple(dist.mean.shape) == shape
    assert torch.equal(dist.logvar, p[:, 4:].clamp(-30.0, 20.0))
    assert torch.equal(dist.std, torch.exp(0.5 * dist.logvar)) and torch.equal(dist.var, torch.exp(dist.logvar))
    # seeded on the device: the module's one torch.randn, and the stream left where that leaves it
    torch.manual_seed(11)
    got = dist.sample()
    after = torch.rand(1, device=DEV)
    torch.manual_seed(11)
    noise = torch.randn(shape, dtype=torch.float16, device=DEV)
    after_plain = torch.rand(1, device=DEV)
    assert got.shape == shape and got.dtype == torch.float16
    assert torch.equal(got, ops.vaeenc_sample(p, noise)) and torch.equal(after, after_plain)
    # a device generator
    got = dist.sample(generator=torch.Generator(DEV).manual_seed(12))
    noise = torch.randn(shape, generator=torch.Generator(DEV).manual_seed(12), dtype=torch.float16, device=DEV)
    assert torch.equal(got, ops.vaeenc_sample(p, noise))
    # a CPU generator draws on the CPU and leaves the device's stream alone
    torch.manual_seed(13)
    got = dist.sample(generator=torch.Generator().manual_seed(14), scale=0.18215)
    after = torch.rand(1, device=DEV)
    torch.manual_seed(13)
    after_plain = torch.rand(1, device=DEV)
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(14), dtype=torch.float16).to(DEV)
    assert torch.equal(got, ops.vaeenc_sample(p, noise, 0.18215)) and torch.equal(after, after_plain)
    # against the module's chain of fp16 operations (context, nothing asserted): close, not equal -- one rounding against four
    chain = (dist.mean + dist.std * noise).double()
    one = ops.vaeenc_sample(p, noise).double()
    mass = dist.mean.double().abs() + (dist.std * noise).double().abs()
    print("sample: worst |one rounding - fp16 chain| / (2^-9 (|mean| + |std noise|)) = %.3f" % float(((one - chain).abs() / (2.0 ** -9 * mass)).max()))


def test_patched_pipe_encodes_natively(vae16, encoder, monkeypatch):
    import fresco_amd
    from fresco_amd import patch_vae, unpatch_vae
    step_mod = sys.modules["fresco_amd.step"]  # (the package exports the function under the module's name)
    case = M.CASES[0]
    z = M.latents(case).to(DEV)
    pipe = types.SimpleNamespace(vae=vae16)

    class Sched:
        alphas_cumprod = torch.cumprod(1.0 - torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2, dim=0)
        one = torch.tensor(1.0)

        def previous_timestep(self, t):
            return t - 50

    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.conv2d was entered")
    seen = {}
    pipe.scheduler = Sched()
    monkeypatch.setattr(vae16, "config", types.SimpleNamespace(scaling_factor=0.5), raising=False)
    monkeypatch.setattr(step_mod, "warp_tensor", lambda image, *a, **k: seen.setdefault("image", image))
    sample, eps = z * 0.7, (_randn(*z.shape, seed=3) * 0.1).half().to(DEV)
    try:
        patch_vae(pipe)
        with monkeypatch.context() as mp:
            mp.setattr(F, "conv2d", refuse)
            with pytest.raises(AssertionError):
                vae16.encoder.conv_in(seen.get("image", torch.zeros(1, 3, 8, 8, dtype=torch.float16, device=DEV)))  # (the trap works)
            torch.manual_seed(7)
            # fresco_amd.step with saliency, flows and occs: decode -> warp -> encode (pipe_FRESCO.py:44-47), both halves native
            prev, x0 = fresco_amd.step(pipe, eps, 701, sample, torch.Generator(DEV).manual_seed(0), flows=[0], occs=[0],
                                       saliency=torch.ones(1))
            direct = pipe.vae.encode(seen["image"], return_dict=False)[0]
        assert seen["image"].shape == (case[0], 3, 8 * case[1], 8 * case[2])
        torch.manual_seed(7)
        want = 0.5 * encoder.encode(seen["image"]).latent_dist.sample()
        assert torch.equal(x0, want) and prev.shape == z.shape and x0.shape == z.shape
        assert torch.equal(direct.parameters, encoder.encode(seen["image"]).latent_dist.parameters)
    finally:
        unpatch_vae(pipe)
    assert "encode" not in vars(vae16) and "decode" not in vars(vae16)
    assert pipe.vae.encode(seen["image"]).latent_dist.parameters.shape == (case[0], 8, case[1], case[2])  # the module's own again
