"""The UNet resnet block on the GPU: the kernels of csrc/unet.hip against float64 on the same operands, the native block
against the float64 records of the restated module (tests/golden/unet_resnet_golden.npz; stand-in weights,
tests/unet_resnet_model.py), and patch_unet_resnets on a stand-in tree.

Bars (e = 2^-24, one fp32 rounding):
  * unet_groupnorm: test_gpu_vae.py's GroupNorm bar with x := x + addend,
    16 e ((|x| + |mean|) rstd |gamma| + |beta|) + 1e-6 + 2^-11 |y|; a second run gives the same bits;
  * unet_temb: (K + 8) e sum |SiLU(t)| |w| + 1e-6: K fp32 additions and the few roundings of SiLU;
  * the block: |got - record| <= 4 x the recorded noise of the reference arithmetic for that tensor x its largest magnitude
    (DESIGN.md sections 16 and 17's margin), for the conv1 + temb tap and the output.
Every comparison prints its ratio to the bar; the block's beside the ratio of PyTorch's own fp16 kernels on the restated
module.
"""
import os

import numpy as np
import pytest
import torch

import unet_resnet_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = 2.0 ** -24
H11 = 2.0 ** -11
WIDTHS = (320, 640, 960, 1280, 1920, 2560)
SLAB_BYTES = {320: 80, 640: 80, 960: 240, 1280: 80, 1920: 240, 2560: 160}  # the LDS form's bytes per pixel (unet.hip)
LDS_PLANE = 96 * 1024


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
# unet_groupnorm
# ---------------------------------------------------------------------------------------------------------------
def _pixel_counts(C):
    pmax = LDS_PLANE // SLAB_BYTES[C]   # the largest plane of the LDS form, and the first of the three-launch form
    return [1, 64, 256, 257, 560, pmax, pmax + 1]


@pytest.mark.parametrize("pi", range(7), ids=["P1", "P64", "P256", "P257", "P560", "Pmax_lds", "Pmax_lds_plus_1"])
@pytest.mark.parametrize("C", WIDTHS, ids=lambda c: "C%d_cpg%d" % (c, c // 32))
def test_groupnorm_matches_float64(C, pi):
    from fresco_amd import _lib, ops
    n, P, eps = 2, _pixel_counts(C)[pi], 1e-5
    form = _lib.load().unet_groupnorm_lds_form(n, P, C)
    assert form == (1 if pi != 6 and (pi != 4 or P * SLAB_BYTES[C] <= LDS_PLANE) else 0), (C, P, form)
    x = _randn(n, P, C, seed=C + P) * 3.0 + 1.5
    x[1] = x[1] * 0.25 - 4.0        # image 1 is shifted and scaled: its statistics differ
    x = x.half().to(DEV)
    gamma, beta = (_randn(C, seed=C + 1) * 0.5 + 1.0).to(DEV), _randn(C, seed=C + 2).to(DEV)
    addend = (_randn(n, C, seed=C + 3) * 2.0).to(DEV)
    addend[1] += 3.0
    cpg = C // 32
    for use_addend in (False, True):
        xa = x.double() + (addend.double()[:, None, :] if use_addend else 0.0)
        g = xa.view(n, P, 32, cpg)
        mean = g.mean((1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(g.var((1, 3), unbiased=False, keepdim=True) + eps)
        norm = ((g - mean) * rstd).view(n, P, C) * gamma.double() + beta.double()
        mass = ((g.abs() + mean.abs()) * rstd).view(n, P, C) * gamma.double().abs() + beta.double().abs()
        for silu in (False, True):
            ref = norm * torch.sigmoid(norm) if silu else norm
            y = ops.unet_groupnorm(x, gamma, beta, eps, silu=silu, addend=addend if use_addend else None)
            assert y.dtype == torch.float16 and y.shape == x.shape
            _check("groupnorm C=%d P=%d form=%s%s%s" % (C, P, "lds" if form else "3-launch", " + addend" if use_addend else "",
                                                       " + SiLU" if silu else ""), y, ref, 16 * E * mass + 1e-6 + H11 * ref.abs())
            again = ops.unet_groupnorm(x, gamma, beta, eps, silu=silu, addend=addend if use_addend else None)
            assert torch.equal(y, again)


def test_groupnorm_takes_any_leading_shape_and_leaves_its_input():
    """(n, H, W, C) as the block passes it, at the narrowest and an in-between width (C = 64: four groups in one 16-byte piece;
    C = 192: groups of 12 bytes)"""
    from fresco_amd import ops
    for C in (64, 192):
        x = (_randn(2, 5, 7, C, seed=C) * 2.0).half().to(DEV)
        keep = x.clone()
        gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        y = ops.unet_groupnorm(x, gamma, beta, 1e-5)
        assert torch.equal(x, keep) and y.shape == x.shape
        g = x.double().view(2, 35, 32, C // 32)
        mean = g.mean((1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(g.var((1, 3), unbiased=False, keepdim=True) + 1e-5)
        ref = ((g - mean) * rstd).view(2, 5, 7, C)
        mass = ((g.abs() + mean.abs()) * rstd).view(2, 5, 7, C)
        _check("groupnorm C=%d (2, 5, 7)" % C, y, ref, 16 * E * mass + 1e-6 + H11 * ref.abs())


# ---------------------------------------------------------------------------------------------------------------
# unet_temb
# ---------------------------------------------------------------------------------------------------------------
def _temb_against_float64(n, K, cout):
    from fresco_amd import ops
    temb = (_randn(n, K, seed=n + K) * 1.5).half().to(DEV)
    temb[-1] = temb[-1] * 0.5 + 1.0
    w = (_randn(cout, K, seed=cout) * (2.0 / K) ** 0.5).half().to(DEV)
    bias, cbias = _randn(cout, seed=cout + 1).to(DEV), _randn(cout, seed=cout + 2).to(DEV)
    out = ops.unet_temb(temb, w, bias, cbias)
    assert out.shape == (n, cout) and out.dtype == torch.float32
    s = temb.double() * torch.sigmoid(temb.double())
    ref = s @ w.double().t() + bias.double() + cbias.double()
    mass = s.abs() @ w.double().abs().t()
    _check("temb n=%d K=%d cout=%d" % (n, K, cout), out, ref, (K + 8) * E * mass + 1e-6)
    assert torch.equal(out, ops.unet_temb(temb, w, bias, cbias))


@pytest.mark.parametrize("cout", [320, 1280])
@pytest.mark.parametrize("n", [1, 3, 16])
def test_temb_matches_float64(n, cout):
    _temb_against_float64(n, 1280, cout)


@pytest.mark.parametrize("n", [17, 33, 64])
def test_temb_past_one_tile_of_images_and_ragged_sizes(n):
    """more than 16 images (the kernel's other instantiations), a K that ends inside a chunk of 512, a last workgroup with two of
    its four channels"""
    _temb_against_float64(n, 520, 322)


# ---------------------------------------------------------------------------------------------------------------
# the block
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_block_matches_the_record(case, gold):
    from fresco_amd import UNetResnet
    cin, cout, n, H, W = case
    key = M.case_key(case)
    mod = M.build(cin, cout, torch.float16).to(DEV)   # the restated module in fp16 on the GPU, with the stand-in weights
    native = UNetResnet.from_module(mod)
    x, temb = (t.to(DEV) for t in M.inputs(case))
    x_cl = x.contiguous(memory_format=torch.channels_last)
    taps, ttaps = {}, {}
    out = native(x_cl, temb, taps=taps)
    with torch.no_grad():
        tout = mod(x, temb, taps=ttaps)   # PyTorch's own kernels in fp16: printed beside ours for context, nothing asserted on it
    assert out.shape == (n, cout, H, W) and out.dtype == torch.float16
    assert out.is_contiguous(memory_format=torch.channels_last) and out.permute(0, 2, 3, 1).is_contiguous()
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    ours = {"tap": taps["conv1_temb"], "out": out.permute(0, 2, 3, 1)}
    theirs = {"tap": ttaps["tap"], "out": tout.permute(0, 2, 3, 1)}
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
    # the same bits from a contiguous input (converted once), from a second call, and in the plain layout
    assert torch.equal(native(x, temb), out)
    assert torch.equal(native(x_cl, temb), out)
    plain = native(x_cl, temb, memory_format=torch.contiguous_format)
    assert plain.is_contiguous() and plain.shape == out.shape and torch.equal(plain, out)
    assert torch.equal(UNetResnet.from_module(mod, memory_format=torch.contiguous_format)(x, temb), out)


def test_patched_tree_runs_natively(monkeypatch):
    from fresco_amd import UNetResnet, patch_unet_resnets, unpatch_unet_resnets
    n, c, H, W = 2, 320, 8, 12
    gen = torch.Generator().manual_seed(7)
    x = (torch.randn(n, c, H, W, generator=gen) * 1.5).half()
    x[-1] = x[-1] * 0.5 + 1.0
    temb = torch.randn(n, M.TEMB_CHANNELS, generator=gen).half()
    with torch.no_grad():
        rec = M.build_tree(torch.float64)(x.double(), temb.double())                    # the unpatched tree in float64 ...
        r16 = M.build_tree(torch.float32)(x.float(), temb.float(), M.round16).double()  # ... and the reference arithmetic's noise
    peak = float(rec.abs().max())
    noise = float((r16 - rec).abs().max() / peak)
    assert noise > 0
    tree = M.build_tree(torch.float16).to(DEV)
    xd, td = x.to(DEV), temb.to(DEV)
    with torch.no_grad():
        own = tree(xd, td)                                                               # PyTorch's fp16 kernels, for context
    seen = []
    own_forward = M.Resnet.forward
    monkeypatch.setattr(M.Resnet, "forward", lambda self, *a, **k: seen.append("module") or own_forward(self, *a, **k))
    assert patch_unet_resnets(tree) == 2
    try:
        calls = []
        for b in (tree.down[0], tree.up["resnets"][0]):
            native = vars(b)["forward"]
            assert isinstance(native, UNetResnet)

            def spy(x_, t_, *a, _native=native, **k):
                o = _native(x_, t_, *a, **k)
                calls.append((tuple(x_.shape), x_.is_contiguous(memory_format=torch.channels_last),
                              o.permute(0, 2, 3, 1).is_contiguous()))
                return o
            b.__dict__["forward"] = spy
        with torch.no_grad():
            got = tree(xd, td)
        assert seen == []                                      # the modules' own forwards did not run
        # the first block got the caller's contiguous tensor; what the consumer permutes and reshapes is NHWC in memory
        assert [c_[0] for c_ in calls] == [(n, c, H, W), (n, 2 * c, H, W)] and calls[0][1] is False
        assert all(c_[2] for c_ in calls)
        bar = 4 * noise * peak
        ratio, tratio = float((got.double().cpu() - rec).abs().max() / bar), float((own.double().cpu() - rec).abs().max() / bar)
        print("patched tree |got - float64| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16 tree: %.3f)"
              % (noise, peak, ratio, tratio))
        assert got.shape == (n, H * W, 64) and ratio <= 1.0
    finally:
        assert unpatch_unet_resnets(tree) == 2
    assert not any("forward" in vars(m) for m in tree.modules())
    with torch.no_grad():
        back = tree(xd, td)
    assert seen == ["module", "module"] and float((back.double() - own.double()).abs().max()) <= 4 * noise * peak
