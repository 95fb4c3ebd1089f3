"""The bf16 forms of vae_conv, unet_groupnorm and unet_temb (csrc/net_bf16.hip) and the bf16 UNetResnet on the GPU.

  1. vae_conv on INTEGER operands (x in -4 .. 4, w in -2 .. 2, integer bias, bias rows and residual): every product and every
     partial sum (|sum| <= 9 * 64 * 8 + small) is exact in fp32 whatever the MFMA's order, so the result must EQUAL the float64
     convolution rounded once to the output type.  A fragment map, swizzle or channel map that is wrong for bf16 cannot pass.
  2. vae_conv on random operands: tests/test_gpu_vae.py's bar with its half-ulp term 2^-11 |ref| replaced by bf16's 2^-8 |ref|
     (8 significant bits): K e sum|x||w| + 2^-8 |ref| + 1e-6, e = 2^-24; a second run gives the same bits.
  3. range: a 3 x 3 convolution and a GroupNorm whose outputs pass fp16's 65504 (about 2e5) are finite and within the same bars.
  4. unet_groupnorm: tests/test_gpu_unet_resnet.py's bar with 2^-8 |y| as the rounding term,
     16 e ((|x| + |mean|) rstd |gamma| + |beta|) + 1e-6 + 2^-8 |y|; both forms; same bits twice; the input untouched.
  5. unet_temb: (K + 8) e sum |SiLU(t)| |w| + 1e-6 (the output is fp32: no rounding term).
  6. the block against tests/golden/unet_resnet_bf16_golden.npz: |got - record| <= 4 x recorded bf16 noise x peak for the
     conv1 + temb tap and the output, printed beside PyTorch's bf16 module (nothing is asserted on PyTorch's).
  7. patch_unet_resnets(tree, dtype=torch.bfloat16) on the stand-in tree.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_resnet_bf16_model as B
import unet_resnet_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = 2.0 ** -24
H8 = 2.0 ** -8          # half an ulp of bf16's 8 significant bits, relative
BF = torch.bfloat16
SLAB_BYTES = {64: 16, 320: 80, 960: 240, 2560: 160}  # the LDS form's bytes per pixel (unet.hip)
LDS_PLANE = 96 * 1024


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=_gen(seed))


def _ints(lo, hi, *shape, seed=0):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).double()


def _check(name, got, ref, bound):
    got, ref, bound = (t.detach().to("cpu", torch.float64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
                       for t in (got, ref, bound))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    print("%s: worst error / bound %.3f" % (name, float((err / bound).max())))
    assert np.isfinite(got).all() and np.all(err <= bound), name


def _conv64(x, w, up2=False):
    """x (n, Hs, Ws, cin), w (cout, cin, k, k) or (n, cout, cin, k, k), float64 on the CPU -> (conv (n, H, W, cout), sum |x||w|)"""
    xc = x.permute(0, 3, 1, 2)
    if up2:
        xc = F.interpolate(xc, scale_factor=2, mode="nearest")
    pad = w.shape[-1] // 2
    if w.dim() == 5:
        pairs = [(xc[i:i + 1], w[i]) for i in range(w.shape[0])]
    else:
        pairs = [(xc, w)]
    ref = torch.cat([F.conv2d(a, b, padding=pad) for a, b in pairs]).permute(0, 2, 3, 1)
    mass = torch.cat([F.conv2d(a.abs(), b.abs(), padding=pad) for a, b in pairs]).permute(0, 2, 3, 1)
    return ref.contiguous(), mass.contiguous()


# ---------------------------------------------------------------------------------------------------------------
# 1. vae_conv, exact
# ---------------------------------------------------------------------------------------------------------------
# name: (Hs, Ws, cout, ksize, options); n = 2 and cin = 64 (two K chunks) throughout; 10 x 14 is ragged against the 8 x 16 tile
# and has two tile rows
EXACT_FORMS = {
    "k3_cout130_one_element_stores": (10, 14, 130, 3, {}),         # a second column tile with two live channels
    "k3_cout192_vector_stores": (10, 14, 192, 3, {"bias": True}),  # 8-byte stores, a dead 32-channel block
    "k3_up2_from_5x7": (5, 7, 192, 3, {"up2": True, "bias": True}),
    "k1_rows140": (140, 1, 130, 1, {"bias": True}),                # two row tiles, the second ragged
    "k1_bias_rows": (140, 1, 192, 1, {"bias_rows": True}),
    "k1_per_image_weights": (10, 14, 192, 1, {"w_per_image": True}),
    "k3_residual_vector": (10, 14, 192, 3, {"bias": True, "residual": True}),
    "k3_residual_one_element": (10, 14, 130, 3, {"bias": True, "residual": True}),
    "k1_ldo_above_cout": (10, 14, 192, 1, {"bias": True, "ldo": 200, "residual": True}),
    "k3_out_f32": (10, 14, 130, 3, {"bias": True, "kind": "f32"}),
    "k3_out_nchw": (10, 14, 130, 3, {"bias": True, "kind": "nchw"}),
}


@pytest.mark.parametrize("form", sorted(EXACT_FORMS))
def test_conv_is_exact_on_integer_operands(form):
    from fresco_amd import _lib, ops
    from fresco_amd.vae import pack_conv_weight
    Hs, Ws, cout, k, opt = EXACT_FORMS[form]
    n, cin = 2, 64
    up2 = opt.get("up2", False)
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    seed = sum(map(ord, form))
    x = _ints(-4, 4, n, Hs, Ws, cin, seed=seed)
    w = _ints(-2, 2, *((n,) if opt.get("w_per_image") else ()), cout, cin, k, k, seed=seed + 1)
    ref, _ = _conv64(x, w, up2)
    bias = None
    if opt.get("bias"):
        bias = _ints(-8, 8, cout, seed=seed + 2)
        ref = ref + bias
    if opt.get("bias_rows"):
        bias = _ints(-8, 8, H * W, seed=seed + 2)
        ref = ref + bias.view(1, H, W, 1)
    ldo = opt.get("ldo", cout)
    res = None
    if opt.get("residual"):
        res = _ints(-16, 16, n, H, W, ldo, seed=seed + 3)
        ref = ref + res[..., :cout]
    assert float(ref.abs().max()) <= 9 * 64 * 8 + 24
    kind = {"f32": _lib.VAE_OUT_F32, "nchw": _lib.VAE_OUT_F16_NCHW}.get(opt.get("kind"), _lib.VAE_OUT_F16)
    wp = (torch.stack([pack_conv_weight(wi, dtype=BF) for wi in w]) if w.dim() == 5 else pack_conv_weight(w, dtype=BF)).to(DEV)
    assert wp.dtype == BF
    out = None
    if ldo != cout:
        out = torch.full((n, H * W, ldo), -7.0, dtype=BF, device=DEV)
    got = ops.vae_conv(x.to(BF).to(DEV), wp, None if bias is None else bias.float().to(DEV), n, H, W, cin, cout, k, up2=up2,
                       residual=None if res is None else res.to(BF).to(DEV), out_kind=kind,
                       w_img_stride=cout * k * k * cin if opt.get("w_per_image") else 0, bias_rows=bool(opt.get("bias_rows")),
                       ldo=ldo, out=out)
    if opt.get("kind") == "f32":
        assert got.dtype == torch.float32 and got.shape == (n, H, W, cout)
        assert torch.equal(got.cpu(), ref.float())                    # (every value is an integer below 2^24)
    elif opt.get("kind") == "nchw":
        assert got.dtype == BF and got.shape == (n, cout, H, W)
        assert torch.equal(got.cpu(), ref.permute(0, 3, 1, 2).to(BF))
    elif ldo != cout:
        assert got is out and torch.equal(got[..., :cout].cpu(), ref.view(n, H * W, cout).to(BF))
        assert bool((got[..., cout:] == -7.0).all())                  # nothing is stored beyond cout
    else:
        assert got.dtype == BF and got.shape == (n, H, W, cout)
        assert torch.equal(got.cpu(), ref.to(BF))


# ---------------------------------------------------------------------------------------------------------------
# 2. and 3. vae_conv on random operands, and beyond fp16's range
# ---------------------------------------------------------------------------------------------------------------
RANDOM_FORMS = {
    # name: (n, Hs, Ws, cin, cout, ksize, up2, scale of x)
    "k3_cout130": (2, 10, 14, 64, 130, 3, False, 1.5),
    "k3_up2": (2, 5, 7, 64, 192, 3, True, 1.5),
    "K2880": (1, 9, 5, 320, 64, 3, False, 1.5),
    "range_2e5": (2, 10, 14, 64, 192, 3, False, 5e4),
}


@pytest.mark.parametrize("form", sorted(RANDOM_FORMS))
def test_conv_matches_float64_on_random_operands(form):
    from fresco_amd import ops
    from fresco_amd.vae import pack_conv_weight
    n, Hs, Ws, cin, cout, k, up2, scale = RANDOM_FORMS[form]
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    seed = sum(map(ord, form))
    x = (_randn(n, Hs, Ws, cin, seed=seed) * scale).to(BF)
    x[-1] = x[-1] * 0.5 + scale / 1.5  # the last image differs in scale and offset: a border that bleeds would show
    w = (_randn(cout, cin, k, k, seed=seed + 1) * (2.0 / (cin * k * k)) ** 0.5).to(BF)
    bias = _randn(cout, seed=seed + 2) * scale
    res = (_randn(n, H, W, cout, seed=seed + 3) * 2.0 * scale).to(BF)
    ref, mass = _conv64(x.double(), w.double(), up2)
    ref = ref + bias.double() + res.double()
    K = cin * k * k
    args = (x.to(DEV), pack_conv_weight(w, dtype=BF).to(DEV), bias.to(DEV), n, H, W, cin, cout, k)
    got = ops.vae_conv(*args, up2=up2, residual=res.to(DEV))
    assert got.dtype == BF and got.shape == (n, H, W, cout)
    if form == "range_2e5":
        print("conv %s: largest |output| %.3g" % (form, float(ref.abs().max())))
        assert float(ref.abs().max()) > 2e5 > 65504.0    # what fp16 cannot hold
    _check("conv %s bf16" % form, got, ref, K * E * mass + H8 * ref.abs() + 1e-6)
    assert torch.equal(got, ops.vae_conv(*args, up2=up2, residual=res.to(DEV)))


# ---------------------------------------------------------------------------------------------------------------
# 4. unet_groupnorm (and 3.'s GroupNorm case)
# ---------------------------------------------------------------------------------------------------------------
def _groupnorm_against_float64(C, P, x, gamma, beta, addend, eps=1e-5):
    from fresco_amd import _lib, ops
    n, cpg = x.shape[0], C // 32
    form = _lib.load().unet_groupnorm_lds_form(n, P, C)
    xd, keep = x.to(DEV), x.clone()
    gamma, beta, addend = gamma.to(DEV), beta.to(DEV), addend.to(DEV)
    for use_addend in (False, True):
        xa = x.double() + (addend.double().cpu()[:, None, :] if use_addend else 0.0)
        g = xa.view(n, P, 32, cpg)
        mean = g.mean((1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(g.var((1, 3), unbiased=False, keepdim=True) + eps)
        norm = ((g - mean) * rstd).view(n, P, C) * gamma.double().cpu() + beta.double().cpu()
        mass = ((g.abs() + mean.abs()) * rstd).view(n, P, C) * gamma.double().cpu().abs() + beta.double().cpu().abs()
        for silu in (False, True):
            ref = norm * torch.sigmoid(norm) if silu else norm
            y = ops.unet_groupnorm(xd, gamma, beta, eps, silu=silu, addend=addend if use_addend else None)
            assert y.dtype == BF and y.shape == x.shape
            _check("groupnorm bf16 C=%d P=%d form=%s%s%s" % (C, P, "lds" if form else "3-launch", " + addend" if use_addend else "",
                                                            " + SiLU" if silu else ""), y, ref, 16 * E * mass + 1e-6 + H8 * ref.abs())
            assert torch.equal(y, ops.unet_groupnorm(xd, gamma, beta, eps, silu=silu, addend=addend if use_addend else None))
    assert torch.equal(xd.cpu(), keep)     # the input is untouched
    return form


@pytest.mark.parametrize("pi", range(4), ids=["P1", "P257", "Pmax_lds", "Pmax_lds_plus_1"])
@pytest.mark.parametrize("C", sorted(SLAB_BYTES), ids=lambda c: "C%d_cpg%d" % (c, c // 32))
def test_groupnorm_matches_float64(C, pi):
    pmax = LDS_PLANE // SLAB_BYTES[C]   # the largest plane of the LDS form, and the first of the three-launch form
    n, P = 2, [1, 257, pmax, pmax + 1][pi]
    x = _randn(n, P, C, seed=C + P) * 3.0 + 1.5
    x[1] = x[1] * 0.25 - 4.0        # image 1 is shifted and scaled: its statistics differ
    addend = _randn(n, C, seed=C + 3) * 2.0
    addend[1] += 3.0
    form = _groupnorm_against_float64(C, P, x.to(BF), _randn(C, seed=C + 1) * 0.5 + 1.0, _randn(C, seed=C + 2), addend)
    assert form == (0 if pi == 3 else 1), (C, P, form)


@pytest.mark.parametrize("P", [64, 1300], ids=["lds", "three_launch"])
def test_groupnorm_beyond_the_range_of_fp16(P):
    C, n = 320, 2
    x = (_randn(n, P, C, seed=P) * 3e4 + 1e5).to(BF)           # inputs and, through gamma, outputs of about 2e5
    gamma, beta = (_randn(C, seed=1) * 0.25 + 1.0) * 5e4, _randn(C, seed=2) * 1e4
    form = _groupnorm_against_float64(C, P, x, gamma, beta, _randn(n, C, seed=3) * 2e4)
    assert form == (1 if P == 64 else 0)
    from fresco_amd import ops
    y = ops.unet_groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV))
    print("groupnorm range: largest |output| %.3g" % float(y.float().abs().max()))
    assert bool(torch.isfinite(y).all()) and float(y.float().abs().max()) > 1.5e5


# ---------------------------------------------------------------------------------------------------------------
# 5. unet_temb
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,cout", [(1280, 320), (520, 322)])
@pytest.mark.parametrize("n", [1, 16, 33])
def test_temb_matches_float64(n, K, cout):
    from fresco_amd import ops
    temb = (_randn(n, K, seed=n + K) * 1.5).to(BF)
    temb[-1] = temb[-1] * 0.5 + 1.0
    w = (_randn(cout, K, seed=cout) * (2.0 / K) ** 0.5).to(BF)
    bias, cbias = _randn(cout, seed=cout + 1), _randn(cout, seed=cout + 2)
    args = (temb.to(DEV), w.to(DEV), bias.to(DEV), cbias.to(DEV))
    out = ops.unet_temb(*args)
    assert out.shape == (n, cout) and out.dtype == torch.float32
    s = temb.double() * torch.sigmoid(temb.double())
    ref = s @ w.double().t() + bias.double() + cbias.double()
    mass = s.abs() @ w.double().abs().t()
    _check("temb bf16 n=%d K=%d cout=%d" % (n, K, cout), out, ref, (K + 8) * E * mass + 1e-6)
    assert torch.equal(out, ops.unet_temb(*args))


# ---------------------------------------------------------------------------------------------------------------
# 6. the block
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return B.load_golden(GOLDEN)


@pytest.mark.parametrize("case", B.CASES, ids=B.case_key)
def test_block_matches_the_record(case, gold):
    from fresco_amd import UNetResnet
    cin, cout, n, H, W = case
    key = B.case_key(case)
    mod = B.build(cin, cout, BF).to(DEV)   # the restated module in bf16 on the GPU, with the stand-in weights
    native = UNetResnet.from_module(mod, dtype=BF)
    x, temb = (t.to(DEV) for t in B.inputs(case))
    x_cl = x.contiguous(memory_format=torch.channels_last)
    taps, ttaps = {}, {}
    out = native(x_cl, temb, taps=taps)
    with torch.no_grad():
        tout = mod(x, temb, taps=ttaps)   # PyTorch's own kernels in bf16: printed beside ours for context, nothing asserted on it
    assert out.shape == (n, cout, H, W) and out.dtype == BF
    assert out.is_contiguous(memory_format=torch.channels_last) and out.permute(0, 2, 3, 1).is_contiguous()
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    ours = {"tap": taps["conv1_temb"], "out": out.permute(0, 2, 3, 1)}
    theirs = {"tap": ttaps["tap"], "out": tout.permute(0, 2, 3, 1)}
    worst = []
    for i, t in enumerate(B.TENSORS):
        rec = gold["%s_%s" % (key, t)]
        a, b = B.thin(ours[t].double()), B.thin(theirs[t].double())
        assert a.shape == rec.shape, (t, a.shape, rec.shape)
        bar = 4 * noise[i] * peak[i]
        ratio, tratio = float(np.abs(a - rec).max() / bar), float(np.abs(b - rec).max() / bar)
        print("%s %-3s |got - record| / (4 x bf16 reference noise %.2e x peak %.3g) = %.3f   (PyTorch bf16 module: %.3f)"
              % (key, t, noise[i], peak[i], ratio, tratio))
        worst.append((ratio, t))
    assert max(worst)[0] <= 1.0, max(worst)
    # the same bits from a contiguous input (converted once), from a second call, and in the plain layout
    assert torch.equal(native(x, temb), out)
    assert torch.equal(native(x_cl, temb), out)
    plain = native(x_cl, temb, memory_format=torch.contiguous_format)
    assert plain.is_contiguous() and plain.shape == out.shape and torch.equal(plain, out)
    assert torch.equal(UNetResnet.from_module(mod, memory_format=torch.contiguous_format, dtype=BF)(x, temb), out)


# ---------------------------------------------------------------------------------------------------------------
# 7. the patched tree
# ---------------------------------------------------------------------------------------------------------------
def test_patched_bf16_tree_runs_natively(monkeypatch):
    from fresco_amd import UNetResnet, patch_unet_resnets, unpatch_unet_resnets
    n, c, H, W = 2, 320, 8, 12
    gen = torch.Generator().manual_seed(7)
    x = (torch.randn(n, c, H, W, generator=gen) * 1.5).to(BF)
    x[-1] = x[-1] * 0.5 + 1.0
    temb = torch.randn(n, M.TEMB_CHANNELS, generator=gen).to(BF)
    with torch.no_grad():
        rec = B.build_tree(torch.float64)(x.double(), temb.double())                        # the unpatched tree in float64 ...
        r16 = B.build_tree(torch.float32)(x.float(), temb.float(), B.round_bf16).double()   # ... and the bf16 arithmetic's noise
    peak = float(rec.abs().max())
    noise = float((r16 - rec).abs().max() / peak)
    assert noise > 0
    tree = B.build_tree(BF).to(DEV)
    xd, td = x.to(DEV), temb.to(DEV)
    with torch.no_grad():
        own = tree(xd, td)                                                                   # PyTorch's bf16 kernels, for context
    seen = []
    own_forward = M.Resnet.forward
    monkeypatch.setattr(M.Resnet, "forward", lambda self, *a, **k: seen.append("module") or own_forward(self, *a, **k))
    assert patch_unet_resnets(tree, dtype=BF) == 2
    try:
        calls = []
        for b in (tree.down[0], tree.up["resnets"][0]):
            native = vars(b)["forward"]
            assert isinstance(native, UNetResnet) and native.dtype == BF

            def spy(x_, t_, *a, _native=native, **k):
                o = _native(x_, t_, *a, **k)
                calls.append((tuple(x_.shape), x_.is_contiguous(memory_format=torch.channels_last),
                              o.permute(0, 2, 3, 1).is_contiguous(), o.dtype))
                return o
            b.__dict__["forward"] = spy
        with torch.no_grad():
            got = tree(xd, td)
        assert seen == []                                      # the modules' own forwards did not run
        # the first block got the caller's contiguous tensor; what the consumer permutes and reshapes is NHWC in memory
        assert [c_[0] for c_ in calls] == [(n, c, H, W), (n, 2 * c, H, W)] and calls[0][1] is False
        assert all(c_[2] and c_[3] == BF for c_ in calls)
        bar = 4 * noise * peak
        ratio, tratio = float((got.double().cpu() - rec).abs().max() / bar), float((own.double().cpu() - rec).abs().max() / bar)
        print("patched bf16 tree |got - float64| / (4 x bf16 reference noise %.2e x peak %.3g) = %.3f   (PyTorch bf16 tree: %.3f)"
              % (noise, peak, ratio, tratio))
        assert got.shape == (n, H * W, 64) and got.dtype == BF and ratio <= 1.0
    finally:
        assert unpatch_unet_resnets(tree) == 2
    assert not any("forward" in vars(m) for m in tree.modules())
    with torch.no_grad():
        back = tree(xd, td)
    assert seen == ["module", "module"] and float((back.double() - own.double()).abs().max()) <= 4 * noise * peak
