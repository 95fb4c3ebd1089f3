"""What is left of the UNet and the ControlNet on the GPU: the kernels of csrc/unet_shell.hip against float64 on the same
operands, each drop-in of fresco_amd.unet_shell against the float64 record of its restated module
(tests/golden/unet_shell_golden.npz; stand-in weights, tests/unet_shell_model.py), and patch_unet_shell on the two stand-in
skeletons, with the kernels torch.profiler records under all four patches.

Bars (e = 2^-24, one fp32 rounding):
  * unet_conv3 without activation: test_gpu_vae.py's convolution bar, 9 cin e mass + 2^-11 |ref| + 1e-6, mass = sum |x| |w|;
  * unet_conv3 with SiLU: 1.1 (9 cin e mass + 4 e |z|) + 2^-11 |ref| + 1e-6, z the pre-activation: 1.1 >= max |SiLU'|, 4 e |z|
    the roundings of the bias add, the exponential, the sum and the quotient;
  * unet_input: exact;
  * the sinusoid: 2^-11 |ref| + 8 e max(1, t) + 1e-6: the fp16 rounding, and the fp32 roundings of the exponent, the exp and
    the product under a slope of at most 1;
  * unet_time_linear: (K + 8) e mass + 2^-11 |ref| + 1e-6 against float64 from the kernel's own fp16 sinusoid, resp. rows;
  * a drop-in: |got - record| <= 4 x the recorded noise of the reference arithmetic x the record's largest magnitude
    (DESIGN.md sections 16 and 17's margin).
Every comparison prints its ratio to the bar, a drop-in's beside the ratio of PyTorch's own fp16 kernels on the restated
module; a second run gives the same bits.  The skeletons hold resnets and the shell modules, no transformer block.  That
unpatching restores bit-equal outputs is checked with PyTorch's convolutions held to their deterministic kernels: with its
default ones two runs of the same unpatched skeleton differed in the last bit on an MI355X.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_shell_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = 2.0 ** -24
H11 = 2.0 ** -11
GUARD = 16384      # elements of 100.0 before and after x and out: more than (W + 1) cin, what a stray tap could reach


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _check(name, got, ref, bound):
    got, ref, bound = (t.detach().to("cpu", torch.float64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
                       for t in (got, ref, bound))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    print("%s: worst error / bound %.3f" % (name, float((err / bound).max())))
    assert np.isfinite(got).all() and np.all(err <= bound), name


def _guarded(numel, dtype=torch.float16):
    """(buffer, view): `numel` elements in the middle of a buffer that holds 100.0 before and after them"""
    buf = torch.full((GUARD + numel + GUARD,), 100.0, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def _guards_untouched(buf, numel):
    return bool((buf[:GUARD] == 100.0).all()) and bool((buf[GUARD + numel:] == 100.0).all())


# ---------------------------------------------------------------------------------------------------------------
# unet_conv3
# ---------------------------------------------------------------------------------------------------------------
def _conv3(shape, stride, silu, edges=False):
    from fresco_amd import _lib, ops
    from fresco_amd.vae import pack_conv_weight
    n, H, W, cin, cout = shape
    seed = sum(shape) + stride
    x = _randn(n, H, W, cin, seed=seed) * 1.5
    x[-1] = x[-1] * 0.5 + 1.0          # the last image is scaled and shifted: a border that bleeds would show
    xbuf, xv = _guarded(x.numel())
    xv.copy_(x.half().reshape(-1))
    xd = xv.view(n, H, W, cin)
    assert xd.data_ptr() % 16 == 0
    w = (_randn(cout, cin, 3, 3, seed=seed + 1) * (2.0 / (9 * cin)) ** 0.5).half().to(DEV)
    bias = _randn(cout, seed=seed + 2).to(DEV)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    obuf, ov = _guarded(n * Ho * Wo * cout)
    wp = pack_conv_weight(w)
    act = _lib.UNET_ACT_SILU if silu else _lib.UNET_ACT_NONE

    def run():
        ov.fill_(-7.0)
        rc = _lib.load().unet_conv3(xd.data_ptr(), wp.data_ptr(), bias.data_ptr(), ov.data_ptr(), n, H, W, cin, cout, stride, act,
                                    torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "unet_conv3 %s" % (shape,))
        return ov.view(n, Ho, Wo, cout).clone()
    got = run()
    # float64 on the same operands: F.unfold of the plane zero-padded by 1 -> (n, cin 9, Ho Wo), k = (ci, ky, kx)
    cols = F.unfold(F.pad(xd.double().permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, stride=stride)
    assert cols.shape == (n, cin * 9, Ho * Wo)
    wm = w.double().reshape(cout, cin * 9)
    z = (wm @ cols + bias.double()[None, :, None]).transpose(1, 2).reshape(n, Ho, Wo, cout)
    mass = (wm.abs() @ cols.abs()).transpose(1, 2).reshape(n, Ho, Wo, cout)
    if silu:
        ref = z * torch.sigmoid(z)
        bound = 1.1 * (9 * cin * E * mass + 4 * E * z.abs()) + H11 * ref.abs() + 1e-6
    else:
        ref = z
        bound = 9 * cin * E * mass + H11 * ref.abs() + 1e-6
    name = "conv3 %s stride %d%s" % (shape, stride, " + SiLU" if silu else "")
    _check(name, got, ref, bound)
    assert _guards_untouched(xbuf, x.numel()) and _guards_untouched(obuf, ov.numel()), name
    assert torch.equal(xv.cpu(), x.half().reshape(-1))
    assert torch.equal(run(), got)                       # the same bits again
    # the tensor-level wrapper is the same call
    assert torch.equal(ops.unet_conv3(xd, wp, bias, stride=stride, silu=silu), got)
    if edges:
        for label, sl in (("first row", (slice(None), slice(0, 1))), ("last row", (slice(None), slice(Ho - 1, Ho))),
                          ("first column", (slice(None), slice(None), slice(0, 1))),
                          ("last column", (slice(None), slice(None), slice(Wo - 1, Wo)))):
            _check("%s, %s" % (name, label), got[sl], ref[sl], bound[sl])


SHAPES = [(1, 6, 10, 32, 6),       # one tile, the scalar-store epilogue, a cout below one MFMA block
          (2, 5, 7, 64, 40),       # odd sides: the bottom and right pad are reached at stride 2
          (3, 1, 1, 32, 32),       # every tap but the centre is outside the plane
          (1, 2, 2, 128, 128),
          (1, 18, 34, 256, 256)]   # ragged tiles in both directions, eight chunks, two column tiles


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3_matches_float64(shape, stride):
    _conv3(shape, stride, False, edges=shape == (2, 5, 7, 64, 40))


def test_conv3_the_downsampler_form():
    _conv3((2, 16, 16, 320, 320), 2, False)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3_with_silu(stride):
    _conv3((1, 9, 17, 32, 32), stride, True)


# ---------------------------------------------------------------------------------------------------------------
# unet_input
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cpad", [8, 32])
@pytest.mark.parametrize("c", [3, 4])
def test_input_is_exact(c, cpad):
    from fresco_amd import ops
    x = (_randn(2, c, 3, 5, seed=c + cpad) * 2.0).half().to(DEV)
    out = ops.unet_input(x, cpad)
    assert out.shape == (2, 3, 5, cpad) and out.dtype == torch.float16
    assert torch.equal(out[..., :c], x.permute(0, 2, 3, 1)) and not out[..., c:].any()
    assert torch.equal(ops.unet_input(x, cpad), out)


# ---------------------------------------------------------------------------------------------------------------
# unet_time_linear
# ---------------------------------------------------------------------------------------------------------------
def _sinusoid64(ts, K):
    half = K // 2
    w = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    arg = ts.double().cpu()[:, None] * w[None, :]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=1)


def test_sinusoid_matches_float64():
    from fresco_amd import ops
    K = 320
    ts = torch.tensor([0.0, 1.0, 251.0, 999.0], dtype=torch.float32, device=DEV)
    w = (_randn(16, K, seed=1) * K ** -0.5).half().to(DEV)
    _, sin = ops.unet_time_linear(ts, w, torch.zeros(16, device=DEV), want_sin=True)
    assert sin.shape == (4, K) and sin.dtype == torch.float16
    ref = _sinusoid64(ts, K)
    tmax = torch.clamp(ts.double().cpu(), min=1.0)[:, None]
    _check("sinusoid K=320 t in (0, 1, 251, 999)", sin, ref, H11 * ref.abs() + 8 * E * tmax + 1e-6)
    assert torch.equal(sin[0, :160].cpu(), torch.ones(160, dtype=torch.float16)) and not sin[0, 160:].any()   # t = 0: cos 1, sin 0


def _time_linear(n, K, cout):
    from fresco_amd import ops
    w = (_randn(cout, K, seed=cout + K) * (2.0 / K) ** 0.5).half().to(DEV)
    bias = _randn(cout, seed=cout + 1).to(DEV)
    # the timesteps: the sinusoid the kernel itself wrote is the operand of the float64 product
    ts = torch.linspace(0.0, 999.0, n, dtype=torch.float32).round().to(DEV)
    out, sin = ops.unet_time_linear(ts, w, bias, want_sin=True)
    assert out.shape == (n, cout) and out.dtype == torch.float16
    ref = sin.double() @ w.double().t() + bias.double()
    mass = sin.double().abs() @ w.double().abs().t()
    _check("time_linear timesteps n=%d K=%d cout=%d" % (n, K, cout), out, ref, (K + 8) * E * mass + H11 * ref.abs() + 1e-6)
    assert torch.equal(ops.unet_time_linear(ts, w, bias), out)          # without the tap, and again: the same bits
    # SiLU rows
    rows = (_randn(n, K, seed=n + K) * 1.5).half().to(DEV)
    rows[-1] = rows[-1] * 0.5 + 1.0
    out = ops.unet_time_linear(rows, w, bias)
    s = rows.double() * torch.sigmoid(rows.double())
    ref = s @ w.double().t() + bias.double()
    mass = s.abs() @ w.double().abs().t()
    _check("time_linear SiLU rows n=%d K=%d cout=%d" % (n, K, cout), out, ref, (K + 8) * E * mass + H11 * ref.abs() + 1e-6)
    assert torch.equal(ops.unet_time_linear(rows, w, bias), out)


@pytest.mark.parametrize("K", [320, 1280])
@pytest.mark.parametrize("n", [1, 16, 17, 64])
def test_time_linear_matches_float64(n, K):
    _time_linear(n, K, 1280)


def test_time_linear_ragged_sizes():
    """a K that ends inside a chunk of 512, a last workgroup with two of its four channels"""
    _time_linear(3, 136, 322)


# ---------------------------------------------------------------------------------------------------------------
# the drop-ins against their records
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


def _native_and_own(case, mod, x):
    """(the drop-in's output, PyTorch's own fp16 module's output, a second run of the drop-in), logical NCHW / (n, C)"""
    from fresco_amd import (ControlNetCondEmbedding, UNetConvIn, UNetConvOut, UNetDownsample, UNetTimeEmbedding, UNetUpsample,
                            UNetZeroConv)
    kind = case[0]
    with torch.no_grad():
        own = mod(x, dtype=torch.float16) if kind == "time" else mod(x)
    if kind == "time":
        native = UNetTimeEmbedding.from_module(mod)
        run = lambda: native(native.proj(x).to(torch.float16))  # noqa: E731  (the model casts what time_proj returns)
    elif kind == "conv_out":
        native = UNetConvOut.from_module(mod)
        run = lambda: native(x)  # noqa: E731
    else:
        cls, m = {"down": (UNetDownsample, mod), "up": (UNetUpsample, mod), "conv_in": (UNetConvIn, mod.conv if kind == "conv_in" else None),
                  "cond": (ControlNetCondEmbedding, mod), "zero": (UNetZeroConv, mod.conv if kind == "zero" else None)}[kind]
        native = cls.from_module(m)
        if kind == "cond":
            native.cache = False
        run = lambda: native(x)  # noqa: E731
    return run(), own, run()


@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_dropin_matches_the_record(case, gold):
    kind, c, n, H, W = case
    key = M.case_key(case)
    mod = M.build(case, torch.float16).to(DEV)     # the restated module in fp16 on the GPU, with the stand-in weights
    x = M.inputs(case).to(DEV)
    if kind not in ("time", "conv_in", "cond"):
        x = x.contiguous(memory_format=torch.channels_last)
    got, own, again = _native_and_own(case, mod, x)
    assert got.dtype == torch.float16 and got.shape == own.shape, (got.shape, own.shape)
    if kind == "conv_out":
        assert got.is_contiguous()                                             # the model's output: plain NCHW
    elif kind != "time":
        assert got.permute(0, 2, 3, 1).is_contiguous()                         # NHWC in memory
    rec, noise, peak = gold[key + "_out"], float(gold[key + "_noise"][0]), float(gold[key + "_peak"][0])
    a, b = M.thin(M.as_record(case, got).double()), M.thin(M.as_record(case, own).double())
    assert a.shape == rec.shape, (a.shape, rec.shape)
    bar = 4 * noise * peak
    ratio, tratio = float(np.abs(a - rec).max() / bar), float(np.abs(b - rec).max() / bar)
    print("%s |got - record| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16 module: %.3f)"
          % (key, noise, peak, ratio, tratio))
    assert np.isfinite(a).all() and ratio <= 1.0, (key, ratio)
    assert torch.equal(again, got)
    if kind in ("down", "up", "zero"):     # the same bits from a contiguous input (converted once)
        assert torch.equal(_native_and_own(case, mod, x.contiguous())[0], got)


def test_upsample_takes_the_exact_output_size_only():
    from fresco_amd import UNetUpsample
    case = ("up", 640, 1, 10, 14)
    mod = M.build(case, torch.float16).to(DEV)
    x = M.inputs(case).to(DEV)
    native = UNetUpsample.from_module(mod, name="up_blocks.1.upsamplers.0")
    assert torch.equal(native(x, output_size=(20, 28)), native(x))
    with pytest.raises(NotImplementedError, match="up_blocks.1.upsamplers.0"):
        native(x, output_size=(21, 28))


def test_condition_cache_on_the_gpu():
    from fresco_amd import ControlNetCondEmbedding
    case = ("cond", 320, 2, 32, 48)
    mod = M.build(case, torch.float16).to(DEV)
    cond = M.inputs(case).to(DEV)
    emb = ControlNetCondEmbedding.from_module(mod)
    one = emb(cond)
    assert emb(cond) is one
    fresh = emb(cond.clone())
    assert fresh is not one and torch.equal(fresh, one)
    cond.mul_(0.5)
    assert not torch.equal(emb(cond), one)


# ---------------------------------------------------------------------------------------------------------------
# patching
# ---------------------------------------------------------------------------------------------------------------
# what torch.profiler may record under the four patches beside this library's kernels (namespace fresco): elementwise adds,
# multiplies and copies (dtype casts and layout changes are copies; torch.cat is a batched copy)
ALLOWED = ("elementwise_kernel", "CatArrayBatchedCopy", "Memcpy", "Memset")
NOT_OURS = ("gemm", "Cijk", "conv", "Conv", "miopen", "MIOpen", "group_norm", "GroupNorm", "RowwiseMoments", "upsample",
            "silu", "batch_norm", "igemm", "winograd", "gemv")


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
    return sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})


def _patch_all(net):
    from fresco_amd import patch_unet_attention, patch_unet_resnets, patch_unet_shell, patch_unet_transformers
    return patch_unet_resnets(net), patch_unet_transformers(net), patch_unet_attention(net), patch_unet_shell(net)


def _unpatch_all(net):
    from fresco_amd import unpatch_unet_attention, unpatch_unet_resnets, unpatch_unet_shell, unpatch_unet_transformers
    unpatch_unet_attention(net)
    unpatch_unet_transformers(net)
    unpatch_unet_resnets(net)
    return unpatch_unet_shell(net)


def _deterministic(fn):
    """fn() with PyTorch's convolution library held to its deterministic kernels (its default choice may add partial sums
    with atomics, and then two runs of the SAME unpatched module differ in the last bit), after one call that lets it settle
    on them"""
    keep = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        fn()
        return fn()
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = keep


def _flat(out):
    """the UNet skeleton's tensor, or the ControlNet skeleton's (list, tensor), as one vector"""
    if isinstance(out, torch.Tensor):
        return out.reshape(-1)
    return torch.cat([t.reshape(-1) for t in out[0]] + [out[1].reshape(-1)])


@pytest.mark.parametrize("kind", ["unet", "controlnet"])
def test_patched_skeleton_runs_natively(kind):
    x, ts, cond = M.skeleton_inputs(2, 8, 8)
    args64 = (x.double(), ts.double()) + ((cond.double(), 0.75) if kind == "controlnet" else ())
    args32 = (x.float(), ts) + ((cond.float(), 0.75) if kind == "controlnet" else ())
    with torch.no_grad():
        rec = _flat(M.build_skeleton(kind, torch.float64)(*args64))                        # the skeleton in float64 ...
        r16 = _flat(M.build_skeleton(kind, torch.float32)(*args32, q=M.round16)).double()   # ... and the arithmetic's noise
    peak = float(rec.abs().max())
    noise = float((r16 - rec).abs().max() / peak)
    assert noise > 0
    net = M.build_skeleton(kind, torch.float16).to(DEV)
    args = (x.to(DEV), ts.to(DEV)) + ((cond.to(DEV), 0.75) if kind == "controlnet" else ())
    before = _kernel_names(lambda: net(*args))
    with torch.no_grad():
        own = _flat(net(*args))                                                          # PyTorch's fp16 kernels
        own_det, own_det2 = _deterministic(lambda: _flat(net(*args))), _deterministic(lambda: _flat(net(*args)))
    print("PyTorch's own two runs of the unpatched %s skeleton differ by at most %.3g" % (kind, float((own_det - own_det2).abs().max())))
    assert torch.equal(own_det, own_det2)     # what the last assertion of this test stands on
    print("unpatched %s skeleton: %s" % (kind, before))
    foreign = [k for k in before if "fresco" not in k and any(s in k for s in NOT_OURS)]
    assert foreign, before       # the profiler sees PyTorch's convolutions and GEMMs: the check below is not vacuous
    counts = _patch_all(net)
    try:
        assert counts[0] == (6 if kind == "unet" else 9) and counts[1] == 0 and counts[2] == 0
        assert counts[3] == ({"down": 3, "up": 3, "conv_in": 1, "conv_out": 1, "time": 1, "cond_embedding": 0, "zero_conv": 0}
                             if kind == "unet" else
                             {"down": 3, "up": 0, "conv_in": 1, "conv_out": 0, "time": 1, "cond_embedding": 1, "zero_conv": 13})
        with torch.no_grad():
            got = _flat(net(*args))
        names = _kernel_names(lambda: net(*args))
        print("patched %s skeleton: %s" % (kind, names))
        assert any("fresco" in k and "unet_conv3_kernel" in k for k in names), names
        for k in names:
            if "fresco" in k:
                continue
            assert any(a in k for a in ALLOWED) and not any(s in k for s in NOT_OURS), k
        bar = 4 * noise * peak
        ratio = float((got.double().cpu() - rec).abs().max() / bar)
        tratio = float((own.double().cpu() - rec).abs().max() / bar)
        print("patched %s skeleton |got - float64| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16: %.3f)"
              % (kind, noise, peak, ratio, tratio))
        assert ratio <= 1.0
        assert float((got.double() - own.double()).abs().max()) <= 2 * bar     # each within its bar of the float64 run
        with torch.no_grad():
            assert torch.equal(_flat(net(*args)), got)
    finally:
        assert _unpatch_all(net) == (12 if kind == "unet" else 20)
    assert not any("forward" in vars(m) for m in net.modules())
    for m in net.modules():
        assert m.forward.__func__ is type(m).forward
    with torch.no_grad():
        assert torch.equal(_deterministic(lambda: _flat(net(*args))), own_det)   # the modules' own forwards again, bit for bit
