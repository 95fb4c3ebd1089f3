"""The EGNet saliency detector on the GPU: the four kernels of csrc/egnet.hip against float64 restatements, and the native
detector end to end -- every recorded tap, the logit and the saliency map -- against the records of the unmodified reference
network (tests/golden/egnet_golden.npz, egnet_wide_golden.npz; stand-in weights, tests/egnet_model.py).

Bars:
  * egnet_input: the plane bound of tests/test_gpu_hed.py, 2^-21 |ref| + 2^-25, against a float64 cv2sod;
  * egnet_pool: fp32 equal to F.max_pool2d(ceil_mode=True); the planes to the plane bound;
  * egnet_resize_add: 4e-6 (interp(|x|) + |addend|) + 1e-6 against float64; same-size copies bit-exact;
  * egnet_saliency: 8 x the distance of a CPU fp32 torch restatement from the float64 one, + 1e-6;
  * end to end: |got - float64 record| <= 8 e_ref + 1e-7 (saliency: + 1e-6), e_ref = the reference's own fp32-vs-fp64 distance
    for that tensor from the golden file; 8 x is the project's standing margin for this GEMM (tests/test_gpu_hed.py).
Every comparison prints its ratio to the bar.
"""
import copy
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import egnet_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCALE = 64.0


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np64(t):
    return t.detach().to("cpu", torch.float64).numpy()


def _planes64(planes):
    return _np64(planes[0]) + _np64(planes[1])


def _plane_bound(v_scaled):
    return 2.0 ** -21 * np.abs(v_scaled) + 2.0 ** -25


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 64), (1, 34, 50), (1, 33, 47)], ids=lambda s: "%dx%dx%d" % s)
def test_input_matches_a_float64_cv2sod(shape):
    from fresco_amd import ops
    n, H, W = shape
    x = np.random.RandomState(H * W).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    x[0, 0, 0] = (0, 255, 128)
    got = ops.egnet_input(_gpu(x))
    assert got.shape == (n, H // 2, W // 2, 3) and got.dtype == torch.float32
    ref = _nhwc(M.cv2sod64(x)).numpy()
    err = np.abs(_np64(got) - ref)
    print("input %s: worst error / bound %.3f" % (shape, (err / _plane_bound(ref)).max()))
    assert np.all(err <= _plane_bound(ref))
    assert torch.equal(ops.egnet_input(_gpu(x)), got)


@pytest.mark.parametrize("shape", [(2, 16, 18), (1, 17, 5), (1, 5, 16), (1, 18, 17), (1, 5, 7), (1, 2, 2)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_pool_matches_ceil_mode_max_pool(shape):
    """16 -> 9, 18 -> 10, 17 -> 9, 5 -> 3, 7 -> 4, 2 -> 2 on either axis (odd sizes: the last window hangs off the map);
    negative values everywhere, so a padded tap must never win"""
    from fresco_amd import ops
    n, H, W = shape
    sizes = {16: 9, 18: 10, 17: 9, 5: 3, 7: 4, 2: 2}
    x = torch.randn(n, H, W, 64, generator=torch.Generator().manual_seed(H * 100 + W)) * 60.0 - 30.0
    x[:, ::3] *= 1e-3
    want = _nhwc(F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, ceil_mode=True))
    assert want.shape == (n, sizes[H], sizes[W], 64) == (n, ops.egnet_pool_size(H), ops.egnet_pool_size(W), 64)
    out, planes = ops.egnet_pool(x.to(DEV), want_f32=True, scale=SCALE)
    assert torch.equal(out.cpu(), want)
    assert planes[0].shape == (n * sizes[H] * sizes[W], 64) and planes[0].dtype == torch.float16
    ref = want.double().numpy().reshape(-1, 64) * SCALE
    err = np.abs(_planes64(planes) - ref)
    print("pool %s: worst plane error / bound %.3f" % (shape, (err / _plane_bound(ref)).max()))
    assert np.all(err <= _plane_bound(ref))
    none, again = ops.egnet_pool(x.to(DEV), scale=SCALE)
    assert none is None and torch.equal(again[0], planes[0]) and torch.equal(again[1], planes[1])


RESIZES = [((3, 3), (5, 5)), ((9, 9), (16, 16)), ((4, 5), (7, 9)), ((6, 7), (6, 7))]


@pytest.mark.parametrize("C", [128, 512])
@pytest.mark.parametrize("sizes", RESIZES, ids=lambda s: "%dx%dto%dx%d" % (s[0] + s[1]))
def test_resize_add_matches_float64_interpolation(sizes, C):
    from fresco_amd import ops
    (h, w), (H, W) = sizes
    n = 2
    g = torch.Generator().manual_seed(1000 * h + 10 * W + C)
    x = torch.randn(n, h, w, C, generator=g) * 40.0
    x[:, :, ::2] *= 1e-2
    add = torch.randn(n, H, W, C, generator=g) * 40.0
    up64 = _nhwc(F.interpolate(x.double().permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True))
    mag = _nhwc(F.interpolate(x.double().abs().permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True))
    for with_add in (False, True):
        for relu in (False, True):
            ref = up64 + add.double() if with_add else up64
            ref = (F.relu(ref) if relu else ref).numpy()
            bound = 4e-6 * (mag.numpy() + (add.double().abs().numpy() if with_add else 0.0)) + 1e-6
            out, planes = ops.egnet_resize_add(x.to(DEV), (H, W), addend=add.to(DEV) if with_add else None, relu=relu,
                                               want_f32=True, want_split=True, scale=SCALE)
            assert out.shape == (n, H, W, C) and planes[0].shape == (n * H * W, C)
            err = np.abs(_np64(out) - ref)
            print("resize_add %s C=%d add=%d relu=%d: worst error / bound %.3f" % (sizes, C, with_add, relu, (err / bound).max()))
            assert np.all(err <= bound)
            if (h, w) == (H, W):  # an exact copy (plus one fp32 add)
                want = x + add if with_add else x
                assert torch.equal(out.cpu(), F.relu(want) if relu else want)
            perr = np.abs(_planes64(planes).reshape(ref.shape) - _np64(out) * SCALE)
            assert np.all(perr <= _plane_bound(_np64(out) * SCALE))  # the planes carry the fp32 result
            only, none = ops.egnet_resize_add(x.to(DEV), (H, W), addend=add.to(DEV) if with_add else None, relu=relu)
            assert none is None and torch.equal(only, out)


def _smooth_logits(n, h, w):
    """smooth fields spanning -12 .. +4"""
    y = torch.linspace(0, 1, h, dtype=torch.float64).view(1, h, 1)
    x = torch.linspace(0, 1, w, dtype=torch.float64).view(1, 1, w)
    k = torch.arange(n, dtype=torch.float64).view(n, 1, 1)
    return (-4.0 + 8.0 * torch.cos(4.4 * y + 0.9 * k) * torch.cos(3.1 * x - 0.5 * k)).float()


@pytest.mark.parametrize("k", [7, 13])
@pytest.mark.parametrize("sizes", [((8, 8), (32, 32)), ((18, 22), (36, 44))], ids=lambda s: "%dx%dto%dx%d" % (s[0] + s[1]))
def test_saliency_tail_matches_float64(sizes, k):
    from fresco_amd import ops
    (h, w), (Hs, Ws) = sizes
    lg = _smooth_logits(2, h, w)
    assert lg.min() < -11.0 and lg.max() > 3.0

    def tail(t):
        up = F.interpolate(t[:, None], (Hs, Ws), mode="bilinear", align_corners=True)
        return up, M.saliency_from_logit(up, k)

    up32, s32 = tail(lg)
    up64, s64 = tail(lg.double())
    e32 = float((s32.double() - s64).abs().max())
    bar = 8 * e32 + 1e-6
    sal, up = ops.egnet_saliency(lg.to(DEV), (Hs, Ws), k=k, want_logit=True)
    assert sal.shape == (2, 1, Hs, Ws) and up.shape == (2, Hs, Ws)
    err = float((sal.cpu().double() - s64).abs().max())
    s = s64.numpy()
    print("saliency %s k=%d: max |d| %.3g, bar %.3g (CPU fp32 restatement %.3g), ratio %.3f; %.0f %% zero, %.0f %% above 0.9"
          % (sizes, k, err, bar, e32, err / bar, 100 * (s == 0).mean(), 100 * (s > 0.9).mean()))
    assert (s == 0).mean() > 0.05 and (s > 0.9).mean() > 0.05  # both clamps and the graded part are exercised
    assert err <= bar
    mag = F.interpolate(lg.double().abs()[:, None], (Hs, Ws), mode="bilinear", align_corners=True)[:, 0]
    assert torch.all((up.cpu().double() - up64[:, 0]).abs() <= 4e-6 * mag + 1e-6)
    assert float(sal.min()) >= 0.0 and float(sal.max()) <= 1.0
    again, none = ops.egnet_saliency(lg.to(DEV), (Hs, Ws), k=k)
    assert none is None and torch.equal(again, sal)
    with pytest.raises(ValueError):
        ops.egnet_saliency(lg.to(DEV), (Hs, Ws), k=8)


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def net():
    """the detector with the stand-in weights on the GPU; its weight planes are made on the first call and reused"""
    from fresco_amd import egnet
    net = egnet.build_model("resnet")
    net.load_state_dict(M.standin_state_dict())
    return net.float().to(DEV).eval()


def _check_against_records(gold, case, logit, sal, taps, what):
    key = M.case_key(case)
    worst = 0.0
    items = [("logit", _np64(logit), 1e-7), ("saliency", _np64(sal), 1e-6)]
    if taps is not None:
        assert list(taps) == list(M.TAPS)
        items += [(name, _np64(taps[name][..., ::M.TAP_STRIDE]), 1e-7) for name in M.TAPS]
    failed = []
    for name, got, floor in items:
        f32, f64 = M.golden_pair(gold, "%s_%s" % (key, name))
        assert got.shape == f64.shape, (name, got.shape, f64.shape)
        e_ref = float(np.abs(f32 - f64).max())
        bar = 8 * e_ref + floor
        err = float(np.abs(got - f64).max())
        print("%s %s %-13s max |d| %.3g, e_ref %.3g, error / bar %.3f" % (what, key, name, err, e_ref, err / bar))
        worst = max(worst, err / bar)
        if not err <= bar:
            failed.append((name, err, bar))
    assert not failed, failed
    return worst


@pytest.mark.parametrize("case", M.CASES + M.WIDE_CASES, ids=M.case_key)
def test_native_detector_matches_the_reference_records(gold, net, case):
    fr = M.frames(case)
    assert str(gold[M.case_key(case) + "_sha256"]) == M.digest(fr)
    taps = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no range trip: the native path computed this
        sal, logit = net.detect(_gpu(fr), k=M.K_DILATE, want_logit=True, taps=taps)
    n, H, W = case
    assert sal.shape == (n, 1, H // 2, W // 2) and logit.shape == (n, H // 2, W // 2) and sal.dtype == torch.float32
    worst = _check_against_records(gold, case, logit, sal, taps, "native")
    print("native %s: worst error / bar %.3f" % (M.case_key(case), worst))
    assert torch.equal(net.saliency_logit(_gpu(fr)), logit)  # the same bits on every run


def test_batch_equals_frame_by_frame_bit_for_bit(net):
    fr = _gpu(M.frames((2, 64, 64)))
    sal, logit = net.detect(fr, want_logit=True)
    one = copy.deepcopy(net)
    one.max_frames = 1  # ... and one frame per pass equals eight
    sal1, logit1 = one.detect(fr, want_logit=True)
    assert torch.equal(sal1, sal) and torch.equal(logit1, logit)
    for f in range(2):
        s, l = net.detect(fr[f:f + 1], want_logit=True)
        assert torch.equal(s, sal[f:f + 1]) and torch.equal(l, logit[f:f + 1])


def test_lowered_split_scales_hold_the_same_bar(gold, net):
    """the documented remedy for a network that overflows the planes: other powers of two per stage"""
    case = (1, 72, 88)
    low = copy.deepcopy(net)
    low.split_scales = (64.0, 32.0, 32.0, 16.0, 16.0, 32.0, 16.0, 32.0)
    taps = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sal, logit = low.detect(_gpu(M.frames(case)), want_logit=True, taps=taps)
    _check_against_records(gold, case, logit, sal, taps, "lowered scales")


def test_library_ops_switch_runs_the_same_module(gold, net, monkeypatch):
    """library_ops=True is the A/B baseline: PyTorch's convolutions between this package's input and tail kernels"""
    case = (1, 72, 88)
    lib = copy.deepcopy(net)
    lib.library_ops = True
    calls = []
    from fresco_amd import ops
    real = ops.fn_gemm
    monkeypatch.setattr(ops, "fn_gemm", lambda *a, **k: calls.append(1) or real(*a, **k))
    taps = {}
    sal, logit = lib.detect(_gpu(M.frames(case)), want_logit=True, taps=taps)
    assert not calls
    _check_against_records(gold, case, logit, sal, taps, "library ops")
    monkeypatch.setenv("FRESCO_EGNET_LIBRARY_OPS", "1")
    net.detect(_gpu(M.frames(case)))
    assert not calls
    monkeypatch.delenv("FRESCO_EGNET_LIBRARY_OPS")
    net.detect(_gpu(M.frames(case)))
    assert len(calls) == 92  # the live graph's 93 convolutions: 92 on fn_gemm, the stem on fn_conv7_rgb


def test_a_range_trip_falls_back_to_library_ops_with_one_warning(gold, net):
    """planes written with 2^14 saturate at |x| = 4: the stem trips the range word, the call is recomputed with library ops"""
    case = (1, 72, 88)
    hot = copy.deepcopy(net)
    hot.split_scales = (16384.0,) + hot.split_scales[1:]
    fr = _gpu(M.frames(case))
    with pytest.warns(RuntimeWarning, match="library ops"):
        sal, logit = hot.detect(fr, want_logit=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # once per module (the library's own notices are not meant)
        sal2, _ = hot.detect(fr)
    _check_against_records(gold, case, logit, sal, None, "fallback")
    # (the library's convolutions do not repeat bit for bit, tests/test_gpu_hed.py: logits move by ~1e-6, a box of 49 sigmoids
    # of slope <= 1/4 by at most 49 / 4 times that)
    assert float((sal2 - sal).abs().max()) <= 1e-4


def test_get_saliency_feeds_warp_tensor(net):
    """the drop-in: a list of frames and a Dilate in, the (n, 1, H / 2, W / 2) tensor warp_tensor takes out"""
    import synth
    import fresco_amd
    from oracle import fresco_oracle as O
    frames = M.frames((2, 64, 64))
    dil = fresco_amd.Dilate(kernel_size=7, device=DEV)
    sal = fresco_amd.get_saliency(list(frames), net, dil)
    assert sal.shape == (2, 1, 32, 32) and sal.dtype == torch.float32 and sal.is_cuda
    assert torch.equal(sal, net.detect(_gpu(frames), k=7)[0])
    assert torch.equal(fresco_amd.get_saliency(torch.from_numpy(frames), net, dil), sal)
    wide = fresco_amd.get_saliency(list(frames), net, fresco_amd.Dilate(kernel_size=13, device=DEV))
    assert torch.all(wide <= sal)  # a wider box can only lower 1 - sum
    oc = synth.make_opt_case(2, 16, 16, 64, seed=1)
    w = fresco_amd.warp_tensor(oc["x"].to(DEV), [f.to(DEV) for f in oc["flows"]], [o.to(DEV) for o in oc["occs"]], sal, 2)
    ref = O.warp_tensor(oc["x"], oc["flows"], oc["occs"], sal.cpu(), 2)
    assert float((w.cpu() - ref).abs().max()) < 5e-5
