"""The EGNet detector at the sizes a batch of eight 512 x 512 frames takes: the code paths of csrc/egnet.hip, of
fresco_fn_gemm's EGNet-only convolution forms and of fresco_amd/egnet.py that the small maps of tests/test_gpu_egnet.py and
tests/test_gpu_egnet_conv.py never reach.  Their bars are reused unchanged and every comparison prints its worst
error / bar.

  A  the three streaming kernels past one pass of their grid-stride loop.  The grid is capped at 2048 blocks of 256
     threads (EG_MAX_BLOCKS, "the rest is a grid-stride loop"): everything past 524 288 work items runs in a later pass.
     Smallest shapes with a ragged second pass; random data per image, so pass two is no repeat of pass one.
  B  the convolution forms EGNet added (1 x 1 / stride 2, 3 x 3 with dilation 2, 5 x 5 and 7 x 7 im2col, the K = 2048
     product) at eight row blocks of 256 rows and more, where fresco_fn_gemm orders workgroups through the XCD-aware map
     (main branch plus rb % 8 tail blocks), with ragged last blocks and row blocks that straddle frames.  Driven by the
     _problem / _convolve / _report helpers of tests/test_gpu_egnet_conv.py.
  C  one output column (final_score's 128 -> 1, 3 x 3): window-in-LDS and im2col forms, up to 128 row blocks; the output
     sits inside a larger poisoned buffer that must stay untouched around it.
  D  the tail kernel's extremes: k = 1, 3, 15 (EG_MAX_K: the LDS tile fills its 30 x 30 array), a same-size resize, one-row
     and one-column destinations, the production 128^2 -> 256^2 resize with three images.
  E  the native detector end to end on eight 512 x 512 frames and on two 372 x 500 frames (odd maps on every scale) against
     the project's own module in float64 on the CPU, |got - f64| <= 8 e_ref + 1e-7 (saliency + 1e-6) with e_ref the same
     module's fp32-vs-float64 distance -- tests/test_gpu_egnet.py's rule with e_ref computed here; taps at full channel
     width.  The frames without a CPU reference are pinned by max_frames = 1 (single-frame passes stay inside one grid pass
     of the input and pool kernels) being bit-equal to the batched run.

Measured on an MI355X, worst error / bar: A input 0.122, pool fp32 equal and planes 0.978, resize_add 0.015 - 0.148 (its
planes up to 0.996: the plane bound is the split's own rounding); B fp32 rows 0.064 - 0.098, planes only 0.065 - 0.103 (a
CPU fp32 conv2d 0.008 - 0.070); C 0.022 - 0.054 with no float outside the column touched; D 0.023 - 0.110; E 0.335
(8 x 512 x 512) and 0.348 (2 x 372 x 500), both at tmp_fea, the logit at 0.243 / 0.216.  DESIGN.md section 13 has the table.

A scratch build in which each streaming kernel's loop is a single pass (`if (idx < total)` in place of the `for`) passes
the kernel tests of tests/test_gpu_egnet.py and fails here: see MUTANT below.
"""
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import egnet_model as M
import test_gpu_egnet as E
import test_gpu_egnet_conv as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALE = 64.0
ONE_PASS = 2048 * 256  # work items of one pass of a streaming kernel's grid-stride loop (EG_MAX_BLOCKS blocks of 256 threads)
FN_BM = 256            # rows of a row block of fresco_fn_gemm

# What the single-pass scratch build (see the module docstring) gave on an MI355X; outputs past the first pass are simply
# never written, so the figures are those of whatever the allocator left there.
MUTANT = """
tests/test_gpu_egnet.py, kernel and end-to-end tests alike: 28 passed.
tests/test_gpu_egnet_fullsize.py: 7 failed, 27 passed --
  test_input_past_one_grid_pass                   worst error / bound 2.1e+06
  test_pool_past_one_grid_pass                    66 048 of 2 163 200 fp32 values differ from F.max_pool2d
  test_resize_add_past_one_grid_pass              17^2 -> 65^2, C = 512: worst error / bound 1.8e+08, planes nan;
                                                  17^2 -> 128^2, C = 128: 2.5e+05; same size 128^2: 2.5e+05, not bit-equal
  test_batch_equals_frame_by_frame_at_full_size   8 x 512 x 512: 441 899 saliency values and all 458 752 logits of frames
                                                  1 - 7 differ from max_frames = 1; 2 x 372 x 500: 31 293 and 35 250
  test_native_detector_matches_float64_at_full_size passes (0.335, 0.348): frame 0 lies inside the first pass of every
  streaming kernel, which is why the other frames are pinned bit for bit against single-frame passes.  B and C read planes
  that ops.fn_prep wrote and D runs the tail kernel, which has no such loop: they pass.
"""


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------
# A. streaming kernels past one grid pass
# ---------------------------------------------------------------------------------------------------------------
def test_input_past_one_grid_pass():
    from fresco_amd import ops
    n, H, W = 2, 600, 592
    assert ONE_PASS < n * (H // 2) * (W // 2) * 3 < 2 * ONE_PASS  # 532 800: a ragged second pass
    x = np.random.RandomState(H * W).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    # known pixels in the last image's last row and column, all of them decoded in pass two
    x[1, -2:, :, :] = (np.arange(W) % 251).astype(np.uint8)[None, :, None]
    x[1, :, -2:, :] = (np.arange(H) % 241).astype(np.uint8)[:, None, None]
    x[1, -2:, -2:] = (0, 255, 128)
    got = ops.egnet_input(_gpu(x))
    assert got.shape == (n, H // 2, W // 2, 3) and got.dtype == torch.float32
    ref = E._nhwc(M.cv2sod64(x)).numpy()
    g = E._np64(got)
    err = np.abs(g - ref)
    print("input %s: worst error / bound %.3f" % ((n, H, W), (err / E._plane_bound(ref)).max()))
    assert np.all(err <= E._plane_bound(ref))
    corner = np.array([0.0, 255.0, 128.0]) - np.array(M.MEANS)
    assert np.all(np.abs(g[1, -1, -1] - corner) <= E._plane_bound(corner))
    p = (np.arange(W) % 251).astype(np.float64)  # the last row but its corner: the mean of columns 2 ox, 2 ox + 1
    want = (0.5 * (p[0:W - 2:2] + p[1:W - 2:2]))[:, None] - np.array(M.MEANS)[None, :]
    assert np.all(np.abs(g[1, -1, :-1] - want) <= E._plane_bound(want))
    assert torch.equal(ops.egnet_input(_gpu(x)), got)


def test_pool_past_one_grid_pass():
    """the production shape: eight stem maps of a 512 x 512 frame, 128 x 128 -> 65 x 65"""
    from fresco_amd import ops
    n, H, W = 8, 128, 128
    assert ops.egnet_pool_size(H) == 65
    assert ONE_PASS < n * 65 * 65 * (64 // 4) < 2 * ONE_PASS  # 540 800
    x = torch.randn(n, H, W, 64, generator=torch.Generator().manual_seed(H * 100 + W)) * 60.0 - 30.0
    x[:, ::3] *= 1e-3
    want = E._nhwc(F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, ceil_mode=True))
    assert want.shape == (n, 65, 65, 64)
    out, planes = ops.egnet_pool(x.to(DEV), want_f32=True, scale=SCALE)
    differ = int((out.cpu() != want).sum())
    print("pool %s: %d of %d fp32 values differ from F.max_pool2d" % ((n, H, W), differ, want.numel()))
    assert torch.equal(out.cpu(), want)
    assert planes[0].shape == (n * 65 * 65, 64) and planes[0].dtype == torch.float16
    ref = want.double().numpy().reshape(-1, 64) * SCALE
    err = np.abs(E._planes64(planes) - ref)
    print("pool %s: worst plane error / bound %.3f" % ((n, H, W), (err / E._plane_bound(ref)).max()))
    assert np.all(err <= E._plane_bound(ref))
    none, again = ops.egnet_pool(x.to(DEV), scale=SCALE)
    assert none is None and torch.equal(again[0], planes[0]) and torch.equal(again[1], planes[1])


# (n, (h, w), (H, W), C, [(with addend, ReLU)])
BIG_RESIZES = [
    (1, (17, 17), (65, 65), 512, [(0, 0), (0, 1), (1, 0), (1, 1)]),     # 540 800 items: a short ragged second pass
    (2, (17, 17), (128, 128), 128, [(0, 0), (0, 1), (1, 0), (1, 1)]),   # merge2's resize to the stem scale; two full passes
    (2, (128, 128), (128, 128), 128, [(1, 1)]),                         # the running sum relu(fea + f): an exact copy + one add
]


@pytest.mark.parametrize("case", BIG_RESIZES, ids=lambda c: "%dx%dx%dto%dx%d_C%d" % ((c[0],) + c[1] + c[2] + (c[3],)))
def test_resize_add_past_one_grid_pass(case):
    from fresco_amd import ops
    n, (h, w), (H, W), Cn, runs = case
    assert n * H * W * (Cn // 4) > ONE_PASS
    g = torch.Generator().manual_seed(1000 * h + 10 * W + Cn)
    x = torch.randn(n, h, w, Cn, generator=g) * 40.0
    x[:, :, ::2] *= 1e-2
    add = torch.randn(n, H, W, Cn, generator=g) * 40.0
    up64 = E._nhwc(F.interpolate(x.double().permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True))
    mag = E._nhwc(F.interpolate(x.double().abs().permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True))
    xg, addg = x.to(DEV), add.to(DEV)
    for with_add, relu in runs:
        ref = up64 + add.double() if with_add else up64
        ref = (F.relu(ref) if relu else ref).numpy()
        bound = 4e-6 * (mag.numpy() + (add.double().abs().numpy() if with_add else 0.0)) + 1e-6
        out, planes = ops.egnet_resize_add(xg, (H, W), addend=addg if with_add else None, relu=bool(relu), want_f32=True,
                                           want_split=True, scale=SCALE)
        assert out.shape == (n, H, W, Cn) and planes[0].shape == (n * H * W, Cn)
        o64 = E._np64(out)
        err = np.abs(o64 - ref)
        perr = np.abs(E._planes64(planes).reshape(ref.shape) - o64 * SCALE)
        pb = E._plane_bound(o64 * SCALE)
        print("resize_add %s add=%d relu=%d: worst error / bound %.3f, planes %.3f"
              % (case[:4], with_add, relu, (err / bound).max(), (perr / pb).max()))
        assert np.all(err <= bound)
        if (h, w) == (H, W):
            want = x + add if with_add else x
            assert torch.equal(out.cpu(), F.relu(want) if relu else want)
        assert np.all(perr <= pb)  # the planes carry the fp32 result
        only, none = ops.egnet_resize_add(xg, (H, W), addend=addg if with_add else None, relu=bool(relu))
        assert none is None and torch.equal(only, out)


# ---------------------------------------------------------------------------------------------------------------
# B. EGNet's convolution forms at eight row blocks and more: (cin, cout, n, H, W, k, stride, pad, dilation)
# ---------------------------------------------------------------------------------------------------------------
FULL_CASES = [
    (256, 512, 2, 65, 65, 1, 2, 0, 1),     # layer2's shortcut: M = 2178 = 8 main row blocks + a 130-row tail; 4 column blocks
    (256, 128, 2, 65, 65, 1, 2, 0, 1),     # layer2 conv1: one column block, the nb == 1 order
    (512, 512, 8, 17, 17, 3, 1, 2, 2),     # layer4: M = 2312 = 8 main + 2 tail blocks; every block straddles frames
    (128, 128, 1, 48, 48, 5, 1, 2, 1),     # final_score's 5 x 5 on whole patches: M = 2304 = 9 row blocks, im2col
    (512, 512, 8, 17, 17, 5, 1, 2, 1),     # a 5 x 5, 512-wide merge-layer convolution on an eight-frame 17 x 17 map
    (512, 512, 7, 17, 17, 7, 1, 3, 1),     # merge's 7 x 7: M = 2023 = exactly 8 row blocks, the last ragged; K = 25088
    (2048, 512, 8, 17, 17, 1, 1, 0, 1),    # convert4 as a plain product at 10 row blocks, K = 2048
]


def _row_blocks(case):
    return -(-C._problem(case)["ref"].shape[0] // FN_BM)


@pytest.mark.parametrize("case", FULL_CASES, ids=C._case_id)
def test_fp32_rows_at_eight_row_blocks_and_more(case):
    p = C._problem(case)
    assert _row_blocks(case) >= 8 and p["peak"] < 1015.0 / 2
    out, planes, tripped = C._convolve(case, True)
    assert planes is None and out.dtype == torch.float32 and not tripped
    C._report(case, "fp32 rows, %d row blocks" % _row_blocks(case), C._np64(out), 4e-6 * p["S"] + 1e-6)
    again, _, _ = C._convolve(case, True)
    assert torch.equal(again, out)  # the same bits on every run


@pytest.mark.parametrize("case", FULL_CASES, ids=C._case_id)
def test_planes_only_at_eight_row_blocks_and_more(case):
    p = C._problem(case)
    assert _row_blocks(case) >= 8
    out, planes, tripped = C._convolve(case, False, 64.0, 64.0)
    assert out is None and not tripped
    hi, lo = planes
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16 and hi.shape == p["ref"].shape == lo.shape
    got = (C._np64(hi) + C._np64(lo)) / 64.0
    bound = 4e-6 * p["S"] + 1e-6 + (2.0 ** -21 * np.abs(p["ref"] * 64.0) + 2.0 ** -25) / 64.0
    C._report(case, "planes only, scales (64, 64), %d row blocks" % _row_blocks(case), got, bound)


# ---------------------------------------------------------------------------------------------------------------
# C. one output column: (n, H, W) of a 128 -> 1, 3 x 3, padding 1 convolution
# ---------------------------------------------------------------------------------------------------------------
ONE_COLUMN = [
    (1, 16, 16),     # window-in-LDS form, one row block
    (9, 16, 16),     # ... nine row blocks
    (1, 9, 11),      # im2col form
    (2, 128, 128),   # the production map: 128 row blocks
]
GUARD, POISON = 4096, -12345.0


@pytest.mark.parametrize("nhw", ONE_COLUMN, ids=lambda s: "%dx%dx%d" % s)
def test_one_output_column_stores_nothing_else(nhw):
    """final_score[2] as TUN_bone._conv runs it: bias, no ReLU, fp32 rows (operand planes need N % 8 = 0).  ops.fn_gemm takes
    the fp32 output as an argument (out_f32, row stride N = 1): the M results sit in the middle of a poisoned buffer whose
    4096 floats on either side must keep their poison -- a column block past N that stored would write up to 63 floats
    past the last row (and over other rows, which the error bound sees)."""
    from fresco_amd import ops
    from fresco_amd.fnweights import WeightPlanes
    n, H, W = nhw
    cin, Mrows = 128, n * H * W
    g = torch.Generator().manual_seed(128001 + 17 * n + H + W)
    rows = torch.randn(Mrows, cin, generator=g).clamp_min(0) * 60.0
    rows[::7] *= 1e-3
    w = (0.9 * (2.0 / (9 * cin)) ** 0.5 * torch.randn(1, cin, 3, 3, generator=g, dtype=torch.float64)).float()
    b = (0.1 * torch.randn(1, generator=g, dtype=torch.float64)).float()
    x = rows.double().reshape(n, H, W, cin).permute(0, 3, 1, 2).contiguous()
    assert float(x.max()) < 1015.0 / 2
    ref = F.conv2d(x, w.double(), b.double(), padding=1).reshape(-1).numpy()
    S = (F.conv2d(x, w.double().abs(), None, padding=1) + b.double().abs()).reshape(-1).numpy()
    lib32 = F.conv2d(x.float(), w, b, padding=1).double().reshape(-1).numpy()
    bound = 4e-6 * S + 1e-6
    assert (ref < 0).mean() > 0.05 and (ref > 0).mean() > 0.05  # no ReLU: both signs must come through

    def run():
        wts = WeightPlanes()
        buf = torch.full((Mrows + 2 * GUARD,), POISON, dtype=torch.float32, device=DEV)
        with ops.fn_range_guard(torch.device(DEV)) as guard:
            _, xs = ops.fn_prep(rows.to(DEV), ld=cin, scale=SCALE)
            wp = wts.get(w.to(DEV), "conv")
            assert wp[0].shape == (1, 9 * cin)
            out, planes = ops.fn_gemm(xs, wp, 1, 9 * cin, bias=b.to(DEV), act=0, conv=(n, H, W, 3, 3, 1, 1, 1),
                                      want_f32=True, want_split=False, out_f32=buf[GUARD:GUARD + Mrows].view(Mrows, 1),
                                      a_scale=SCALE, out_scale=SCALE)
        assert planes is None and not guard.tripped() and not wts.out_of_range
        return buf.cpu(), out

    buf, out = run()
    assert out.shape == (Mrows, 1) and out.data_ptr() != 0
    got = buf[GUARD:GUARD + Mrows].double().numpy()
    err = np.abs(got - ref)
    print("128to1_%dx%dx%d (%d row blocks): max |d| %.3g, worst error / bound %.3f (CPU fp32 conv2d %.3f); %d guard floats "
          "overwritten" % (n, H, W, -(-Mrows // FN_BM), err.max(), (err / bound).max(), (np.abs(lib32 - ref) / bound).max(),
                           int((buf[:GUARD] != POISON).sum() + (buf[GUARD + Mrows:] != POISON).sum())))
    assert np.all(np.isfinite(got)) and np.all(err <= bound)
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + Mrows:] == POISON).all())
    assert torch.equal(run()[0], buf)  # the same bits on every run


# ---------------------------------------------------------------------------------------------------------------
# D. the tail kernel's extremes: (images, ((h, w), (Hs, Ws)), k, what the field allows)
# ---------------------------------------------------------------------------------------------------------------
# "both": the condition of test_saliency_tail_matches_float64 (both clamps and the graded part); k = 1 is a single sigmoid
# below 1, so nothing saturates and the map must be positive everywhere
TAILS = [
    (2, ((18, 22), (36, 44)), 1, "positive"),
    (2, ((18, 22), (36, 44)), 3, "both"),
    (2, ((18, 22), (36, 44)), 15, "both"),      # EG_MAX_K: the 30 x 30 tile
    (3, ((128, 128), (256, 256)), 7, "both"),   # the production resize, 16 x 16 x 3 blocks
    (2, ((20, 24), (20, 24)), 7, "both"),       # same size: every weight 0
    (2, ((8, 8), (1, 32)), 7, "both"),          # one destination row: egnet_tap's dst == 1 branch
    (2, ((8, 8), (32, 1)), 7, "both"),          # ... one column
]


@pytest.mark.parametrize("case", TAILS, ids=lambda c: "%dx%dx%dto%dx%d_k%d" % ((c[0],) + c[1][0] + c[1][1] + (c[2],)))
def test_saliency_tail_extremes(case):
    from fresco_amd import ops
    n, ((h, w), (Hs, Ws)), k, field = case
    lg = E._smooth_logits(n, h, w)
    assert lg.min() < -11.0 and lg.max() > 3.0

    def tail(t):
        up = F.interpolate(t[:, None], (Hs, Ws), mode="bilinear", align_corners=True)
        return up, M.saliency_from_logit(up, k)

    up32, s32 = tail(lg)
    up64, s64 = tail(lg.double())
    e32 = float((s32.double() - s64).abs().max())
    bar = 8 * e32 + 1e-6
    sal, up = ops.egnet_saliency(lg.to(DEV), (Hs, Ws), k=k, want_logit=True)
    assert sal.shape == (n, 1, Hs, Ws) and up.shape == (n, Hs, Ws)
    err = float((sal.cpu().double() - s64).abs().max())
    s = s64.numpy()
    print("saliency %s k=%d n=%d: max |d| %.3g, bar %.3g (CPU fp32 restatement %.3g), ratio %.3f; %.0f %% zero, %.0f %% above "
          "0.9, min %.3g" % (case[1], k, n, err, bar, e32, err / bar, 100 * (s == 0).mean(), 100 * (s > 0.9).mean(), s.min()))
    if field == "both":
        assert (s == 0).mean() > 0.05 and (s > 0.9).mean() > 0.05
    else:
        assert k == 1 and s.min() > 0
    assert err <= bar
    mag = F.interpolate(lg.double().abs()[:, None], (Hs, Ws), mode="bilinear", align_corners=True)[:, 0]
    assert torch.all((up.cpu().double() - up64[:, 0]).abs() <= 4e-6 * mag + 1e-6)
    if (h, w) == (Hs, Ws):
        assert torch.equal(up.cpu(), lg)
    assert float(sal.min()) >= 0.0 and float(sal.max()) <= 1.0
    again, none = ops.egnet_saliency(lg.to(DEV), (Hs, Ws), k=k)
    assert none is None and torch.equal(again, sal)


# ---------------------------------------------------------------------------------------------------------------
# E. end to end at full size
# ---------------------------------------------------------------------------------------------------------------
# eight 512 x 512 frames: the call FRESCO makes.  two 372 x 500 frames: 186 x 250 -> stem 93 x 125 -> pool 47 x 63, odd maps
# on every scale, no map of whole patches (im2col throughout).  Frame 0 of either draw meets the conditions below.
FULL_SIZES = [(8, 512, 512), (2, 372, 500)]
REF_FRAME = 0

net = E.net  # the detector with the stand-in weights on the GPU (module-scoped here as there)


@pytest.fixture(scope="module")
def cpu_nets():
    """the project's own module on the CPU, in fp32 and as a float64 copy of the same weight values"""
    from fresco_amd import egnet
    n32 = egnet.build_model("resnet")
    n32.load_state_dict(M.standin_state_dict())
    n32 = n32.float().eval()
    return n32, copy.deepcopy(n32).double()


@pytest.fixture(scope="module")
def full_refs(cpu_nets):
    """case -> [(name, fp32 result, float64 result, floor)] of REF_FRAME, NHWC numpy: every tap, the logit, the saliency;
    computed once per case"""
    n32, n64 = cpu_nets
    cache = {}

    def get(case):
        if case not in cache:
            fr = M.frames(case)[REF_FRAME:REF_FRAME + 1]
            runs = []
            with torch.no_grad():
                for m, dtype in ((n32, torch.float32), (n64, torch.float64)):
                    taps = {}
                    logit = m.live_logit(M.cv2sod64(fr, dtype), taps)
                    sal = M.saliency_from_logit(logit, M.K_DILATE)
                    run = [("logit", logit[:, 0], 1e-7), ("saliency", sal, 1e-6)]
                    run += [(name, taps[name].permute(0, 2, 3, 1), 1e-7) for name in M.TAPS]
                    runs.append(run)
            cache[case] = [(name, a.double().numpy(), b.numpy(), floor)
                           for (name, a, floor), (_, b, _) in zip(*runs)]
        return cache[case]
    return get


@pytest.fixture(scope="module")
def native_runs(net):
    """case -> (saliency, logit, taps) of the batched native run, with warnings as errors; computed once per case"""
    cache = {}

    def get(case):
        if case not in cache:
            taps = {}
            with warnings.catch_warnings():
                warnings.simplefilter("error")  # no range trip: the native path computed this
                sal, logit = net.detect(_gpu(M.frames(case)), k=M.K_DILATE, want_logit=True, taps=taps)
            cache[case] = (sal, logit, taps)
        return cache[case]
    return get


@pytest.mark.parametrize("case", FULL_SIZES, ids=M.case_key)
def test_native_detector_matches_float64_at_full_size(case, net, full_refs, native_runs):
    n, H, W = case
    assert net.max_frames >= n  # one chunk: the taps are those of all n frames
    refs = dict((name, (f32, f64, floor)) for name, f32, f64, floor in full_refs(case))
    # conditions on the reference alone: empty, saturated and graded regions in the frame that is compared
    s = refs["saliency"][1]
    zero, high, graded = float((s == 0).mean()), float((s > 0.9).mean()), float(((s >= 0.05) & (s <= 0.9)).mean())
    l64 = refs["logit"][1]
    peak = max(float(np.abs(refs[t][1]).max()) for t in M.TAPS)
    print("%s frame %d, float64: %.3f zero, %.3f above 0.9, %.3f graded; logits %.1f .. %.1f; peak activation %.0f"
          % (M.case_key(case), REF_FRAME, zero, high, graded, l64.min(), l64.max(), peak))
    assert zero >= 0.02 and graded >= 0.01 and 0.5 <= high <= 0.97
    assert peak < 1015.0 / 2

    sal, logit, taps = native_runs(case)
    assert sal.shape == (n, 1, H // 2, W // 2) and logit.shape == (n, H // 2, W // 2) and sal.dtype == torch.float32
    assert list(taps) == list(M.TAPS)
    got = {"logit": logit, "saliency": sal}
    got.update(taps)
    worst, failed = 0.0, []
    for name in ["logit", "saliency"] + list(M.TAPS):
        f32, f64, floor = refs[name]
        assert got[name].shape[0] == n, (name, got[name].shape)
        g = E._np64(got[name][REF_FRAME:REF_FRAME + 1])
        assert g.shape == f64.shape, (name, g.shape, f64.shape)
        e_ref = float(np.abs(f32 - f64).max())
        bar = 8 * e_ref + floor
        err = float(np.abs(g - f64).max())
        print("native %s %-13s max |d| %.3g, e_ref %.3g, error / bar %.3f" % (M.case_key(case), name, err, e_ref, err / bar))
        worst = max(worst, err / bar)
        if not err <= bar:
            failed.append((name, err, bar))
    print("native %s: worst error / bar %.3f" % (M.case_key(case), worst))
    assert not failed, failed


@pytest.mark.parametrize("case", FULL_SIZES, ids=M.case_key)
def test_batch_equals_frame_by_frame_at_full_size(case, net, native_runs):
    """the frames without a CPU reference: one frame per pass stays inside one grid pass of the input and pool kernels, so
    this pins the later passes of the batched run against the first"""
    sal, logit, _ = native_runs(case)
    one = copy.deepcopy(net)
    one.max_frames = 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sal1, logit1 = one.detect(_gpu(M.frames(case)), k=M.K_DILATE, want_logit=True)
    print("%s: batched vs max_frames = 1: %d saliency values and %d logits differ"
          % (M.case_key(case), int((sal1 != sal).sum()), int((logit1 != logit).sum())))
    assert torch.equal(sal1, sal) and torch.equal(logit1, logit)
    again = net.detect(_gpu(M.frames(case)), k=M.K_DILATE, want_logit=True)
    assert torch.equal(again[0], sal) and torch.equal(again[1], logit)  # the same bits on every run
