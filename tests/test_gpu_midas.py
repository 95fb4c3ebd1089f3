"""The MiDaS depth detector on the GPU: the kernels of csrc/midas.hip (and the stem's "same" origin) against float64
restatements, and the native detector end to end -- every recorded tap, the depth and the two uint8 maps -- against the
records of the reference's code around the restated backbone (tests/golden/midas_golden.npz; stand-in weights,
tests/midas_model.py).

Bars (e = 2^-24, one fp32 rounding):
  * products on the split-fp16 GEMM (stem, 3 x 3 stride-2 convolution): 2^-20 sum |x| |w| + 1e-6 -- an operand plane pair
    carries a value to 2^-22, three products per term, fp32 accumulation;
  * GroupNorm: 16 e ((|x| + |mean|) rstd |gamma| + |beta| + |residual|) + 1e-6 against float64 -- the statistics are fp64 sums
    rounded once, the apply pass five fp32 operations; planes: + 2^-21 |y|;
  * pool, head merge (fp32): equal; LayerNorm: 2^-18 (|y - beta| + |beta|) + 2^-20 max|x| rstd |gamma| (768 fp32 adds per sum);
  * readout row: 16 e (|t| + |GELU(t)|) + 1e-6; tail: equal to the numpy restatement (IEEE operations in its order);
  * end to end: |got - record| <= 4 x the reference's own fp32-vs-float64 noise of that tensor (golden file) x its largest
    magnitude; uint8 maps: no value 2 or more apart, at most 2 % one apart.
Every comparison prints its ratio to the bar.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import midas_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCALE = 64.0
E = 2.0 ** -24


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np64(t):
    return t.detach().to("cpu", torch.float64).numpy()


def _planes64(planes, scale=SCALE):
    return (_np64(planes[0]) + _np64(planes[1])) / scale


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _check(name, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    print("%s: worst error / bound %.3f" % (name, float((err / bound).max())))
    assert np.all(err <= bound), name


# ---------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------
def _groupnorm_against_float64(n, H, W, C, residual):
    from fresco_amd import ops
    x = _randn(n, H, W, C, seed=C) * 3.0 + 1.5
    x[1] = x[1] * 0.25 - 4.0
    gamma, beta = _randn(C, seed=C + 1) * 0.5 + 1.0, _randn(C, seed=C + 2)
    res = _randn(n, H, W, C, seed=C + 3) if residual else None
    x64 = x.double().permute(0, 3, 1, 2)
    ref = F.group_norm(x64, 32, gamma.double(), beta.double(), 1e-5)
    g = x64.reshape(n, 32, -1)
    mean, rstd = g.mean(2), 1.0 / torch.sqrt(g.var(2, unbiased=False) + 1e-5)
    if residual:
        ref = F.relu(ref + res.double().permute(0, 3, 1, 2))
    else:
        ref = F.relu(ref)
    ref = ref.permute(0, 2, 3, 1).numpy()
    per_c = lambda t: t.repeat_interleave(C // 32, 1)[:, None, None, :].numpy()  # noqa: E731
    bound = 16 * E * ((np.abs(x.double().numpy()) + np.abs(per_c(mean))) * per_c(rstd) * np.abs(gamma.double().numpy())
                      + np.abs(beta.double().numpy()) + (np.abs(res.double().numpy()) if residual else 0.0)) + 1e-6
    y, planes = ops.midas_groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), relu=not residual,
                                    residual=None if res is None else res.to(DEV), want_f32=True, want_split=True)
    _check("groupnorm C=%d fp32" % C, _np64(y), ref, bound)
    _check("groupnorm C=%d planes" % C, _planes64(planes).reshape(n, H, W, C), ref, bound + 2.0 ** -21 * np.abs(ref))
    _, bordered = ops.midas_groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), relu=not residual,
                                      residual=None if res is None else res.to(DEV), want_f32=False, want_split=True,
                                      far_border=True)
    for k in (0, 1):
        b = bordered[k].view(n, H + 1, W + 1, C)
        assert torch.equal(b[:, :H, :W], planes[k].view(n, H, W, C))
        assert not b[:, H].any() and not b[:, :, W].any()


@pytest.mark.parametrize("C", [64, 256, 1024], ids=lambda c: "C%d_cpg%d" % (c, c // 32))
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
def test_groupnorm_matches_float64(C, residual):
    """(n, 18, 30): 540 pixels = three workgroups of the statistics pass, the last one partly filled; image 1 has its own
    statistics; the planes also go into the far-side bordered buffer"""
    _groupnorm_against_float64(2, 18, 30, C, residual)


@pytest.mark.parametrize("C", [64, 1024], ids=lambda c: "C%d_cpg%d" % (c, c // 32))
@pytest.mark.parametrize("size", [(1, 1), (17, 16)], ids=lambda s: "%dx%d" % s)
def test_groupnorm_at_one_pixel_and_a_short_second_chunk(C, size):
    """the edges of the statistics pass (csrc/groupnorm_stats.h): one pixel per image; 272 pixels = a full chunk and one of 16.
    C = 1024: 256 quads, each thread walks its chunk one pixel per step; C = 64: two channels per group, so the two halves of
    every quad belong to different groups"""
    _groupnorm_against_float64(2, size[0], size[1], C, False)


def _conv_bound(x64, w64, stride, pad4):
    mag = F.conv2d(F.pad(x64.abs(), pad4), w64.abs(), None, stride)
    return (2.0 ** -20 * mag + 1e-6).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("shape", [(2, 32, 64), (1, 36, 18)], ids=lambda s: "%dx%dx%d" % s)
def test_stem_conv_pads_two_before_and_three_after(shape):
    from fresco_amd import ops
    n, H, W = shape
    x = _randn(n, H, W, 3, seed=H) .clamp(-1, 1)
    w = _randn(64, 3, 7, 7, seed=W) * 0.2
    x64, w64 = x.double().permute(0, 3, 1, 2), w.double()
    ref = F.conv2d(F.pad(x64, (2, 3, 2, 3)), w64, None, 2).permute(0, 2, 3, 1).numpy()
    got = ops.midas_stem_conv(x.to(DEV), ops.fn_conv7_weight(w.to(DEV)))
    assert got.shape == (n, H // 2, W // 2, 64)
    bound = _conv_bound(x64, w64, 2, (2, 3, 2, 3))
    _check("stem %s" % (shape,), _np64(got), ref, bound)
    _check("stem %s last row" % (shape,), _np64(got)[:, -1], ref[:, -1], bound[:, -1])
    _check("stem %s last column" % (shape,), _np64(got)[:, :, -1], ref[:, :, -1], bound[:, :, -1])
    symmetric = F.conv2d(F.pad(x64, (3, 3, 3, 3)), w64, None, 2).permute(0, 2, 3, 1).numpy()[:, :H // 2, :W // 2]
    assert np.abs(symmetric - ref).max() > 100 * bound.max()  # (the two origins are far apart on this input)


@pytest.mark.parametrize("shape", [(2, 16, 24, 64), (1, 10, 6, 128)], ids=lambda s: "%dx%dx%dx%d" % s)
def test_same_stride2_conv_reads_the_far_border(shape):
    """GroupNorm planes with the far-side zero border -> fn_gemm 3 x 3 / stride 2 / pad 0 = StdConv2dSame's (0, 1) padding"""
    from fresco_amd import ops
    n, H, W, C = shape
    x = _randn(n, H, W, C, seed=H + C)
    gamma, beta = torch.ones(C), torch.zeros(C)
    w = _randn(C, C, 3, 3, seed=W) * (2.0 / (9 * C)) ** 0.5
    y, planes = ops.midas_groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), relu=True, want_f32=True, want_split=True,
                                    far_border=True)
    _, wp = ops.fn_prep(w.permute(0, 2, 3, 1).reshape(C, -1).contiguous().to(DEV), scale=ops.FN_W_SCALE)
    got, _ = ops.fn_gemm(planes, wp, C, 9 * C, conv=(n, H + 1, W + 1, 3, 3, 2, 0))
    y64, w64 = y.cpu().double().permute(0, 3, 1, 2), w.double()
    ref = F.conv2d(F.pad(y64, (0, 1, 0, 1)), w64, None, 2).permute(0, 2, 3, 1).numpy()
    got = _np64(got).reshape(n, H // 2, W // 2, C)
    bound = _conv_bound(y64, w64, 2, (0, 1, 0, 1))
    _check("same conv %s" % (shape,), got, ref, bound)
    _check("same conv %s last row" % (shape,), got[:, -1], ref[:, -1], bound[:, -1])
    _check("same conv %s last column" % (shape,), got[:, :, -1], ref[:, :, -1], bound[:, :, -1])
    symmetric = F.conv2d(y64, w64, None, 2, padding=1).permute(0, 2, 3, 1).numpy()
    assert symmetric.shape == ref.shape and np.abs(symmetric - ref).max() > 100 * bound.max()  # (nn.Conv2d's origin is another)


@pytest.mark.parametrize("shape", [(2, 16, 20), (1, 6, 34), (1, 2, 2), (2, 6, 4)], ids=lambda s: "%dx%dx%d" % s)
def test_pool_windows_start_at_the_even_pixel(shape):
    """negative values everywhere, so padding must never win; the last output row / column see two input rows / columns
    (2 x 2: the one window is the whole map)"""
    from fresco_amd import ops
    n, H, W = shape
    x = _randn(n, H, W, 64, seed=H * W) * 40.0 - 60.0
    want = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1), value=float("-inf")), 3, 2).permute(0, 2, 3, 1)
    out, planes = ops.midas_pool(x.to(DEV), want_f32=True)
    assert torch.equal(out.cpu(), want.contiguous())
    ref = want.double().numpy()
    _check("pool planes", _planes64(planes).reshape(ref.shape), ref, 2.0 ** -21 * np.abs(ref) + 2.0 ** -25)
    ceil_mode = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, ceil_mode=True).permute(0, 2, 3, 1)[:, :H // 2, :W // 2]
    if min(H, W) > 2:  # (on a 2 x 2 map both windows hold all four pixels)
        assert not torch.equal(ceil_mode, want)  # (EGNet's pool starts one pixel earlier)


def _layernorm_against_float64(M_, C):
    """-> ((x, gamma, beta), fp32 rows, planes) of the both-outputs run, after its comparison with float64"""
    from fresco_amd import ops
    x = _randn(M_, C, seed=1) * 4.0 + _randn(M_, 1, seed=2) * 10.0
    gamma, beta = _randn(C, seed=3) * 0.3 + 1.0, _randn(C, seed=4)
    x64 = x.double()
    ref = F.layer_norm(x64, (C,), gamma.double(), beta.double(), 1e-6).numpy()
    rstd = (1.0 / torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-6)).numpy()
    b64 = beta.double().numpy()
    bound = 2.0 ** -18 * (np.abs(ref - b64) + np.abs(b64)) + 2.0 ** -20 * x64.abs().max(1, keepdim=True)[0].numpy() * rstd \
        * np.abs(gamma.double().numpy())
    y, planes = ops.midas_layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), eps=1e-6, want_f32=True, want_split=True)
    _check("layernorm (%d, %d) fp32" % (M_, C), _np64(y), ref, bound)
    _check("layernorm (%d, %d) planes" % (M_, C), _planes64(planes), ref, bound + 2.0 ** -21 * np.abs(ref))
    return (x, gamma, beta), y, planes


def test_layernorm_768():
    _layernorm_against_float64(37, 768)  # 37 rows: ten workgroups of four, the last one with one row


def _tokens_equal(n, L, C):
    from fresco_amd import ops
    grid, cls, pos = _randn(n, L - 1, C, seed=5), _randn(C, seed=6), _randn(L, C, seed=7)
    tok = ops.midas_tokens(grid.to(DEV), cls.to(DEV), pos.to(DEV))
    want = torch.cat([cls.expand(n, 1, C), grid], 1) + pos
    print("tokens (%d, %d, %d): %d values differ" % (n, L, C, int((tok.cpu() != want).sum())))
    assert torch.equal(tok.cpu(), want)


def _head_merge_equal(n, L, heads):
    from fresco_amd import ops
    o = _randn(heads * n, L, 64, seed=8) * 20.0
    merged, planes = ops.midas_head_merge(o.to(DEV), n, want_f32=True, want_split=True)
    want = o.view(heads, n, L, 64).permute(1, 2, 0, 3).reshape(n * L, heads * 64)
    print("head merge (%d, %d, %d): %d values differ" % (heads * n, L, 64, int((merged.cpu() != want).sum())))
    assert torch.equal(merged.cpu(), want)
    ref = want.double().numpy()
    _check("head merge planes", _planes64(planes), ref, 2.0 ** -21 * np.abs(ref) + 2.0 ** -25)


def test_tokens_and_head_merge():
    _tokens_equal(2, 25, 768)
    _head_merge_equal(2, 25, 12)


def _readout_against_float64(n, rows, C, spread=0.0):
    """spread: how far apart the images' bias rows lie (row i is shifted by spread * (i - (n - 1) / 2)).
    -> (x, rowbias, fp32 result, float64 reference, bound)"""
    from fresco_amd import ops
    x, rb = _randn(n * rows, C, seed=9) * 2.0, _randn(n, C, seed=10) * 2.0
    rb = rb + spread * (torch.arange(n, dtype=torch.float32)[:, None] - 0.5 * (n - 1))
    t = x.double() + rb.double().repeat_interleave(rows, 0)
    ref = F.gelu(t).numpy()
    bound = 16 * E * (np.abs(t.numpy()) + np.abs(ref)) + 1e-6
    out, planes = ops.midas_rowbias_gelu(x.to(DEV), rb.to(DEV), rows, want_f32=True, want_split=True)
    _check("readout fp32", _np64(out), ref, bound)
    _check("readout planes", _planes64(planes), ref, bound + 2.0 ** -21 * np.abs(ref))
    return x, rb, out, ref, bound


def test_readout_row_bias():
    _readout_against_float64(3, 24, 768)


def _tail_frames():
    """frame 0: smooth with a minimum of 3.5 (not 0); frame 1: a flat region at the minimum (below bg_th) with a step edge
    and noise elsewhere; frame 2: constant"""
    H, W = 40, 56
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    rs = np.random.RandomState(3)
    f0 = (3.5 + 20.0 * (np.sin(xx / 7.0) * np.cos(yy / 5.0) + 1.0)).astype(np.float32)
    f1 = (1.0 + 30.0 * rs.rand(H, W)).astype(np.float32)
    f1[8:24, 10:30] = 0.25
    f2 = np.full((H, W), 7.0, np.float32)
    return np.stack([f0, f1, f2])


def _tail_against_numpy(d, cond_dtype):
    """ops.midas_tail of the frames d (n, H, W) float32 numpy: both uint8 maps equal to midas_model.tail frame by frame, the
    condition equal to the torch expression -> (depth images, normal images)"""
    from fresco_amd import ops
    dimg, nimg, cond = ops.midas_tail(_gpu(d), M.A, M.BG_TH, cond_dtype=cond_dtype)
    for f in range(d.shape[0]):
        want_d, want_n = M.tail(d[f])
        got_d, got_n = dimg[f].cpu().numpy(), nimg[f].cpu().numpy()
        print("tail %s %s frame %d: depth image differs in %d values, normal image in %d"
              % (d.shape, cond_dtype, f, (got_d != want_d).sum(), (got_n != want_n).sum()))
        assert np.array_equal(got_d, want_d) and np.array_equal(got_n, want_n)
    want = (dimg.float()[:, None].repeat(1, 3, 1, 1) / 255.0 * 2 - 1) * 0.5 + 0.5
    assert cond.dtype == cond_dtype and torch.equal(cond, want.to(cond_dtype))
    return dimg, nimg


def test_tail_matches_the_numpy_restatement():
    d = _tail_frames()
    dimg, nimg = _tail_against_numpy(d, torch.float16)
    assert d[0].min() > 3 and (dimg[1].cpu().numpy()[8:24, 10:30] == 0).all()
    assert (nimg[1].cpu().numpy()[10:22, 12:28] == (127, 127, 255)).all()      # masked: the flat normal
    assert not dimg[2].any() and (nimg[2].cpu().numpy() == (127, 127, 255)).all()  # the constant frame


# ---------------------------------------------------------------------------------------------------------------
# the detector
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def detector(gold):
    import fresco_amd
    net = fresco_amd.DPTDepthModel()
    shapes = [tuple(int(v) for v in s.split("x")) if s else () for s in gold["param_shapes"]]
    net.load_state_dict(M.standin_state_dict(zip(gold["param_names"].tolist(), shapes)), strict=True)
    return fresco_amd.MidasDetector(network=net.float().to(DEV))


@pytest.fixture(scope="module")
def runs(detector):
    """case -> (taps, depth, depth images, normal images) of ONE native run per case, shared by the tests below"""
    out = {}
    for case in M.CASES:
        taps = {}
        fr = _gpu(M.frames(case))
        depth = detector.model.depth(fr, taps)
        dimg, nimg = detector.detect_batch(fr)
        out[case] = (taps, depth, dimg, nimg)
    assert not detector.model._warned  # (the native path, not its library-ops recomputation)
    return out


@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_taps_and_depth_match_the_record(case, gold, runs):
    key = M.case_key(case)
    taps, depth = runs[case][:2]
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    worst = []
    for i, t in enumerate(M.TAPS + ("depth",)):
        got = M.thin_depth(depth) if t == "depth" else M.thin(taps[t])
        rec = gold["%s_%s" % (key, t)]
        assert got.shape == rec.shape, t
        ratio = float(np.abs(got.astype(np.float64) - rec).max() / (4 * noise[i] * peak[i]))
        print("%s %-8s |got - record| / (4 x reference noise %.2e x peak %.3g) = %.3f" % (key, t, noise[i], peak[i], ratio))
        worst.append((ratio, t))
    assert max(worst)[0] <= 1.0, max(worst)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_uint8_maps_match_the_record(case, gold, runs):
    key = M.case_key(case)
    for name, got in (("depth_image", runs[case][2]), ("normal_image", runs[case][3])):
        rec = gold["%s_%s" % (key, name)]
        diff = np.abs(got.cpu().numpy().astype(int) - rec.astype(int))
        print("%s %s: %.3f %% one apart, largest difference %d" % (key, name, 100 * (diff == 1).mean(), diff.max()))
        assert diff.max() <= 1 and (diff == 1).mean() <= 0.02, name


def test_batch_equals_single_calls_and_host_arrays(detector, runs):
    case = M.CASES[0]
    fr = M.frames(case)
    dimg, nimg = runs[case][2:]
    for f in range(case[0]):
        d1, n1 = detector(fr[f])  # a host array through __call__
        assert isinstance(d1, np.ndarray) and d1.shape == fr[f].shape[:2] and n1.shape == fr[f].shape
        assert np.array_equal(d1, dimg[f].cpu().numpy()) and np.array_equal(n1, nimg[f].cpu().numpy())
        d2 = detector.model.depth(_gpu(fr[f:f + 1]))
        assert torch.equal(d2[0], runs[case][1][f])
    saved, detector.model.max_frames = detector.model.max_frames, 1
    try:
        d3, n3 = detector.detect_batch(list(fr))
    finally:
        detector.model.max_frames = saved
    assert torch.equal(d3, dimg) and torch.equal(n3, nimg)


def test_control_image_is_the_torch_expression(detector, runs):
    case = M.CASES[0]
    fr = _gpu(M.frames(case))
    dimg = runs[case][2]
    for dtype in (torch.float16, torch.float32):
        want = ((dimg.float()[:, None].repeat(1, 3, 1, 1) / 255.0 * 2 - 1) * 0.5 + 0.5).to(dtype)
        cond = detector.control_image(fr, dtype)
        assert cond.shape == (2 * case[0], 3) + tuple(fr.shape[1:3]) and cond.dtype == dtype
        assert torch.equal(cond, torch.cat([want] * 2))
    assert torch.equal(detector.control_image(fr, torch.float16, guidance=False), want.half())


def test_library_ops_path_agrees(detector, gold, runs):
    case = M.CASES[1]
    key = M.case_key(case)
    detector.model.library_ops = True
    try:
        lib = detector.model.depth(_gpu(M.frames(case)))
    finally:
        detector.model.library_ops = False
    bar = 4 * gold[key + "_noise"][-1] * gold[key + "_peak"][-1]
    ratio = float((lib - runs[case][1]).abs().max()) / (2 * bar)
    print("%s: |library ops - native| / (2 x the end-to-end bar) = %.3f" % (key, ratio))
    assert ratio <= 1.0
