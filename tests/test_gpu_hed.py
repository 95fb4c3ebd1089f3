"""The HED annotator on the GPU: the three kernels of csrc/hed.hip against float64 restatements, and the native detector
end to end against records of the unmodified reference (tests/golden/hed_golden.npz and hed_wide_golden.npz, stand-in
weights and frames of tests/hed_model.py).  tests/test_gpu_hed_conv.py holds each convolution alone to a float64 one.

Bounds.
  * Operand planes: hi + lo carries 22 bits, |hi + lo - v s| <= 2^-21 |v s|; lo is an fp16 whose spacing below 2^-14 is
    2^-24, so half a spacing (2^-25, in scaled units) is added for values that small.
  * Side projection: 4e-6 sum |h| |w|, the bar tests/test_gpu_flownet.py holds fp32-accumulated products to.
  * Fuse: 2e-6 + 2e-6 |ref| against the golden's float64 fused logit, from the reference's fp32 side maps (the golden's
    own fp32 fuse is at most 1.2e-6 from that record); the guard band of the uint8 rule is taken from the same record.
    Also held, tighter: the same bar against a float64 fuse of the SAME fp32 maps (pure fp32 interpolation error).
  * End to end: e_ref = the reference's own |fp32 run - fp64 run| per map; the native path may be 8 e_ref + 1e-7 from the
    fp64 record (22-bit operands against fp32's 24: 4 x, a different summation order: 2 x).
  * uint8 maps: equal to the reference's wherever 255 sigmoid(logit64) is farther than 0.02 from an integer, at most one
    apart elsewhere, and that band holds at most 6 % of a case's pixels (hed_model.check_u8).

Measured on an MI355X, worst native distance / bar over a case's recorded frames (side maps 1-5, then the fused logit):
  2 x 64 x 64   0.16 0.20 0.42 0.65 0.67 | 0.46        1 x 64 x 128  0.16 0.24 0.27 0.33 0.32 | 0.32
  2 x 96 x 80   0.20 0.25 0.30 0.41 0.37 | 0.31        1 x 72 x 88   0.14 0.24 0.22 0.52 0.31 | 0.38
  1 x 128 x 128 0.16 0.25 0.25 0.32 0.28 | 0.30        (hed_model.WIDE_CASES: blocks 1 to 4 in the window-in-LDS form)
(test_native_detector_matches_the_reference_records prints them; DESIGN.md section 12 has the table.)
"""
import copy
import os
import types
import warnings

import numpy as np
import pytest
import torch

import hed_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SCALE = 64.0


@pytest.fixture(scope="module")
def hed_golden():
    return M.load_golden(os.path.join(ROOT, "tests", "golden"))


@pytest.fixture(scope="module")
def net():
    import fresco_amd
    m = fresco_amd.ControlNetHED_Apache2()
    m.load_state_dict(M.standin_state_dict())
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def detector(net):
    import fresco_amd
    return fresco_amd.HEDdetector(network=net)


def _gpu(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _np64(t):
    return t.detach().to("cpu", torch.float64).numpy()


def _planes64(planes):
    return _np64(planes[0]) + _np64(planes[1])


def _plane_bound(v_scaled):
    return 2.0 ** -21 * np.abs(v_scaled) + 2.0 ** -25


# ---------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 7, 9), (1, 16, 12), (3, 5, 5)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_side_pool_matches_the_float64_restatement(C, shape):
    _check_side_pool(C, shape)


def test_side_pool_past_the_grid_cap():
    """194 x 193 quads = 2341 workgroups' worth against the cap of 2048: some workgroups take a second trip of the
    grid-stride loop, the last one with part of its quads outside the problem; odd H and W"""
    _check_side_pool(64, (1, 387, 385))


def _check_side_pool(C, shape):
    from fresco_amd import ops
    n, H, W = shape
    rs = np.random.RandomState(100 * C + 10 * H + W)
    h = (np.maximum(rs.standard_normal((n, H, W, C)), 0.0) * 60.0).astype(np.float32)  # post-ReLU, up to a few hundred
    w = (rs.standard_normal(C) * 0.05).astype(np.float32)
    b = np.array([0.3], np.float32)
    hg, wg, bg = _gpu(h.reshape(-1, C)), _gpu(w), _gpu(b)
    proj, planes = ops.hed_side_pool(hg, n, H, W, wg, bg, scale=SCALE)
    h64 = h.astype(np.float64)
    ref = h64 @ w.astype(np.float64) + float(b[0])
    bar = 4e-6 * (np.abs(h64) @ np.abs(w.astype(np.float64)))
    err = np.abs(_np64(proj) - ref)
    print("side %s C=%d: max |d| %.3g, worst error / bound %.3f" % (shape, C, err.max(), (err / bar).max()))
    assert proj.shape == (n, H, W) and np.all(err <= bar)
    PH, PW = H // 2, W // 2
    pooled = h64[:, :2 * PH, :2 * PW].reshape(n, PH, 2, PW, 2, C).max(axis=(2, 4)) * SCALE
    got = _planes64(planes).reshape(n, PH, PW, C)
    assert planes[0].dtype == torch.float16 and planes[0].shape == (n * PH * PW, C)
    perr = np.abs(got - pooled)
    print("pool %s C=%d: worst error / bound %.3f" % (shape, C, (perr / _plane_bound(pooled)).max()))
    assert np.all(perr <= _plane_bound(pooled))
    # each output alone, and a second run of both: the same bits
    proj_only, none = ops.hed_side_pool(hg, n, H, W, wg, bg, want_pool=False)
    none2, planes_only = ops.hed_side_pool(hg, n, H, W, wg, bg, want_proj=False, scale=SCALE)
    proj2, planes2 = ops.hed_side_pool(hg, n, H, W, wg, bg, scale=SCALE)
    assert none is None and none2 is None
    for a in (proj_only, proj2):
        assert torch.equal(a, proj)
    for a in (planes_only, planes2):
        assert torch.equal(a[0], planes[0]) and torch.equal(a[1], planes[1])
    # no bias pointer: the plain dot product
    proj0, _ = ops.hed_side_pool(hg, n, H, W, wg, None, want_pool=False)
    assert np.all(np.abs(_np64(proj0) - (ref - float(b[0]))) <= bar)


def test_side_pool_flags_values_beyond_the_planes():
    from fresco_amd import ops
    h = torch.full((4 * 4, 64), 2000.0, device=DEV)
    w = torch.zeros(64, device=DEV)
    with ops.fn_range_guard(h.device) as g:
        ops.hed_side_pool(h, 1, 4, 4, w, scale=SCALE)  # 2000 * 64 > 65000
    assert g.tripped()
    with ops.fn_range_guard(h.device) as g:
        ops.hed_side_pool(h, 1, 4, 4, w, scale=16.0)
    assert not g.tripped()


def test_input_planes():
    _check_input_planes(2, 17, 19)


def _check_input_planes(n, H, W):
    from fresco_amd import ops
    rs = np.random.RandomState(5)
    x = rs.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    x[0, 0, 0] = (0, 255, 128)
    norm = np.array(M.NORM, np.float32)
    hi, lo = ops.hed_input(_gpu(x), _gpu(norm), scale=SCALE)
    assert hi.shape == (n * H * W, 32) and hi.dtype == torch.float16 and lo.shape == hi.shape
    got = _np64(hi) + _np64(lo)
    ref = (x.astype(np.float64) - norm.astype(np.float64)).reshape(-1, 3) * SCALE
    assert np.all(np.abs(got[:, :3] - ref) <= _plane_bound(ref))
    assert not hi[:, 3:].any() and not lo[:, 3:].any()


def test_input_planes_past_the_grid_cap():
    """369 x 367 pixels x 4 pieces = 2116 workgroups' worth against the cap of 2048"""
    _check_input_planes(1, 369, 367)


def _fuse64(sides, H, W):
    """float64 restatement of fresco_hed_fuse's mean for one frame: cv2's source positions (formed in double, rounded to
    float, clamped), the interpolation and the mean in float64"""
    def taps(dst, src):
        f = ((np.arange(dst, dtype=np.float64) + 0.5) * (float(src) / float(dst)) - 0.5).astype(np.float32)
        i0 = np.floor(f).astype(np.int64)
        f = (f - i0.astype(np.float32)).astype(np.float32)
        f[i0 < 0] = 0
        i0[i0 < 0] = 0
        f[i0 >= src - 1] = 0
        i0[i0 >= src - 1] = src - 1
        return i0, np.minimum(i0 + 1, src - 1), f.astype(np.float64)
    total = 0.0
    for p in sides:
        p = np.asarray(p, np.float64)
        if p.shape != (H, W):
            y0, y1, fy = taps(H, p.shape[0])
            x0, x1, fx = taps(W, p.shape[1])
            r0 = p[y0][:, x0] * (1 - fx) + p[y0][:, x1] * fx
            r1 = p[y1][:, x0] * (1 - fx) + p[y1][:, x1] * fx
            p = r0 * (1 - fy[:, None]) + r1 * fy[:, None]
        total = total + p
    return total / 5.0


def test_fuse_past_the_grid_cap():
    """737 x 735 pixels = 2116 workgroups' worth against the cap of 2048, odd sizes at every level; random side maps"""
    from fresco_amd import ops
    H, W = 737, 735
    rs = np.random.RandomState(11)
    sides = [rs.standard_normal((1, h, w)).astype(np.float32) for h, w in M.level_sizes(H, W)]
    u8, logit, cond = ops.hed_fuse([_gpu(t) for t in sides], want_logit=True, cond_dtype=torch.float32)
    ref = _fuse64([t[0] for t in sides], H, W)
    err = np.abs(_np64(logit[0]) - ref)
    bar = 2e-6 + 2e-6 * np.abs(ref)
    print("fuse %d x %d: max |d| %.3g, worst error / bound %.3f" % (H, W, err.max(), (err / bar).max()))
    assert np.all(err <= bar)
    want = np.clip(255.0 / (1.0 + np.exp(-ref)), 0.0, 255.0).astype(np.uint8)
    M.check_u8(u8[0].cpu().numpy(), want, ref, "fuse %d x %d" % (H, W))
    c = ((u8[0].float() / 255.0 * 2.0 - 1.) * 0.5 + 0.5)
    assert tuple(cond.shape) == (1, 3, H, W) and all(torch.equal(cond[0, ch], c) for ch in range(3))


@pytest.mark.parametrize("case", M.CASES + M.WIDE_CASES, ids=M.case_key)
def test_fuse_on_the_reference_side_maps(hed_golden, case):
    from fresco_amd import ops
    n, H, W = case
    nf = M.GOLDEN_FRAMES[case]
    recs = [M.golden_sides(hed_golden, case, f) for f in range(nf)]
    sides = [_gpu(np.stack([r[0][k] for r in recs], 0)) for k in range(5)]
    u8, logit, cond = ops.hed_fuse(sides, want_logit=True)
    assert cond is None and u8.dtype == torch.uint8 and u8.shape == (nf, H, W)
    u8_only = ops.hed_fuse(sides)[0]
    assert torch.equal(u8_only, u8)
    for f in range(nf):
        l64 = recs[f][3]  # the golden's float64 fused logit
        same = M.fuse_logit64(recs[f][0], H, W)  # a float64 fuse of the very maps the kernel was given
        for name, ref in (("golden fp64 logit", l64), ("fp64 fuse of the same maps", same)):
            err = np.abs(_np64(logit[f]) - ref)
            bar = 2e-6 + 2e-6 * np.abs(ref)
            print("%s frame %d vs %s: max |d| %.3g, worst error / bound %.3f" % (M.case_key(case), f, name, err.max(),
                                                                                (err / bar).max()))
            assert np.all(err <= bar), name
        M.check_u8(u8[f].cpu().numpy(), recs[f][4], l64, "%s frame %d" % (M.case_key(case), f))


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES + M.WIDE_CASES, ids=M.case_key)
def test_native_detector_matches_the_reference_records(hed_golden, net, case):
    n, H, W = case
    frames = _gpu(M.frames(case))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the stand-in network stays inside the planes' range: no fallback, no warning
        sides = net.side_maps(frames)
        u8, logit, _ = net.detect(frames, want_logit=True)
    assert [tuple(s.shape) for s in sides] == [(n,) + hw for hw in M.level_sizes(H, W)]
    for f in range(M.GOLDEN_FRAMES[case]):
        p32, p64, l32, l64, ref_u8 = M.golden_sides(hed_golden, case, f)
        pairs = [("side %d" % (k + 1), _np64(sides[k][f]), p32[k], p64[k]) for k in range(5)]
        pairs.append(("fused logit", _np64(logit[f]), l32, l64))
        for name, got, r32, r64 in pairs:
            e_ref = np.abs(r32.astype(np.float64) - r64).max()
            err = np.abs(got - r64).max()
            bar = 8.0 * e_ref + 1e-7
            print("%s frame %d %s: native %.3g, reference fp32 %.3g, native / bar %.3f"
                  % (M.case_key(case), f, name, err, e_ref, err / bar))
            assert err <= bar, (name, err, bar)
        M.check_u8(u8[f].cpu().numpy(), ref_u8, l64, "%s frame %d" % (M.case_key(case), f))


def test_lowered_split_scales_hold_the_same_bar(hed_golden, net):
    """the documented remedy for a network that overflows the planes: other powers of two per block, through the
    convolutions (a_scale / out_scale) and the pooled planes written with the next block's scale"""
    case = (1, 72, 88)
    low = copy.deepcopy(net)
    low.split_scales = (64.0, 32.0, 32.0, 16.0, 16.0)
    frames = _gpu(M.frames(case))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sides = low.side_maps(frames)
        u8, logit, _ = low.detect(frames, want_logit=True)
    p32, p64, l32, l64, ref_u8 = M.golden_sides(hed_golden, case, 0)
    pairs = [("side %d" % (k + 1), _np64(sides[k][0]), p32[k], p64[k]) for k in range(5)]
    pairs.append(("fused logit", _np64(logit[0]), l32, l64))
    for name, got, r32, r64 in pairs:
        e_ref = np.abs(r32.astype(np.float64) - r64).max()
        err = np.abs(got - r64).max()
        print("scales (64, 32, 32, 16, 16) %s: native %.3g, native / bar %.3f" % (name, err, err / (8.0 * e_ref + 1e-7)))
        assert err <= 8.0 * e_ref + 1e-7, (name, err)
    M.check_u8(u8[0].cpu().numpy(), ref_u8, l64, "scales (64, 32, 32, 16, 16)")


def test_library_ops_switch_runs_the_same_module(hed_golden, net):
    """library_ops=True is the A/B baseline: PyTorch's convolutions, this package's fuse -- the same records, fp32 bound"""
    case = (1, 72, 88)
    lib = copy.deepcopy(net)
    lib.library_ops = True
    frames = _gpu(M.frames(case))
    u8, logit, _ = lib.detect(frames, want_logit=True)
    p32, p64, l32, l64, ref_u8 = M.golden_sides(hed_golden, case, 0)
    e_ref = np.abs(l32.astype(np.float64) - l64).max()
    assert np.abs(_np64(logit[0]) - l64).max() <= 8.0 * e_ref + 1e-7
    M.check_u8(u8[0].cpu().numpy(), ref_u8, l64, "library ops")


# ---------------------------------------------------------------------------------------------------------------
# protocol
# ---------------------------------------------------------------------------------------------------------------
def test_call_protocol_and_condition(detector):
    fr = M.frames((2, 64, 64))
    batch = detector.detect_batch([fr[0], fr[1]])
    assert batch.dtype == torch.uint8 and batch.is_cuda and tuple(batch.shape) == (2, 64, 64)
    assert torch.equal(detector.detect_batch(_gpu(fr)), batch)
    for f in range(2):
        e = detector(fr[f])
        assert isinstance(e, np.ndarray) and e.dtype == np.uint8 and e.shape == (64, 64)
        assert np.array_equal(e, batch[f].cpu().numpy())
    # run_fresco.py:199-202 on the edge maps, evaluated by PyTorch on the device as the reference does
    ref = torch.cat([(batch[f].float() / 255.0 * 2.0 - 1.)[None, None] for f in range(2)], 0).repeat(1, 3, 1, 1) * 0.5 + 0.5
    c32 = detector.control_image(_gpu(fr), torch.float32, guidance=False)
    assert c32.dtype == torch.float32 and tuple(c32.shape) == (2, 3, 64, 64) and torch.equal(c32, ref)
    c16 = detector.control_image([fr[0], fr[1]], torch.float16)
    assert c16.dtype == torch.float16 and tuple(c16.shape) == (4, 3, 64, 64)
    assert torch.equal(c16, torch.cat([ref.to(torch.float16)] * 2))
    cb = detector.control_image(_gpu(fr), torch.bfloat16, guidance=False)
    assert torch.equal(cb, ref.to(torch.bfloat16))


def test_chunked_batch_equals_single_frames(net):
    """three frames two at a time against each alone: chunking, and nothing leaks across the image borders of a batch
    (72 x 88: the convolutions' 256-row blocks straddle the frames)"""
    fr = _gpu(M.frames((3, 72, 88)))
    chunked = copy.deepcopy(net)
    chunked.max_frames = 2
    u8, logit, _ = chunked.detect(fr, want_logit=True)
    assert tuple(u8.shape) == (3, 72, 88)
    for f in range(3):
        u1, l1, _ = net.detect(fr[f:f + 1], want_logit=True)
        assert torch.equal(u1[0], u8[f]) and torch.equal(l1[0], logit[f])


def test_patch_hed_rebinds_the_detector(net):
    import fresco_amd
    stand_in = types.ModuleType("annotator.hed")
    stand_in.HEDdetector = None
    fresco_amd.patch_hed(stand_in)
    det = stand_in.HEDdetector(network=net)
    assert isinstance(det, fresco_amd.HEDdetector)
    assert det(M.frames((1, 64, 128))[0]).shape == (64, 128)


# ---------------------------------------------------------------------------------------------------------------
# range policy
# ---------------------------------------------------------------------------------------------------------------
def test_out_of_range_activations_fall_back_to_library_ops(net):
    hot = copy.deepcopy(net)
    with torch.no_grad():
        for conv in hot.block1.convs:
            conv.weight.mul_(8.0)  # activations from block 1 on are 64 x larger: far beyond 65000 / 64
        for blk in hot.blocks:
            blk.projection.weight.div_(64.0)  # ... and the logits stay where they were: the uint8 map keeps its levels
    lib = copy.deepcopy(hot)
    lib.library_ops = True
    fr = _gpu(M.frames((1, 64, 128)))
    with pytest.warns(RuntimeWarning, match="library ops"):
        u8, logit, _ = hot.detect(fr, want_logit=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once per module
        u8b, _, _ = hot.detect(fr)
        want_u8, want_logit, _ = lib.detect(fr, want_logit=True)
        again_u8, again_logit, _ = lib.detect(fr, want_logit=True)
    # Seen on an MI355X: the library's convolutions do not repeat bit for bit -- two runs of the SAME library_ops module on
    # the same input differ in the logits' last bits, and so does the fallback against it (max |d| 9.5e-7 here).  Both are
    # fp32 evaluations of one network, each within the reference's own fp32-vs-fp64 distance of the exact result -- 1.2e-6
    # on logits of magnitude 3.5 in the golden, 3.4e-7 relative -- so they lie within twice that of each other, and the
    # uint8 maps obey the guard-band rule.  Saturated planes would be off by orders of magnitude.
    print("library_ops module, two runs: logits %s" % ("equal" if torch.equal(again_logit, want_logit) else "differ"))
    assert torch.isfinite(logit).all() and len(torch.unique(want_u8)) >= 64
    bound = 2 * 3.4e-7 * float(want_logit.abs().max())
    d = float((logit - want_logit).abs().max())
    print("fallback vs library_ops: logits %s, max |d| %.3g, bound %.3g"
          % ("equal" if torch.equal(logit, want_logit) else "differ", d, bound))
    assert d <= bound
    for got in (u8, u8b):
        M.check_u8(got[0].cpu().numpy(), want_u8[0].cpu().numpy(), _np64(want_logit[0]), "fallback vs library_ops")
