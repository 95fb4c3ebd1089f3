"""GPU tests of the video_blend backend (fresco_amd.blend, csrc/blend.hip) past the shapes and contents of
test_gpu_blend.py: frames larger than 512^2 (where the pixel kernels' grid-stride loops take a second trip and
blend_tables' too), the smallest and the largest sides, clipped gradients and saturated solutions, constant channels,
mask bytes other than 0 / 1, distinct gradient weights, exact fixed points of the Poisson solve up to 4096^2, and the
host boundary (workspace reuse, views, streams).

The bars are test_gpu_blend.py's: mask equal to the model; histogram Lab within 1 LSB and >= 99.9 % equal; Poisson Lab
within 1 LSB and >= 99.5 % equal per channel (poisson_bars); whole frames through lab_neighbour_ok with at most 1.8 % of
pixels differing.  Where poisson_bars is given the model's float64 solution x it leaves out values whose x lies within
2e-3 of an integer; such a case first asserts, on the model alone, that at most 2 % per channel is left out (0.37 -
0.48 % on the non-degenerate frames tried on the CPU).  Channels that are degenerate by construction (weight 0,
constant channels, fixed points) are asserted for equality with the known bytes instead.  Every case that exists to
reach a branch asserts on the model's side that its input reaches it before the GPU result is looked at.

Inputs whose blended channel would be constant only because the two transfers cancel (correlation -1 at equal
weights) are ill-conditioned in the model and in the kernel alike and are kept out."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import blend_model as M  # noqa: E402
import make_blend_golden as G  # noqa: E402
from test_blend_cpu import poisson_bars  # noqa: E402
from test_gpu_blend import cpu, gpu, lab_neighbour_ok  # noqa: E402

from fresco_amd import blend as B  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.uint64


# ---------------------------------------------------------------------------------------------------------------------
# inputs (integer hashes, as in make_blend_golden.py)
# ---------------------------------------------------------------------------------------------------------------------
def hash_mask(seed, h, w, values=(0, 0, 0, 0, 0, 0, 0, 1, 1, 1)):
    """uint8 (h, w): values[hash % len(values)]"""
    return np.asarray(values, np.uint8)[(G._noise(seed, (h, w)) % U(len(values))).astype(np.int64)]


def blocks(seed, h, w, cell=8):
    """8-px blocks by hash: half of them black, white, pure red or pure blue; the others 0, 255 or texture per
    channel"""
    by, bx = (h + cell - 1) // cell, (w + cell - 1) // cell

    def up(k):
        return np.repeat(np.repeat(k, cell, 0), cell, 1)[:h, :w]

    kind = up((G._noise(seed, (by, bx, 3)) % U(4)).astype(np.int64))
    out = np.where(kind == 0, 0, np.where(kind == 1, 255, G.image(seed + 1, h, w))).astype(np.uint8)
    whole = up((G._noise(seed + 5, (by, bx)) % U(8)).astype(np.int64))
    for k, colour in enumerate(((0, 0, 0), (255, 255, 255), (0, 0, 255), (255, 0, 0))):
        out[whole == k] = colour
    return out


def black_and_white(seed, h, w, cell=8):
    k = (G._noise(seed, ((h + cell - 1) // cell, (w + cell - 1) // cell)) % U(2)).astype(np.uint8) * np.uint8(255)
    return np.ascontiguousarray(np.repeat(np.repeat(np.repeat(k, cell, 0), cell, 1)[:h, :w, None], 3, -1))


def grey(img):
    return np.ascontiguousarray(np.repeat(img[..., 1:2], 3, -1))


def flat(h, w, bgr=(40, 120, 200)):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(bgr, np.uint8), (h, w, 3)))


@functools.lru_cache(maxsize=2)
def band_noise(h, w):
    """band-limited noise: hashed values on a 6-px grid, bilinear in between, all of 0..255 in every channel"""
    return np.clip(G.smooth(31, h, w, 3, 6) // 4, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=2)
def flats_and_ramps(h, w):
    """high contrast: 300-px flats of 0 and of 255 joined by 100-px ramps along x + y / 2, the three channels out of
    phase so that the ramps are coloured; L runs from 0 to 255"""
    t = (np.arange(w, dtype=np.int32)[None, :] + (np.arange(h, dtype=np.int32) // 2)[:, None])
    out = np.empty((h, w, 3), np.uint8)
    for c, off in enumerate((0, 37, 90)):
        u = (t + off) % 800
        out[..., c] = np.minimum(np.clip((u - 300) * 255 // 100, 0, 255), np.clip((800 - u) * 255 // 100, 0, 255))
    return out


def frame_inputs(seed, h, w, make=G.image):
    return dict(oa=make(10 * seed, h, w), ob=make(10 * seed + 3, h, w), d1=G.error_map(10 * seed + 6, h, w),
                d2=G.error_map(10 * seed + 7, h, w), prev=hash_mask(10 * seed + 8, h, w),
                flow=G.flow_field(10 * seed + 9, h, w))


# ---------------------------------------------------------------------------------------------------------------------
# what the model says about an input, and the bars
# ---------------------------------------------------------------------------------------------------------------------
def raw_steps(I1, I2, mask):
    """poisson_fusion's forward differences before the clip (int, zero on the last row / column)"""
    la, lb = M.bgr_to_lab(I1).astype(int), M.bgr_to_lab(I2).astype(int)
    m = (np.asarray(mask) > 0)[..., None]
    gx, gy = np.zeros_like(la), np.zeros_like(la)
    gx[:-1] = np.where(m[:-1], lb[:-1] - lb[1:], la[:-1] - la[1:])
    gy[:, :-1] = np.where(m[:, :-1], lb[:, :-1] - lb[:, 1:], la[:, :-1] - la[:, 1:])
    return gx, gy


def clipped_share(I1, I2, mask):
    gx, gy = raw_steps(I1, I2, mask)
    return float(((np.abs(gx) > 100).sum() + (np.abs(gy) > 100).sum()) / (2.0 * gx.size))


def left_out_within_cap(x, channels=(0, 1, 2)):
    """the share of values poisson_bars(got, ref, x) leaves out, from the model alone: at most 2 % per channel"""
    share = [float((np.abs(x[..., c] - np.round(x[..., c])) < 2e-3).mean()) for c in channels]
    assert all(v <= 0.02 for v in share), share
    return share


def hist_bars(got, want):
    d = np.abs(got.astype(int) - want.astype(int))
    eq = float((d == 0).mean())
    assert d.max() <= 1 and eq >= 0.999, (int(d.max()), eq)
    return eq


def run_frame(f, weight1, **kw):
    img, mask = B.blend_frame(gpu(f["oa"]), gpu(f["ob"]), gpu(f["d1"]), gpu(f["d2"]), weight1, gpu(f["prev"]),
                              gpu(f["flow"]), **kw)
    return cpu(img), cpu(mask)


def check_frame(f, weight1, tag, x=None, exact=(), degenerate=(), ref=None):
    """whole blend_frame and its two stages on the model's intermediates against M.blend_frame.  x: the model's float64
    Poisson solution for poisson_bars; exact: channels whose Poisson bytes must equal the model's everywhere;
    degenerate: channels where much of x is an integer by construction, so the 99.5 % counts every value, none left
    out (the guard is there to make exactly those truncate like the model)."""
    if ref is None:
        ref = M.blend_frame(f["oa"], f["ob"], f["d1"], f["d2"], weight1, f["prev"], f["flow"])
    img, mask = run_frame(f, weight1)
    assert np.array_equal(mask, ref["mask"]), tag
    me = M.min_error_image(f["oa"], f["ob"], ref["mask"])
    hw1, hw2 = 1 - weight1, 1 - (1 - weight1)
    out, lab = B.histogram_blend(gpu(f["oa"]), gpu(f["ob"]), gpu(me), hw1, hw2, return_lab=True)
    eq_h = hist_bars(cpu(lab), ref["hist_lab"])
    assert np.array_equal(cpu(out), M.lab_to_bgr(cpu(lab))), tag
    out, lab = B.poisson_fusion(gpu(ref["hist"]), gpu(f["oa"]), gpu(f["ob"]), gpu(ref["mask"]), return_lab=True)
    lab = cpu(lab)
    eq_p, eq_kept = poisson_bars(lab, ref["poisson_lab"], x)
    for c in exact:
        assert np.array_equal(lab[..., c], ref["poisson_lab"][..., c]), (tag, c)
    for c in degenerate:
        assert eq_p[c] >= 0.995, (tag, c, eq_p)
    assert np.array_equal(cpu(out), M.lab_to_bgr(lab)), tag
    frac = lab_neighbour_ok(img, ref["poisson_lab"])
    print("%s: histogram Lab equal %.5f, Poisson Lab equal %s (well-defined %s), %.4f %% of the frame's pixels differ"
          % (tag, eq_h, np.round(eq_p, 5).tolist(), np.round(eq_kept, 5).tolist(), 100 * frac))
    assert frac <= 0.018, (tag, frac)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(512, 896), (896, 512), (2, 2), (2, 67), (65, 2), (3, 130), (2, 4096), (4096, 2)])
def test_frame_sizes(h, w):
    """512 x 896: blend_prep / blend_rhs take a second, partly filled grid-stride trip and blend_tables too (32 at a
    side of 4096); sides of 2 and 3: K = 2 in the GEMMs and one partly filled tile.  (512^2 sits exactly on both launch
    caps of a 256-CU device: 4 x CUs workgroups of 256 pixels, and 2048 workgroups for the 2 x 512^2 table entries.)"""
    check_frame(frame_inputs(40 + (h * 7 + w) % 50, h, w), 0.4, "%dx%d" % (h, w))


def test_propagated_mask_above_512():
    """the warp reads q % w and q / w inside the strided loop: exact against the model's restatement at 600 x 1000,
    with previous-mask bytes other than 0 / 1 carried through"""
    h, w = 600, 1000
    for values in ((0, 0, 1), (0, 1, 2, 255)):
        prev = hash_mask(77, h, w, values)
        flow = G.flow_field(78, h, w)
        z = gpu(np.zeros((h, w), np.float32))
        img = gpu(np.zeros((h, w, 3), np.uint8))
        _, got = B.blend_frame(img, img, z, z, 0.0, gpu(prev), gpu(flow), gradient=False)
        want = M.warp_nearest(prev, flow)
        assert len(np.unique(want)) == len(set(values))
        assert np.array_equal(cpu(got), want), values


# ---------------------------------------------------------------------------------------------------------------------
# content
# ---------------------------------------------------------------------------------------------------------------------
CONTENT_SIZES = [(200, 328), (512, 896)]


@pytest.mark.parametrize("h,w", CONTENT_SIZES)
def test_blocky_frame_clips_and_saturates(h, w):
    """8-px blocks of black / white / red / blue / 0 / 255 / texture: gradients at the +-100 clip, L solutions beyond
    both ends of the byte range, and a histogram transfer that saturates L at both ends"""
    f = frame_inputs(61, h, w, blocks)
    ref = M.blend_frame(f["oa"], f["ob"], f["d1"], f["d2"], 0.4, f["prev"], f["flow"])
    share = clipped_share(f["oa"], f["ob"], ref["mask"])
    assert share >= 0.01, share
    x = M.poisson_solution(ref["hist"], f["oa"], f["ob"], ref["mask"])
    # beyond a whole level at both ends: a conversion that wraps or saturates differently from the clamp shows
    assert x[..., 0].min() <= -1.5 and x[..., 0].max() >= 256.5, (x[..., 0].min(), x[..., 0].max())
    me = M.min_error_image(f["oa"], f["ob"], ref["mask"])
    v = M.histogram_blend_values(f["oa"], f["ob"], me, 1 - 0.4, 1 - (1 - 0.4))[..., 0]
    assert (v < -0.5).mean() >= 1e-3 and (v > 255.5).mean() >= 1e-3, ((v < -0.5).mean(), (v > 255.5).mean())
    left_out_within_cap(x)
    print("%dx%d blocky: %.2f %% of gradients clipped, L solutions in [%.1f, %.1f]" % (h, w, 100 * share,
                                                                                        x[..., 0].min(), x[..., 0].max()))
    check_frame(f, 0.4, "%dx%d blocky" % (h, w), x, ref=ref)


def test_poisson_solutions_far_outside_the_byte_range():
    """black and white blocks under the gradients of two unrelated blocky images: the L solution leaves [0, 255] by
    tens of levels at both ends (one clamp serves L, a and b), and the clip decides many gradients"""
    h, w = 200, 328
    blend, i1, i2 = black_and_white(71, h, w), blocks(72, h, w), blocks(73, h, w)
    mask = hash_mask(74, h, w)
    x = M.poisson_solution(blend, i1, i2, mask)
    assert x.min() <= -1.5 and x.max() >= 256.5, (x.min(), x.max())
    assert clipped_share(i1, i2, mask) >= 0.01
    left_out_within_cap(x)
    _, lab = B.poisson_fusion(gpu(blend), gpu(i1), gpu(i2), gpu(mask), return_lab=True)
    eq, eq_kept = poisson_bars(cpu(lab), M.poisson_fusion_lab(blend, i1, i2, mask), x)
    print("blocky Poisson, solutions in [%.1f, %.1f]: equal %s" % (x.min(), x.max(), np.round(eq, 5).tolist()))


def test_histogram_transfer_saturates_a_and_b():
    """a min-error image of saturated colours has a far larger a / b spread than the textured propagations, so the
    transfer's outliers leave the byte range in a and b at both ends"""
    h, w = 200, 328
    a, b = G.image(81, h, w), G.image(84, h, w)
    k = np.repeat(np.repeat((G._noise(85, (h // 8, w // 8)) % U(4)).astype(np.int64), 8, 0), 8, 1)
    me = np.asarray([(0, 0, 255), (0, 255, 0), (255, 0, 0), (0, 255, 255)], np.uint8)[k]
    v = M.histogram_blend_values(a, b, me, 0.6, 0.4)
    for c in (1, 2):
        assert (v[..., c] < -0.5).any() and (v[..., c] > 255.5).any(), (c, v[..., c].min(), v[..., c].max())
    _, lab = B.histogram_blend(gpu(a), gpu(b), gpu(me), 0.6, 0.4, return_lab=True)
    hist_bars(cpu(lab), M.histogram_blend_lab(a, b, me, 0.6, 0.4))


def constant_case(name, h, w):
    f = frame_inputs(91, h, w)
    if name == "grey":
        f["oa"], f["ob"] = grey(f["oa"]), grey(f["ob"])
        return f, (1, 2), (1, 2)
    if name == "half_grey":
        f["oa"] = grey(f["oa"])
        return f, (1, 2), ()
    if name == "flat":
        f["oa"] = flat(h, w)
        return f, (0, 1, 2), ()
    raise KeyError(name)


@pytest.mark.parametrize("name,weight1,h,w", [("grey", 0.4, 200, 328), ("grey", 0.4, 512, 896),
                                              ("half_grey", 0.4, 200, 328), ("half_grey", 0.4, 512, 896),
                                              ("flat", 0.0, 200, 328), ("flat", 0.4, 200, 328), ("flat", 1.0, 200, 328),
                                              ("flat", 0.4, 512, 896)])
def test_constant_channels(name, weight1, h, w):
    """Channels with std 0 (what a black-and-white video gives: every grey BGR has Lab a = b = 128) transfer to the
    target mean.  Where oa and ob are both constant in a channel the histogram blend is the min-error image's mean in
    every value and the Poisson solution is that constant, so the bytes are known and must be equal."""
    f, const_a, const_ab = constant_case(name, h, w)
    la, lb = M.bgr_to_lab(f["oa"]), M.bgr_to_lab(f["ob"])
    ca, cb = M.constant_channels(la), M.constant_channels(lb)
    assert tuple(np.nonzero(ca)[0]) == const_a and tuple(np.nonzero(ca & cb)[0]) == const_ab, (ca, cb)
    ref = M.blend_frame(f["oa"], f["ob"], f["d1"], f["d2"], weight1, f["prev"], f["flow"])
    x = M.poisson_solution(ref["hist"], f["oa"], f["ob"], ref["mask"])
    for c in const_ab:
        assert (ref["hist_lab"][..., c] == 128).all() and (ref["poisson_lab"][..., c] == 128).all()
    if name == "flat" and weight1 == 0.0:
        # mask all 0 but for the propagated part; ab is constant in all three channels (ob carries weight 0)
        assert all(len(np.unique(ref["hist_lab"][..., c])) == 1 for c in range(3))
    # flat oa at weight1 = 0: a constant histogram blend under zero gradients wherever the mask is 0; at weight1 = 1 the
    # histogram blend is Lab(ob) under ob's own gradients: integer solutions over much of the frame by construction
    degenerate = (0, 1, 2) if name == "flat" and weight1 in (0.0, 1.0) else ()
    left_out_within_cap(x, [c for c in range(3) if c not in const_ab and c not in degenerate])
    check_frame(f, weight1, "%dx%d %s w1=%g" % (h, w, name, weight1), x, exact=tuple(const_ab), degenerate=degenerate,
                ref=ref)


@pytest.mark.parametrize("h,w", CONTENT_SIZES)
def test_equal_propagations(h, w):
    """oa is ob: correlation 1, the blend's std is the transfer's std and the histogram blend returns Lab(oa)"""
    f = frame_inputs(95, h, w)
    f["ob"] = f["oa"]
    ref = M.blend_frame(f["oa"], f["ob"], f["d1"], f["d2"], 0.4, f["prev"], f["flow"])
    assert np.array_equal(ref["hist_lab"], M.bgr_to_lab(f["oa"]))
    check_frame(f, 0.4, "%dx%d equal" % (h, w), ref=ref)


def test_mask_bytes_above_one_select_the_second_image():
    """poisson_fusion takes I2's gradients where mask > 0, and blend_frame's mask ORs warped bytes in: masks drawn from
    {0, 1, 2, 255}"""
    h, w = 200, 328
    values = (0, 0, 1, 2, 255)
    f = frame_inputs(101, h, w)
    mask = hash_mask(102, h, w, values)
    assert set(np.unique(mask)) == {0, 1, 2, 255}
    blend = G.image(103, h, w)
    x = M.poisson_solution(blend, f["oa"], f["ob"], mask)
    assert np.abs(x - M.poisson_solution(blend, f["oa"], f["ob"], (mask == 1).astype(np.uint8))).max() > 1
    left_out_within_cap(x)
    _, lab = B.poisson_fusion(gpu(blend), gpu(f["oa"]), gpu(f["ob"]), gpu(mask), return_lab=True)
    poisson_bars(cpu(lab), M.poisson_fusion_lab(blend, f["oa"], f["ob"], mask), x)
    f["prev"] = mask
    ref = M.blend_frame(f["oa"], f["ob"], f["d1"], f["d2"], 0.4, f["prev"], f["flow"])
    assert (ref["mask"] > 1).mean() > 0.05
    img, got_mask = run_frame(f, 0.4)
    assert np.array_equal(got_mask, ref["mask"])
    assert lab_neighbour_ok(img, ref["poisson_lab"]) <= 0.018


@pytest.mark.parametrize("gw", [(0.0, 1.5, 3.0), (3.0, 0.0, 1.5)])
def test_distinct_gradient_weights(gw):
    """three distinct weights, each channel against the model with its own; at weight 0 the solve is the identity and
    the guard makes the truncation exact: the channel equals Lab(blendI) in every byte"""
    h, w = 200, 328
    blend, i1, i2 = G.image(111, h, w), G.image(112, h, w), G.image(113, h, w)
    mask = hash_mask(114, h, w)
    x = M.poisson_solution(blend, i1, i2, mask, gw)
    zero = gw.index(0.0)
    left_out_within_cap(x, [c for c in range(3) if c != zero])
    want = M.poisson_fusion_lab(blend, i1, i2, mask, gw)
    assert np.array_equal(want[..., zero], M.bgr_to_lab(blend)[..., zero])
    # the model itself tells the weights apart: swapping a and b's moves more than the bars allow
    swapped = M.poisson_fusion_lab(blend, i1, i2, mask, (gw[0], gw[2], gw[1]))
    assert (swapped[..., 1:] != want[..., 1:]).mean() > 0.05
    _, lab = B.poisson_fusion(gpu(blend), gpu(i1), gpu(i2), gpu(mask), grad_weight=gw, return_lab=True)
    lab = cpu(lab)
    eq, eq_kept = poisson_bars(lab, want, x)
    assert np.array_equal(lab[..., zero], want[..., zero])
    print("grad_weight %s: equal %s" % (gw, np.round(eq, 5).tolist()))


@pytest.mark.parametrize("weights", [(0.7, 0.6), (1.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("make", [G.image, blocks], ids=["smooth", "blocky"])
def test_histogram_weights(weights, make):
    """weights that do not sum to 1 move the blend's mean off 128 (204.8 at 0.7 + 0.6); a weight of 0 drops an image"""
    h, w = 200, 328
    a, b = make(121, h, w), make(124, h, w)
    me = M.min_error_image(a, b, hash_mask(125, h, w))
    _, lab = B.histogram_blend(gpu(a), gpu(b), gpu(me), weights[0], weights[1], return_lab=True)
    eq = hist_bars(cpu(lab), M.histogram_blend_lab(a, b, me, *weights))
    print("histogram weights %s: equal %.5f" % (weights, eq))


# ---------------------------------------------------------------------------------------------------------------------
# host boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_workspace_reuse_and_oversize():
    shapes = [(37, 53), (72, 56)]
    frames = [frame_inputs(131 + k, h, w) for k, (h, w) in enumerate(shapes)]

    def run(f, ws):
        return B.blend_frame(gpu(f["oa"]), gpu(f["ob"]), gpu(f["d1"]), gpu(f["d2"]), 0.4, gpu(f["prev"]),
                             gpu(f["flow"]), workspace=ws)

    fresh = [run(f, torch.empty(B.workspace_bytes(*s), dtype=torch.uint8, device="cuda"))
             for f, s in zip(frames, shapes)]
    shared = torch.full((max(B.workspace_bytes(*s) for s in shapes) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    for k in (0, 1, 0, 1):
        img, mask = run(frames[k], shared)
        assert torch.equal(img, fresh[k][0]) and torch.equal(mask, fresh[k][1]), k


def test_views_equal_their_contiguous_copies():
    h, w = 72, 56
    f = frame_inputs(141, h, w)
    base = B.blend_frame(gpu(f["oa"]), gpu(f["ob"]), gpu(f["d1"]), gpu(f["d2"]), 0.4, gpu(f["prev"]), gpu(f["flow"]))
    wide = np.zeros((h, 2 * w, 3), np.uint8)
    wide[:, ::2] = f["oa"]
    oa = gpu(wide)[:, ::2]
    d1 = gpu(np.ascontiguousarray(f["d1"].T)).t()
    flow = gpu(np.ascontiguousarray(f["flow"][0].transpose(1, 2, 0))).permute(2, 0, 1)
    prev = gpu(np.ascontiguousarray(f["prev"].T)).t()
    assert not (oa.is_contiguous() or d1.is_contiguous() or flow.is_contiguous() or prev.is_contiguous())
    assert flow.shape == (2, h, w)
    got = B.blend_frame(oa, gpu(f["ob"]), d1, gpu(f["d2"]), 0.4, prev, flow)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    lab = B.poisson_fusion(oa, oa, gpu(f["ob"]), prev)
    assert torch.equal(lab, B.poisson_fusion(gpu(f["oa"]), gpu(f["oa"]), gpu(f["ob"]), gpu(f["prev"])))
    assert torch.equal(B.histogram_blend(oa, gpu(f["ob"]), oa), B.histogram_blend(gpu(f["oa"]), gpu(f["ob"]), gpu(f["oa"])))


def test_side_stream_equals_default_stream():
    h, w = 200, 328
    f = frame_inputs(151, h, w)
    args = (gpu(f["oa"]), gpu(f["ob"]), gpu(f["d1"]), gpu(f["d2"]), 0.4, gpu(f["prev"]), gpu(f["flow"]))
    base = B.blend_frame(*args)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = B.blend_frame(*args)
    side.synchronize()
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


# ---------------------------------------------------------------------------------------------------------------------
# the largest frames: one HD frame against the model, and fixed points (the frame fused with its own gradients)
# ---------------------------------------------------------------------------------------------------------------------
def test_frame_1080x1920():
    """about 8 grid-stride trips; 1080 is a multiple of neither 64 nor 16"""
    check_frame(frame_inputs(47, 1080, 1920), 0.4, "1080x1920")


@pytest.mark.parametrize("h,w", [(512, 512), (1080, 1920), (2048, 2048), (4096, 4096)])
@pytest.mark.parametrize("content", [band_noise, flats_and_ramps], ids=["noise", "contrast"])
def test_fixed_point_is_exact(content, h, w):
    """poisson_fusion(I, I, I2, mask = 0) with every Lab step of I inside +-100 has the exact solution Lab(I), an
    integer everywhere: the returned Lab bytes equal bgr_to_lab(I), all of them, and the same with mask = 255 and the
    roles of I and I2 swapped.  The solve's error has to stay below the 1/1024 guard for that, at every size: with one
    fp32 fmaf chain over the whole of K the high-contrast frame came back one level low in 2 L bytes at 2048^2 and in
    18 815 at 4096^2 (on an MI355X), which is why blend_gemm sums its k-steps in fp64.
    At 2048^2 and above the Lab oracle is the device's bgr_to_lab (pinned over all 2^24 colours by
    test_lab_conversions_over_all_colours); below, the model's."""
    I = content(h, w)
    I2 = 255 - I[::-1]
    gI, gI2 = gpu(I), gpu(I2)
    want = B.bgr_to_lab(gI) if h * w >= 2048 * 2048 else gpu(M.bgr_to_lab(I))
    s = want.to(torch.int16)
    step = max(int((s[1:] - s[:-1]).abs().max()), int((s[:, 1:] - s[:, :-1]).abs().max()))
    assert step < 100, step
    assert int(s[..., 0].min()) <= 5 and int(s[..., 0].max()) >= 250  # L over the whole range
    for mask_value, i1, i2 in ((0, gI, gI2), (255, gI2, gI)):
        mask = torch.full((h, w), mask_value, dtype=torch.uint8, device=gI.device)
        _, lab = B.poisson_fusion(gI, i1, i2, mask, return_lab=True)
        torch.cuda.synchronize()
        bad = (lab != want)
        n_bad = int(bad.sum())
        low = int((lab.to(torch.int16) - s)[bad].min()) if n_bad else 0
        print("fixed point %s %dx%d mask %d: %d of %d bytes differ (lowest difference %d), largest Lab step %d"
              % (content.__name__, h, w, mask_value, n_bad, bad.numel(), low, step))
        assert n_bad == 0, (content.__name__, h, w, mask_value, n_bad, [int(v) for v in bad.sum((0, 1))])
