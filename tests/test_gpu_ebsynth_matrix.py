"""Ebsynth HIP backend against tests/ebsynth_model.py (this backend's `snapshot` schedule), bit for bit, over the branches
the kernels are specialised on: record width 1 and 2 (<= 16 and 17..32 style + guide channels), with and without a
modulation image, plain and weighted votes, the 3x3 extra pass, patch sizes 3 to 9, a target larger than the source on
one axis, 1 and 8 style channels, and per-level iteration counts and stop thresholds.

Every case uses distinct non-negative integer weights, with a 0 in every case of more than two channels, so a kernel
that reads the wrong weight slot changes E.  The patch error may be contracted to FMAs on the device; it stays exact only while every weighted product and
partial sum is an fp32 integer below 2^24.  `assert_exact_regime` checks that bound on the inputs before each run, and
`case_inputs` picks each channel's byte range from its weight so that the bound holds."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from fresco_amd import ebsynth_run

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ebsynth_model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT_LIMIT = 1 << 24


def smooth(rng, h, w, c, cell=6):
    """smooth noise in [0, 255]: uniform noise on a grid of `cell`-pixel cells, bilinearly upsampled"""
    g = torch.from_numpy(rng.uniform(0, 255, (1, c, h // cell + 2, w // cell + 2)).astype(np.float32))
    up = torch.nn.functional.interpolate(g, size=(h + 2 * cell, w + 2 * cell), mode="bilinear", align_corners=False)
    return up[0, :, cell:cell + h, cell:cell + w].permute(1, 2, 0).clamp(0, 255).to(torch.int64).numpy()


def banded(rng, h, w, lo, band):
    """smooth noise confined to [lo_c, lo_c + band_c] in channel c"""
    lo, band = np.asarray(lo), np.asarray(band)
    return (lo + smooth(rng, h, w, len(band)) * band // 255).astype(np.uint8)


def byte_range(*imgs):
    """per-channel max - min over all the images given"""
    hi = np.max([a.reshape(-1, a.shape[-1]).max(0) for a in imgs], 0).astype(np.int64)
    lo = np.min([a.reshape(-1, a.shape[-1]).min(0) for a in imgs], 0).astype(np.int64)
    return hi - lo


def assert_exact_regime(patch, ss, sg, tg, sw, gw, mod=None):
    """patch^2 * sum_c w_c * range_c^2 < 2^24, with integer weights: then every product w_c * d^2 and every partial sum of
    a patch error is an exact fp32 integer, contracted or not, at every level (coarse levels and votes stay within the
    finest images' byte ranges).  A modulation must be 0 or 255, so that mod / 255 is exactly 0 or 1."""
    w = np.asarray(list(sw) + list(gw), np.float64)
    assert np.all(w >= 0) and np.all(w == np.round(w)), "weights must be non-negative integers"
    if mod is not None:
        assert np.isin(mod, (0, 255)).all(), "modulation bytes must be 0 or 255"
    rng_ = np.concatenate([byte_range(ss), byte_range(sg, tg)]).astype(np.float64)
    total = patch * patch * float((w * rng_ * rng_).sum())
    assert total < EXACT_LIMIT, "patch error can reach %.0f >= 2^24: not exact in fp32" % total


# name: channels, source and target (h, w), ebsynth_run arguments.  Defaults: patch 5, uniformity 3500, the most levels.
CASES = {
    "rw1_16ch_weighted": dict(ns=3, ng=13, src=(48, 56), tgt=(40, 44),
                              kw=dict(search_vote_iters=2, patchmatch_iters=2, vote_mode="weighted")),
    "rw2_17ch": dict(ns=4, ng=13, src=(48, 56), tgt=(40, 44), kw=dict(search_vote_iters=2, patchmatch_iters=2)),
    "rw2_8x24_patch7_weighted": dict(ns=8, ng=24, src=(64, 72), tgt=(61, 53),
                                     kw=dict(patch_size=7, search_vote_iters=2, patchmatch_iters=2,
                                             vote_mode="weighted")),
    "rw1_1x1_patch3_no_uniformity": dict(ns=1, ng=1, src=(35, 29), tgt=(31, 38), zero_weight=False,
                                         kw=dict(patch_size=3, uniformity=0.0, search_vote_iters=3,
                                                 patchmatch_iters=2)),
    "rw1_patch9_side19": dict(ns=3, ng=3, src=(19, 23), tgt=(21, 19),
                              kw=dict(patch_size=9, pyramid_levels=1, search_vote_iters=2, patchmatch_iters=2)),
    "rw1_modulation": dict(ns=3, ng=4, src=(48, 56), tgt=(40, 44), mod=True,
                           kw=dict(search_vote_iters=2, patchmatch_iters=2)),
    "rw2_modulation_weighted_extra_pass": dict(ns=3, ng=18, src=(48, 56), tgt=(40, 44), mod=True,
                                               kw=dict(search_vote_iters=2, patchmatch_iters=1, vote_mode="weighted",
                                                       extra_pass_3x3=True)),
    "rw2_extra_pass": dict(ns=8, ng=12, src=(40, 36), tgt=(38, 42),
                           kw=dict(search_vote_iters=2, patchmatch_iters=1, extra_pass_3x3=True)),
    # target larger than the source along y, smaller along x; 3 levels: source 11x16, 22x33, 45x67, target 20x13,
    # 40x26, 81x53
    "rw2_target_larger_per_level": dict(ns=4, ng=14, src=(45, 67), tgt=(81, 53),
                                        kw=dict(search_vote_iters=[2, 2, 3], patchmatch_iters=[1, 1, 1],
                                                stop_threshold=[5, 5, 255], vote_mode="weighted")),
    # level 0: stop threshold 0 (every pixel searched again); level 1: no search/vote iteration; level 2: votes over
    # error passes only (no PatchMatch)
    "rw1_per_level": dict(ns=3, ng=4, src=(45, 67), tgt=(81, 53),
                          kw=dict(search_vote_iters=[3, 0, 3], patchmatch_iters=[2, 1, 0], stop_threshold=[0, 5, 255])),
}


def case_inputs(name):
    """Seeded inputs of one case.  Weights: a permutation of 1 .. n-1 with a 0 inserted before the last channel, whose
    bytes span 0..255 (without `zero_weight`: a permutation of 1 .. n).  So at 17 channels the one byte of the second
    record weighs, and at 32 the zero sits in the second record.  Every other channel's byte range is as wide as the
    exact-regime budget allows for its weight, at most 255.  Source and target guides share each channel's range; the
    modulation is 0 or 255 per byte."""
    c = CASES[name]
    ns, ng = c["ns"], c["ng"]
    n = ns + ng
    patch = c["kw"].get("patch_size", 5)
    rng = np.random.default_rng(sum(map(ord, name)))
    if c.get("zero_weight", True):
        w = np.insert(rng.permutation(np.arange(1, n)), n - 2, 0).astype(np.float64)
    else:
        w = rng.permutation(np.arange(1, n + 1)).astype(np.float64)
    budget = 0.98 * EXACT_LIMIT / (patch * patch * np.count_nonzero(w))
    band = np.array([255 if wc == 0 else min(255, int(math.sqrt(budget / wc))) for wc in w])
    lo = rng.integers(0, 256 - band)
    ss = banded(rng, *c["src"], lo[:ns], band[:ns])
    sg = banded(rng, *c["src"], lo[ns:], band[ns:])
    tg = banded(rng, *c["tgt"], lo[ns:], band[ns:])
    mod = (rng.random(c["tgt"] + (ng,)) < 0.7).astype(np.uint8) * 255 if c.get("mod") else None
    return dict(ss=ss, sg=sg, tg=tg, mod=mod, sw=[float(v) for v in w[:ns]], gw=[float(v) for v in w[ns:]], kw=c["kw"])


def run_model(ci, seed, stats):
    kw = ci["kw"]
    return ebsynth_model.run(ci["ss"], ci["sg"], ci["tg"], mod=ci["mod"], sw=ci["sw"], gw=ci["gw"],
                             uniformity=kw.get("uniformity", 3500.0), patch=kw.get("patch_size", 5),
                             vote_mode=kw.get("vote_mode", "plain"), levels=kw.get("pyramid_levels", -1),
                             svi=kw["search_vote_iters"], pmi=kw["patchmatch_iters"], stop=kw.get("stop_threshold", 5),
                             extra_pass_3x3=kw.get("extra_pass_3x3", False), seed=seed, omega="snapshot", stats=stats)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_matches_numpy_restatement_exactly(name):
    """NNF, E and image equal to the `snapshot` model.  With a uniformity term, some pixels must accept two or more
    candidates in one pass, where the occupancy of the moved patch matters."""
    ci = case_inputs(name)
    kw = ci["kw"]
    assert_exact_regime(kw.get("patch_size", 5), ci["ss"], ci["sg"], ci["tg"], ci["sw"], ci["gw"], ci["mod"])
    seed = 17
    out, err, nnf = ebsynth_run(gpu(ci["ss"]), gpu(ci["sg"]), gpu(ci["tg"]),
                                target_modulation=None if ci["mod"] is None else gpu(ci["mod"]), style_weights=ci["sw"],
                                guide_weights=ci["gw"], seed=seed, return_nnf=True, **kw)
    stats = {"multi_accept": 0}
    m_out, m_err, m_nnf = run_model(ci, seed, stats)
    if kw.get("uniformity", 3500.0) > 0:
        assert stats["multi_accept"] > 0
    np.testing.assert_array_equal(nnf.cpu().numpy(), m_nnf)
    np.testing.assert_array_equal(err.cpu().numpy(), m_err)
    np.testing.assert_array_equal(out.cpu().numpy(), m_out)
