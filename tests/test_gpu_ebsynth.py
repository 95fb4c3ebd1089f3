"""Ebsynth HIP backend on the GPU: the deterministic stages against numpy restatements, known-answer shifts, quality
parity with the reference CPU build on the golden cases (tests/golden/ebsynth_golden.npz and ebsynth_wide_golden.npz,
make_ebsynth_golden.py), bit-reproducibility, refused arguments, and the command line end to end.  The exact-match
matrix over record widths, patches and shapes is tests/test_gpu_ebsynth_matrix.py."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import fresco_amd
from fresco_amd import FrescoHipError, _lib, ebsynth_run
from fresco_amd import ebsynth as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ebsynth_model  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ebsynth_golden.npz")
GOLDEN_WIDE = os.path.join(ROOT, "tests", "golden", "ebsynth_wide_golden.npz")
DEV = "cuda:0"
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements of single stages (the whole loop: tests/ebsynth_model.py)
def hash64(seed, pixel, pss, step):
    """the backend's counter-based random bits (splitmix64 finaliser), on uint64 arrays"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (np.uint64(0x9E3779B97F4A7C15) * (pixel.astype(np.uint64) + np.uint64(1)))
        z = z + np.uint64(((pss << 32) | step) & M64) * np.uint64(0xD6E8FEB86659FD93)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def random_nnf(th, tw, sh, sw, r, seed):
    h = hash64(seed, np.arange(th * tw), 0xFFFFFFFF, 0)
    x = r + (h & np.uint64(0xFFFFFFFF)) % np.uint64(sw - 2 * r)
    y = r + (h >> np.uint64(32)) % np.uint64(sh - 2 * r)
    return np.stack([x, y], -1).astype(np.int64).reshape(th, tw, 2)


def upscale_nnf(prev, th, tw, sh, sw, patch):
    ph, pw = prev.shape[:2]
    ys, xs = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
    p = prev[np.clip(ys // 2, 0, ph - 1), np.clip(xs // 2, 0, pw - 1)]
    return np.stack([np.clip(p[..., 0] * 2 + xs % 2, patch, sw - patch - 1),
                     np.clip(p[..., 1] * 2 + ys % 2, patch, sh - patch - 1)], -1)


def _clamped(a, y, x):
    return a[np.clip(y, 0, a.shape[0] - 1), np.clip(x, 0, a.shape[1] - 1)]


def vote(src_style, nnf, patch, err=None):
    th, tw = nnf.shape[:2]
    ns = src_style.shape[2]
    r = patch // 2
    ys, xs = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
    acc = np.zeros((th, tw, ns), np.float32)
    wsum = np.zeros((th, tw), np.float32)
    for py in range(-r, r + 1):
        for px in range(-r, r + 1):
            n = _clamped(nnf, ys + py, xs + px)
            s = src_style[n[..., 1] - py, n[..., 0] - px].astype(np.float32)
            if err is None:
                w = np.ones((th, tw), np.float32)
            else:
                w = np.float32(1.0) / (np.float32(1.0) + _clamped(err, ys + py, xs + px) / np.float32(patch * patch * ns))
            acc = acc + w[..., None] * s
            wsum = wsum + w
    return (acc / wsum[..., None]).astype(np.uint8)


def patch_error(tstyle, tguide, sstyle, sguide, nnf, sw_, gw_, patch, mod=None):
    th, tw = nnf.shape[:2]
    r = patch // 2
    ys, xs = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
    e = np.zeros((th, tw), np.float64)
    gw = np.asarray(gw_, np.float64)
    for py in range(-r, r + 1):
        for px in range(-r, r + 1):
            ty, tx = np.clip(ys + py, 0, th - 1), np.clip(xs + px, 0, tw - 1)
            sy, sx = nnf[..., 1] + py, nnf[..., 0] + px
            d = tstyle[ty, tx].astype(np.float64) - sstyle[sy, sx]
            e += (d * d * np.asarray(sw_, np.float64)).sum(-1)
            d = tguide[ty, tx].astype(np.float64) - sguide[sy, sx]
            w = gw if mod is None else gw * (mod[ty, tx] / 255.0)
            e += (d * d * w).sum(-1)
    return e


def resample(img, oh, ow):
    ih, iw = img.shape[:2]
    sc = np.float32(iw) / np.float32(ow)
    ys, xs = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    fx, fy = sc * xs.astype(np.float32), sc * ys.astype(np.float32)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    s, t = (fx - ix.astype(np.float32))[..., None], (fy - iy.astype(np.float32))[..., None]
    one = np.float32(1.0)
    f = img.astype(np.float32)
    v = ((one - s) * (one - t) * _clamped(f, iy, ix) + s * (one - t) * _clamped(f, iy, ix + 1)
         + (one - s) * t * _clamped(f, iy + 1, ix) + s * t * _clamped(f, iy + 1, ix + 1))
    return v.astype(np.uint8)


def stop_mask(new, old, thr, patch):
    m = (np.abs(new.astype(np.int32) - old).max(-1) >= thr)
    h, w = m.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    r = patch // 2
    out = np.zeros_like(m)
    for py in range(-r, r + 1):
        for px in range(-r, r + 1):
            out |= _clamped(m, ys + py, xs + px)
    return out.astype(np.uint8) * 255


# ---------------------------------------------------------------------------------------------------------------------
def smooth(rng, h, w, c, cell=6):
    g = torch.from_numpy(rng.uniform(0, 255, (1, c, h // cell + 2, w // cell + 2)).astype(np.float32))
    up = torch.nn.functional.interpolate(g, size=(h + 2 * cell, w + 2 * cell), mode="bilinear", align_corners=False)
    return up[0, :, cell:cell + h, cell:cell + w].permute(1, 2, 0).clamp(0, 255).to(torch.uint8).numpy()


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(3)
    h, w = 48, 56
    return dict(ss=smooth(rng, h, w, 3), sg=smooth(rng, h, w, 4), tg=smooth(rng, 40, 44, 4),
                mod=rng.integers(0, 256, (40, 44, 4), dtype=np.uint8), sw=[0.5, 0.25, 1.0], gw=[1.0, 0.5, 2.0, 0.25])


@pytest.fixture(scope="module")
def wide_case():
    """8 style + 20 guide channels (two 16-byte records per pixel), a distinct fractional weight per channel"""
    rng = np.random.default_rng(29)
    return dict(ss=smooth(rng, 37, 43, 8), sg=smooth(rng, 37, 43, 20), tg=smooth(rng, 33, 40, 20),
                mod=rng.integers(0, 256, (33, 40, 20), dtype=np.uint8),
                sw=[float(v) for v in np.float32(rng.permutation(8) + 1) / np.float32(7)],
                gw=[float(v) for v in np.float32(rng.permutation(20) + 1) / np.float32(13)])


def test_stage_random_init_and_plain_vote(case):
    """levels = 1, no search: the NNF is the random initialisation, the image its plain vote, E stays 0."""
    c = case
    out, err, nnf = ebsynth_run(gpu(c["ss"]), gpu(c["sg"]), gpu(c["tg"]), pyramid_levels=1, search_vote_iters=0,
                                seed=11, return_nnf=True)
    want = random_nnf(40, 44, 48, 56, 2, 11)
    np.testing.assert_array_equal(nnf.cpu().numpy(), want)
    np.testing.assert_array_equal(out.cpu().numpy(), vote(c["ss"], want, 5))
    assert float(err.abs().max()) == 0.0


@pytest.mark.parametrize("which,mode,with_mod", [
    pytest.param("case", "plain", False, id="plain-False"), pytest.param("case", "weighted", False, id="weighted-False"),
    pytest.param("case", "weighted", True, id="weighted-True"),
    pytest.param("wide_case", "plain", False, id="rw2-plain-False"),
    pytest.param("wide_case", "weighted", False, id="rw2-weighted-False"),
    pytest.param("wide_case", "weighted", True, id="rw2-weighted-True"),
    pytest.param("wide_case", "plain", True, id="rw2-plain-True")])
def test_stage_patch_error_and_vote(request, which, mode, with_mod):
    """levels = 1, one search/vote iteration, no PatchMatch: E = patch error of the initial NNF against the first plain
    vote, then a plain or weighted vote with that E.  Per-channel weights all differ, so E depends on each channel
    reading its own weight; the wide case's second record holds style + guide bytes 16..27."""
    c = request.getfixturevalue(which)
    mod = c["mod"] if with_mod else None
    (sh, sw), (th, tw) = c["ss"].shape[:2], c["tg"].shape[:2]
    out, err, nnf = ebsynth_run(gpu(c["ss"]), gpu(c["sg"]), gpu(c["tg"]),
                                target_modulation=None if mod is None else gpu(mod), style_weights=c["sw"],
                                guide_weights=c["gw"], pyramid_levels=1, search_vote_iters=1, patchmatch_iters=0,
                                vote_mode=mode, seed=5, return_nnf=True)
    n = nnf.cpu().numpy()
    np.testing.assert_array_equal(n, random_nnf(th, tw, sh, sw, 2, 5))
    v1 = vote(c["ss"], n, 5)
    e = patch_error(v1, c["tg"], c["ss"], c["sg"], n, c["sw"], c["gw"], 5, mod)
    np.testing.assert_allclose(err.cpu().numpy(), e, rtol=1e-5)
    want = vote(c["ss"], n, 5, err.cpu().numpy() if mode == "weighted" else None)
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_stage_nnf_upscale(case):
    """two levels, no search: the fine NNF is the x2 upscale (+ parity, clamped) of the coarse random one."""
    c = case
    out, _, nnf = ebsynth_run(gpu(c["ss"]), gpu(c["sg"]), gpu(c["tg"]), pyramid_levels=2, search_vote_iters=0,
                              seed=2, return_nnf=True)
    coarse = random_nnf(20, 22, 24, 28, 2, 2)
    want = upscale_nnf(coarse, 40, 44, 48, 56, 5)
    np.testing.assert_array_equal(nnf.cpu().numpy(), want)
    np.testing.assert_array_equal(out.cpu().numpy(), vote(c["ss"], want, 5))


@pytest.mark.parametrize("ih,iw,oh,ow,nc", [(48, 56, 24, 28, 3), (97, 130, 48, 65, 16), (64, 64, 8, 8, 5),
                                            (31, 77, 15, 38, 1)])
def test_stage_resample(ih, iw, oh, ow, nc):
    img = np.random.default_rng(ih).integers(0, 256, (ih, iw, nc), dtype=np.uint8)
    got = E.resample(gpu(img), (oh, ow)).cpu().numpy()
    np.testing.assert_array_equal(got, resample(img, oh, ow))


@pytest.mark.parametrize("thr,patch,nc", [
    pytest.param(5, 5, 3, id="5-5"), pytest.param(1, 3, 3, id="1-3"), pytest.param(0, 5, 3, id="0-5"),
    pytest.param(40, 7, 3, id="40-7"), pytest.param(5, 5, 1, id="5-5-1ch"), pytest.param(1, 3, 8, id="1-3-8ch"),
    pytest.param(3, 5, 8, id="3-5-8ch")])
def test_stage_stop_mask(thr, patch, nc):
    rng = np.random.default_rng(thr)
    old = rng.integers(0, 256, (37, 45, nc), dtype=np.uint8)
    new = np.clip(old.astype(np.int32) + rng.integers(-6, 7, old.shape) * (rng.random(old.shape) < 0.02), 0,
                  255).astype(np.uint8)
    got = E.stop_mask(gpu(new), gpu(old), thr, patch).cpu().numpy()
    np.testing.assert_array_equal(got, stop_mask(new, old, thr, patch))


@pytest.mark.parametrize("kw", [dict(pyramid_levels=1, search_vote_iters=2, patchmatch_iters=2),
                                dict(search_vote_iters=3, patchmatch_iters=2, vote_mode="weighted"),
                                dict(search_vote_iters=2, patchmatch_iters=1, extra_pass_3x3=True)],
                         ids=["one_level", "pyramid_weighted", "extra_pass"])
def test_search_matches_numpy_restatement_exactly(case, kw):
    """PatchMatch with the uniformity term (propagation, random search, Omega bookkeeping, stop mask, votes, pyramid)
    against tests/ebsynth_model.py in this backend's schedule.  Unit weights keep every error an exact fp32 integer, so
    the NNF, E and image must match bit for bit.  The run must include pixels that accept two or more candidates in
    one pass, where the occupancy of the moved patch matters."""
    c = case
    seed = 3
    out, err, nnf = ebsynth_run(gpu(c["ss"]), gpu(c["sg"]), gpu(c["tg"]), style_weights=[1.0] * 3,
                                guide_weights=[1.0] * 4, seed=seed, return_nnf=True, **kw)
    stats = {"multi_accept": 0}
    m_out, m_err, m_nnf = ebsynth_model.run(
        c["ss"], c["sg"], c["tg"], sw=[1.0] * 3, gw=[1.0] * 4, levels=kw.get("pyramid_levels", -1),
        svi=kw["search_vote_iters"], pmi=kw["patchmatch_iters"], vote_mode=kw.get("vote_mode", "plain"),
        extra_pass_3x3=kw.get("extra_pass_3x3", False), seed=seed, omega="snapshot", stats=stats)
    assert stats["multi_accept"] > 0
    np.testing.assert_array_equal(nnf.cpu().numpy(), m_nnf)
    np.testing.assert_array_equal(err.cpu().numpy(), m_err)
    np.testing.assert_array_equal(out.cpu().numpy(), m_out)


# ---------------------------------------------------------------------------------------------------------------------
def shift_case(n=256, shift=(5, -3), seed=0):
    rng = np.random.default_rng(seed)
    ss = smooth(rng, n, n, 3, 5)
    sg = smooth(rng, n, n, 3, 4)
    dx, dy = shift
    ys = np.clip(np.arange(n) - dy, 0, n - 1)
    xs = np.clip(np.arange(n) - dx, 0, n - 1)
    return ss, sg, sg[ys][:, xs], ss[ys][:, xs]


@pytest.mark.parametrize("kw", [{}, {"vote_mode": "weighted"}, {"modulation": True}, {"extra_pass_3x3": True}],
                         ids=["plain", "weighted", "modulation", "extra_pass_3x3"])
def test_known_shift(kw):
    """target guide = source guide shifted by (5, -3): the interior NNF is p - shift and the image the shifted style,
    for >= 99 % of interior pixels.  At 96^2 the reference's GPU algorithm, restated in numpy (tests/ebsynth_model.py,
    live Omega), gets 1.000 / 0.998 plain and 0.997 / 0.987 with this modulation; at 256^2 see DESIGN.md section 9."""
    kw = dict(kw)
    n, (dx, dy) = 96, (5, -3)
    ss, sg, tg, want = shift_case(n)
    if kw.pop("modulation", False):  # a smooth modulation in [128, 255]
        kw["target_modulation"] = gpu(128 + smooth(np.random.default_rng(9), n, n, 3) // 2)
    out, err, nnf = ebsynth_run(gpu(ss), gpu(sg), gpu(tg), return_nnf=True, **kw)
    nnf, out = nnf.cpu().numpy(), out.cpu().numpy()
    m = 12
    ys, xs = np.meshgrid(np.arange(m, n - m), np.arange(m, n - m), indexing="ij")
    hit = (nnf[m:n - m, m:n - m, 0] == xs - dx) & (nnf[m:n - m, m:n - m, 1] == ys - dy)
    # the weighted mean of equal values can round just below them and truncate one LSB low (the reference's too)
    tol = 1 if kw.get("vote_mode") == "weighted" else 0
    same = np.all(np.abs(out[m:n - m, m:n - m].astype(int) - want[m:n - m, m:n - m]) <= tol, -1)
    print("known shift %s: NNF exact %.4f, image exact %.4f" % (list(kw), hit.mean(), same.mean()))
    floor_img = 0.99
    if "target_modulation" in kw:
        # the truncated mean of a modulated match leaves the image short of 0.99 for the reference's algorithm too:
        # the bar is what the numpy restatement (live Omega) reaches on the same inputs
        m_out, _, _ = ebsynth_model.run(ss, sg, tg, mod=kw["target_modulation"].cpu().numpy(), omega="live")
        floor_img = min(0.99, float(np.all(m_out[m:n - m, m:n - m] == want[m:n - m, m:n - m], -1).mean()))
    assert hit.mean() >= 0.99 and same.mean() >= floor_img


# ---------------------------------------------------------------------------------------------------------------------
def golden_cases():
    z = np.load(GOLDEN)
    return sorted({k.split("/")[0] for k in z.files})


def golden_args(name, path=GOLDEN):
    z = np.load(path)
    g = lambda k: z[name + "/" + k]  # noqa: E731
    args = [str(a) for a in g("args")]
    cli = E.parse_cli(["-style", "s"] + sum([["-guide", "a", "b"] for _ in g("guide_counts")], []) + args)
    counts, wcli = g("guide_counts"), g("guide_weights_cli")
    gw = []
    for c, w in zip(counts, wcli):
        w = np.float32(1.0 / len(counts)) if w < 0 else np.float32(w)
        gw += [float(w / np.float32(c))] * int(c)
    ns = g("style").shape[2]
    return g, [float(np.float32(1.0) / np.float32(ns))] * ns, gw, cli


def run_golden(name, seed, path=GOLDEN):
    g, sw, gw, cli = golden_args(name, path)
    out, err = ebsynth_run(gpu(g("style")), gpu(g("source_guide")), gpu(g("target_guide")), style_weights=sw,
                           guide_weights=gw, uniformity=cli["uniformity"], patch_size=cli["patchsize"],
                           search_vote_iters=cli["searchvoteiters"], patchmatch_iters=cli["patchmatchiters"],
                           stop_threshold=cli["stopthreshold"], seed=seed)
    return out.cpu().numpy(), err.cpu().numpy(), g


def run_golden_model(name, seed, path=GOLDEN):
    """the reference GPU backend's algorithm (live Omega, one pass per random-search radius), restated in numpy"""
    g, sw, gw, cli = golden_args(name, path)
    out, err, _ = ebsynth_model.run(g("style"), g("source_guide"), g("target_guide"), sw=sw, gw=gw,
                                    uniformity=cli["uniformity"], patch=cli["patchsize"], svi=cli["searchvoteiters"],
                                    pmi=cli["patchmatchiters"], stop=cli["stopthreshold"], seed=seed, omega="live")
    return out, err


# The four-guide case (video_blend.py's shape) is held to the reference CPU build directly: mean E <= 1.10x, mean
# |output - reference| within three times the reference's own 1-LSB spread + 1.  On the small cases the reference's GPU
# algorithm itself, restated in numpy with its live Omega schedule, does not reach 1.10x of the CPU build (E ratio
# 1.14 / 1.44 / 1.17 at 64^2 over seeds 0 / 7 / 99): there the backend is held to that restatement, same bars.
@pytest.mark.parametrize("seed", [0, 7, 99])
@pytest.mark.parametrize("name", ["sq64", "rect96x128", "four_guides"])
def test_parity_with_reference_quality(name, seed):
    out, err, g = run_golden(name, seed)
    ref_out, ref_err = g("ref_out"), g("ref_err")
    assert out.shape == ref_out.shape
    ratio = float(err.mean() / ref_err.mean())
    mad = float(np.abs(out.astype(np.float64) - ref_out).mean())
    spread = 3.0 * float(g("spread_mean_abs").max()) + 1.0
    if name == "four_guides":
        base_ratio, base_mad = 1.0, 0.0
    else:
        m_out, m_err = run_golden_model(name, seed)
        base_ratio = float(m_err.mean() / ref_err.mean())
        base_mad = float(np.abs(m_out.astype(np.float64) - ref_out).mean())
    print("%s seed %d: mean E / CPU reference %.3f (bar %.3f), mean |out - CPU reference| %.3f (bar %.3f)"
          % (name, seed, ratio, 1.10 * base_ratio, mad, base_mad + spread))
    assert ratio <= 1.10 * base_ratio
    assert mad <= base_mad + spread


# Outside those shapes (tests/golden/ebsynth_wide_golden.npz, make_ebsynth_golden.py --wide): 8 RGB guides (3 + 24
# channels, two 16-byte records) with mixed weights and patch 7, and an RGBA style whose target guide has another size
# than the source.  Held to the small cases' bars: the numpy restatement of the reference's GPU algorithm on the same
# inputs.
@pytest.mark.parametrize("seed", [0, 7, 99])
@pytest.mark.parametrize("name", ["eight_rgb_guides", "rgba_style_resized_target"])
def test_parity_with_reference_quality_wide(name, seed):
    out, err, g = run_golden(name, seed, GOLDEN_WIDE)
    ref_out, ref_err = g("ref_out"), g("ref_err")
    assert out.shape == ref_out.shape
    ratio = float(err.mean() / ref_err.mean())
    mad = float(np.abs(out.astype(np.float64) - ref_out).mean())
    spread = 3.0 * float(g("spread_mean_abs").max()) + 1.0
    m_out, m_err = run_golden_model(name, seed, GOLDEN_WIDE)
    base_ratio = float(m_err.mean() / ref_err.mean())
    base_mad = float(np.abs(m_out.astype(np.float64) - ref_out).mean())
    print("%s seed %d: mean E / CPU reference %.3f (bar %.3f), mean |out - CPU reference| %.3f (bar %.3f)"
          % (name, seed, ratio, 1.10 * base_ratio, mad, base_mad + spread))
    assert ratio <= 1.10 * base_ratio
    assert mad <= base_mad + spread


def test_bit_reproducible():
    ss, sg, tg, _ = shift_case(128, (3, 2), seed=4)
    runs = [ebsynth_run(gpu(ss), gpu(sg), gpu(tg), vote_mode="weighted", seed=123, return_nnf=True) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    other = ebsynth_run(gpu(ss), gpu(sg), gpu(tg), vote_mode="weighted", seed=124, return_nnf=True)
    assert not torch.equal(other[2], runs[0][2])  # the seed does reach the search


# ---------------------------------------------------------------------------------------------------------------------
def _raw_run(ns, ng, w, h, patch, ws_bytes=None):
    lib = _lib.load()
    st = torch.zeros(h, w, ns, dtype=torch.uint8, device=DEV)
    gd = torch.zeros(h, w, ng, dtype=torch.uint8, device=DEV)
    out = torch.full((h, w, ns), 77, dtype=torch.uint8, device=DEV)
    err = torch.full((h, w), 3.0, device=DEV)
    need = lib.fresco_ebsynth_workspace_bytes(ns, ng, w, h, w, h, patch, -1, 0)
    n = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=DEV)
    c = _lib._c
    ones = lambda k: (c.c_float * k)(*([1.0] * k))  # noqa: E731
    lv = (c.c_int * 8)(*([1] * 8))
    rc = lib.fresco_ebsynth_run(st.data_ptr(), gd.data_ptr(), gd.data_ptr(), None, ones(ns), ones(ng), ns, ng, w, h,
                                w, h, 3500.0, patch, 1, -1, lv, lv, lv, 0, 0, None, out.data_ptr(), err.data_ptr(),
                                ws.data_ptr(), n, fresco_amd.ops._stream())
    torch.cuda.synchronize()
    untouched = bool((out == 77).all()) and bool((err == 3.0).all())
    return rc, untouched


@pytest.mark.parametrize("ns,ng,size,patch,ws,status", [
    (9, 3, 32, 5, None, -2), (3, 25, 32, 5, None, -2), (3, 3, 32, 4, None, -2), (3, 3, 10, 5, None, -2),
    (3, 3, 32, 5, 1000, -3)], ids=["9_style", "25_guide", "even_patch", "too_small", "short_workspace"])
def test_refused_before_any_launch(ns, ng, size, patch, ws, status):
    if ws is None and status == -2 and (ns > 8 or ng > 24 or patch % 2 == 0):
        ws = 1 << 20  # the workspace query itself refuses these shapes (returns 0)
    rc, untouched = _raw_run(ns, ng, size, size, patch, ws)
    assert rc == status and untouched
    with pytest.raises(FrescoHipError, match="FRESCO_EUNSUPPORTED|FRESCO_EWORKSPACE"):
        _lib.check(rc, "fresco_ebsynth_run")
    if status == -2:
        s = torch.zeros(size, size, ns, dtype=torch.uint8, device=DEV)
        g = torch.zeros(size, size, ng, dtype=torch.uint8, device=DEV)
        with pytest.raises(FrescoHipError, match="FRESCO_EUNSUPPORTED"):
            ebsynth_run(s, g, g, patch_size=patch)


# ---------------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path):
    """The shim answers the command string video_blend.py builds (video_blend.py:96-101) with a .png and a .bin that
    load_error's format accepts."""
    from PIL import Image
    n = 64
    ss, sg, tg, _ = shift_case(n, (2, 1), seed=8)
    Image.fromarray(ss).save(tmp_path / "key.png")
    cmd = "%s -style %s" % (os.path.join(ROOT, "fresco_amd", "bin", "ebsynth"), tmp_path / "key.png")
    for k, (w, a, b) in enumerate([(6, sg, tg), (0.5, sg[..., 0], tg[..., 0]), (0.5, ss, ss), (2, sg, tg)]):
        Image.fromarray(a).save(tmp_path / ("g%d_s.png" % k))
        Image.fromarray(b).save(tmp_path / ("g%d_t.png" % k))
        cmd += " -guide %s %s -weight %s" % (tmp_path / ("g%d_s.png" % k), tmp_path / ("g%d_t.png" % k), w)
    out = tmp_path / "out" / "0002.png"
    out.parent.mkdir()
    cmd += " -output %s -searchvoteiters 12 -patchmatchiters 6" % out
    env = dict(os.environ, PYTHON=sys.executable)
    r = subprocess.run(cmd, shell=True, capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    img = np.asarray(Image.open(out))
    assert img.shape == (n, n, 3)
    raw = open(str(out)[:-4] + ".bin", "rb").read()
    assert len(raw) == 8 + 4 * n * n and struct.unpack("q", raw[:8])[0] == n * n
    e = np.array(struct.unpack("f" * n * n, raw[8:]), np.float32)
    assert np.isfinite(e).all() and (e >= 0).all()
