"""The Canny kernels (csrc/canny.hip) on the paths the small maps of tests/test_gpu_canny.py never reach, against the numpy
restatement of the rules (tests/canny_model.py).  All integer: every comparison is for equality.

  A  the tile kernels (classify, tile union, border union) past one pass of their grid-stride loop.  The grid is capped at
     CANNY_MAX_BLOCKS = 2^20 workgroups, one tile each per pass: 2^20 + 3000 frames of 3 x 3 are one tile each, so 3000
     tiles run in a second pass.  Hysteresis walks the exhaustive pool of all 3^9 class maps over {0, 1, 2} (frame i is
     entry i mod 19 683: pass two starts at entry 5377, no repeat of pass one); classify a pool of 4096 coarse-level frames.
  B  the pixel kernels (seed, emit) past one pass: 2^20 workgroups of 256 threads are 2^28 pixels; 16 400 frames of
     128 x 128 are 2^28 + 262 144, with the fp16 condition.  Built, run and compared on the device.
  C  hysteresis on 512 tiles (8 x 256 x 256): more workgroups than one XCD holds link through agent-scope atomics, over
     components that span every tile and are seeded far from their root.  Random maps below, near and above the percolation
     threshold, serpentines and spirals seeded at their last pixel, both staircases, an all-weak frame before an all-strong
     one, a 4096-pixel row and column.  Each map runs three times and must give the same bits each time.
  D  the detector end to end at the workload's size, 8 x 512 x 512 at 50 / 100, and on 1 x 1030 x 1027 (33 x 33 tiles, ragged
     on both sides), edge map and bf16 condition under guidance.

A scratch build in which every kernel's grid-stride loop is a single pass (`if` in place of `for`) passes
tests/test_gpu_canny.py as it stood before this file and fails here: see MUTANT below.
"""
import functools

import numpy as np
import pytest
import torch

import canny_model as M
import test_gpu_canny as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_BLOCKS = 1 << 20          # CANNY_MAX_BLOCKS
ONE_TILE_PASS = MAX_BLOCKS    # tiles one pass of a tile kernel covers
ONE_PIXEL_PASS = MAX_BLOCKS * 256

# What the single-pass scratch build (see the module docstring) gave on an MI355X: `tile += tl.total` and `idx += total` as
# the five loops' increments, nothing else.  A later pass's parents are then never written, so the scratch build's finds
# also stop at an index outside the map instead of following it; outputs past the first pass are whatever the allocator
# left there, mostly zero.
MUTANT = """
tests/test_gpu_canny.py as it stood before this file: 31 passed.  With the tests added since: 56 passed.
tests/test_gpu_canny_fullsize.py: 3 failed, 11 passed --
  test_hysteresis_tile_loops_past_one_pass   no frame of pass one and 2 714 of the 3 000 frames of pass two differ,
                                             7 984 of 9 464 184 bytes
  test_classify_tile_loop_past_one_pass      at 10 / 30 no frame of pass one and all 3 000 of pass two, 13 949 bytes
  test_pixel_loops_past_one_pass             no frame of pass one and all 16 of pass two, 4 193 of 268 697 600 bytes
  C and D stay inside one pass of every loop: they pass.
"""


def _gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared inputs are read-only)


def _differ(got, want):
    return "%d of %d bytes differ" % (int((got != want).sum()), want.numel())


# ---------------------------------------------------------------------------------------------------------------
# A. tile kernels past one grid pass
# ---------------------------------------------------------------------------------------------------------------
N_SMALL = MAX_BLOCKS + 3000


def test_hysteresis_tile_loops_past_one_pass():
    from fresco_amd import ops
    pool = M.all_3x3_class_maps()
    assert pool.shape == (19683, 3, 3) and ONE_TILE_PASS % len(pool) == 5377  # where pass two starts in the pool
    want_pool = M.hysteresis(pool)
    assert 0 < int((want_pool == 255).sum()) < int((pool > 0).sum())  # kept and refused components
    idx = torch.arange(N_SMALL, device=DEV) % len(pool)
    cls = _gpu(pool)[idx]
    want = _gpu(want_pool)[idx]
    assert cls.is_contiguous() and tuple(cls.shape) == (N_SMALL, 3, 3)
    got, cond = ops.canny_hysteresis(cls)
    assert cond is None and got.dtype == torch.uint8 and got.shape == want.shape
    bad = (got != want).reshape(N_SMALL, -1).any(1)
    print("frames that differ: %d in pass one, %d in pass two"
          % (int(bad[:ONE_TILE_PASS].sum()), int(bad[ONE_TILE_PASS:].sum())))
    assert torch.equal(got, want), _differ(got, want)
    assert bool((want[ONE_TILE_PASS:] == 255).any())


def test_classify_tile_loop_past_one_pass():
    """test_classify_degenerate_sizes's coarse levels.  Their magnitudes are multiples of 24, so at 10 / 30 a weak pixel needs
    m = 24 exactly: 4 of the pool's 36 864 pixels have it and none of them is a local maximum (no seed out of twelve gave
    one).  So 10 / 30 must show classes 0 and 2, and the pool runs at 50 / 100 too, where all three occur (168 weak)."""
    from fresco_amd import ops
    pool = (np.random.RandomState(33).randint(0, 6, (4096, 3, 3, 3)) * 12).astype(np.uint8)
    idx = torch.arange(N_SMALL, device=DEV) % len(pool)
    frames = _gpu(pool)[idx]
    assert frames.is_contiguous() and tuple(frames.shape) == (N_SMALL, 3, 3, 3)
    for low, high, classes in ((10, 30, (0, 2)), (50, 100, (0, 1, 2))):
        want_pool = M.classify_batch(pool, low, high)
        for k in classes:
            assert (want_pool == k).any(), (low, high, k)
        want = _gpu(want_pool)[idx]
        got = ops.canny_classify(frames, low, high)
        bad = (got != want).reshape(N_SMALL, -1).any(1)
        print("%d / %d: frames that differ: %d in pass one, %d in pass two"
              % (low, high, int(bad[:ONE_TILE_PASS].sum()), int(bad[ONE_TILE_PASS:].sum())))
        assert torch.equal(got, want), (low, high, _differ(got, want))
        assert bool((want[ONE_TILE_PASS:] == 2).any())


# ---------------------------------------------------------------------------------------------------------------
# B. pixel kernels past one grid pass
# ---------------------------------------------------------------------------------------------------------------
def test_pixel_loops_past_one_pass():
    from fresco_amd import ops
    n, S, P = 16400, 128, 64
    assert ONE_PIXEL_PASS < n * S * S < ONE_PIXEL_PASS + (1 << 20) and ONE_PIXEL_PASS % (S * S) == 0
    first_later = ONE_PIXEL_PASS // (S * S)  # the first frame of pass two: 16 384
    pool = np.concatenate([M.random_classes(1, S, S, 0.2 + 0.25 * k / (P - 1), 0.002, seed=100 + k) for k in range(P)])
    want_pool = M.hysteresis(pool)
    idx = torch.arange(n, device=DEV) % P
    cls = _gpu(pool)[idx]
    want = _gpu(want_pool)[idx]
    got, cond = ops.canny_hysteresis(cls, cond_dtype=torch.float16)
    del cls
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert cond.dtype == torch.float16 and tuple(cond.shape) == (n, 3, S, S)
    bad = (got != want).reshape(n, -1).any(1)
    print("frames that differ: %d in pass one, %d in pass two"
          % (int(bad[:first_later].sum()), int(bad[first_later:].sum())))
    assert torch.equal(got, want), _differ(got, want)
    del got, bad
    ref = (want == 255).to(torch.float16)
    for c in range(3):
        assert torch.equal(cond[:, c], ref), "condition channel %d: %s" % (c, _differ(cond[:, c], ref))
    later = want[first_later:]
    assert later.shape[0] == 16 and bool((later == 255).any()) and bool((later == 0).any())


# ---------------------------------------------------------------------------------------------------------------
# C. many workgroups
# ---------------------------------------------------------------------------------------------------------------
def _frames(*maps):
    return np.stack([np.ascontiguousarray(m) for m in maps]).astype(np.uint8)


def _serpentines():
    last, none, first = (M.serpentine(256, 256, seed=s) for s in ("last", False, True))
    return _frames(last, none, first, last.T, none.T, first.T, last[:, ::-1], last[::-1])


def _spirals():
    last, none, first = (M.spiral(256, 256, seed=s) for s in ("last", False, "first"))
    return _frames(last, first, none, last.T, last[::-1], last[:, ::-1], first[::-1, ::-1], none.T)


def _staircases():
    st, anti = M.staircase(256, 256), M.anti_staircase(256, 256)
    weak = (st > 0).astype(np.uint8)
    return _frames(st, anti, st[::-1, ::-1], anti[::-1, ::-1], M.seed_last(weak), M.seed_last(weak[:, ::-1]), weak, st | anti)


def _weak_before_strong():
    z, w, s = (np.full((256, 256), v, np.uint8) for v in (0, 1, 2))
    return _frames(w, s, w, z, w, w, s, w)


MANY_TILES = {
    "random_0.20": lambda: M.random_classes(8, 256, 256, 0.20, 0.02, seed=21),
    "random_0.40": lambda: M.random_classes(8, 256, 256, 0.40, 0.001, seed=22),
    "random_0.60": lambda: M.random_classes(8, 256, 256, 0.60, 0.0005, seed=23),
    "serpentines": _serpentines,
    "spirals": _spirals,
    "staircases": _staircases,
    "weak_before_strong": _weak_before_strong,
    "row_4096": lambda: M.line(1, 4096, seed="last")[None],
    "column_4096": lambda: M.line(4096, 1, vertical=True, seed="last")[None],
}


@pytest.mark.parametrize("name", list(MANY_TILES))
def test_hysteresis_many_workgroups(name):
    from fresco_amd import ops
    cls = MANY_TILES[name]()
    want = M.hysteresis(cls)
    dev = _gpu(cls)
    runs = [ops.canny_hysteresis(dev)[0].cpu().numpy() for _ in range(3)]
    for k, got in enumerate(runs):
        assert np.array_equal(got, want), "run %d: %d pixels differ" % (k, int((got != want).sum()))
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    # what the case is there for
    lit = (want == 255).reshape(len(want), -1).sum(1).tolist()
    if name == "random_0.40":
        kept, dropped = float(((cls == 1) & (want == 255)).mean()), float(((cls == 1) & (want == 0)).mean())
        print("weak kept %.1f %%, weak dropped %.1f %%" % (100 * kept, 100 * dropped))
        assert kept >= 0.02 and dropped >= 0.02
    elif name.startswith("random"):
        assert (want[cls == 1] == 255).any() and (want[cls == 1] == 0).any()
    elif name == "serpentines":
        assert lit == [32896, 0, 32896, 32896, 0, 32896, 32896, 32896]
    elif name == "spirals":
        assert lit[0] == int((cls[0] > 0).sum()) > 32000 and lit[2] == 0 and lit[7] == 0
        assert all(v == lit[0] for k, v in enumerate(lit) if k not in (2, 7))
    elif name == "staircases":
        assert lit == [256, 256, 256, 256, 256, 256, 0, 512]  # (the last: the two diagonals cross)
    elif name == "weak_before_strong":
        assert lit == [0, 65536, 0, 0, 0, 0, 65536, 0]
    else:
        assert cls.size == 4096 and lit == [4096] and cls.reshape(-1)[-1] == 2 and (cls.reshape(-1)[:-1] == 1).all()


# ---------------------------------------------------------------------------------------------------------------
# D. the workload's size, end to end
# ---------------------------------------------------------------------------------------------------------------
FULL_SIZE = ((8, 512, 512, 0), (1, 1030, 1027, 3))  # (n, H, W, seed) of the natural field at standard deviation 10


@functools.lru_cache(maxsize=None)
def _full_size(case):
    frames = M.natural_case(case, 10.0)
    edges = M.canny_batch(frames, 50, 100)
    frames.setflags(write=False)
    edges.setflags(write=False)
    return frames, edges


@pytest.mark.parametrize("case", FULL_SIZE, ids=M.case_id)
def test_detector_at_full_size(case):
    import fresco_amd
    frames, edges = _full_size(case)
    n, H, W = frames.shape[:3]
    assert 0.2 < float((edges == 255).mean()) < 0.4
    det = fresco_amd.CannyDetector()
    dev = _gpu(frames)
    got = det.detect_batch(dev, 50, 100)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (n, H, W)
    got = got.cpu().numpy()
    assert np.array_equal(got, edges), "%d pixels differ" % int((got != edges).sum())
    cond = det.control_image(dev, torch.bfloat16, guidance=True)
    want = G._reference_condition(edges, torch.bfloat16, True)
    assert cond.dtype == torch.bfloat16 and tuple(cond.shape) == (2 * n, 3, H, W)
    assert torch.equal(cond, want), _differ(cond, want)
