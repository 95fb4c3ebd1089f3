"""fresco_amd's Canny kernels on the GPU against the numpy restatement of the rules (tests/canny_model.py): all integer, so
every comparison is for equality.  The classify pass alone, the hysteresis passes alone on constructed class maps (long
paths, corner connections, components that span many tiles, frame boundaries, every 3 x 3 pattern across a corner of four
tiles), the workspace the C entry point is handed, and the detector end to end with the condition tensor.  The large
and many-frame paths are in tests/test_gpu_canny_fullsize.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import canny_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NATURAL = [(case, setting) for case in M.NATURAL_CASES for setting in M.NATURAL_SETTINGS]
NATURAL_IDS = ["%s-%d-%d" % (M.case_id(c), s[1], s[2]) for c, s in NATURAL]


@functools.lru_cache(maxsize=None)
def natural(case, std):
    fr = M.natural_case(case, std)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def natural_classes(case, setting):
    c = M.classify_batch(natural(case, setting[0]), setting[1], setting[2])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def natural_edges(case, setting):
    e = M.hysteresis(natural_classes(case, setting))
    e.setflags(write=False)
    return e


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared inputs are read-only)


def classify_gpu(frames, low, high):
    from fresco_amd import ops
    return ops.canny_classify(gpu(frames), low, high).cpu().numpy()


def hysteresis_gpu(cls, cond_dtype=None):
    from fresco_amd import ops
    out, cond = ops.canny_hysteresis(gpu(cls), cond_dtype=cond_dtype)
    return out.cpu().numpy(), cond


# ---- classify alone
@pytest.mark.parametrize("case,setting", NATURAL, ids=NATURAL_IDS)
def test_classify_natural_fields(case, setting):
    got = classify_gpu(natural(case, setting[0]), setting[1], setting[2])
    want = natural_classes(case, setting)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), "%d pixels differ" % int((got != want).sum())


def test_classify_swaps_low_above_high():
    case, setting = M.NATURAL_CASES[1], M.NATURAL_SETTINGS[0]
    assert np.array_equal(classify_gpu(natural(case, 10.0), 100, 50), natural_classes(case, setting))


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (2, 2)], ids=lambda v: str(v))
def test_classify_degenerate_sizes(H, W):
    rs = np.random.RandomState(10 * H + W)
    # coarse levels: differences around both thresholds, and equal channels often enough for ties
    frames = (rs.randint(0, 6, (4, H, W, 3)) * 12).astype(np.uint8)
    for low, high in ((50, 100), (10, 30)):
        assert np.array_equal(classify_gpu(frames, low, high), M.classify_batch(frames, low, high))
    if (H, W) == (1, 7):
        row = np.zeros((1, 1, 7, 3), np.uint8)
        row[..., 3:, :] = 100
        got = classify_gpu(row, 50, 100)
        assert np.array_equal(got, M.classify_batch(row, 50, 100)) and got.tolist() == [[[0, 0, 2, 0, 0, 0, 0]]]


def test_classify_constant_colour_and_steps():
    flat = np.empty((2, 70, 75, 3), np.uint8)
    flat[0] = (200, 30, 90)
    flat[1] = 255
    assert not classify_gpu(flat, 50, 100).any()
    for img in (M.step_columns(), M.step_rows(), M.step_columns(70, 75, 32, 100), M.step_rows(70, 75, 64, 40)):
        got = classify_gpu(img[None], 50, 100)[0]
        assert np.array_equal(got, M.classify(img, 50, 100))
    assert np.array_equal(classify_gpu(M.step_columns()[None], 50, 100)[0][:, 3], np.full(6, 2, np.uint8))
    assert np.array_equal(classify_gpu(M.step_rows()[None], 50, 100)[0][2], np.full(8, 2, np.uint8))


# the largest gradients an 8-bit image has (dx, dy = +-1020, m = 1530 on the blocky frames; +-885 on the uniform one), at
# thresholds below, between and above them, equal, zero and negative
LARGE_FRAMES = {
    "blocky": lambda: M.blocky(2, 70, 75, 3, seed=1),
    "uniform": lambda: M.uniform(1, 70, 75, seed=0),
}
LARGE_THRESHOLDS = ((50, 100), (500, 900), (1000, 1500), (1529, 1530), (0, 0), (-5, 3000), (2040, 2041), (700, 700))


@pytest.mark.parametrize("name", list(LARGE_FRAMES))
def test_classify_full_range_gradients(name):
    frames = LARGE_FRAMES[name]()
    for low, high in LARGE_THRESHOLDS:
        got, want = classify_gpu(frames, low, high), M.classify_batch(frames, low, high)
        assert np.array_equal(got, want), (low, high, "%d pixels differ" % int((got != want).sum()))
        if (low, high) == (2040, 2041):
            assert not got.any()
        elif (low, high) == (-5, 3000):
            assert (got == 1).any() and not (got == 2).any()
        elif (low, high) == ((1000, 1500) if name == "blocky" else (500, 900)):
            assert (got == 1).any() and (got == 2).any()


@pytest.mark.parametrize("direction", ["right", "left", "down", "up"])
def test_classify_steps_of_255(direction):
    """dx = +-1020 with dy = 0, dy = +-1020 with dx = 0: the packed word's extremes, one at a time"""
    for H, W, at in ((70, 75, 33), (70, 75, 32), (6, 8, 4)):
        img = M.step(H, W, direction, at)
        dx, dy = M.gradients(img)
        if direction in ("right", "left"):
            assert not dy.any() and (dx.max() if direction == "right" else -dx.min()) == 1020
        else:
            assert not dx.any() and (dy.max() if direction == "down" else -dy.min()) == 1020
        for low, high in ((50, 100), (1019, 1020), (1020, 1021)):
            got = classify_gpu(img[None], low, high)[0]
            assert np.array_equal(got, M.classify(img, low, high)), (H, W, at, low, high)
            assert int((got == 2).sum()) == (0 if high >= 1020 else (H if direction in ("right", "left") else W))


@pytest.mark.parametrize("H,W", [(1, 97), (97, 1), (2, 65), (33, 32), (32, 32), (31, 33)], ids=lambda v: str(v))
def test_classify_thin_frames_across_tile_seams(H, W):
    """the clamped halo and the seam halo in one tile; a tile exactly filled, one pixel more, one less"""
    rs = np.random.RandomState(10 * H + W)
    coarse = (rs.randint(0, 6, (3, H, W, 3)) * 12).astype(np.uint8)
    for frames, pairs in ((coarse, ((50, 100), (10, 30))), (M.natural(2, H, W, 10.0, seed=H), ((50, 100),)),
                          (M.uniform(2, H, W, seed=W), ((500, 900),))):
        for low, high in pairs:
            got, want = classify_gpu(frames, low, high), M.classify_batch(frames, low, high)
            assert np.array_equal(got, want), (low, high, "%d pixels differ" % int((got != want).sum()))


# ---- hysteresis alone
def _all(v, n=1):
    return np.full((n, 70, 75), v, np.uint8)


def _three_frames():
    return np.stack([np.full((70, 75), 2), np.ones((70, 75)), np.ones((70, 75))]).astype(np.uint8)


def _odd_bytes():
    """the serpentine cut by a byte 3 and a byte 255 on its path, others scattered over the background"""
    c = M.serpentine()
    c[0, 40] = 3
    c[2, 10] = 255
    c[1, 5] = 3
    c[33, 33] = 255
    return c


CLASS_MAPS = {
    "serpentine": lambda: M.serpentine()[None],
    "serpentine_unseeded": lambda: M.serpentine(seed=False)[None],
    "staircase": lambda: M.staircase()[None],
    "checkerboard": lambda: M.checkerboard()[None],
    "all_weak": lambda: _all(1, 2),
    "all_strong": lambda: _all(2, 2),
    "all_zero": lambda: _all(0, 2),
    "two_blobs": lambda: M.two_blobs()[None],
    "three_frames": _three_frames,
    "odd_bytes": lambda: _odd_bytes()[None],
    "random_near_percolation": lambda: M.random_classes(2, 130, 150, 0.45, 0.002),
    # seeded at the component's last pixel in raster order: the root is at the other end of every chain of parents
    "serpentine_seeded_last": lambda: M.serpentine(seed="last")[None],
    "row_seeded_last": lambda: M.line(70, 75, seed="last")[None],
    "column_seeded_last": lambda: M.line(70, 75, vertical=True, seed="last")[None],
    "one_pixel_high": lambda: M.line(1, 97, seed="last")[None],
    "one_pixel_wide": lambda: M.line(97, 1, vertical=True, seed="last")[None],
    "spiral": lambda: M.spiral()[None],
    "spiral_unseeded": lambda: M.spiral(seed=False)[None],
}
# the maps on which every named defect of the two union passes shows (tests/test_canny_cpu.py): NE and NW links across
# tile seams and tile corners
SEAM_MAPS = {
    "anti_staircase_64": lambda: M.anti_staircase(64, 64)[None],
    "anti_staircase": lambda: M.anti_staircase()[None],
    "random_sparse": lambda: M.random_classes(2, 130, 150, 0.20, 0.02, seed=11),
}
CLASS_MAPS.update(SEAM_MAPS)


@pytest.mark.parametrize("name", list(CLASS_MAPS))
def test_hysteresis_constructed_maps(name):
    cls = CLASS_MAPS[name]()
    want = M.hysteresis(cls)
    got, cond = hysteresis_gpu(cls)
    assert cond is None and got.dtype == np.uint8 and got.shape == cls.shape
    assert np.array_equal(got, want), "%d pixels differ" % int((got != want).sum())
    # what the case is there for
    lit = int((want == 255).sum())
    if name in ("serpentine", "staircase", "checkerboard", "all_strong", "serpentine_seeded_last", "row_seeded_last",
                "column_seeded_last", "one_pixel_high", "one_pixel_wide", "spiral", "anti_staircase_64", "anti_staircase"):
        assert lit == int((cls > 0).sum()) and lit > 0
        if name in ("serpentine", "serpentine_seeded_last"):
            assert lit == 2660
        if name.endswith("seeded_last") or name.startswith("one_pixel"):
            assert int((cls == 2).sum()) == 1 and np.flatnonzero(cls)[-1] == np.flatnonzero(cls == 2)[0]
    elif name in ("serpentine_unseeded", "all_weak", "all_zero", "spiral_unseeded"):
        assert lit == 0
    elif name == "two_blobs":
        assert lit == 30 * 33 and not want[0][:, 36:].any()
    elif name == "three_frames":
        assert want[0].all() and not want[1:].any()
    elif name == "odd_bytes":
        assert lit == 40 and not want[0][0, 40:].any()  # row 0 up to the byte 3
    elif name == "random_sparse":
        weak = cls == 1
        assert (want[weak] == 255).mean() > 0.02 and (want[weak] == 0).mean() > 0.02  # small components, most refused
    else:
        assert name == "random_near_percolation"
        weak = cls == 1
        assert (want[weak] == 255).mean() > 0.5 and (want[weak] == 0).mean() > 0.02  # large components, and refused ones


def test_hysteresis_every_pattern_across_a_tile_corner():
    """11 264 frames of 34 x 34, four tiles each: every 3 x 3 pattern, every choice of its strong pixel, every cut"""
    cls = M.corner_patterns()
    assert cls.shape == (4 * 2816, 34, 34)
    want = M.hysteresis(cls)
    got, _ = hysteresis_gpu(cls)
    bad = (got != want).reshape(len(cls), -1).any(1)
    assert np.array_equal(got, want), "%d frames differ, the first: %s" % (int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


# ---- the workspace, through the C entry point
def _hysteresis_c(cls, ws_ptr, ws_bytes):
    from fresco_amd import _lib, ops
    n, H, W = cls.shape
    out = torch.full((n, H, W), 77, dtype=torch.uint8, device=DEV)
    rc = _lib.load().fresco_canny_hysteresis(cls.data_ptr(), out.data_ptr(), None, _lib.F32, ctypes.c_void_p(ws_ptr),
                                             ws_bytes, n, H, W, ops._stream())
    assert rc == 0, rc
    return out.cpu().numpy()


def test_hysteresis_workspace_contents_alignment_and_size():
    from fresco_amd import _lib
    cls = M.random_classes(2, 70, 75, 0.45, 0.004, seed=5)
    want = M.hysteresis(cls)
    n, H, W = cls.shape
    need = _lib.load().fresco_canny_workspace_bytes(n, H, W)
    assert need >= 5 * cls.size
    dev = gpu(cls)
    # every byte 0xff: parent = -1 and flag = 255 wherever a kernel relied on what it found
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    assert np.array_equal(_hysteresis_c(dev, ws.data_ptr(), need), want)
    # what an all-strong map of the same shape left (every flag and root of it set), then an all-weak map: nothing is lit
    assert _hysteresis_c(gpu(np.full(cls.shape, 2, np.uint8)), ws.data_ptr(), need).all()
    assert not _hysteresis_c(gpu(np.ones(cls.shape, np.uint8)), ws.data_ptr(), need).any()
    assert np.array_equal(_hysteresis_c(dev, ws.data_ptr(), need), want)
    # 4-byte alignment is all the entry point asks for; the bytes around the workspace stay as they were
    guard = 64
    buf = torch.full((guard + 4 + need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    assert np.array_equal(_hysteresis_c(dev, buf.data_ptr() + guard + 4, need), want)
    torch.cuda.synchronize()
    assert bool((buf[:guard + 4] == 0xA5).all()) and bool((buf[guard + 4 + need:] == 0xA5).all())
    # a larger workspace_bytes than needed
    big = torch.full((2 * need + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    assert np.array_equal(_hysteresis_c(dev, big.data_ptr(), 2 * need + 4096), want)
    assert bool((big[need:] == 0xFF).all())


def test_hysteresis_condition_dtypes():
    cls = M.random_classes(2, 70, 75, 0.45, 0.004, seed=5)
    want = M.hysteresis(cls)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        got, cond = hysteresis_gpu(cls, cond_dtype=dtype)
        assert np.array_equal(got, want)
        assert cond.dtype == dtype and tuple(cond.shape) == (2, 3, 70, 75)
        ref = torch.from_numpy(want == 255).to(DEV).to(dtype)[:, None].expand(-1, 3, -1, -1)
        assert torch.equal(cond, ref)


# ---- end to end
def _reference_condition(edges, dtype, guidance):
    """run_fresco.py:199-202 with torch, from the edge maps (numpy2tensor of src/utils.py restated)"""
    def numpy2tensor(img):
        x0 = torch.from_numpy(img.copy()).float().to(DEV) / 255.0 * 2.0 - 1.
        x0 = torch.stack([x0], dim=0)
        return x0.permute(0, 3, 1, 2)

    c = torch.cat([numpy2tensor(e[:, :, None]) for e in edges], dim=0).repeat(1, 3, 1, 1) * 0.5 + 0.5
    c = c.to(dtype)
    return torch.cat([c] * 2) if guidance else c


def test_detector_call_is_the_reference_protocol():
    import fresco_amd
    case, setting = M.NATURAL_CASES[3], M.NATURAL_SETTINGS[0]
    img = natural(case, 10.0)[0].copy()
    det = fresco_amd.CannyDetector()
    got = det(img, 50, 100)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == img.shape[:2]
    assert np.array_equal(got, natural_edges(case, setting)[0])
    assert np.array_equal(det(img, 100.9, 50.9), got)  # floats floored, low > high swapped

    def apply_control(x, detector, config):  # the reference's, run_fresco.py:102-109
        if config['controlnet_type'] == 'canny':
            detected_map = detector(x, 50, 100)
        return detected_map

    assert np.array_equal(apply_control(img, det, {'controlnet_type': 'canny'}), got)


def test_detect_batch_list_tensor_and_frames_one_by_one():
    import fresco_amd
    case, setting = M.NATURAL_CASES[1], M.NATURAL_SETTINGS[0]
    frames = natural(case, 10.0)
    det = fresco_amd.CannyDetector()
    from_tensor = det.detect_batch(gpu(frames))
    assert from_tensor.is_cuda and from_tensor.dtype == torch.uint8 and tuple(from_tensor.shape) == frames.shape[:3]
    assert np.array_equal(from_tensor.cpu().numpy(), natural_edges(case, setting))
    from_list = det.detect_batch([f.copy() for f in frames])
    assert torch.equal(from_list, from_tensor)
    for i in range(len(frames)):
        assert torch.equal(det.detect_batch(gpu(frames[i:i + 1]))[0], from_tensor[i])
    assert torch.equal(det.detect_batch(gpu(frames)), from_tensor)  # two runs, the same bits
    case20, setting20 = M.NATURAL_CASES[2], M.NATURAL_SETTINGS[1]
    got = det.detect_batch(gpu(natural(case20, 20.0)), 100, 200)
    assert np.array_equal(got.cpu().numpy(), natural_edges(case20, setting20))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_control_image(dtype):
    import fresco_amd
    case, setting = M.NATURAL_CASES[1], M.NATURAL_SETTINGS[0]
    frames, edges = natural(case, 10.0), natural_edges(case, setting)
    det = fresco_amd.CannyDetector()
    for guidance in (True, False):
        got = det.control_image(gpu(frames), dtype, guidance=guidance)
        want = _reference_condition(edges, dtype, guidance)
        assert got.dtype == dtype and tuple(got.shape) == ((6 if guidance else 3), 3, 70, 75)
        assert torch.equal(got, want)
        assert bool(((got == 0) | (got == 1)).all()) and bool((got == 1).any())
    assert torch.equal(det.control_image([f.copy() for f in frames], dtype, guidance=False), want)


def test_detect_batch_on_a_side_stream():
    import fresco_amd
    case, setting = M.NATURAL_CASES[2], M.NATURAL_SETTINGS[0]
    frames = gpu(natural(case, 10.0))
    det = fresco_amd.CannyDetector()
    on_default = det.detect_batch(frames)
    cond_default = det.control_image(frames, torch.float16, guidance=False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = det.detect_batch(frames)
        cond_side = det.control_image(frames, torch.float16, guidance=False)
    side.synchronize()
    assert torch.equal(on_side, on_default) and torch.equal(cond_side, cond_default)
    assert np.array_equal(on_side.cpu().numpy(), natural_edges(case, setting))
