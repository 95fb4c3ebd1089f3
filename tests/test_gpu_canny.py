"""fresco_amd's Canny kernels on the GPU against the numpy restatement of the rules (tests/canny_model.py): all integer, so
every comparison is for equality.  The classify pass alone, the hysteresis passes alone on constructed class maps (long
paths, corner connections, components that span many tiles, frame boundaries), and the detector end to end with the
condition tensor."""
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
}


@pytest.mark.parametrize("name", list(CLASS_MAPS))
def test_hysteresis_constructed_maps(name):
    cls = CLASS_MAPS[name]()
    want = M.hysteresis(cls)
    got, cond = hysteresis_gpu(cls)
    assert cond is None and got.dtype == np.uint8 and got.shape == cls.shape
    assert np.array_equal(got, want), "%d pixels differ" % int((got != want).sum())
    # what the case is there for
    lit = int((want == 255).sum())
    if name in ("serpentine", "staircase", "checkerboard", "all_strong"):
        assert lit == int((cls > 0).sum()) and lit > 0
        if name == "serpentine":
            assert lit == 2660
    elif name in ("serpentine_unseeded", "all_weak", "all_zero"):
        assert lit == 0
    elif name == "two_blobs":
        assert lit == 30 * 33 and not want[0][:, 36:].any()
    elif name == "three_frames":
        assert want[0].all() and not want[1:].any()
    elif name == "odd_bytes":
        assert lit == 40 and not want[0][0, 40:].any()  # row 0 up to the byte 3
    else:
        weak = cls == 1
        assert (want[weak] == 255).mean() > 0.5 and (want[weak] == 0).mean() > 0.02  # large components, and refused ones


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
