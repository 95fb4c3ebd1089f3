"""fresco_amd's Canny detector without a GPU: the numpy restatement of the rules (tests/canny_model.py) on the hand cases and
its threshold handling, the proof that the shared inputs can tell the rules apart -- the eight rule variants of classify, and
fourteen defects of the two union passes on the class maps the GPU tests use --, the flood fill against the union model and,
where scipy can be imported, against scipy's labelling, the C entry points on the header /
binding surface of the library and their argument checks (fake pointers: every check answers before any HIP call),
the Python surface, and -- only where cv2 can be imported -- the restatement against a real OpenCV."""
import ctypes
import types

import numpy as np
import pytest
import torch

import canny_model as M

NEW_SYMBOLS = ("fresco_canny_workspace_bytes", "fresco_canny_classify", "fresco_canny_hysteresis")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NATURAL = [(case, setting) for case in M.NATURAL_CASES for setting in M.NATURAL_SETTINGS]
NATURAL_IDS = ["%s-%d-%d" % (M.case_id(c), s[1], s[2]) for c, s in NATURAL]


# ---- the model
def test_hand_cases():
    e = M.canny(M.step_columns(6, 8, 4, 100), 50, 100)
    want = np.zeros((6, 8), np.uint8)
    want[:, 3] = 255
    assert np.array_equal(e, want)
    e = M.canny(M.step_rows(6, 8, 3, 100), 50, 100)
    want = np.zeros((6, 8), np.uint8)
    want[2] = 255
    assert np.array_equal(e, want)
    row = np.zeros((1, 7, 3), np.uint8)
    row[:, 3:] = 100
    assert M.canny(row, 50, 100).tolist() == [[0, 0, 255, 0, 0, 0, 0]]
    for v in (0, 77, 255):
        assert M.canny(np.full((1, 1, 3), v, np.uint8), 50, 100).tolist() == [[0]]


def test_threshold_handling():
    img = M.natural_case(M.NATURAL_CASES[0], 10.0)[0]
    base = M.classify(img, 50, 100)
    assert (base == 1).any() and (base == 2).any()
    assert np.array_equal(M.classify(img, 100, 50), base)
    assert np.array_equal(M.classify(img, 50.9, 100.9), base)
    assert not np.array_equal(M.classify(img, 60, 120), base)  # (the thresholds do matter on this image)


def test_hysteresis_model_on_the_constructed_maps():
    s = M.serpentine()
    assert int((s > 0).sum()) == 2660 and int((M.hysteresis(s) == 255).sum()) == 2660
    assert not M.hysteresis(M.serpentine(seed=False)).any()
    st = M.staircase()
    assert np.array_equal(M.hysteresis(st) == 255, st > 0)  # 8-connected
    cb = M.checkerboard()
    assert np.array_equal(M.hysteresis(cb) == 255, cb > 0)
    b = M.hysteresis(M.two_blobs())
    assert b[:, :36].sum() == 255 * 30 * 33 and not b[:, 36:].any()
    three = np.stack([np.full((9, 11), 2), np.ones((9, 11)), np.ones((9, 11))]).astype(np.uint8)
    assert M.hysteresis(three)[0].all() and not M.hysteresis(three)[1:].any()
    odd = np.array([[2, 3, 1], [255, 0, 0], [0, 0, 0]], np.uint8)  # 3 and 255 count as 0: the 1 is cut off
    assert M.hysteresis(odd).tolist() == [[255, 0, 0], [0, 0, 0], [0, 0, 0]]


@pytest.mark.parametrize("case,setting", NATURAL, ids=NATURAL_IDS)
def test_the_inputs_can_tell_the_rules_apart(case, setting):
    """on every frame of the natural batches each rule variant changes at least one pixel of the class map, and hysteresis
    has both work to do and something to refuse: at least 2 % of all pixels are weak and end kept, 2 % weak and dropped"""
    std, low, high = setting
    for f in M.natural_case(case, std):
        base = M.classify(f, low, high)
        for name in M.VARIANT_NAMES:
            d = int((M.classify(f, low, high, name) != base).sum())
            assert d >= 1, (name, d)
        kept, dropped = M.weak_fate(f, low, high)
        print("%s std %g: weak kept %.1f %%, weak dropped %.1f %%" % (M.case_id(case), std, 100 * kept, 100 * dropped))
        assert kept >= 0.02 and dropped >= 0.02


def _gpu_class_maps():
    """name -> class map, for every map the two GPU files hand to the hysteresis kernels by name"""
    import test_gpu_canny as small
    import test_gpu_canny_fullsize as full
    maps = {name: make() for name, make in small.CLASS_MAPS.items()}
    maps.update({"many_tiles_" + name: make() for name, make in full.MANY_TILES.items()})
    maps["corner_patterns"] = M.corner_patterns()
    maps["all_3x3"] = M.all_3x3_class_maps()
    return maps


def _seam_maps():
    import test_gpu_canny as small
    maps = {name: make() for name, make in small.SEAM_MAPS.items()}
    maps["corner_patterns"] = M.corner_patterns()
    return maps


def test_union_model_equals_hysteresis_on_every_map():
    """the two union passes as the kernels specify them label what the flood fill labels"""
    for name, cls in _gpu_class_maps().items():
        want = M.hysteresis(cls)
        got = M.union_hysteresis(cls)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    one = M.random_classes(1, 70, 75, 0.45, 0.004, seed=5)[0]
    assert np.array_equal(M.union_hysteresis(one), M.hysteresis(one))  # (H, W) as well as (n, H, W)


def test_the_maps_can_tell_the_union_defects_apart():
    """each named defect of the union passes (one link or one group of border pixels left out) changes a pixel of some
    small class map of the GPU tests -- and of some seam map (the anti-staircases, the sparse random map, the corner
    patterns), which cover all of them by themselves; the sparse random map alone shows each one through 3 pixels or more"""
    import test_gpu_canny as small
    assert len(M.UNION_DEFECT_NAMES) == 14 and len(set(M.UNION_DEFECT_NAMES)) == 14
    seam = _seam_maps()
    maps = {name: make() for name, make in small.CLASS_MAPS.items()}
    maps.update(seam)
    base = {name: M.hysteresis(cls) for name, cls in maps.items()}
    for defect in M.UNION_DEFECT_NAMES:
        seen = {name: int((M.union_hysteresis(cls, defect) != base[name]).sum()) for name, cls in maps.items()}
        print(defect, {k: v for k, v in seen.items() if v})
        assert any(seen[name] for name in small.CLASS_MAPS), defect
        assert any(seen[name] for name in seam), defect
        assert seen["random_sparse"] >= 3, (defect, seen["random_sparse"])
    # the link nothing saw before these maps: NE from a tile's top-right pixel into the tile diagonally above
    d = "border_ne_not_across_corner"
    assert int((M.union_hysteresis(maps["anti_staircase_64"], d) != base["anti_staircase_64"]).sum()) == 32
    old = ("serpentine", "serpentine_unseeded", "staircase", "checkerboard", "all_weak", "all_strong", "all_zero",
           "two_blobs", "three_frames", "odd_bytes", "random_near_percolation")
    assert all(np.array_equal(M.union_hysteresis(maps[name], d), base[name]) for name in old)


def test_hysteresis_model_equals_scipy_labelling():
    """rule 5 from an independent implementation: scipy's labelling of the class 1 / 2 pixels with the 3 x 3 structure"""
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, cls in _gpu_class_maps().items():
        want = np.zeros(cls.shape, np.uint8)
        for f, c in enumerate(cls):
            c = np.where(c <= 2, c, 0)
            lab, count = ndimage.label(c > 0, structure=np.ones((3, 3), int))
            keep = np.zeros(count + 1, bool)
            keep[lab[c == 2]] = True
            keep[0] = False
            want[f] = keep[lab] * 255
        assert np.array_equal(M.hysteresis(cls), want), name


def test_new_maps_are_what_they_are_for():
    a = M.anti_staircase(64, 64)
    assert a[0, 63] == 2 and int((a > 0).sum()) == 64 and a[31, 32] == 1 and a[32, 31] == 1  # the step across the corner
    for c in (M.serpentine(seed="last"), M.line(70, 75), M.line(70, 75, vertical=True), M.line(1, 97), M.line(97, 1, True)):
        assert int((c == 2).sum()) == 1 and np.flatnonzero(c)[-1] == np.flatnonzero(c == 2)[0]
        assert np.array_equal(M.hysteresis(c) == 255, c > 0)
    assert np.argwhere(M.serpentine(256, 256, seed="last") == 2).tolist() == [[255, 0]]
    for H, W in ((70, 75), (256, 256)):
        sp = M.spiral(H, W)
        count = int((sp > 0).sum())
        assert 0.45 * H * W < count < 0.55 * H * W and int((sp == 2).sum()) == 1 and sp[0, 0] == 1
        assert np.array_equal(M.hysteresis(sp) == 255, sp > 0)
        # one path and no way round: cut in its first arm, the inner seed lights all but the cut-off piece, the outer seed
        # that piece alone
        for seed, lit in (("last", count - 1 - W // 2), ("first", W // 2)):
            cut = M.spiral(H, W, seed=seed)
            cut[0, W // 2] = 0
            assert int((M.hysteresis(cut) == 255).sum()) == lit
        assert not M.hysteresis(M.spiral(H, W, seed=False)).any()
    cp = M.corner_patterns()
    assert cp.shape == (11264, 34, 34) and cp.dtype == np.uint8
    assert not cp[:, :30].any() and not cp[:, :, :30].any() and int((cp == 2).reshape(len(cp), -1).sum(1).max()) == 1
    for k, (r0, c0) in enumerate(((30, 30), (30, 31), (31, 30), (31, 31))):  # the four cuts, 2 816 different maps at each
        block = cp[2816 * k:2816 * (k + 1)]
        assert len({c.tobytes() for c in block}) == 2816 and block[-1, r0:r0 + 3, c0:c0 + 3].all()
    pool = M.all_3x3_class_maps()
    assert pool.shape == (19683, 3, 3) and len({c.tobytes() for c in pool}) == 19683 and pool.max() == 2


def test_the_large_gradient_frames_reach_the_ends_of_the_range():
    """the blocky frames reach dx, dy = +-1020 and m = 1530, take each of the three NMS branches with a component above 512,
    and hold weak and strong pixels at 1000 / 1500; on the uniform frame at 500 / 900 every rule variant changes a pixel"""
    for f in M.blocky(2, 70, 75, 3, seed=1):
        dx, dy = M.gradients(f)
        assert dx.min() == -1020 and dx.max() == 1020 and dy.min() == -1020 and dy.max() == 1020
        assert (np.abs(dx) + np.abs(dy)).max() == 1530
        branch, big = M.nms_branch(dx, dy), np.maximum(np.abs(dx), np.abs(dy)) > 512
        c = M.classify(f, 1000, 1500)
        for k in range(3):
            assert (big & (branch == k) & (c > 0)).any(), k
        print("blocky at 1000 / 1500: %d weak, %d strong" % (int((c == 1).sum()), int((c == 2).sum())))
        assert (c == 1).sum() > 500 and (c == 2).sum() > 250
    c = M.classify(M.blocky(1, 70, 75, 3, seed=1)[0], 1000, 1500)
    assert (int((c == 1).sum()), int((c == 2).sum())) == (1139, 557)
    u = M.uniform(1, 70, 75, seed=0)[0]
    dx, dy = M.gradients(u)
    assert dx.max() == 885 and dx.min() < -800 and dy.max() > 800 and dy.min() < -800
    base = M.classify(u, 500, 900)
    assert (base == 1).sum() > 1000 and (base == 2).sum() > 200
    for name in M.VARIANT_NAMES:
        assert int((M.classify(u, 500, 900, name) != base).sum()) >= 1, name
    for d in ("right", "left", "down", "up"):
        dx, dy = M.gradients(M.step(70, 75, d, 33))
        want = {"right": (0, 1020, 0, 0), "left": (-1020, 0, 0, 0), "down": (0, 0, 0, 1020), "up": (0, 0, -1020, 0)}[d]
        assert (dx.min(), dx.max(), dy.min(), dy.max()) == want


def test_uniform_noise_would_not_do():
    """the reason for the filtered field: on uniform uint8 noise hardly a survivor is weak"""
    img = np.random.RandomState(0).randint(0, 256, (64, 64, 3)).astype(np.uint8)
    c = M.classify(img, 50, 100)
    assert (c == 2).mean() > 0.05 and (c == 1).mean() < 0.01


# ---- the C surface
def test_entry_points_are_on_the_c_abi_surface():
    """per new symbol: the header's prototype (include/fresco_hip.h, section n) is the binding's, argument lists included, and
    libfresco_hip.so exports it; tests/test_capi_surface_cpu.py compares header, binding and exports as whole sets"""
    import test_capi_surface_cpu as surface
    from fresco_amd import _lib
    protos = surface._prototypes()
    exported = surface._exported_fresco_functions(_lib.LIB_PATH)
    assert {n for n in protos if "canny" in n} == set(NEW_SYMBOLS)
    assert {n for n in exported if "canny" in n} == set(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        res, args = _lib.SIGNATURES[name]
        assert res is protos[name][0] and list(args) == protos[name][1], name
    assert _lib.SIGNATURES["fresco_canny_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["fresco_canny_classify"][0] is ctypes.c_int
    assert _lib.SIGNATURES["fresco_canny_hysteresis"][0] is ctypes.c_int
    surface.test_binding_matches_the_header_prototypes()


def test_entry_points_check_their_arguments_before_any_launch():
    from fresco_amd import _lib
    lib = _lib.load()
    p = 4096  # fake, aligned, never touched
    n, H, W = 2, 70, 75
    need = lib.fresco_canny_workspace_bytes(n, H, W)
    assert need >= 4 * n * H * W
    assert lib.fresco_canny_workspace_bytes(1, 1, 1) >= 4
    for bad in ((0, H, W), (n, 0, W), (n, H, -1), (2, 32768, 32768), (1, 1 << 30, 2)):
        assert lib.fresco_canny_workspace_bytes(*bad) == 0
    assert lib.fresco_canny_workspace_bytes(1, 32768, 65535) >= 4 * 32768 * 65535  # just below 2^31

    def classify(frames=p, cls=p, n=n, H=H, W=W):
        return lib.fresco_canny_classify(frames, cls, n, H, W, 50, 100, None)

    assert classify(frames=None) == EINVAL
    assert classify(cls=None) == EINVAL
    for k in ("n", "H", "W"):
        assert classify(**{k: 0}) == EINVAL
        assert classify(**{k: -3}) == EINVAL
    assert classify(n=2, H=32768, W=32768) == EUNSUPPORTED

    def hyst(cls=p, out=p, cond=None, dt=_lib.F16, ws=p, wsb=need, n=n, H=H, W=W):
        return lib.fresco_canny_hysteresis(cls, out, cond, dt, ws, wsb, n, H, W, None)

    assert hyst(cls=None) == EINVAL
    assert hyst(out=None) == EINVAL
    assert hyst(ws=None) == EINVAL
    for k in ("n", "H", "W"):
        assert hyst(**{k: 0}) == EINVAL
    assert hyst(cond=p, dt=7) == EINVAL
    assert hyst(cond=p, dt=-1) == EINVAL
    assert hyst(ws=p + 2) == EINVAL                 # parent is read as 32-bit words
    assert hyst(cond=p + 2, dt=_lib.F32) == EINVAL
    assert hyst(wsb=need - 1) == EWORKSPACE
    assert hyst(wsb=0) == EWORKSPACE
    assert hyst(cond=p, dt=_lib.BF16, wsb=need - 1) == EWORKSPACE
    assert hyst(n=2, H=32768, W=32768, wsb=1 << 40) == EUNSUPPORTED
    assert hyst(dt=7, wsb=need - 1) == EWORKSPACE   # an unknown dtype matters only with a condition


# ---- the Python surface
def test_exports_and_patch_canny(monkeypatch):
    import sys
    import fresco_amd
    from fresco_amd import canny
    assert fresco_amd.CannyDetector is canny.CannyDetector and fresco_amd.patch_canny is canny.patch_canny
    assert "CannyDetector" in fresco_amd.__all__ and "patch_canny" in fresco_amd.__all__
    star = types.ModuleType("run_fresco_standin")  # a module that imported the name
    star.CannyDetector = object
    assert canny.patch_canny(star) is star and star.CannyDetector is canny.CannyDetector
    annotator, mod = types.ModuleType("annotator"), types.ModuleType("annotator.canny")
    annotator.canny = mod
    mod.CannyDetector = object
    monkeypatch.setitem(sys.modules, "annotator", annotator)
    monkeypatch.setitem(sys.modules, "annotator.canny", mod)
    assert canny.patch_canny() is mod and mod.CannyDetector is canny.CannyDetector


def test_python_side_refusals():
    from fresco_amd import canny, FrescoHipError
    det = canny.CannyDetector()
    ok = np.zeros((8, 9, 3), np.uint8)
    for bad in (np.zeros((8, 9), np.uint8), np.zeros((8, 9, 1), np.uint8)):
        with pytest.raises((TypeError, ValueError), match="Canny"):
            det(bad, 50, 100)
        with pytest.raises((TypeError, ValueError), match="Canny"):
            det.detect_batch([bad])
    with pytest.raises((TypeError, ValueError), match="Canny"):
        det.detect_batch(torch.zeros(2, 8, 9, 1, dtype=torch.uint8))
    with pytest.raises(TypeError, match="Canny"):
        det(ok.astype(np.float32), 50, 100)
    with pytest.raises(TypeError, match="Canny"):
        det.detect_batch(torch.zeros(1, 8, 9, 3))
    with pytest.raises(ValueError, match="Canny.*share a size"):
        det.detect_batch([ok, np.zeros((8, 10, 3), np.uint8)])
    with pytest.raises(ValueError, match="Canny"):
        det.detect_batch([])
    for low, high in ((float("nan"), 100), (50, float("inf")), (float("-inf"), 100)):
        with pytest.raises(ValueError, match="Canny"):
            det.detect_batch([ok], low, high)
    with pytest.raises(TypeError, match="Canny"):
        det.detect_batch([ok], "50", 100)
    with pytest.raises(TypeError, match="Canny"):
        det.control_image([ok], torch.float64)
    # a tensor batch stays where it is: on the CPU the operators refuse it
    with pytest.raises(FrescoHipError, match="GPU only"):
        det.detect_batch(torch.zeros(1, 8, 9, 3, dtype=torch.uint8))
    assert canny.check_thresholds(50.9, 100.9) == (50, 100) and canny.check_thresholds(np.float32(7.5), 3) == (7, 3)


# ---- against a real OpenCV, where there is one
@pytest.mark.parametrize("case,setting", NATURAL, ids=NATURAL_IDS)
def test_model_equals_cv2_where_cv2_exists(case, setting):
    cv2 = pytest.importorskip("cv2")
    std, low, high = setting
    for f in M.natural_case(case, std):
        assert np.array_equal(M.canny(f, low, high), cv2.Canny(f, low, high))
