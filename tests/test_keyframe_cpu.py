"""fresco_amd's key-frame selection without a GPU: the numpy restatement of OpenCV's rules (tests/keyframe_model.py) against
independent definitions, the proof that the shared inputs can tell the rule variants apart, the error formula against torch's
fp32 mse_loss, the greedy selection against the golden recorded from the unmodified reference
(tests/golden/make_keyframe_golden.py), the keyframe_* entry points on the header / binding / export surface and their
argument checks (fake pointers: every check answers before any HIP call), the Python surface, and -- only where cv2 can be
imported -- the restatement against a real OpenCV."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import keyframe_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("keyframe_resize_table_bytes", "keyframe_resize_table", "keyframe_resize_area_u8", "keyframe_workspace_bytes",
               "keyframe_frame_errors")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
# the largest |model blur - fp64 separable Gaussian (scipy, mode='mirror')| over error_inputs(), in grey levels, measured on
# the CPU: what OpenCV's 8-bit weights [4 13 30 51 60 51 30 13 4] / 256 and its two roundings cost, not a kernel's error
MEASURED_BLUR_DEVIATION = 1.6281


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "keyframe_golden.npz")))


@pytest.fixture(scope="module")
def resized():
    return {name: M.resize_area(M.resize_input(name), *M.RESIZE_CASES[name][3:5]) for name in M.RESIZE_CASES}


# ---- the model against independent definitions
def test_blur_weights_by_error_diffusion():
    assert tuple(M.blur_weights()) == M.WEIGHTS and sum(M.WEIGHTS) == 256
    plain = M.blur_weights(plain=True)
    assert plain[4] == 61 and sum(plain) == 257 and plain[:4] == list(M.WEIGHTS[:4])


def test_constant_images_are_fixed_points(resized):
    for v in (0, 1, 77, 254, 255):
        assert (M.blur(np.full((2, 9, 13, 3), v, np.uint8)) == v).all()
        for name, (n, H0, W0, H, W, _) in M.RESIZE_CASES.items():
            if H0 * W0 <= 135 * 240:
                assert (M.resize_area(np.full((H0, W0, 3), v, np.uint8), H, W) == v).all(), (name, v)


def test_integer_factors_give_the_rounded_block_mean(resized):
    for name in ("factor2", "factor3", "factor4", "factor2x4", "identity"):
        n, H0, W0, H, W, _ = M.RESIZE_CASES[name]
        iy, ix = H0 // H, W0 // W
        s = M.resize_input(name).reshape(n, H, iy, W, ix, 3).astype(np.int64).sum((2, 4))
        if (iy, ix) == (2, 2):
            want = (s + 2) // 4                    # half up, in integers
        else:
            want = np.rint(s / float(iy * ix))     # half to even (numpy), exact in fp64
        assert np.array_equal(resized[name], want.astype(np.uint8)), name
    assert np.array_equal(resized["identity"], M.resize_input("identity"))


def _box_integral_mean(img, H, W):
    """the mean of the piecewise-constant image over each output cell, from cumulative sums interpolated at the cell edges"""
    H0, W0 = img.shape[:2]
    c = np.zeros((H0 + 1, W0 + 1, 3))
    c[1:, 1:] = img.astype(np.float64).cumsum(0).cumsum(1)

    def at(c, pos, axis):
        pos = np.minimum(pos, c.shape[axis] - 1.0)
        lo = np.minimum(np.floor(pos).astype(int), c.shape[axis] - 2)
        frac = (pos - lo).reshape([-1 if a == axis else 1 for a in range(3)])
        return np.take(c, lo, axis) * (1 - frac) + np.take(c, lo + 1, axis) * frac

    ys, xs = np.arange(H + 1) * (H0 / H), np.arange(W + 1) * (W0 / W)
    g = at(at(c, ys, 0), xs, 1)
    box = g[1:, 1:] - g[:-1, 1:] - g[1:, :-1] + g[:-1, :-1]
    return box / ((H0 / H) * (W0 / W))


def test_resize_stays_within_one_level_of_the_box_integral(resized):
    for name, (n, H0, W0, H, W, _) in M.RESIZE_CASES.items():
        src = M.resize_input(name)
        for f in range(n):
            d = np.abs(resized[name][f].astype(np.float64) - _box_integral_mean(src[f], H, W)).max()
            assert d <= 1.0, (name, d)


def test_blur_against_an_fp64_separable_gaussian():
    ndimage = pytest.importorskip("scipy.ndimage")
    k = M.gaussian_kernel()
    worst = 0.0
    for name, f in M.error_inputs().items():
        g = ndimage.correlate1d(ndimage.correlate1d(f.astype(np.float64), k, axis=2, mode="mirror"), k, axis=1, mode="mirror")
        d = float(np.abs(M.blur(f).astype(np.float64) - g).max())
        print("%s: %.4f levels" % (name, d))
        worst = max(worst, d)
    assert worst <= MEASURED_BLUR_DEVIATION + 1.0, worst


def test_the_inputs_can_tell_the_rules_apart(resized):
    inputs = M.error_inputs()
    for variant in ("plain_rounded_weights", "reflect", "truncate"):
        for name in ("5x5", "ragged", "narrow", "five"):
            f = inputs[name]
            assert (M.blur(f, variant) != M.blur(f)).any(), (variant, name)
            assert M.sq_diffs(f, variant=variant) != M.sq_diffs(f), (variant, name)
    for variant, names in (("half_up", ("factor4", "factor2x4")), ("two_by_two_float", ("factor2",))):
        for name in names:
            got = M.resize_area(M.resize_input(name), *M.RESIZE_CASES[name][3:5], variant=variant)
            assert (got != resized[name]).any(), (variant, name)
    assert set(M.VARIANT_NAMES) == {"plain_rounded_weights", "reflect", "truncate", "half_up", "two_by_two_float"}


def test_the_tables_cover_each_cell_once():
    for ssize, dsize in ((1080, 512), (1920, 896), (135, 64), (240, 112), (100, 37), (75, 75), (77, 31), (1500, 1400)):
        ofs, si, alpha = M.area_table(ssize, dsize)
        assert si.min() >= 0 and si.max() == ssize - 1 and len(ofs) == dsize + 1 and alpha.dtype == np.float32
        for d in range(dsize):
            a, s = alpha[ofs[d]:ofs[d + 1]], si[ofs[d]:ofs[d + 1]]
            assert abs(float(a.astype(np.float64).sum()) - 1.0) < 1e-6 and (np.diff(s) == 1).all(), (ssize, dsize, d)
    assert M.area_scale(1080, 512) == (2.109375, 2, False) and M.area_scale(96, 32)[1:] == (3, True)


def test_the_library_builds_the_model_tables():
    """keyframe_resize_table (host memory, no HIP call) against the numpy restatement: every offset, index and float"""
    from fresco_amd import _lib
    lib = _lib.load()
    for name, (n, H0, W0, H, W, _) in list(M.RESIZE_CASES.items()) + [("1080p", (1, 1080, 1920, 512, 896, None))]:
        need = lib.keyframe_resize_table_bytes(H0, W0, H, W)
        host = (ctypes.c_int32 * (need // 4))()
        assert lib.keyframe_resize_table(H0, W0, H, W, ctypes.addressof(host), need) == 0
        words, floats = np.frombuffer(host, np.int32), np.frombuffer(host, np.float32)
        at = 0
        for ssize, dsize in ((W0, W), (H0, H)):
            cap = ssize + 2 * dsize
            ofs, si, alpha = words[at:at + dsize + 1], words[at + dsize + 1:][:cap], floats[at + dsize + 1 + cap:][:cap]
            at += dsize + 1 + 2 * cap
            want_ofs, want_si, want_alpha = M.area_table(ssize, dsize)
            k = len(want_si)
            assert k <= cap and np.array_equal(ofs, want_ofs) and np.array_equal(si[:k], want_si), name
            assert np.array_equal(alpha[:k], want_alpha) and not si[k:].any() and not alpha[k:].any(), name
        assert at * 4 == need


def test_error_inputs_are_what_they_are_for():
    inputs = M.error_inputs()
    assert M.sq_diffs(inputs["identical"]) == [0, 0] and M.sq_diffs(inputs["single"]) == [0]
    sat = M.sq_diffs(inputs["saturated"])
    assert sat == [0, 160 * 144 * 3 * 255 * 255] and sat[1] > 2 ** 32
    five = inputs["five"]
    whole = M.sq_diffs(five)
    parts = M.sq_diffs(five[:2]) + M.sq_diffs(five[2:4], carry=five[1]) + M.sq_diffs(five[4:], carry=five[3])
    assert parts == whole and all(v > 0 for v in whole[1:])
    with pytest.raises(ValueError):
        M.blur(np.zeros((4, 9, 3), np.uint8))


# ---- the formula and the selection
def test_error_formula_is_the_reference_mse_loss():
    """S * 4 / (65025 * 3 H W) against F.mse_loss(x / 255 * 2 - 1, ...) in fp32 on the CPU: 1e-4 relative.  Each operand
    carries two fp32 roundings (the division, the multiplication; the subtraction of 1 is then exact or one more), 2^-23
    relative to values up to 1 against a smallest non-zero difference of 2 / 255: about 3e-5 relative per difference."""
    for name in ("ragged", "five", "5x5", "saturated"):
        f = M.error_inputs()[name]
        H, W = f.shape[1:3]
        ours = M.error_curve(M.sq_diffs(f), H, W)
        t = [torch.from_numpy(b.copy()).float() / 255.0 * 2.0 - 1. for b in M.blur(f)]
        for i in range(1, len(f)):
            ref = float(torch.nn.functional.mse_loss(t[i - 1], t[i]))
            assert abs(ours[i] - ref) <= 1e-4 * ref, (name, i, ours[i], ref)
        assert ours[0] == 0.0


def test_package_curve_formula_equals_the_model():
    from fresco_amd import keyframe
    sums = torch.tensor([0, 123456789, 4494528000, 17], dtype=torch.int64)
    assert np.array_equal(keyframe._curve(sums, (160, 144)), M.error_curve(sums.tolist(), 160, 144))
    assert keyframe._curve(None, None).tolist() == [0.0]


def test_select_keyframes_reproduces_the_golden(golden):
    from fresco_amd import select_keyframes
    assert sorted(golden["names"].tolist()) == sorted(M.GOLDEN_CASES)
    for name in M.GOLDEN_CASES:
        served, reported, lastframen, mininterv, maxinterv = golden[name + "_args"].tolist()
        assert (served, reported, lastframen, mininterv, maxinterv) == M.GOLDEN_CASES[name]
        if mininterv == maxinterv:
            continue
        assert select_keyframes(golden[name + "_err"], mininterv, maxinterv) == golden[name + "_keys"].tolist(), name
    assert golden["ordinary_keys"].tolist() == [0, 9, 24, 39]
    assert golden["short_keys"].tolist() == [0, 7] and golden["mininterv_zero_keys"].tolist() == [0, 7]
    assert golden["equal_intervals_keys"].tolist() == list(range(0, 37, 5))


def test_select_keyframes_quirks():
    from fresco_amd import select_keyframes
    err = [0, 1, 5, 2, 9, 3, 4, 8, 1, 2, 3, 7]
    assert select_keyframes(err, 2, 3) == [0, 4, 7, 9, 11]
    assert select_keyframes(err, 0, 3) == [0, 11]                  # err[-0:] blanks everything
    # the first index of the maximum, and err[ind - 1 : ind + 1] blanks ind - 1 and ind only: ind + 1 is the next key
    assert select_keyframes([0, 3, 3, 3, 3, 3, 3], 1, 2) == [0, 1, 2, 3, 4, 6]
    assert select_keyframes([0.0], 5, 20) == [0, 0]                # one frame (or none): n - 1 = 0
    assert select_keyframes(err, 5, 100) == [0, 11]                # nothing to do
    given = np.array(err, dtype=np.float64)
    select_keyframes(given, 2, 3)
    assert given.tolist() == err                                   # the caller's curve is left alone


def test_model_curve_matches_the_golden_curves(golden):
    """the reference's fp32 mse_loss curve against the formula on the same (model) frames, through the whole golden chain"""
    frames = M.synthetic_frames(int(golden["seed"]), int(golden["frames"]))[:12]  # (the draws depend on the count)
    H, W, k = M.resize_size(*frames.shape[1:3], 512)
    assert (H, W) == (512, 576) and k < 1
    ours = M.error_curve(M.sq_diffs(M.resize_area(frames, H, W)), H, W)
    ref = golden["ordinary_err"][:12]
    assert ours[0] == ref[0] == 0
    assert np.all(np.abs(ours[1:] - ref[1:]) <= 1e-4 * ref[1:])


# ---- the C surface
def _keyframe_prototypes():
    """name -> (restype, argtypes) of the keyframe_* prototypes of include/fresco_keyframe.h (the idea of
    tests/test_capi_surface_cpu.py's _prototypes, for the other header and prefix)"""
    scalars = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
               "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}

    def ctype(decl):
        if "*" in decl:
            return ctypes.c_void_p
        return scalars[re.sub(r"\bconst\b", " ", decl).split()[0]]

    header = open(os.path.join(ROOT, "include", "fresco_keyframe.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s]*?\*?)\s*\b(keyframe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        assert name not in protos, name
        protos[name] = (scalars[ret.split()[-1]], [ctype(a) for a in params.split(",")])
    assert "fresco_" not in header  # it declares no fresco_* name
    return protos


def test_header_binding_and_exports_agree():
    import test_capi_surface_cpu as surface
    from fresco_amd import _lib
    protos = _keyframe_prototypes()
    assert set(protos) == set(_lib.KEYFRAME_SIGNATURES) == set(NEW_SYMBOLS)
    for name, (res, args) in protos.items():
        assert _lib.KEYFRAME_SIGNATURES[name][0] is res, name
        assert list(_lib.KEYFRAME_SIGNATURES[name][1]) == args, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is protos[name][0] and list(fn.argtypes) == protos[name][1]
    assert not set(_lib.KEYFRAME_SIGNATURES) & set(_lib.SIGNATURES)
    assert not [n for n in surface._exported_fresco_functions(_lib.LIB_PATH) if "keyframe" in n]
    assert _exported_keyframe_functions(_lib.LIB_PATH) == set(NEW_SYMBOLS)


def _exported_keyframe_functions(path):
    """names of the defined global functions `keyframe_*` in the .dynsym of an ELF64 shared object"""
    import struct
    data = open(path, "rb").read()
    assert data[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, sh_type, _, _, off, size, link, _, _, entsize in sections:
        if sh_type != 11:  # SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for i in range(size // entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", data, off + i * entsize)
            name = data[str_off + st_name:data.index(b"\0", str_off + st_name)].decode()
            if st_shndx != 0 and st_info >> 4 in (1, 2) and st_info & 15 == 2 and name.startswith("keyframe_"):
                names.add(name)
    return names


def test_entry_points_check_their_arguments_before_any_launch():
    from fresco_amd import _lib
    lib = _lib.load()
    p = 4096  # fake, aligned, never touched

    tb = lib.keyframe_resize_table_bytes(135, 240, 64, 112)
    assert tb == 4 * (113 + 2 * (240 + 224) + 65 + 2 * (135 + 128))
    for bad in ((0, 240, 64, 112), (135, 240, 0, 112), (135, 240, 136, 112), (135, 240, 64, 241), ((1 << 24) + 1, 8, 8, 8)):
        assert lib.keyframe_resize_table_bytes(*bad) == 0
    host = (ctypes.c_int32 * (tb // 4))()
    assert lib.keyframe_resize_table(135, 240, 64, 112, None, tb) == EINVAL
    assert lib.keyframe_resize_table(135, 240, 64, 112, ctypes.addressof(host), tb - 1) == EWORKSPACE
    assert lib.keyframe_resize_table(135, 240, 64, 241, ctypes.addressof(host), tb) == EUNSUPPORTED
    assert lib.keyframe_resize_table(135, -1, 64, 112, ctypes.addressof(host), tb) == EINVAL
    assert not any(host)                                                     # nothing was written by the refused calls

    def resize(src=p, dst=p, tab=p, tbytes=tb, n=2, H0=135, W0=240, H=64, W=112):
        return lib.keyframe_resize_area_u8(src, dst, tab, tbytes, n, H0, W0, H, W, None)

    assert resize(src=None) == EINVAL and resize(dst=None) == EINVAL and resize(tab=None) == EINVAL
    assert resize(tab=p + 2) == EINVAL
    for k in ("n", "H0", "W0", "H", "W"):
        assert resize(**{k: 0}) == EINVAL and resize(**{k: -2}) == EINVAL
    assert resize(H=136) == EUNSUPPORTED and resize(W=241) == EUNSUPPORTED   # a side enlarged
    assert resize(H0=64, H=65, W0=240, W=100) == EUNSUPPORTED
    assert resize(n=1 << 20, H0=1 << 12, W0=1 << 12, H=64, W=64, tbytes=1 << 30) == EUNSUPPORTED   # 3 x 2^44 bytes
    assert resize(n=1 << 12, H0=1 << 10, W0=1 << 10, H=1 << 10, W=1 << 10, tbytes=1 << 30) == EUNSUPPORTED  # 2^32 pixels
    assert resize(tbytes=tb - 1) == EWORKSPACE and resize(tbytes=0) == EWORKSPACE

    n, H, W = 3, 70, 131
    need = lib.keyframe_workspace_bytes(n, H, W)
    assert need >= n * 3 * 5 * 8                                             # one 64-bit partial per tile and pair
    assert lib.keyframe_workspace_bytes(1, 5, 5) >= 8
    for bad in ((0, H, W), (n, 0, W), (n, H, -1), (n, 4, W), (n, H, 4), (1 << 20, 1 << 12, 1 << 12)):
        assert lib.keyframe_workspace_bytes(*bad) == 0

    def errors(frames=p, carry=None, err=p, ws=p, wsb=need, n=n, H=H, W=W):
        return lib.keyframe_frame_errors(frames, carry, err, ws, wsb, n, H, W, None)

    assert errors(frames=None) == EINVAL and errors(err=None) == EINVAL and errors(ws=None) == EINVAL
    for k in ("n", "H", "W"):
        assert errors(**{k: 0}) == EINVAL
    assert errors(err=p + 4) == EINVAL and errors(ws=p + 4) == EINVAL        # 64-bit words
    assert errors(H=4) == EUNSUPPORTED and errors(W=4) == EUNSUPPORTED      # the reflection would fold twice
    assert errors(n=1 << 20, H=1 << 12, W=1 << 12, wsb=1 << 40) == EUNSUPPORTED
    assert errors(wsb=need - 1) == EWORKSPACE and errors(wsb=0) == EWORKSPACE
    assert errors(carry=p, wsb=need - 1) == EWORKSPACE


# ---- the Python surface
def test_resize_size_against_hand_computed_sizes():
    from fresco_amd import resize_size
    assert resize_size(1080, 1920, 512)[:2] == (512, 896)     # 910.2 / 64 = 14.2
    assert resize_size(720, 1280, 512)[:2] == (512, 896)      # 910.2 again
    assert resize_size(576, 640, 512)[:2] == (512, 576)       # 568.9 / 64 = 8.9
    assert resize_size(512, 512, 512) == (512, 512, 1.0)
    assert resize_size(800, 600, 512)[:2] == (704, 512)       # 682.7 / 64 = 10.7
    assert resize_size(1080, 1080 * 3 // 2 + 60, 512)[:2] == (512, 768)   # 796.4 / 64 = 12.4
    assert resize_size(512, 800, 512)[:2] == (512, 768)       # 12.5: np.round goes to the even 12
    assert resize_size(512, 928, 512)[:2] == (512, 896)       # 14.5 -> 14
    assert resize_size(270, 480, 512)[2] > 1
    for args in ((1080, 1920, 512), (576, 640, 512), (512, 800, 512), (333, 517, 256)):
        assert resize_size(*args) == M.resize_size(*args)


def test_exports_and_patch_keyframe_selection(monkeypatch):
    import sys
    import fresco_amd
    from fresco_amd import keyframe
    names = ("get_keyframe_ind", "frame_errors", "select_keyframes", "resize_frames", "resize_image", "resize_size",
             "patch_keyframe_selection")
    for name in names:
        assert getattr(fresco_amd, name) is getattr(keyframe, name) and name in fresco_amd.__all__
    star = types.ModuleType("run_fresco_standin")  # a module that imported the name
    star.get_keyframe_ind = object
    assert keyframe.patch_keyframe_selection(star) is star and star.get_keyframe_ind is keyframe.get_keyframe_ind
    src, mod = types.ModuleType("src"), types.ModuleType("src.keyframe_selection")
    src.keyframe_selection = mod
    mod.get_keyframe_ind = object
    monkeypatch.setitem(sys.modules, "src", src)
    monkeypatch.setitem(sys.modules, "src.keyframe_selection", mod)
    assert keyframe.patch_keyframe_selection() is mod and mod.get_keyframe_ind is keyframe.get_keyframe_ind


def test_python_side_refusals():
    import fresco_amd
    from fresco_amd import FrescoHipError, ops
    cpu = torch.zeros(2, 600, 800, 3, dtype=torch.uint8)
    with pytest.raises(FrescoHipError, match="GPU only"):
        fresco_amd.resize_frames(cpu)                                    # no host fallback
    with pytest.raises(FrescoHipError, match="GPU only"):
        fresco_amd.frame_errors(torch.zeros(2, 8, 9, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="LANCZOS"):
        fresco_amd.resize_frames(torch.zeros(1, 270, 480, 3, dtype=torch.uint8))   # k > 1
    with pytest.raises(NotImplementedError, match="enlarges a side"):
        fresco_amd.resize_frames(torch.zeros(1, 600, 500, 3, dtype=torch.uint8), 500)   # k = 1, but 500 -> 512 > W0
    with pytest.raises(TypeError):
        fresco_amd.resize_frames(torch.zeros(1, 600, 800, 3))
    with pytest.raises(ValueError):
        fresco_amd.resize_frames(torch.zeros(600, 800, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        fresco_amd.resize_image(np.zeros((600, 800, 3), np.float32), 512)
    with pytest.raises(TypeError):
        fresco_amd.frame_errors(np.zeros((2, 8, 9, 3), np.float32))
    with pytest.raises(TypeError):
        ops.resize_area_u8(torch.zeros(1, 8, 9, 3), 4, 4)
    with pytest.raises(ValueError):
        ops.resize_area_u8(torch.zeros(1, 8, 9, 1, dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError):
        ops.resize_area_u8(torch.zeros(1, 8, 9, 3, dtype=torch.uint8), 0, 4)
    with pytest.raises(ValueError):
        ops.frame_sq_diffs(torch.zeros(2, 8, 9, 3, dtype=torch.uint8), torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.frame_sq_diffs(torch.zeros(2, 8, 9, 3, dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(NotImplementedError, match="viz"):
        fresco_amd.get_keyframe_ind([np.zeros((600, 800, 3), np.uint8)], viz=True)
    # equal intervals: the reference's range, no frame touched -- and its TypeError for the default lastframen
    assert fresco_amd.get_keyframe_ind(None, 37, 5, 5) == list(range(0, 37, 5))
    with pytest.raises(TypeError):
        fresco_amd.get_keyframe_ind(None, mininterv=5, maxinterv=5)


def test_a_file_name_needs_cv2(monkeypatch):
    import sys
    import fresco_amd
    monkeypatch.setitem(sys.modules, "cv2", None)  # import cv2 -> ImportError
    with pytest.raises(fresco_amd.FrescoHipError, match="cv2"):
        fresco_amd.get_keyframe_ind("video.mp4")


# ---- against a real OpenCV, where there is one
@pytest.mark.parametrize("name", sorted(M.RESIZE_CASES))
def test_resize_model_equals_cv2_where_cv2_exists(name, resized):
    cv2 = pytest.importorskip("cv2")
    n, H0, W0, H, W, _ = M.RESIZE_CASES[name]
    for f, want in zip(M.resize_input(name), resized[name]):
        assert np.array_equal(cv2.resize(f, (W, H), interpolation=cv2.INTER_AREA), want)


def test_blur_model_equals_cv2_where_cv2_exists():
    cv2 = pytest.importorskip("cv2")
    for name, frames in M.error_inputs().items():
        for f in frames:
            assert np.array_equal(cv2.GaussianBlur(f, (9, 9), 0), M.blur(f)), name
