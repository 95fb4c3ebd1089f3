"""fresco_amd's tap resizes (INTER_LANCZOS4, and INTER_AREA where a side is enlarged) without a GPU: the library's host-side
tap tables against the numpy restatement (tests/resize_model.py), the int32 bound of the Lanczos accumulator derived from the
restatement's tables, the frame_resize_* entry points on the header / binding / export surface and their argument checks (fake
pointers: every check answers before any HIP call), the restatement against independent fp64 definitions, the proof that the
shared inputs can tell the rule variants apart, the dispatch of resize_image, the Python surface, and -- only where cv2 can be
imported -- the restatement against a real OpenCV."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import keyframe_model as KM
import resize_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("frame_resize_table_bytes", "frame_resize_table", "frame_resize_u8")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
# the largest |restatement - fp64 separable Lanczos-4 (sinc(x) sinc(x / 4), replicate borders, the same sample positions,
# clipped to 0..255)| over the LANCZOS4 cases of TAPS_CASES, in grey levels, measured on the CPU: what OpenCV's 11-bit
# coefficients (sums 2046 .. 2050, not 2048) and the one rounding cost, not a kernel's error
MEASURED_LANCZOS_DEVIATION = 0.8519
# the same for LINEAR_AREA against its own weights (1 - fx, fx) evaluated in fp64: the 11-bit coefficients, the two
# truncating shifts of the vertical pass and the final rounding
MEASURED_LINEAR_AREA_DEVIATION = 0.7590


@pytest.fixture(scope="module")
def resized():
    return {name: R.resize_taps(R.taps_input(name), c[4], c[5], c[0]) for name, c in R.TAPS_CASES.items()}


def _axes():
    """every (ssize, dsize) the shared geometries and the named ones hold"""
    axes = set(R.TABLE_AXES)
    for method, n, H0, W0, H, W, _ in R.TAPS_CASES.values():
        axes.update(((W0, W), (H0, H)))
    return sorted(axes)


# ---- the library's tables
def _library_table(lib, H0, W0, H, W, method):
    K = R.TAPS[method]
    need = lib.frame_resize_table_bytes(H0, W0, H, W, method)
    assert need == 4 * W + 2 * K * W + 4 * H + 2 * K * H
    host = (ctypes.c_int32 * (need // 4))()
    assert lib.frame_resize_table(H0, W0, H, W, method, ctypes.addressof(host), need) == 0
    raw, at, out = np.frombuffer(host, np.uint8), 0, []
    for dsize in (W, H):
        first = raw[at:at + 4 * dsize].view(np.int32)
        coef = raw[at + 4 * dsize:at + (4 + 2 * K) * dsize].view(np.int16).reshape(dsize, K)
        at += (4 + 2 * K) * dsize
        out.append((first, coef))
    assert at == need
    return out


@pytest.mark.parametrize("method", [R.LANCZOS4, R.LINEAR_AREA])
def test_the_library_builds_the_model_tables(method):
    """frame_resize_table (host memory, no HIP call) against the numpy restatement: every index and every coefficient"""
    from fresco_amd import _lib
    lib = _lib.load()
    axes = _axes()
    assert set(R.TABLE_AXES) <= set(axes)
    for i, (ssize, dsize) in enumerate(axes):
        other = axes[(i + 1) % len(axes)]  # x and y of one call: two different axes
        (xf, xc), (yf, yc) = _library_table(lib, other[0], ssize, other[1], dsize, method)
        for got, (s, d) in (((xf, xc), (ssize, dsize)), ((yf, yc), other)):
            want_first, want_coef = R.taps_table(s, d, method)
            assert np.array_equal(got[0], want_first), (method, s, d)
            assert np.array_equal(got[1], want_coef), (method, s, d)


def test_lanczos_accumulator_stays_inside_int32():
    """over 4096 phases: P the largest positive, N the largest negative coefficient mass of one axis; the vertical pass of a
    0 / 255 image is bounded by 255 (P^2 + N^2), and with the rounding constant that stays below 2^31"""
    P = N = 0
    sums = set()
    for i in range(4096):
        c = R.lanczos_phase(np.float32(i / 4096.0))
        P, N = max(P, sum(v for v in c if v > 0)), max(N, -sum(v for v in c if v < 0))
        sums.add(sum(c))
    assert R.lanczos_phase(np.float32(0)) == [0, 0, 0, 2048, 0, 0, 0, 0]
    assert (min(sums), max(sums)) == (2046, 2050)   # no renormalisation: constants are checked below, not assumed
    assert (P, N) == (2780, 732)
    bound = 255 * (P * P + N * N) + (1 << 21)
    print("accumulator bound", bound, "of", 2 ** 31)
    assert bound == 2109474272 and bound < 2 ** 31
    # every axis the tests use stays inside the scan
    for ssize, dsize in _axes():
        c = R.lanczos_table(ssize, dsize)[1].astype(np.int64)
        assert np.where(c > 0, c, 0).sum(1).max() <= P and np.where(c < 0, -c, 0).sum(1).max() <= N, (ssize, dsize)


def test_adversarial_frame_reaches_the_extremes_of_its_geometry():
    frame, (ya, xa, top), (yb, xb, bottom) = R.adversarial(45, 80, 64, 128)
    raw = R.lanczos_raw(frame, 64, 128)[0]
    assert raw.max() == raw[ya, xa, 0] == top and raw.min() == raw[yb, xb, 0] == bottom
    assert top > 2 ** 30 and top + (1 << 21) < 2 ** 31 and bottom < -(2 ** 29)
    out = R.resize_lanczos4(frame, 64, 128)[0]
    assert out[ya, xa, 0] == 255 and out[yb, xb, 0] == 0


# ---- the C surface
def _resize_prototypes():
    """name -> (restype, argtypes) of the frame_resize_* prototypes of include/fresco_resize.h"""
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}

    def ctype(decl):
        if "*" in decl:
            return ctypes.c_void_p
        return scalars[re.sub(r"\bconst\b", " ", decl).split()[0]]

    header = open(os.path.join(ROOT, "include", "fresco_resize.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s]*?\*?)\s*\b(frame_resize_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        assert name not in protos, name
        protos[name] = (scalars[ret.split()[-1]], [ctype(a) for a in params.split(",")])
    assert "fresco_" not in header and "keyframe_" not in header  # it declares no name of the pinned surfaces
    return protos


def _exported_functions(path, prefix):
    """names of the defined global functions `prefix*` in the .dynsym of an ELF64 shared object"""
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
            if st_shndx != 0 and st_info >> 4 in (1, 2) and st_info & 15 == 2 and name.startswith(prefix):
                names.add(name)
    return names


def test_header_binding_and_exports_agree():
    from fresco_amd import _lib
    protos = _resize_prototypes()
    assert set(protos) == set(_lib.RESIZE_SIGNATURES) == set(NEW_SYMBOLS)
    for name, (res, args) in protos.items():
        assert _lib.RESIZE_SIGNATURES[name][0] is res, name
        assert list(_lib.RESIZE_SIGNATURES[name][1]) == args, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is protos[name][0] and list(fn.argtypes) == protos[name][1]
    assert not set(_lib.RESIZE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.KEYFRAME_SIGNATURES))
    assert _exported_functions(_lib.LIB_PATH, "frame_") == set(NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "fresco_resize.h")).read()
    assert re.search(r"#define FRAME_RESIZE_LANCZOS4 %d\b" % _lib.RESIZE_LANCZOS4, header)
    assert re.search(r"#define FRAME_RESIZE_LINEAR_AREA %d\b" % _lib.RESIZE_LINEAR_AREA, header)
    assert (_lib.RESIZE_LANCZOS4, _lib.RESIZE_LINEAR_AREA) == (R.LANCZOS4, R.LINEAR_AREA)


def test_entry_points_check_their_arguments_before_any_launch():
    from fresco_amd import _lib
    lib = _lib.load()
    p = 4096  # fake, aligned, never touched
    tb = lib.frame_resize_table_bytes(45, 80, 64, 128, R.LANCZOS4)
    assert tb == (4 + 16) * (128 + 64)
    assert lib.frame_resize_table_bytes(45, 80, 64, 128, R.LINEAR_AREA) == (4 + 4) * (128 + 64)
    method, n, H0, W0, H, W = R.REFUSED_CASE
    bad_geometries = ((0, 80, 64, 128, 0), (45, 80, 0, 128, 0), (45, 80, 64, -1, 1), (45, 80, 64, 128, 2), (45, 80, 64, 128, -1),
                      (H0, W0, H, W, method), (64, 129, 64, 64, R.LINEAR_AREA), ((1 << 24) + 1, 8, 1 << 24, 8, 0))
    for bad in bad_geometries:
        assert lib.frame_resize_table_bytes(*bad) == 0, bad
    assert lib.frame_resize_table_bytes(128, 64, 64, 64, R.LANCZOS4) > 0  # exactly 2 is taken
    host = (ctypes.c_int32 * (tb // 4))()
    addr = ctypes.addressof(host)
    assert lib.frame_resize_table(45, 80, 64, 128, 0, None, tb) == EINVAL
    assert lib.frame_resize_table(45, 80, 64, 128, 0, addr + 2, tb) == EINVAL
    assert lib.frame_resize_table(45, 80, 64, 128, 0, addr, tb - 1) == EWORKSPACE
    assert lib.frame_resize_table(45, 80, 64, 128, 7, addr, tb) == EINVAL
    assert lib.frame_resize_table(45, -1, 64, 128, 0, addr, tb) == EINVAL
    assert lib.frame_resize_table(H0, W0, H, W, method, addr, tb) == EUNSUPPORTED
    assert not any(host)                                                     # nothing was written by the refused calls

    def resize(src=p, dst=p, tab=p, tbytes=tb, n=2, H0=45, W0=80, H=64, W=128, method=R.LANCZOS4):
        return lib.frame_resize_u8(src, dst, tab, tbytes, n, H0, W0, H, W, method, None)

    assert resize(src=None) == EINVAL and resize(dst=None) == EINVAL and resize(tab=None) == EINVAL
    assert resize(tab=p + 2) == EINVAL
    for k in ("n", "H0", "W0", "H", "W"):
        assert resize(**{k: 0}) == EINVAL and resize(**{k: -2}) == EINVAL
    assert resize(method=2) == EINVAL and resize(method=-1) == EINVAL
    assert resize(H0=129) == EUNSUPPORTED and resize(W0=257) == EUNSUPPORTED   # a side shrinks by more than 2
    assert resize(H0=129, method=R.LINEAR_AREA) == EUNSUPPORTED
    assert resize(H0=(1 << 24) + 1, H=1 << 24, W0=1, W=1, tbytes=1 << 40) == EUNSUPPORTED
    assert resize(n=1 << 20, H0=1 << 12, W0=1 << 12, H=1 << 11, W=1 << 11, tbytes=1 << 30) == EUNSUPPORTED  # 3 x 2^44 bytes
    assert resize(n=1 << 12, H0=1 << 10, W0=1 << 10, H=1 << 10, W=1 << 10, tbytes=1 << 30) == EUNSUPPORTED  # 2^32 pixels
    assert resize(n=1 << 24, H0=1, W0=1, H=1, W=1, tbytes=1 << 30) == EUNSUPPORTED                          # 2^24 tiles
    assert resize(tbytes=tb - 1) == EWORKSPACE and resize(tbytes=0) == EWORKSPACE
    assert resize(method=R.LINEAR_AREA, tbytes=8 * 192 - 1) == EWORKSPACE


# ---- the restatement against independent definitions
def test_constant_images_are_fixed_points():
    """checked, not assumed: the Lanczos coefficients of a phase sum to 2046 .. 2050, and 255 * 2050^2 + 2^21 >> 22 is still
    255"""
    for v in (0, 1, 128, 254, 255):
        for name, (method, n, H0, W0, H, W, _) in R.TAPS_CASES.items():
            assert (R.resize_taps(np.full((H0, W0, 3), v, np.uint8), H, W, method) == v).all(), (name, v)


def _lanczos_fp64(img, H, W):
    """separable Lanczos-4 in fp64: L(u) = sinc(u) sinc(u / 4) on |u| < 4, the eight weights of a sample normalised to sum 1,
    replicate borders, samples at (d + 0.5) ssize / dsize - 0.5"""
    out = img.astype(np.float64)
    for axis, dsize in ((1, W), (0, H)):
        ssize = out.shape[axis]
        x = (np.arange(dsize) + 0.5) * (ssize / dsize) - 0.5
        s = np.floor(x).astype(int)
        acc, total = 0.0, 0.0
        shape = [-1 if a == axis else 1 for a in range(3)]
        for k in range(-3, 5):
            u = x - (s + k)
            w = np.sinc(u) * np.sinc(u / 4.0)
            acc = acc + w.reshape(shape) * np.take(out, np.clip(s + k, 0, ssize - 1), axis)
            total = total + w
        out = acc / total.reshape(shape)
    return np.clip(out, 0, 255)


def _linear_area_fp64(img, H, W):
    """the two-tap rule with its own weights in fp64: no fixed point, no shifts"""
    out = img.astype(np.float64)
    for axis, dsize in ((1, W), (0, H)):
        ssize = out.shape[axis]
        inv = dsize / ssize
        s = np.floor(np.arange(dsize) / inv).astype(int)
        fx = (np.arange(dsize) + 1) - (s + 1) * inv
        fx = np.where(fx <= 0, 0.0, fx - np.floor(fx))
        fx = np.where(s + 1 >= ssize, 0.0, fx)
        s = np.minimum(s, ssize - 1)
        shape = [-1 if a == axis else 1 for a in range(3)]
        out = (1 - fx).reshape(shape) * np.take(out, s, axis) + fx.reshape(shape) * np.take(out, np.minimum(s + 1, ssize - 1), axis)
    return out


def test_restatement_stays_near_the_fp64_interpolations(resized):
    worst = {R.LANCZOS4: 0.0, R.LINEAR_AREA: 0.0}
    for name, (method, n, H0, W0, H, W, _) in R.TAPS_CASES.items():
        src = R.taps_input(name)
        ref = _lanczos_fp64 if method == R.LANCZOS4 else _linear_area_fp64
        d = max(float(np.abs(resized[name][f].astype(np.float64) - ref(src[f], H, W)).max()) for f in range(n))
        print("%s: %.4f levels" % (name, d))
        worst[method] = max(worst[method], d)
    assert worst[R.LANCZOS4] <= MEASURED_LANCZOS_DEVIATION + 1.0, worst
    assert worst[R.LINEAR_AREA] <= MEASURED_LINEAR_AREA_DEVIATION + 1.0, worst


def test_an_axis_of_equal_sizes_is_a_copy(resized):
    for ssize in (1, 2, 64, 69, 512):
        first, coef = R.linear_area_table(ssize, ssize)
        assert np.array_equal(first, np.arange(ssize)) and (coef == (2048, 0)).all()
        first, coef = R.lanczos_table(ssize, ssize)
        assert np.array_equal(first, np.arange(ssize) - 3) and (coef == (0, 0, 0, 2048, 0, 0, 0, 0)).all()
    src = R.taps_input("linear_copy_axis")                       # 64 x 69 -> 64 x 72: rows are copies
    rows_only = R.resize_linear_area(src, 64, 69)
    assert np.array_equal(rows_only, src)
    cols = R.resize_linear_area(src[:, :1], 1, 72)               # one row, resized along x alone
    assert np.array_equal(resized["linear_copy_axis"][:, :1], cols)
    noise = KM.noise(1, 33, 47, 3)
    assert np.array_equal(R.resize_linear_area(noise, 33, 47), noise)
    assert np.array_equal(R.resize_lanczos4(noise, 33, 47), noise)


def test_clamped_values_on_the_fractional_case():
    """the Lanczos overshoot is there to be clamped: about 2 % of the values at each end on textured(1, 45, 80, 7)"""
    method, n, H0, W0, H, W, _ = R.TAPS_CASES["lanczos_fractional"]
    src = R.taps_input("lanczos_fractional")
    assert np.array_equal(src, KM.textured(1, 45, 80, 7))
    v = (R.lanczos_raw(src, H, W) + (1 << 21)) >> 22
    low, high = float((v < 0).mean()), float((v > 255).mean())
    print("clamped: %.4f at 0, %.4f at 255" % (low, high))
    assert 0.01 < low < 0.04 and 0.01 < high < 0.04


def test_the_inputs_can_tell_the_rules_apart(resized):
    for variant in R.LANCZOS_VARIANTS:
        for name in ("lanczos_fractional", "lanczos_three_frames", "lanczos_shrinks", "lanczos_near_half", "lanczos_odd_rows"):
            method, n, H0, W0, H, W, _ = R.TAPS_CASES[name]
            assert (R.resize_lanczos4(R.taps_input(name), H, W, variant) != resized[name]).any(), (variant, name)
    # single_shift needs both axes to interpolate: with beta = (2048, 0) -- a copied axis, and every index of the exact
    # 2 x, where the area rule repeats pixels -- ((h >> 9) + 2) >> 2 and (2048 h + 2^21) >> 22 are the same number
    linear = {"centre_rule": ("linear_copy_axis", "linear_shrink_grow", "linear_2x", "linear_odd_rows", "linear_ragged"),
              "single_shift": ("linear_shrink_grow", "linear_odd_rows", "linear_ragged")}
    for variant in R.LINEAR_VARIANTS:
        for name in linear[variant]:
            method, n, H0, W0, H, W, _ = R.TAPS_CASES[name]
            assert (R.resize_linear_area(R.taps_input(name), H, W, variant) != resized[name]).any(), (variant, name)
    assert set(R.LANCZOS_VARIANTS) == {"renormalised", "truncate", "reflect101", "corner"}
    assert set(R.LINEAR_VARIANTS) == {"centre_rule", "single_shift"}
    # the two methods differ from each other and from the area rule where both apply
    src = R.taps_input("linear_shrink_grow")
    assert (R.resize_lanczos4(src, 64, 72) != resized["linear_shrink_grow"]).any()
    same = KM.textured(1, 66, 70, 5)
    assert (R.resize_linear_area(same, 64, 64) != KM.resize_area(same, 64, 64)).any()


# ---- the dispatch and the Python surface
def test_dispatch_follows_resize_image_and_cv_resize():
    from fresco_amd import resize_size
    for (H0, W0), (H, W, how) in R.DISPATCH_CASES.items():
        assert R.dispatch(H0, W0, 512) == (H, W, how), (H0, W0)
        assert resize_size(H0, W0, 512)[:2] == (H, W)
        k = resize_size(H0, W0, 512)[2]
        assert (k > 1) == (how == "lanczos4")
        if how == "linear_area":
            assert H > H0 or W > W0
        # every geometry resize_image can produce stays inside the kernels' factor-2 bound
        assert H0 <= 2 * H and W0 <= 2 * W
    for how, ((n, H0, W0), (H, W)) in R.SMALL_DISPATCH.items():
        assert R.dispatch(H0, W0, 64) == (H, W, how.split("_shrinking")[0]), how
    assert R.dispatch(511, 530, 512)[:2] == (512, 512) and 530 > 512 > 511   # one side grows, one shrinks: Lanczos on both


def test_resize_frames_dispatches_with_enlarge(monkeypatch):
    """which binding each geometry reaches, with the bindings replaced: no GPU"""
    import fresco_amd
    from fresco_amd import keyframe, ops
    calls = []
    monkeypatch.setattr(keyframe.ops, "resize_taps_u8", lambda f, H, W, method: calls.append(("taps", H, W, method)))
    monkeypatch.setattr(keyframe.ops, "resize_area_u8", lambda f, H, W: calls.append(("area", H, W)))
    names = {"lanczos4": ("taps", ops.RESIZE_LANCZOS4), "linear_area": ("taps", ops.RESIZE_LINEAR_AREA), "area": ("area",)}
    for (H0, W0), (H, W, how) in R.DISPATCH_CASES.items():
        del calls[:]
        fresco_amd.resize_frames(torch.zeros(1, H0, W0, 3, dtype=torch.uint8), 512, enlarge=True)
        assert calls == [(names[how][0], H, W) + names[how][1:]], (H0, W0, calls)
        del calls[:]
        if how == "area":
            fresco_amd.resize_frames(torch.zeros(1, H0, W0, 3, dtype=torch.uint8), 512)
            assert calls == [("area", H, W)]
        else:
            with pytest.raises(NotImplementedError, match="enlarge=True"):
                fresco_amd.resize_frames(torch.zeros(1, H0, W0, 3, dtype=torch.uint8), 512)
            assert not calls


def test_python_side_refusals():
    import fresco_amd
    from fresco_amd import FrescoHipError, ops
    for shape, resolution in (((1, 270, 480, 3), 512), ((1, 512, 550, 3), 512), ((1, 600, 500, 3), 500)):
        with pytest.raises(FrescoHipError, match="GPU only"):       # dispatched, then refused for the device: no host fallback
            fresco_amd.resize_frames(torch.zeros(shape, dtype=torch.uint8), resolution, enlarge=True)
    with pytest.raises(NotImplementedError, match="LANCZOS"):        # the default is what it was
        fresco_amd.resize_frames(torch.zeros(1, 270, 480, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="enlarges a side"):
        fresco_amd.resize_frames(torch.zeros(1, 512, 550, 3, dtype=torch.uint8))
    with pytest.raises(FrescoHipError, match="GPU only"):
        fresco_amd.frame_errors(torch.zeros(2, 270, 480, 3, dtype=torch.uint8), 512)
    with pytest.raises(FrescoHipError, match="GPU only"):
        ops.resize_taps_u8(torch.zeros(1, 8, 9, 3, dtype=torch.uint8), 16, 16, ops.RESIZE_LANCZOS4)
    with pytest.raises(TypeError):
        ops.resize_taps_u8(torch.zeros(1, 8, 9, 3), 16, 16, ops.RESIZE_LANCZOS4)
    with pytest.raises(ValueError):
        ops.resize_taps_u8(torch.zeros(1, 8, 9, 1, dtype=torch.uint8), 16, 16, ops.RESIZE_LANCZOS4)
    with pytest.raises(ValueError):
        ops.resize_taps_u8(torch.zeros(1, 8, 9, 3, dtype=torch.uint8), 0, 16, ops.RESIZE_LANCZOS4)
    with pytest.raises(ValueError, match="method"):
        ops.resize_taps_u8(torch.zeros(1, 8, 9, 3, dtype=torch.uint8), 16, 16, 2)


def test_the_small_golden_is_what_its_generator_records():
    """the recorded cases are the shared ones, their sizes follow the dispatch, and the restatement's curve on the first
    frames matches the reference's fp32 mse_loss curve to the project's 1e-4"""
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "keyframe_small_golden.npz")))
    assert sorted(golden["names"].tolist()) == sorted(R.SMALL_GOLDEN_CASES)
    for name, (seed, n, H0, W0, mininterv, maxinterv) in R.SMALL_GOLDEN_CASES.items():
        assert golden[name + "_args"].tolist() == [seed, n, H0, W0, mininterv, maxinterv]
        err, keys = golden[name + "_err"], golden[name + "_keys"].tolist()
        assert len(err) == n and err[0] == 0 and keys[0] == 0 and keys[-1] == n - 1
        live = np.sort(err[1:])
        assert (np.diff(live) > 1e-3 * live[1:]).all(), name     # no argmax hangs on the summation order
        from fresco_amd import select_keyframes
        assert select_keyframes(err, mininterv, maxinterv) == keys, name
        H, W, how = R.dispatch(H0, W0, 512)
        assert golden[name + "_size"].tolist() == [H, W]
        assert how == ("lanczos4" if name.startswith("lanczos") else "linear_area")
        frames = KM.synthetic_frames(seed, n, H0, W0)[:3]
        small = R.resize_reference(frames, 512)
        assert small.shape == (3, H, W, 3)
        ours = KM.error_curve(KM.sq_diffs(small), H, W)
        assert np.all(np.abs(ours[1:] - err[1:3]) <= 1e-4 * err[1:3]), name


# ---- against a real OpenCV, where there is one
@pytest.mark.parametrize("name", sorted(n for n, c in R.TAPS_CASES.items() if c[0] == R.LANCZOS4))
def test_lanczos4_model_equals_cv2_where_cv2_exists(name, resized):
    cv2 = pytest.importorskip("cv2")
    method, n, H0, W0, H, W, _ = R.TAPS_CASES[name]
    for f, want in zip(R.taps_input(name), resized[name]):
        assert np.array_equal(cv2.resize(f, (W, H), interpolation=cv2.INTER_LANCZOS4), want)


@pytest.mark.parametrize("name", sorted(n for n, c in R.TAPS_CASES.items() if c[0] == R.LINEAR_AREA))
def test_linear_area_model_equals_cv2_where_cv2_exists(name, resized):
    cv2 = pytest.importorskip("cv2")
    method, n, H0, W0, H, W, _ = R.TAPS_CASES[name]
    for f, want in zip(R.taps_input(name), resized[name]):
        assert np.array_equal(cv2.resize(f, (W, H), interpolation=cv2.INTER_AREA), want)
