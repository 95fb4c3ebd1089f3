"""A numpy restatement of the rules fresco_amd's tap-resize kernels reproduce ("Enlarging"): what
cv2.resize does to an 8-bit image with INTER_LANCZOS4, and with INTER_AREA when a side is enlarged (a bilinear variant on the
area rule's sample positions), both through OpenCV's 11-bit fixed-point coefficients and 32-bit integer passes.  Like
tests/keyframe_model.py the rules are written from memory of OpenCV 4.x's resize.cpp (resizeGeneric_, interpolateLanczos4,
HResizeLanczos4 / VResizeLanczos4, HResizeLinear / VResizeLinear for uchar, int, short); tests/test_resize_cpu.py checks them
against independent definitions and, only where cv2 can be imported, against a real OpenCV.

variant=None is the rule; the named variants each break one of them, for the proof that the test inputs can tell them apart.
math.sin / math.cos are libm's, what the C side calls.  Also here: the cases the CPU and the GPU tests share, the dispatch of
resize_image, and a stand-in cv2 whose resize follows the interpolation flag it is given.
"""
import math

import numpy as np

import keyframe_model as KM

LANCZOS4, LINEAR_AREA = 0, 1          # the `method` codes of include/fresco_resize.h
TAPS = {LANCZOS4: 8, LINEAR_AREA: 2}
COEF_ONE = 2048                       # INTER_RESIZE_COEF_SCALE: 11 bits
LANCZOS_VARIANTS = ("renormalised", "truncate", "reflect101", "corner")
LINEAR_VARIANTS = ("centre_rule", "single_shift")
FLT_EPSILON = float(np.finfo(np.float32).eps)
_R = 0.70710678118654752440
_CS = ((1, 0), (-_R, -_R), (0, 1), (_R, -_R), (-1, 0), (_R, _R), (0, -1), (-_R, _R))
_PI = 3.1415926535897932384626433832795  # CV_PI


def axis_scale(ssize, dsize):
    """(inv, scale) as cv::resize forms them, in double"""
    inv = dsize / ssize
    return inv, 1.0 / inv


def _fixed(c):
    """short(round-half-even(c * 2048)) for a float32 c: the product is exact (a power of two)"""
    return int(np.rint(np.float32(c) * np.float32(COEF_ONE)))


def lanczos_coeffs(fx):
    """interpolateLanczos4 for a float32 phase fx in [0, 1): eight float32 coefficients.  x + 3 - i is formed in float; the
    angle, the sine / cosine and the quotient in double; the sum and the normalisation in float"""
    fx = np.float32(fx)
    if fx < np.float32(FLT_EPSILON):
        return [np.float32(v) for v in (0, 0, 0, 1, 0, 0, 0, 0)]
    y0 = -float(fx + np.float32(3)) * _PI * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c, total = [], np.float32(0)
    for i in range(8):
        y = -float(fx + np.float32(3) - np.float32(i)) * _PI * 0.25
        v = np.float32((_CS[i][0] * s0 + _CS[i][1] * c0) / (y * y))
        c.append(v)
        total = np.float32(total + v)
    inv = np.float32(np.float32(1) / total)
    return [np.float32(v * inv) for v in c]


def lanczos_phase(fx):
    """the eight fixed-point coefficients of a float32 phase"""
    return [_fixed(v) for v in lanczos_coeffs(fx)]


def lanczos_table(ssize, dsize, variant=None):
    """(first, coef): per output index the source index of the first of its eight taps (s - 3, unclamped) and the eight
    int16 coefficients"""
    _, scale = axis_scale(ssize, dsize)
    first, coef = np.empty(dsize, np.int64), np.empty((dsize, 8), np.int64)
    for d in range(dsize):
        fx = np.float32(d * scale) if variant == "corner" else np.float32((d + 0.5) * scale - 0.5)
        s = math.floor(fx)
        fx = np.float32(fx - np.float32(s))
        c = lanczos_phase(fx)
        if variant == "renormalised":  # the largest coefficient takes the remainder
            c[int(np.argmax(c))] += COEF_ONE - sum(c)
        first[d], coef[d] = s - 3, c
    assert np.abs(coef).max() < 32768
    return first, coef.astype(np.int16)


def linear_area_table(ssize, dsize, variant=None):
    """(first, coef): INTER_AREA's enlarging rule per axis -- s = floor(d * scale), the weight of s + 1 from the area
    overlap (d + 1) - (s + 1) * inv; taps s and s + 1, int16 coefficients (1 - fx, fx) * 2048"""
    inv, scale = axis_scale(ssize, dsize)
    first, coef = np.empty(dsize, np.int64), np.empty((dsize, 2), np.int64)
    for d in range(dsize):
        if variant == "centre_rule":  # INTER_LINEAR
            fx = np.float32((d + 0.5) * scale - 0.5)
            s = math.floor(fx)
            fx = np.float32(fx - np.float32(s))
            if s < 0:
                s, fx = 0, np.float32(0)
            if s >= ssize - 1:
                s, fx = ssize - 1, np.float32(0)
        else:
            s = math.floor(d * scale)
            fx = np.float32((d + 1) - (s + 1) * inv)
            fx = np.float32(0) if fx <= 0 else np.float32(fx - np.float32(math.floor(fx)))
            if s < 0:
                s, fx = 0, np.float32(0)
            if s + 1 >= ssize:
                s, fx = ssize - 1, np.float32(0)
        first[d] = s
        coef[d] = _fixed(np.float32(1) - fx), _fixed(fx)
    return first, coef.astype(np.int16)


def taps_table(ssize, dsize, method, variant=None):
    return lanczos_table(ssize, dsize, variant) if method == LANCZOS4 else linear_area_table(ssize, dsize, variant)


def _border(i, n, reflect):
    if not reflect:
        return np.clip(i, 0, n - 1)
    if n == 1:
        return np.zeros_like(i)
    i = np.abs(i) % (2 * n - 2)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _pass(src, tab, axis, reflect=False):
    """sum_k coef[d, k] * src[border(first[d] + k)] along `axis`, in integers"""
    first, coef = tab
    src = np.moveaxis(src, axis, 0)
    n = src.shape[0]
    out = np.zeros((len(first),) + src.shape[1:], np.int64)
    shape = (-1,) + (1,) * (src.ndim - 1)
    for k in range(coef.shape[1]):
        out += coef[:, k].astype(np.int64).reshape(shape) * src[_border(first + k, n, reflect)]
    return np.moveaxis(out, 0, axis)


def _frames(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3 and img.ndim in (3, 4)
    return img, img.ndim == 3


def lanczos_raw(img, H, W, variant=None):
    """the 32-bit accumulator before the shift: sum_j beta_j (sum_i alpha_i src[y_j][x_i]), rows first as resizeGeneric_"""
    img, _ = _frames(img)
    H0, W0 = img.shape[-3:-1]
    tv = variant if variant in ("renormalised", "corner") else None
    reflect = variant == "reflect101"
    h = _pass(img.astype(np.int64), lanczos_table(W0, W, tv), img.ndim - 2, reflect)
    v = _pass(h, lanczos_table(H0, H, tv), img.ndim - 3, reflect)
    assert np.abs(v).max() + (1 << 21) < 2 ** 31  # what the int32 of the kernel holds
    return v


def resize_lanczos4(img, H, W, variant=None):
    """cv2.resize(img, (W, H), interpolation=cv2.INTER_LANCZOS4) for uint8 (H0, W0, 3) or (n, H0, W0, 3)"""
    v = lanczos_raw(img, H, W, variant)
    v = (v >> 22) if variant == "truncate" else ((v + (1 << 21)) >> 22)  # arithmetic shifts
    return np.clip(v, 0, 255).astype(np.uint8)


def resize_linear_area(img, H, W, variant=None):
    """cv2.resize(img, (W, H), interpolation=cv2.INTER_AREA) where a side is enlarged: both axes take the two-tap rule"""
    img, _ = _frames(img)
    H0, W0 = img.shape[-3:-1]
    tv = variant if variant == "centre_rule" else None
    h = _pass(img.astype(np.int64), linear_area_table(W0, W, tv), img.ndim - 2)
    first, coef = linear_area_table(H0, H, tv)
    if variant == "single_shift":
        return np.clip((_pass(h, (first, coef), img.ndim - 3) + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    h = np.moveaxis(h, img.ndim - 3, 0)
    shape = (-1,) + (1,) * (h.ndim - 1)
    b0, b1 = (coef[:, k].astype(np.int64).reshape(shape) for k in (0, 1))
    h0, h1 = h[np.clip(first, 0, H0 - 1)], h[np.clip(first + 1, 0, H0 - 1)]
    v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    return np.moveaxis(np.clip(v, 0, 255).astype(np.uint8), 0, img.ndim - 3)


def resize_taps(img, H, W, method, variant=None):
    return resize_lanczos4(img, H, W, variant) if method == LANCZOS4 else resize_linear_area(img, H, W, variant)


# ---- the dispatch of resize_image + cv::resize
def dispatch(H0, W0, resolution):
    """(H, W, "lanczos4" | "area" | "linear_area")"""
    H, W, k = KM.resize_size(H0, W0, resolution)
    if k > 1:
        return H, W, "lanczos4"
    return H, W, ("area" if H <= H0 and W <= W0 else "linear_area")


def resize_reference(img, resolution):
    """src/utils.py resize_image on the restatements, for (H0, W0, 3) or (n, H0, W0, 3)"""
    img, _ = _frames(img)
    H, W, how = dispatch(img.shape[-3], img.shape[-2], resolution)
    if how == "lanczos4":
        return resize_lanczos4(img, H, W)
    return KM.resize_area(img, H, W) if how == "area" else resize_linear_area(img, H, W)


def standin_cv2(frames, reported_count=None):
    """keyframe_model's stand-in cv2 with a resize that follows the interpolation flag as cv::resize does"""
    cv2 = KM.standin_cv2(frames, reported_count)
    area_only = cv2.resize

    def resize(img, dsize, interpolation=None):
        W, H = dsize
        if interpolation == cv2.INTER_LANCZOS4:
            return resize_lanczos4(img, H, W)
        assert interpolation == cv2.INTER_AREA
        if H > img.shape[0] or W > img.shape[1]:
            return resize_linear_area(img, H, W)
        return area_only(img, dsize, interpolation=interpolation)

    cv2.resize = resize
    return cv2


# ---- the cases the CPU and the GPU tests share: name -> (method, n, H0, W0, H, W, input)
TAPS_CASES = {
    "lanczos_2x": (LANCZOS4, 2, 16, 24, 32, 48, "noise"),                # exact 2 x: two phases
    "lanczos_fractional": (LANCZOS4, 1, 45, 80, 64, 128, "textured7"),   # both fractional; clamps at 0 and at 255
    "lanczos_three_frames": (LANCZOS4, 3, 45, 80, 64, 128, "textured"),  # the frame stride
    "lanczos_3x5": (LANCZOS4, 1, 3, 5, 64, 64, "noise"),                 # every tap clamps, on both sides at once
    "lanczos_1x1": (LANCZOS4, 1, 1, 1, 64, 64, "noise"),
    "lanczos_shrinks": (LANCZOS4, 1, 66, 70, 64, 64, "textured"),        # both sides shrink slightly
    "lanczos_near_half": (LANCZOS4, 1, 120, 250, 64, 128, "textured"),   # near the factor-2 limit: the largest LDS window
    "lanczos_odd_rows": (LANCZOS4, 2, 45, 77, 64, 128, "textured"),      # rows at every byte phase (also fed off alignment)
    "lanczos_ragged": (LANCZOS4, 1, 30, 41, 37, 45, "textured"),         # partial tiles at the right and the bottom
    "linear_copy_axis": (LINEAR_AREA, 2, 64, 69, 64, 72, "textured"),    # one axis a copy
    "linear_shrink_grow": (LINEAR_AREA, 1, 65, 69, 64, 72, "textured"),  # one shrinks, one grows
    "linear_2x": (LINEAR_AREA, 1, 64, 64, 128, 128, "noise"),
    "linear_odd_rows": (LINEAR_AREA, 2, 45, 77, 64, 128, "textured"),
    "linear_ragged": (LINEAR_AREA, 1, 33, 40, 37, 45, "textured"),
}
REFUSED_CASE = (LANCZOS4, 1, 129, 64, 64, 64)   # a side shrinks by more than 2
# the axes the table test walks beside the shared ones: (ssize, dsize)
TABLE_AXES = ((270, 512), (480, 896), (480, 512), (640, 704), (550, 576), (513, 512), (530, 512))
# resize_image's geometries: (H0, W0) -> (H, W, branch)
DISPATCH_CASES = {
    (270, 480): (512, 896, "lanczos4"),
    (480, 640): (512, 704, "lanczos4"),
    (511, 530): (512, 512, "lanczos4"),
    (512, 550): (512, 576, "linear_area"),
    (513, 551): (512, 576, "linear_area"),
    (600, 800): (512, 704, "area"),
}
# end to end at resolution 64: branch -> ((n, H0, W0), (H, W))
SMALL_DISPATCH = {
    "lanczos4": ((2, 45, 80), (64, 128)),
    "lanczos4_shrinking_side": ((1, 63, 70), (64, 64)),         # k > 1; 71.1 / 64 rounds to 1: W shrinks through Lanczos
    "linear_area": ((2, 64, 104), (64, 128)),   # k = 1; 104 / 64 = 1.625 rounds to 2: W grows
    "linear_area_shrinking_side": ((1, 65, 105), (64, 128)),  # k < 1; 103.4 / 64 = 1.6 rounds to 2
    "area": ((1, 75, 100), (64, 64)),           # 85.3 / 64 = 1.33 rounds to 1
}


def taps_input(name):
    method, n, H0, W0, _, _, kind = TAPS_CASES[name]
    if kind == "textured7":
        return KM.textured(n, H0, W0, 7)
    seed = 40 + sorted(TAPS_CASES).index(name)
    return KM.noise(n, H0, W0, seed) if kind == "noise" else KM.textured(n, H0, W0, seed)


def adversarial(H0, W0, H, W):
    """One frame for LANCZOS4 (H0, W0) -> (H, W) that drives the accumulator to both extremes: 255 under the positive
    coefficient products of the output pixel with the largest positive mass, and, in a disjoint window, 255 under the
    negative products of the pixel with the largest negative mass.  -> (frame, (y, x, value) of the maximum, of the minimum)"""
    (fx, cx), (fy, cy) = lanczos_table(W0, W), lanczos_table(H0, H)
    cx, cy = cx.astype(np.int64), cy.astype(np.int64)

    def inside(first, ssize):  # windows that no clamp folds
        return (first >= 0) & (first + 7 <= ssize - 1)

    def mass(c, sign):
        return np.where(c * sign > 0, c * sign, 0).sum(1)

    frame = np.zeros((H0, W0, 3), np.uint8)
    found = []
    for sign, ys, xs in ((1, np.arange(H) < H // 2, np.ones(W, bool)), (-1, np.arange(H) >= H // 2 + 8, np.ones(W, bool))):
        ok_y, ok_x = inside(fy, H0) & ys, inside(fx, W0) & xs
        # sign > 0: P_y P_x + N_y N_x (products of like signs); sign < 0: P_y N_x + N_y P_x
        py, ny, px_, nx = mass(cy, 1), mass(cy, -1), mass(cx, 1), mass(cx, -1)
        score = (np.outer(py, px_) + np.outer(ny, nx)) if sign > 0 else (np.outer(py, nx) + np.outer(ny, px_))
        score = np.where(np.outer(ok_y, ok_x), score, -1)
        y, x = np.unravel_index(int(np.argmax(score)), score.shape)
        prod = np.outer(cy[y], cx[x]) * sign
        frame[fy[y]:fy[y] + 8, fx[x]:fx[x] + 8][prod > 0] = 255
        found.append((int(y), int(x), int(sign * 255 * score[y, x])))
    return frame[None], found[0], found[1]


# ---- the golden cases (tests/golden/make_keyframe_small_golden.py): name -> (seed, frames, H0, W0, mininterv, maxinterv)
SMALL_GOLDEN_CASES = {
    "lanczos_270x480": (4, 40, 270, 480, 5, 20),
    "lanczos_511x530": (6, 24, 511, 530, 3, 8),       # H grows, W shrinks, both through Lanczos (seeds 4 and 5 put two
                                                      # error values within 2e-3 relative of each other)
    "linear_area_512x550": (4, 24, 512, 550, 3, 8),
}
