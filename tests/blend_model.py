"""numpy restatement of video_blend.py's per-frame blending (process_seq, blender/histogram_blend.py,
blender/poisson_fusion.py) -- the definition the HIP backend (fresco_amd/csrc/blend.hip) is tested against.

Lab is OpenCV's documented 8-bit COLOR_BGR2Lab / COLOR_Lab2BGR formula in float64 (sRGB gamma, OpenCV's RGB <-> XYZ
matrices, D65 white, the 0.008856 / 7.787 / 903.3 branches, L * 255 / 100, a + 128, b + 128, round half to even,
saturate).  Whether it equals OpenCV's fixed-point 8-bit path bit for bit is not verified (no cv2 here): +-1 LSB is
expected.  The Poisson least-squares system is solved either like the reference (``lsqr`` on the stacked
[w Gx; w Gy; I] system, scipy) or exactly, by the DCT-II diagonalisation of the normal matrix with dense cosine
matrices (numpy only).
"""
import numpy as np

T_MEAN = 0.5 * 256
T_STD = np.float32((1 / 36) * 256)
GRAD_WEIGHT = (2.5, 0.5, 0.5)
# grey levels the exact solve adds before truncating: where the blend's Lab agrees with the gradients (every frame at
# weight1 = 0 or 1) the exact solution is an integer, and rounding noise of either sign would flip its truncation
TRUNC_GUARD = 1.0 / 1024


# ---------------------------------------------------------------------------------------------------------------------
# Lab
# ---------------------------------------------------------------------------------------------------------------------
def _sat(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def bgr_to_lab(bgr):
    x = np.asarray(bgr, dtype=np.float64) / 255.0
    lin = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    b, g, r = lin[..., 0], lin[..., 1], lin[..., 2]
    X = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.950456
    Y = 0.212671 * r + 0.715160 * g + 0.072169 * b
    Z = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.088754

    def f(t):
        return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)

    fx, fy, fz = f(X), f(Y), f(Z)
    L = np.where(Y > 0.008856, 116.0 * np.cbrt(Y) - 16.0, 903.3 * Y)
    return np.stack([_sat(L * 255.0 / 100.0), _sat(500.0 * (fx - fy) + 128.0), _sat(200.0 * (fy - fz) + 128.0)], -1)


def lab_to_bgr(lab):
    lab = np.asarray(lab)
    li = lab[..., 0] * 100.0 / 255.0
    ai = lab[..., 1] - 128.0
    bi = lab[..., 2] - 128.0
    low = li <= 903.3 * 0.008856
    y = np.where(low, li / 903.3, ((li + 16.0) / 116.0) ** 3)
    fy = np.where(low, 7.787 * (li / 903.3) + 16.0 / 116.0, (li + 16.0) / 116.0)

    def finv(f):
        return np.where(f <= 7.787 * 0.008856 + 16.0 / 116.0, (f - 16.0 / 116.0) / 7.787, f * f * f)

    x = finv(fy + ai / 500.0) * 0.950456
    z = finv(fy - bi / 200.0) * 1.088754
    R = 3.240479 * x - 1.53715 * y - 0.498535 * z
    G = -0.969256 * x + 1.875991 * y + 0.041556 * z
    B = 0.055648 * x - 0.204043 * y + 1.057311 * z

    def gamma(c):
        c = np.clip(c, 0.0, 1.0)
        return np.where(c <= 0.0031308, 12.92 * c, 1.055 * c ** (1.0 / 2.4) - 0.055)

    return np.stack([_sat(gamma(B) * 255.0), _sat(gamma(G) * 255.0), _sat(gamma(R) * 255.0)], -1)


# ---------------------------------------------------------------------------------------------------------------------
# mask
# ---------------------------------------------------------------------------------------------------------------------
def error_mask(d1, d2, weight1, weight2):
    """video_blend.py g_error_mask: 0 where weight1 d1 < weight2 d2 (in double), else 1; weight1 == 0 -> all 0,
    otherwise weight2 == 0 -> all 1."""
    if weight1 == 0:
        return np.zeros(np.shape(d1), np.uint8)
    if weight2 == 0:
        return np.ones(np.shape(d1), np.uint8)
    return np.where(weight1 * np.asarray(d1, np.float64) < weight2 * np.asarray(d2, np.float64), 0, 1).astype(np.uint8)


def warp_nearest(prev, flow):
    """flow_calc.warp(prev, flow, 'nearest'): grid_sample(nearest, zeros, align_corners=True) at pixel + flow, through
    flow_utils.py's normalise / unnormalise round trip in float32.  flow (2, h, w) or (1, 2, h, w), x first."""
    flow = np.asarray(flow, np.float32).reshape(2, *np.shape(prev))
    h, w = np.shape(prev)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    one, two = np.float32(1), np.float32(2)
    gx = two * (x.astype(np.float32) + flow[0]) / np.float32(w - 1) - one
    gy = two * (y.astype(np.float32) + flow[1]) / np.float32(h - 1) - one
    ix = np.rint((gx + one) * (np.float32(w - 1) / two))
    iy = np.rint((gy + one) * (np.float32(h - 1) / two))
    ok = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    out = np.zeros((h, w), np.uint8)
    out[ok] = np.asarray(prev)[iy[ok].astype(np.int64), ix[ok].astype(np.int64)]
    return out


def min_error_image(a, b, mask):
    return np.where(np.asarray(mask)[..., None] == 0, a, b)


# ---------------------------------------------------------------------------------------------------------------------
# histogram blend
# ---------------------------------------------------------------------------------------------------------------------
def constant_channels(lab):
    """bool (3,): the channels of a uint8 (h, w, 3) image that hold one value everywhere (std exactly 0)"""
    flat = np.asarray(lab).reshape(-1, 3)
    return flat.min(axis=0) == flat.max(axis=0)


def _transform(img, means, stds, target_means, target_stds, const=None):
    """(img - mean) * target_std / std + target_mean per channel.  The zero-std rule, stated
    here once: a channel flagged in ``const`` (std 0, where the reference divides by zero) becomes the target mean.
    Channels that are not flagged are computed exactly as without the argument."""
    x = img.astype(np.float32)
    if const is None or not const.any():
        return (x - means.reshape(1, 1, 3)) * target_stds.reshape(1, 1, 3) / stds.reshape(1, 1, 3) + \
            target_means.reshape(1, 1, 3)
    out = (x - means.reshape(1, 1, 3)) * target_stds.reshape(1, 1, 3) / np.where(const, 1, stds).reshape(1, 1, 3) + \
        target_means.reshape(1, 1, 3)
    out[..., const] = np.asarray(target_means, out.dtype)[const]
    return out


def histogram_blend_lab(a, b, min_error, weight1=0.5, weight2=0.5):
    """histogram_blend.blend up to (and including) the rounded uint8 Lab result"""
    return np.clip(np.round(histogram_blend_values(a, b, min_error, weight1, weight2)), 0, 255).astype(np.uint8)


def histogram_blend_values(a, b, min_error, weight1=0.5, weight2=0.5):
    """histogram_blend.blend's Lab values before the rounding and the clip to uint8: float (h, w, 3).

    Zero-std rule: a constant channel of a or of b transfers to the target mean (128), and so does the blend ab onto
    the min-error image's mean where ab is constant.  "Constant" is decided from the inputs, never from a threshold on
    a floating-point std: a and b by their Lab bytes (min == max), ab where each of a and b is constant or carries
    weight 0.  (ab.std() of such a channel is 0 only up to float32 rounding.)  An ab that is constant only because the
    two transfers cancel (correlation -1 at equal weights) is not covered: that input is ill-conditioned here and in
    the kernel alike.  With no constant channel the result is bit-identical to the plain formula."""
    a, b, m = bgr_to_lab(a), bgr_to_lab(b), bgr_to_lab(min_error)
    t_mean = np.ones([3], np.float32) * T_MEAN
    t_std = np.ones([3], np.float32) * T_STD
    ca, cb = constant_channels(a), constant_channels(b)
    cab = (ca | (weight1 == 0)) & (cb | (weight2 == 0))
    A = _transform(a, a.mean(axis=(0, 1)), a.std(axis=(0, 1)), t_mean, t_std, ca)
    B = _transform(b, b.mean(axis=(0, 1)), b.std(axis=(0, 1)), t_mean, t_std, cb)
    ab = (A * weight1 + B * weight2 - T_MEAN) / 0.5 + T_MEAN
    return _transform(ab, ab.mean(axis=(0, 1)), ab.std(axis=(0, 1)), m.mean(axis=(0, 1)), m.std(axis=(0, 1)), cab)


def histogram_blend(a, b, min_error, weight1=0.5, weight2=0.5):
    return lab_to_bgr(histogram_blend_lab(a, b, min_error, weight1, weight2))


# ---------------------------------------------------------------------------------------------------------------------
# Poisson fusion
# ---------------------------------------------------------------------------------------------------------------------
def poisson_gradients(I1, I2, mask):
    """(gx, gy) of poisson_fusion: forward differences of Lab(I1), or Lab(I2) where mask > 0, last row / column 0,
    clipped to +-100; float64 (h, w, 3)."""
    Ia = bgr_to_lab(I1).astype(float)
    Ib = bgr_to_lab(I2).astype(float)
    m = (np.asarray(mask) > 0).astype(float)[:, :, None]
    gx = np.zeros_like(Ia)
    gy = np.zeros_like(Ia)
    gx[:-1] = (Ia[:-1] - Ia[1:]) * (1 - m[:-1]) + (Ib[:-1] - Ib[1:]) * m[:-1]
    gy[:, :-1] = (Ia[:, :-1] - Ia[:, 1:]) * (1 - m[:, :-1]) + (Ib[:, :-1] - Ib[:, 1:]) * m[:, :-1]
    return np.clip(gx, -100, 100), np.clip(gy, -100, 100)


def dct_matrix(n):
    """orthonormal DCT-II matrix C[k, m] = s_k cos(pi (2m + 1) k / 2n)"""
    k = np.arange(n)[:, None]
    m = np.arange(n)[None, :]
    c = np.cos(np.pi * ((2 * m + 1) * k % (4 * n)) / (2.0 * n))
    c[0] *= np.sqrt(1.0 / n)
    c[1:] *= np.sqrt(2.0 / n)
    return c


def _solve_dct(gx, gy, im, w):
    """exact minimiser of |w Gx x - w gx|^2 + |w Gy x - w gy|^2 + |x - im|^2 (Gx: rows, Gy: columns)"""
    h, wd = im.shape
    r = im.copy()
    r += w * w * gx
    r[1:] -= w * w * gx[:-1]
    r += w * w * gy
    r[:, 1:] -= w * w * gy[:, :-1]
    ch, cw = dct_matrix(h), dct_matrix(wd)
    lam = 2 - 2 * np.cos(np.pi * np.arange(h) / h)
    mu = 2 - 2 * np.cos(np.pi * np.arange(wd) / wd)
    spec = ch @ r @ cw.T / (1 + w * w * (lam[:, None] + mu[None, :]))
    return ch.T @ spec @ cw


_A_CACHE = {}


def _stacked_system(h, w, weight):
    """poisson_fusion.construct_A's vstack([w Gx, w Gy, I]) for one channel (built vectorised)"""
    import scipy.sparse as sp
    key = (h, w, weight)
    if key not in _A_CACHE:
        idx = np.arange(h * w).reshape(h, w)
        rx = idx[:-1].ravel()
        ry = idx[:, :-1].ravel()
        gx = sp.coo_array((np.r_[np.ones(rx.size), -np.ones(rx.size)], (np.r_[rx, rx], np.r_[rx, rx + w])),
                          shape=(h * w, h * w)).tocsc()
        gy = sp.coo_array((np.r_[np.ones(ry.size), -np.ones(ry.size)], (np.r_[ry, ry], np.r_[ry, ry + 1])),
                          shape=(h * w, h * w)).tocsc()
        eye = sp.coo_array((np.ones(h * w), (np.arange(h * w), np.arange(h * w))), shape=(h * w, h * w)).tocsc()
        _A_CACHE[key] = sp.vstack([gx * weight, gy * weight, eye])
    return _A_CACHE[key]


def _solve_lsqr(gx, gy, im, w):
    from scipy.sparse.linalg import lsqr
    h, wd = im.shape
    A = _stacked_system(h, wd, w)
    b = np.vstack([gx.reshape(-1, 1) * w, gy.reshape(-1, 1) * w, im.reshape(-1, 1)])
    return lsqr(A, b)[0].reshape(h, wd)


def poisson_solution(blendI, I1, I2, mask, grad_weight=GRAD_WEIGHT, solver="dct"):
    """float64 (h, w, 3): x + mean per channel, before the clip and the uint8 cast"""
    Iab = bgr_to_lab(blendI).astype(float)
    gx, gy = poisson_gradients(I1, I2, mask)
    solve = {"dct": _solve_dct, "lsqr": _solve_lsqr}[solver]
    out = []
    for c in range(3):
        im = Iab[:, :, c]
        mean = im.mean()
        out.append(solve(gx[:, :, c], gy[:, :, c], im - mean, grad_weight[c]) + mean)
    return np.stack(out, -1)


def poisson_fusion_lab(blendI, I1, I2, mask, grad_weight=GRAD_WEIGHT, solver="dct", guard=None):
    """poisson_fusion's Lab bytes: clip(x + mean, 0, 255).astype(uint8) truncates (after TRUNC_GUARD for the exact
    solve; the lsqr solver is the reference's, unguarded)"""
    guard = (TRUNC_GUARD if solver == "dct" else 0.0) if guard is None else guard
    return np.clip(poisson_solution(blendI, I1, I2, mask, grad_weight, solver) + guard, 0, 255).astype(np.uint8)


def poisson_fusion(blendI, I1, I2, mask, grad_weight=GRAD_WEIGHT, solver="dct"):
    return lab_to_bgr(poisson_fusion_lab(blendI, I1, I2, mask, grad_weight, solver))


# ---------------------------------------------------------------------------------------------------------------------
# one frame, one interval
# ---------------------------------------------------------------------------------------------------------------------
def blend_frame(oa, ob, d1, d2, weight1, prev_mask=None, flow=None, gradient=True, solver="dct"):
    """process_seq's body for one in-between frame -> dict(mask, hist_lab, hist, poisson_lab (gradient), image)"""
    weight2 = 1 - weight1
    mask = error_mask(d1, d2, weight1, weight2)
    if prev_mask is not None:
        mask = warp_nearest(prev_mask, flow) | mask
    me = min_error_image(oa, ob, mask)
    hist_lab = histogram_blend_lab(oa, ob, me, 1 - weight1, 1 - weight2)
    hist = lab_to_bgr(hist_lab)
    res = dict(mask=mask, hist_lab=hist_lab, hist=hist, image=hist)
    if gradient:
        res["poisson_lab"] = poisson_fusion_lab(hist, oa, ob, mask, solver=solver)
        res["image"] = lab_to_bgr(res["poisson_lab"])
    return res


def blend_interval(oas, obs, d1s, d2s, flows, gradient=True, solver="dct"):
    """process_seq's loop over the n in-between frames of one key interval: frame k has weight1 = k / n;
    flows[k - 1] carries frame k - 1's mask to frame k -> list of blend_frame dicts"""
    n = len(oas)
    out, prev = [], None
    for k in range(n):
        r = blend_frame(oas[k], obs[k], d1s[k], d2s[k], k / n, prev, flows[k - 1] if k else None, gradient, solver)
        out.append(r)
        prev = r["mask"]
    return out
