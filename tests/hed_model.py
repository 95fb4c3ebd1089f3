"""Stand-ins and restatements shared by tests/golden/make_hed_golden.py, tests/test_hed_cpu.py and tests/test_gpu_hed.py.

The published HED checkpoint (ControlNetHED.pth) is not available to the tests, and neither is cv2:

  * weights: closed-form stand-ins, seeded by parameter name, drawn in float64 and cast -- He-style convolutions with gain
    0.9 (activations stay in the hundreds through 13 layers), projections with gain 0.03 (fused logits of order one: the
    sigmoid is not saturated), biases 0.1 N(0, 1), norm = (123.7, 116.3, 103.5);
  * frames: a smooth random colour field (a coarse (H/8 + 1, W/8 + 1) grid upsampled with Catmull-Rom cubics) plus 8 %
    noise, quantised to uint8 -- numpy float64 element-wise arithmetic only, so every machine builds the same bytes (the
    golden file keeps their sha256);
  * cv2.resize(e, (W, H), interpolation=INTER_LINEAR) on a float32 single-channel map: `resize_standin`, which is
    F.interpolate(mode="bilinear", align_corners=False, size=(H, W)) in fp32.  For the upscaling the detector does, that is
    INTER_LINEAR's sampling (half-pixel centres, edge samples repeated, no antialiasing) up to rounding order: torch forms
    the source position in fp32 from an fp32 scale and blends the four taps in one expression, cv2 forms the position in
    double and runs a horizontal pass, then a vertical one.

`fuse_u8` restates what the detector does with its five side maps (resize, mean, float64 sigmoid, truncation);
`fuse_logit64` is the same mean carried in float64, the reference the GPU tests measure against.
"""
import hashlib
import zlib

import numpy as np
import torch
import torch.nn.functional as F

# (n, H, W): level 5 of 64 x 64 is 4 x 4 (sub-tile M, all-border windows); non-square; not a multiple of 64 with exact
# pooling down to 6 x 5; pooling that floors (9 -> 4, 11 -> 5) with resize scales that are no powers of two
CASES = [(2, 64, 64), (1, 64, 128), (2, 96, 80), (1, 72, 88)]
# frames of each case whose reference records are kept in the golden file (the others are covered by the batch tests)
GOLDEN_FRAMES = {(2, 64, 64): 2, (1, 64, 128): 1, (2, 96, 80): 1, (1, 72, 88): 1, (1, 128, 128): 1}
# recorded in a file of its own (tests/golden/hed_wide_golden.npz): levels of 128, 64, 32, 16 and 8 pixels, so blocks 1 to 4
# run their convolutions in the window-in-LDS form (maps of whole 16 x 16 patches, up to 512 channels) and block 5 in the
# im2col form -- the CASES above reach that form on 16 x 16 maps of at most 256 channels
WIDE_CASES = [(1, 128, 128)]
GOLDEN_FILES = ("hed_golden.npz", "hed_wide_golden.npz")  # under tests/golden: CASES, WIDE_CASES
BLOCKS = ((3, 64, 2), (64, 128, 2), (128, 256, 3), (256, 512, 3), (512, 512, 3))  # cin, cout, convolutions
NORM = (123.7, 116.3, 103.5)
CONV_GAIN, PROJ_GAIN, BIAS_STD, NOISE = 0.9, 0.03, 0.1, 0.08
GUARD = 0.02   # |255 sigmoid(logit) - nearest integer| below which a uint8 value may differ by one
GUARD_CAP = 0.06  # share of a case's pixels that may lie in the guard band


def load_golden(golden_dir):
    """the records of CASES and WIDE_CASES as one dict (the entries the two files share are equal)"""
    import os
    gold = {}
    for name in GOLDEN_FILES:
        gold.update(np.load(os.path.join(golden_dir, name)))
    return gold


def case_key(case):
    return "hed_%dx%dx%d" % case


def level_sizes(H, W):
    return [(H >> k, W >> k) for k in range(5)]


def param_shapes():
    """name -> shape, in the module's registration order"""
    out = {"norm": (1, 3, 1, 1)}
    for k, (cin, cout, layers) in enumerate(BLOCKS, 1):
        for j in range(layers):
            out["block%d.convs.%d.weight" % (k, j)] = (cout, cin if j == 0 else cout, 3, 3)
            out["block%d.convs.%d.bias" % (k, j)] = (cout,)
        out["block%d.projection.weight" % k] = (1, cout, 1, 1)
        out["block%d.projection.bias" % k] = (1,)
    return out


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def standin_state_dict(dtype=torch.float32):
    sd = {}
    for name, shape in param_shapes().items():
        if name == "norm":
            v = np.array(NORM, np.float64).reshape(shape)
        elif name.endswith(".bias"):
            v = BIAS_STD * _rs(name).standard_normal(shape)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            gain = PROJ_GAIN if ".projection." in name else CONV_GAIN
            v = gain * np.sqrt(2.0 / fan_in) * _rs(name).standard_normal(shape)
        sd[name] = torch.from_numpy(v).to(dtype)
    return sd


def _cubic_weights(t):
    """Catmull-Rom weights of the four neighbours for fractions t (float64)"""
    t2, t3 = t * t, t * t * t
    return (-0.5 * t3 + t2 - 0.5 * t, 1.5 * t3 - 2.5 * t2 + 1.0, -1.5 * t3 + 2.0 * t2 + 0.5 * t, 0.5 * t3 - 0.5 * t2)


def _upsample_axis(a, out, axis):
    """cubic upsampling of `a` along `axis` from its grid (spacing 8 pixels, first node at pixel 0) to `out` samples"""
    n = a.shape[axis]
    pos = np.arange(out, dtype=np.float64) / 8.0
    i = np.floor(pos).astype(np.int64)
    w = _cubic_weights(pos - i)
    res = 0.0
    for k in range(4):
        idx = np.clip(i - 1 + k, 0, n - 1)
        shape = [1] * a.ndim
        shape[axis] = out
        res = res + np.take(a, idx, axis=axis) * w[k].reshape(shape)
    return res


def frames(case):
    """uint8 (n, H, W, 3) RGB frames of a case"""
    n, H, W = case
    rs = np.random.RandomState(7000 + 131 * H + W)
    coarse = rs.uniform(0.05, 0.95, (n, H // 8 + 1, W // 8 + 1, 3))
    smooth = _upsample_axis(_upsample_axis(coarse, H, 1), W, 2)
    x = smooth + NOISE * rs.standard_normal((n, H, W, 3))
    return np.floor(np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def weights_digest():
    sd = standin_state_dict()
    return digest(*[sd[k].numpy() for k in sd])


def resize_standin(e, W, H, interpolation=None):
    """stand-in of cv2.resize(e, (W, H), interpolation=cv2.INTER_LINEAR) for a 2-D float array (see the module docstring);
    computes in e's own precision"""
    t = torch.from_numpy(np.ascontiguousarray(e))[None, None]
    if tuple(t.shape[2:]) == (H, W):
        return e.copy()
    return F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)[0, 0].numpy()


def fuse_u8(projs, H, W):
    """five (h, w) float32 side maps of one frame -> (their mean at (H, W) in float32, the detector's uint8 edge map)"""
    maps = np.stack([resize_standin(np.asarray(p, np.float32), W, H) for p in projs], axis=2)
    mean = np.mean(maps, axis=2)  # float32, as numpy reduces a float32 array
    sig = np.reciprocal(1.0 + np.exp(-mean.astype(np.float64)))
    return mean, np.clip(sig * 255.0, 0.0, 255.0).astype(np.uint8)  # the cast truncates


def fuse_logit64(projs, H, W):
    """the mean of the five resized maps with everything in float64"""
    maps = np.stack([resize_standin(np.asarray(p, np.float64), W, H) for p in projs], axis=2)
    return np.mean(maps, axis=2)


def guard_band(logit64):
    """True where 255 sigmoid(logit) is within GUARD of an integer: a uint8 truncation boundary is that close"""
    v = 255.0 / (1.0 + np.exp(-np.asarray(logit64, np.float64)))
    return np.abs(v - np.round(v)) <= GUARD


def check_u8(u8, ref_u8, logit64, what):
    """the guard-band rule: equal outside the band, at most one apart inside, and the band holds at most GUARD_CAP of the
    pixels"""
    band = guard_band(logit64)
    share = float(band.mean())
    d = np.abs(u8.astype(np.int32) - ref_u8.astype(np.int32))
    print("%s: %.2f %% of pixels in the guard band, %d differ inside it, %d outside, max |d| %d"
          % (what, 100 * share, int((d[band] > 0).sum()), int((d[~band] > 0).sum()), int(d.max())))
    assert share <= GUARD_CAP, (what, share)
    assert d[~band].max(initial=0) == 0, (what, int((d[~band] > 0).sum()))
    assert d.max(initial=0) <= 1, (what, int(d.max()))


def golden_sides(gold, case, f):
    """-> (five fp32 side maps, five fp64 ones, logit32, logit64, u8) of frame f of a case.  The float64 records are stored
    as the float32 record plus a float32 difference (exact to 2^-24 of the difference: < 1e-12 here)."""
    key = "%s_f%d" % (case_key(case), f)
    p32 = [gold["%s_p%d_f32" % (key, k)] for k in range(1, 6)]
    p64 = [p.astype(np.float64) + gold["%s_p%d_d64" % (key, k)].astype(np.float64) for k, p in enumerate(p32, 1)]
    l32 = gold[key + "_logit_f32"]
    l64 = l32.astype(np.float64) + gold[key + "_logit_d64"].astype(np.float64)
    return p32, p64, l32, l64, gold[key + "_u8"]
