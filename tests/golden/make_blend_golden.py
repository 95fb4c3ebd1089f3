"""Generate tests/golden/blend_golden.npz: video_blend.py's per-frame blending on seeded synthetic inputs, computed by the
numpy restatement tests/blend_model.py with the reference-shaped solver (scipy lsqr on the stacked [w Gx; w Gy; I]
system, default settings, weights 2.5 / 0.5 / 0.5).

The reference's own blender (src/ebsynth/blender + video_blend.py) cannot run here: it needs cv2 and numba, and neither
is installed.  The model restates it operation by operation (tests/blend_model.py's docstring has what that does and
does not pin down).

Run:  python tests/golden/make_blend_golden.py

Cases (h x w):
  single_*   64 x 96, one frame at weight1 = 0, 0.5 and 1 (same inputs), no previous mask
  interval_* 72 x 56, one key interval of 6 (5 blended frames): the mask propagates through fractional flows, flows
             that leave the frame and coordinates exactly on .5
  odd_*      37 x 53, one frame at weight1 = 0.4 with a previous mask and flow
The inputs are not stored: cases() rebuilds them from an integer hash (no floating point, no numpy random stream, so
they are the same on every machine) and the file keeps their sha256 to prove it.  Stored per frame: the mask, the
histogram blend's Lab bytes and the Poisson fusion's Lab bytes (the final image is their Lab -> BGR conversion).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import blend_model as M  # noqa: E402

OUT = os.path.join(HERE, "blend_golden.npz")


def _hash(x):
    """32-bit integer mix (lowbias32) of a uint64 array: no floating point, so the inputs are the same everywhere"""
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def _noise(seed, shape):
    return _hash(np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9)).reshape(shape)


def smooth(seed, h, w, c, cell):
    """integer bilinear upsampling of a coarse grid of hashed values: int64 (h, w, c) in [0, 1023]"""
    g = (_noise(seed, (h // cell + 2, w // cell + 2, c)) % np.uint64(1024)).astype(np.int64)
    y, x = np.arange(h), np.arange(w)
    y0, fy = (y // cell)[:, None], (y % cell)[:, None, None]
    x0, fx = (x // cell)[None, :], (x % cell)[None, :, None]
    top = g[y0, x0] * (cell - fx) + g[y0, x0 + 1] * fx
    bot = g[y0 + 1, x0] * (cell - fx) + g[y0 + 1, x0 + 1] * fx
    return (top * (cell - fy) + bot * fy) // (cell * cell)


def image(seed, h, w):
    x = smooth(seed, h, w, 3, 9) * 200 // 1024 + smooth(seed + 1, h, w, 3, 3) * 50 // 1024
    x += (_noise(seed + 2, (h, w, 3)) % np.uint64(3)).astype(np.int64)
    return np.clip(x, 0, 255).astype(np.uint8)


def error_map(seed, h, w):
    """integer-valued patch errors in [0, 4000) (ties between the weighted maps happen: the mask takes 1 there)"""
    return (smooth(seed, h, w, 1, 7)[..., 0] * 4000 // 1024).astype(np.float32)


def flow_field(seed, h, w):
    """(1, 2, h, w): fractional flow in [-3, 3] in 1/8 steps, a band that leaves the frame, and blocks whose sample
    points land on half-pixel coordinates"""
    f = ((smooth(seed, h, w, 2, 8) * 48 // 1024 - 24) / 8.0).transpose(2, 0, 1).astype(np.float32)
    f[0, :, : w // 8] -= 40.0
    f[1, h - h // 8:, :] += 30.0
    f[:, h // 3: h // 3 + 6, w // 3: w // 3 + 6] = 0.5
    f[0, h // 2: h // 2 + 4, w // 2: w // 2 + 4] = -1.5
    return np.ascontiguousarray(f[None])


def frame(seed, h, w):
    return dict(oa=image(10 * seed, h, w), ob=image(10 * seed + 3, h, w), d1=error_map(10 * seed + 6, h, w),
                d2=error_map(10 * seed + 7, h, w))


def cases():
    """name -> dict(oa, ob, d1, d2, weight1[, prev_mask, flow]); interval_k frames chain: their prev_mask is None here
    and is the previous frame's mask"""
    out = {}
    inp = frame(1, 64, 96)
    for tag, w1 in (("w0", 0.0), ("w05", 0.5), ("w1", 1.0)):
        out["single_" + tag] = dict(inp, weight1=w1)
    n = 5
    for k in range(n):
        out["interval_%d" % k] = dict(frame(2 + k, 72, 56), weight1=k / n,
                                      flow=flow_field(100 + k, 72, 56) if k else None)
    out["odd"] = dict(frame(9, 37, 53), weight1=0.4, flow=flow_field(200, 37, 53),
                      prev_mask=(_noise(201, (37, 53)) % np.uint64(10) < np.uint64(3)).astype(np.uint8))
    return out


def digest(case):
    import hashlib
    h = hashlib.sha256()
    for k in ("oa", "ob", "d1", "d2", "flow", "prev_mask"):
        if case.get(k) is not None:
            h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()


def run_case(name, case, prev=None, solver="lsqr"):
    """the model on one case; interval_k (k >= 1) takes the previous frame's mask as prev"""
    p = case.get("prev_mask", prev) if case.get("flow") is not None else None
    return M.blend_frame(case["oa"], case["ob"], case["d1"], case["d2"], case["weight1"], p,
                         case["flow"] if p is not None else None, solver=solver)


def main():
    out = {}
    prev = None
    for name, case in cases().items():
        res = run_case(name, case, prev if name.startswith("interval_") else None)
        prev = res["mask"]
        out[name + "_sha256"] = np.array(digest(case))
        for k in ("mask", "hist_lab", "poisson_lab"):
            out["%s_%s" % (name, k)] = res[k]
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes, %d arrays)" % (OUT, os.path.getsize(OUT), len(out)))


if __name__ == "__main__":
    main()
