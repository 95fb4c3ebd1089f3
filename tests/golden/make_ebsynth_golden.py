"""Generate tests/golden/ebsynth_golden.npz (and, with --wide, tests/golden/ebsynth_wide_golden.npz) by running the
UNMODIFIED reference Ebsynth CPU backend.

Run in the build container only:  python tests/golden/make_ebsynth_golden.py [--ref /path/to/FRESCO] [--wide]

The reference's CPU build (src/ebsynth/deps/ebsynth: ebsynth.cpp + ebsynth_cpu.cpp + ebsynth_nocuda.cpp) does not link
as shipped: ebsynth.cpp dispatches to an ebsynthRunCuda that takes an outputErrorData argument, ebsynth_nocuda.cpp
defines one without it.  The script compiles the three files unmodified, plus a stub of its own that defines the missing
symbol, into a temporary directory outside the repository, then runs the binary on seeded synthetic PNGs.

Stored per case: the inputs as the binary's command line packs them (channel-interleaved style / guides, per-channel
weights), the reference's output image and its .bin error map, and the reference's own spread: the mean |output
difference| and the mean-error ratio between a run on the inputs and runs on copies whose target guides are perturbed by
1 LSB.  The random streams of two implementations differ, so the GPU tests compare quality against these numbers.

  --wide              the cases outside the first file's shapes (WIDE_CASES): 8 RGB guides (style + guide channels in
                      two 16-byte records) with mixed weights and patch 7, and an RGBA style with a target of another
                      size than the source; own seeded random stream, the first file is left as it is
  --binary-only DIR   only build the reference binary into DIR (e.g. to time it elsewhere)
  --time BIN          time BIN on the 512x512 four-guide frame of video_blend.py (12 search/vote, 6 PatchMatch iters)
"""
import argparse
import io
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ebsynth_golden.npz")
OUT_WIDE = os.path.join(HERE, "ebsynth_wide_golden.npz")

STUB = r"""
// ebsynthRunCuda with the signature ebsynth.cpp dispatches to; never called (ebsynthBackendAvailableCuda() is 0).
void ebsynthRunCuda(int, int, int, int, void*, void*, int, int, void*, void*, float*, float*, float, int, int, int,
                    int*, int*, int*, int, void*, void*, void*) {}
"""


def build_reference(ref_root, out_dir):
    src = os.path.join(ref_root, "src", "ebsynth", "deps", "ebsynth")
    stub = os.path.join(out_dir, "cuda_stub.cpp")
    with open(stub, "w") as f:
        f.write(STUB)
    exe = os.path.join(out_dir, "ebsynth")
    cmd = ["g++", "-O3", "-DNDEBUG", "-fopenmp", "-std=c++17", "-I", os.path.join(src, "include"),
           os.path.join(src, "src", "ebsynth.cpp"), os.path.join(src, "src", "ebsynth_cpu.cpp"),
           os.path.join(src, "src", "ebsynth_nocuda.cpp"), stub, "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def smooth_noise(rng, h, w, c, cell):
    """Bilinearly upsampled uniform noise: a random image with structure at the scale of `cell` pixels."""
    gh, gw = h // cell + 3, w // cell + 3
    g = rng.uniform(0, 255, (gh, gw, c)).astype(np.float32)
    out = np.stack([np.asarray(Image.fromarray(g[..., k]).resize((w + 3 * cell, h + 3 * cell), Image.BILINEAR))
                    for k in range(c)], -1)
    return np.clip(out[cell:cell + h, cell:cell + w], 0, 255).astype(np.uint8)


def shifted(img, dx, dy):
    """target(x, y) = source(x - dx, y - dy), edges replicated."""
    h, w = img.shape[:2]
    ys = np.clip(np.arange(h) - dy, 0, h - 1)
    xs = np.clip(np.arange(w) - dx, 0, w - 1)
    return img[ys][:, xs]


def save_png(path, a):
    Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a).save(path)


def eval_num_channels(rgba):
    """ebsynth.cpp evalNumChannels: gray if r == g == b everywhere, +1 if any alpha < 255."""
    gray = bool(np.all((rgba[..., 0] == rgba[..., 1]) & (rgba[..., 1] == rgba[..., 2])))
    alpha = bool(np.any(rgba[..., 3] < 255))
    return (1 if gray else 3) + (1 if alpha else 0)


def pick(rgba, n):
    """The channels ebsynth.cpp keeps for an image counted as n channels."""
    idx = {1: [0], 2: [0, 3], 3: [0, 1, 2], 4: [0, 1, 2, 3]}[n]
    return rgba[..., idx]


def rgba_of(path):
    return np.asarray(Image.open(path).convert("RGBA"))


def make_case(rng, h, w, guide_kinds, shift):
    """guide_kinds: list of (channels, weight); style = smooth colour noise; source guides smooth noise; target guides
    = source guides shifted by `shift` plus a little independent noise."""
    style = smooth_noise(rng, h, w, 3, 6)
    guides = []
    for c, wt in guide_kinds:
        src = smooth_noise(rng, h, w, c, 5)
        tgt = shifted(src, *shift).astype(np.int16) + rng.integers(-2, 3, src.shape)
        guides.append((src, np.clip(tgt, 0, 255).astype(np.uint8), wt))
    return style, guides


def run_reference(exe, d, style, guides, args, tag):
    sp = os.path.join(d, tag + "_style.png")
    save_png(sp, style)
    cmd = [exe, "-style", sp]
    for i, (s, t, wt) in enumerate(guides):
        a, b = os.path.join(d, "%s_g%d_s.png" % (tag, i)), os.path.join(d, "%s_g%d_t.png" % (tag, i))
        save_png(a, s)
        save_png(b, t)
        cmd += ["-guide", a, b]
        if wt is not None:
            cmd += ["-weight", repr(float(wt))]
    out = os.path.join(d, tag + "_out.png")
    cmd += ["-output", out] + args
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    img = np.asarray(Image.open(out))
    if img.ndim == 2:
        img = img[..., None]
    raw = open(out[:-4] + ".bin", "rb").read()
    n = int(np.frombuffer(raw[:8], np.int64)[0])
    err = np.frombuffer(raw[8:], np.float32)
    assert n == img.shape[0] * img.shape[1] == err.size, (n, img.shape, err.size)
    return img, err.reshape(img.shape[:2]).copy(), dt, cmd


def packed_inputs(d, tag, n_guides):
    """Re-read the PNGs the way ebsynth.cpp does and pack style / guides / weights like its main()."""
    st = rgba_of(os.path.join(d, tag + "_style.png"))
    ns = eval_num_channels(st)
    src_g, tgt_g, counts = [], [], []
    for i in range(n_guides):
        s = rgba_of(os.path.join(d, "%s_g%d_s.png" % (tag, i)))
        t = rgba_of(os.path.join(d, "%s_g%d_t.png" % (tag, i)))
        c = max(eval_num_channels(s), eval_num_channels(t))
        counts.append(c)
        src_g.append(pick(s, c))
        tgt_g.append(pick(t, c))
    return pick(st, ns), np.concatenate(src_g, -1), np.concatenate(tgt_g, -1), counts


CASES = [
    # name, (h, w), guides [(channels, -weight or None)], shift, binary args
    ("sq64", (64, 64), [(3, None)], (3, -2), []),
    ("rect96x128", (96, 128), [(1, None), (3, 2.0)], (-4, 3), ["-patchsize", "5", "-uniformity", "2000"]),
    ("four_guides", (112, 112), [(3, 6.0), (1, 0.5), (3, 0.5), (3, 2.0)], (5, -3),
     ["-searchvoteiters", "12", "-patchmatchiters", "6"]),
]


# Outside the shapes above (--wide, written to OUT_WIDE): record width 2 and patch 7, and a 4-channel style with a target
# of another size than the source.  name, style channels, source (h, w), target (h, w), guides [(channels, -weight or
# None)], shift, binary args
WIDE_CASES = [
    ("eight_rgb_guides", 3, (56, 60), (56, 60),
     [(3, 2.0), (3, None), (3, 0.5), (3, 1.0), (3, None), (3, 4.0), (3, 0.25), (3, None)], (2, -3),
     ["-patchsize", "7", "-searchvoteiters", "4", "-patchmatchiters", "3"]),
    ("rgba_style_resized_target", 4, (60, 68), (52, 77), [(3, None)], (-3, 2), []),
]


def make_wide_case(rng, ns, src_hw, tgt_hw, guide_kinds, shift):
    """make_case, with a style of ns = 3 or 4 channels (the 4th an alpha in [64, 255], some of it below 255) and target
    guides resized (bilinear) to tgt_hw before the shift and noise."""
    h, w = src_hw
    style = smooth_noise(rng, h, w, 3, 6)
    if ns == 4:
        style = np.concatenate([style, (64 + smooth_noise(rng, h, w, 1, 8).astype(np.int32) * 3 // 4)
                                .astype(np.uint8)], -1)
    guides = []
    for c, wt in guide_kinds:
        src = smooth_noise(rng, h, w, c, 5)
        rs = src
        if tuple(tgt_hw) != tuple(src_hw):
            rs = np.stack([np.asarray(Image.fromarray(src[..., k]).resize(tgt_hw[::-1], Image.BILINEAR))
                           for k in range(c)], -1)
        tgt = shifted(rs, *shift).astype(np.int16) + rng.integers(-2, 3, rs.shape)
        guides.append((src, np.clip(tgt, 0, 255).astype(np.uint8), wt))
    return style, guides


def reference_case(exe, d, rng, name, style, guides, args):
    """Run the reference on one case and on two 1-LSB perturbations of its target guides; the arrays to store."""
    img, err, _, cmd = run_reference(exe, d, style, guides, args, name)
    st, sg, tg, counts = packed_inputs(d, name, len(guides))
    # the reference's own spread: target guides perturbed by one LSB (seeded, two draws)
    diffs, ratios = [], []
    for k in range(2):
        pg = []
        for s, t, wt in guides:
            p = t.astype(np.int16) + rng.integers(-1, 2, t.shape)
            pg.append((s, np.clip(p, 0, 255).astype(np.uint8), wt))
        img2, err2, _, _ = run_reference(exe, d, style, pg, args, name + "_p%d" % k)
        diffs.append(float(np.abs(img2.astype(np.float64) - img).mean()))
        ratios.append(float(err2.mean() / err.mean()))
    print("%-12s out %s  mean E %.1f  spread: mean|d| %s  E ratio %s" %
          (name, img.shape, err.mean(), ["%.3f" % v for v in diffs], ["%.3f" % v for v in ratios]))
    return {
        name + "/style": st,
        name + "/source_guide": sg,
        name + "/target_guide": tg,
        name + "/guide_counts": np.array(counts, np.int32),
        name + "/guide_weights_cli": np.array([-1.0 if wt is None else wt for _, _, wt in guides], np.float32),
        name + "/args": np.array(args, dtype="U32"),
        name + "/ref_out": img,
        name + "/ref_err": err,
        name + "/spread_mean_abs": np.array(diffs, np.float64),
        name + "/spread_err_ratio": np.array(ratios, np.float64),
    }


def save(store, path):
    buf = io.BytesIO()
    np.savez_compressed(buf, **store)
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s (%d bytes)" % (path, len(buf.getvalue())))


def generate(exe):
    rng = np.random.default_rng(20261015)
    store = {}
    with tempfile.TemporaryDirectory() as d:
        for name, (h, w), kinds, shift, args in CASES:
            style, guides = make_case(rng, h, w, kinds, shift)
            store.update(reference_case(exe, d, rng, name, style, guides, args))
    save(store, OUT)


def generate_wide(exe):
    rng = np.random.default_rng(20261016)
    store = {}
    with tempfile.TemporaryDirectory() as d:
        for name, ns, src_hw, tgt_hw, kinds, shift, args in WIDE_CASES:
            style, guides = make_wide_case(rng, ns, src_hw, tgt_hw, kinds, shift)
            store.update(reference_case(exe, d, rng, name, style, guides, args))
    save(store, OUT_WIDE)


def time_frame(exe, runs=3):
    """The frame of tools/bench_ebsynth.py: 512x512, style RGB, four guides (3 + 1 + 3 + 3 = 10 channels) with
    video_blend.py's weights and iteration counts."""
    rng = np.random.default_rng(1)
    style, guides = make_case(rng, 512, 512, [(3, 6.0), (1, 0.5), (3, 0.5), (3, 2.0)], (5, -3))
    ts = []
    with tempfile.TemporaryDirectory() as d:
        for i in range(runs):
            ts.append(run_reference(exe, d, style, guides, ["-searchvoteiters", "12", "-patchmatchiters", "6"],
                                    "t%d" % i)[2])
    print("reference CPU, 512x512 four guides: %s s per frame (OMP_NUM_THREADS=%s)" %
          (["%.2f" % t for t in ts], os.environ.get("OMP_NUM_THREADS", "unset")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("FRESCO_REFERENCE", "/root/reference"),
                    help="root of the reference FRESCO checkout")
    ap.add_argument("--binary-only", metavar="DIR")
    ap.add_argument("--time", metavar="BIN")
    ap.add_argument("--wide", action="store_true", help="write %s instead" % os.path.basename(OUT_WIDE))
    a = ap.parse_args()
    if a.time:
        time_frame(a.time)
        return
    if a.binary_only:
        os.makedirs(a.binary_only, exist_ok=True)
        print(build_reference(a.ref, a.binary_only))
        return
    with tempfile.TemporaryDirectory() as d:
        (generate_wide if a.wide else generate)(build_reference(a.ref, d))


if __name__ == "__main__":
    sys.exit(main())
