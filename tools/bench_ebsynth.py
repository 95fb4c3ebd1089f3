"""Ebsynth backend on one frame of video_blend.py's shape: 512x512, RGB style, four guides (colour 3 + edge 1 +
temporal 3 + positional 3 = 10 channels, weights 6 / 0.5 / 0.5 / 2), -searchvoteiters 12 -patchmatchiters 6.

Prints one JSON line: median ms per frame over >= 5 timed runs after warm-up (host clock around a synchronised call),
the same with extra_pass_3x3, the per-level split (HIP events of the library's opt-in profiler, one extra run), the
launches per frame, and with --cli the wall time of one `fresco_amd/bin/ebsynth` process (what video_blend.py pays per
frame) next to the interpreter + torch + library start-up alone."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fresco_amd import _lib, ebsynth_run  # noqa: E402
from fresco_amd import ebsynth as E  # noqa: E402

PROF_LEVEL = 13  # FRESCO_PROF_EBSYNTH_LEVEL


def make_frame(n, seed=1):
    """smooth random style and guides; target guides = source guides shifted by (5, -3) plus 1-2 LSB of noise"""
    g = torch.Generator().manual_seed(seed)

    def smooth(c, cell):
        x = torch.rand(1, c, n // cell + 2, n // cell + 2, generator=g) * 255
        x = torch.nn.functional.interpolate(x, size=(n + 2 * cell, n + 2 * cell), mode="bilinear", align_corners=False)
        return x[0, :, cell:cell + n, cell:cell + n].permute(1, 2, 0)

    style = smooth(3, 6).to(torch.uint8)
    src = torch.cat([smooth(c, 5) for c in (3, 1, 3, 3)], -1)
    tgt = torch.roll(src, shifts=(-3, 5), dims=(0, 1)) + torch.randint(-2, 3, src.shape, generator=g)
    return style, src.clamp(0, 255).to(torch.uint8), tgt.clamp(0, 255).to(torch.uint8)


def weights():
    gw = []
    for c, w in zip((3, 1, 3, 3), (6.0, 0.5, 0.5, 2.0)):
        gw += [w / c] * c
    return [1.0 / 3] * 3, gw


def launches_per_frame(levels, svi, pmi, extra, uniformity, modulation=False, nnf_out=False):
    """Launches + async copies/memsets fresco_ebsynth_run enqueues (ebsynth.hip, driver): 2-3 packs; per level 1 copy
    (finest) or 2-3 resamples, NNF init/upscale, E and Omega memsets, Omega build; per search/vote pass 1 vote +
    1 mask memset, per iteration 2 error passes + 4 kernels per PatchMatch iteration (+4 Omega snapshots when the
    uniformity weight is not 0), 1 vote, 2 mask kernels but the last; then unpack + 1-2 copies."""
    n = 3 if modulation else 2
    for level in range(levels):
        fine = level == levels - 1
        n += (1 if fine else (3 if modulation else 2)) + 4
        for p in range(2 if (fine and extra) else 1):
            lam = uniformity if p == 0 else 0.0
            n += 2
            for v in range(svi):
                n += (2 + pmi * (4 + (4 if lam != 0 else 0))) if pmi > 0 else 1
                n += 1 + (2 if v < svi - 1 else 0)
    return n + 2 + (1 if nnf_out else 0)


def time_runs(args, kw, warmup, runs):
    for _ in range(warmup):
        ebsynth_run(*args, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ebsynth_run(*args, **kw)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def level_split(args, kw):
    lib = _lib.load()
    lib.fresco_prof_enable(64)
    ebsynth_run(*args, **kw)
    torch.cuda.synchronize()
    tags, dims, ms = (_lib._c.c_int * 64)(), (_lib._c.c_int * 256)(), (_lib._c.c_float * 64)()
    n = lib.fresco_prof_read(64, tags, dims, ms)
    lib.fresco_prof_disable()
    return [dict(level=dims[4 * i], size="%dx%d" % (dims[4 * i + 1], dims[4 * i + 2]), patch=dims[4 * i + 3],
                 ms=round(ms[i], 3)) for i in range(n) if tags[i] == PROF_LEVEL]


def cli_cost(style, src, tgt, tmp):
    from PIL import Image
    Image.fromarray(style.numpy()).save(os.path.join(tmp, "key.png"))
    cmd = [os.path.join(ROOT, "fresco_amd", "bin", "ebsynth"), "-style", os.path.join(tmp, "key.png")]
    c0 = 0
    for k, (c, w) in enumerate(zip((3, 1, 3, 3), (6, 0.5, 0.5, 2))):
        for side, img in (("s", src), ("t", tgt)):
            a = img[..., c0:c0 + c].numpy()
            Image.fromarray(a[..., 0] if c == 1 else a).save(os.path.join(tmp, "g%d%s.png" % (k, side)))
        cmd += ["-guide", os.path.join(tmp, "g%ds.png" % k), os.path.join(tmp, "g%dt.png" % k), "-weight", str(w)]
        c0 += c
    cmd += ["-output", os.path.join(tmp, "out.png"), "-searchvoteiters", "12", "-patchmatchiters", "6"]
    env = dict(os.environ, PYTHON=sys.executable)
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, env=env, timeout=600)
    wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    subprocess.run([sys.executable, "-c", "import torch, fresco_amd; fresco_amd._lib.load(); torch.zeros(1, device='cuda')"],
                   check=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    startup = time.perf_counter() - t0
    return dict(cli_process_s=round(wall, 3), python_torch_startup_s=round(startup, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cli", action="store_true", help="also time one shim process per frame")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ebsynth needs a GPU"
    dev = "cuda:0"
    style, src, tgt = make_frame(a.size)
    sw, gw = weights()
    args = (style.to(dev), src.to(dev), tgt.to(dev))
    kw = dict(style_weights=sw, guide_weights=gw, search_vote_iters=12, patchmatch_iters=6)
    levels = E.max_pyramid_levels((a.size, a.size), (a.size, a.size), 5)
    ts = time_runs(args, kw, a.warmup, a.runs)
    ts3 = time_runs(args, dict(kw, extra_pass_3x3=True), a.warmup, a.runs)
    res = dict(metric="ebsynth_ms_per_frame", size=a.size, n_style=3, n_guide=10, levels=levels,
               ms_per_frame=round(statistics.median(ts), 3), ms_runs=[round(t, 3) for t in ts],
               ms_per_frame_extra_pass_3x3=round(statistics.median(ts3), 3),
               launches_per_frame=launches_per_frame(levels, 12, 6, False, 3500.0),
               launches_per_frame_extra_pass_3x3=launches_per_frame(levels, 12, 6, True, 3500.0),
               per_level=level_split(args, kw))
    out, err = ebsynth_run(*args, **kw)
    res["mean_error"] = round(float(err.mean()), 2)
    if a.cli:
        with tempfile.TemporaryDirectory() as tmp:
            res.update(cli_cost(style, src, tgt, tmp))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
