"""video_blend backend on process_seq's shape: 512x512, one key interval of 8 in-between frames, gradient (Poisson)
blending on, the method of tools/bench_ebsynth.py.

Prints one JSON line: median ms per frame over --runs timed runs of the whole interval after --warmup warm-ups (host
clock around a synchronised blend_interval call, divided by the frame count), the launches per frame, and for
comparison the numpy + scipy restatement of the reference's per-frame step (tests/blend_model.py with the
reference-shaped lsqr solve) timed on this host's CPUs: its Poisson solve alone and the whole frame."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from fresco_amd import blend as B  # noqa: E402
import blend_model as M  # noqa: E402
import make_blend_golden as G  # noqa: E402

# memset + prep + rhs + tables + 4 GEMMs + finish (blend.hip, fresco_blend_frame); 3 without gradient blending
LAUNCHES_GRADIENT, LAUNCHES_HISTOGRAM = 9, 3


def make_interval(size, n):
    frames = [G.frame(40 + k, size, size) for k in range(n)]
    flows = [G.flow_field(90 + k, size, size) for k in range(n - 1)]
    return frames, flows


def time_gpu(args, kw, warmup, runs, n):
    for _ in range(warmup):
        B.blend_interval(*args, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        B.blend_interval(*args, **kw)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / n)
    return ts


def time_cpu(frames, flows, k):
    """one in-between frame (k >= 1, so the mask warp runs) of the numpy + scipy lsqr restatement; the stacked sparse
    system is built before the clock starts, as the reference caches it across frames"""
    f = frames[k]
    n = len(frames)
    prev = M.blend_frame(frames[k - 1]["oa"], frames[k - 1]["ob"], frames[k - 1]["d1"], frames[k - 1]["d2"],
                         (k - 1) / n, gradient=False)["mask"]
    res = M.blend_frame(f["oa"], f["ob"], f["d1"], f["d2"], k / n, prev, flows[k - 1], gradient=False)
    hist = res["hist"]
    M.poisson_fusion(hist, f["oa"], f["ob"], res["mask"], solver="lsqr")  # builds and caches the system
    t0 = time.perf_counter()
    M.poisson_fusion(hist, f["oa"], f["ob"], res["mask"], solver="lsqr")
    solve = time.perf_counter() - t0
    t0 = time.perf_counter()
    M.blend_frame(f["oa"], f["ob"], f["d1"], f["d2"], k / n, prev, flows[k - 1], solver="lsqr")
    frame = time.perf_counter() - t0
    return solve * 1e3, frame * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=8, help="in-between frames of the interval")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy + scipy comparison")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_blend needs a GPU"
    dev = "cuda:0"
    frames, flows = make_interval(a.size, a.frames)

    def g(x, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype)

    args = ([g(f["oa"]) for f in frames], [g(f["ob"]) for f in frames], [g(f["d1"]) for f in frames],
            [g(f["d2"]) for f in frames], [g(f) for f in flows])
    ts = time_gpu(args, dict(gradient=True), a.warmup, a.runs, a.frames)
    th = time_gpu(args, dict(gradient=False), a.warmup, a.runs, a.frames)
    res = dict(metric="blend_ms_per_frame", size=a.size, frames=a.frames, gradient=True,
               ms_per_frame=round(statistics.median(ts), 3), ms_runs=[round(t, 3) for t in ts],
               ms_per_frame_histogram_only=round(statistics.median(th), 3),
               launches_per_frame=LAUNCHES_GRADIENT, launches_per_frame_histogram_only=LAUNCHES_HISTOGRAM)
    if not a.no_cpu:
        solve, frame = time_cpu(frames, flows, 1)
        res.update(cpu_threads=torch.get_num_threads(), cpu_lsqr_poisson_ms=round(solve, 1),
                   cpu_lsqr_frame_ms=round(frame, 1), speedup_vs_cpu_frame=round(frame / res["ms_per_frame"], 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
