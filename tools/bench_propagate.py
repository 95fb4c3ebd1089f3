"""Batched Ebsynth and the in-process video_blend driver (fresco_amd.propagate) on video_blend.py's frame shape:
512x512, RGB style, four guides (colour 3 + edge 1 + temporal 3 + positional 3 = 10 channels, weights
6 / 0.5 / 0.5 / 2), -searchvoteiters 12 -patchmatchiters 6 (tools/bench_ebsynth.py's frame).

  --mode batch   per-frame synthesis time of ebsynth_run_batch for n in --ns, with ebsynth_run alongside (median of
                 --runs timed runs after --warmup, host clock around a device-synchronised call); one JSON line.
  --mode n16     --runs batches of 16 and nothing else: the workload of a `rocprofv3 --kernel-trace --stats` run.
  --mode driver  wall time of propagate.run_ebsynth on a synthetic sequence with tests/video_blend_standins.py's
                 cv2 / flow / path stand-ins (key frames every --interval frames), split into flows, guide kernels,
                 host work and synthesis.  The stand-in codecs are cheap: real cv2 JPEG and Telea inpaint costs are
                 not in these numbers.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fresco_amd import ebsynth_run, ebsynth_run_batch  # noqa: E402
from fresco_amd import ebsynth as E  # noqa: E402
from bench_ebsynth import make_frame, weights  # noqa: E402

DEV = "cuda:0"
KW = dict(search_vote_iters=12, patchmatch_iters=6)


def frames(size, n):
    """n distinct problems: bench_ebsynth's frame with per-problem seeds"""
    fs = [make_frame(size, seed=1 + b) for b in range(n)]
    return [torch.stack([f[k] for f in fs]).to(DEV) for k in range(3)]


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def mode_batch(a):
    sw, gw = weights()
    kw = dict(KW, style_weights=sw, guide_weights=gw)
    res = dict(metric="ebsynth_batch_ms_per_frame", size=a.size, n_style=3, n_guide=10, runs=a.runs,
               warmup=a.warmup, by_n={})
    top = frames(a.size, max(a.ns))
    one = [t[0] for t in top]
    ts = timed(lambda: ebsynth_run(*one, **kw), a.warmup, a.runs)
    res["single_ms"] = round(statistics.median(ts), 3)
    res["single_ms_runs"] = [round(t, 3) for t in ts]
    for n in a.ns:
        args = [t[:n] for t in top]
        ws = torch.empty(E.batch_workspace_bytes(n, 3, 10, (a.size, a.size), (a.size, a.size)), dtype=torch.uint8,
                         device=DEV)
        ts = timed(lambda: ebsynth_run_batch(*args, workspace=ws, seeds=list(range(n)), **kw), a.warmup, a.runs)
        med = statistics.median(ts)
        res["by_n"][n] = dict(ms_per_batch=round(med, 3), ms_per_frame=round(med / n, 3),
                              ms_runs=[round(t, 3) for t in ts])
        del ws
    # the batch's members equal single calls (spot check, problem 1 of the largest batch)
    n = max(a.ns)
    img, err = ebsynth_run_batch(*top, seeds=list(range(n)), **kw)
    i1, e1 = ebsynth_run(*[t[1] for t in top], seed=1, **kw)
    res["member_equals_single"] = bool(torch.equal(img[1], i1) and torch.equal(err[1], e1))
    res["n16_over_n1_per_frame"] = round(res["by_n"][16]["ms_per_frame"] / res["by_n"][1]["ms_per_frame"], 3) \
        if 16 in res["by_n"] and 1 in res["by_n"] else None
    print(json.dumps(res))


def mode_n16(a):
    sw, gw = weights()
    args = frames(a.size, 16)
    for _ in range(a.runs):
        ebsynth_run_batch(*args, seeds=list(range(16)), style_weights=sw, guide_weights=gw, **KW)
    torch.cuda.synchronize()
    print(json.dumps(dict(metric="ebsynth_batch_n16_runs", size=a.size, runs=a.runs)))


def mode_driver(a):
    import video_blend_standins as S
    from fresco_amd import propagate as P
    sys.modules["blender.guide"] = types.SimpleNamespace(read_flow=S.read_flow, read_mask=S.read_mask)
    key_ind = list(range(0, a.frames, a.interval))
    if key_ind[-1] != a.frames - 1:
        key_ind.append(a.frames - 1)
    walls, stats = [], []
    for r in range(a.warmup + a.runs):
        with tempfile.TemporaryDirectory() as tmp:
            S.make_video(tmp, key_ind, h=a.size, w=a.size)
            vs = S.VideoSequence(tmp, key_ind)
            vb = types.SimpleNamespace(cv2=S.cv2, flow_calc=types.SimpleNamespace(get_flow=S.get_flow))
            st = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.run_ebsynth(vb, vs, stats=st, max_batch=a.max_batch)
            torch.cuda.synchronize()
            if r >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stats.append(st)
    med = statistics.median(walls)
    k = walls.index(med) if med in walls else 0
    split = {key: round(stats[k][key], 3) for key in ("flows", "guide_kernels", "host", "synthesis")}
    n_frames = sum(stats[k]["batches"])
    print(json.dumps(dict(metric="propagate_driver_wall_s", size=a.size, key_ind=key_ind, frames_synthesised=n_frames,
                          batches=stats[k]["batches"], wall_s=round(med, 3), wall_runs=[round(w, 3) for w in walls],
                          split_s=split, synthesis_ms_per_frame=round(1e3 * split["synthesis"] / n_frames, 2),
                          note="stand-in cv2 codecs and inpaint: real JPEG / Telea costs not measured")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batch", "n16", "driver"), default="batch")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ns", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=21, help="driver: frames of the synthetic sequence")
    ap.add_argument("--interval", type=int, default=10, help="driver: key frame every INTERVAL frames")
    ap.add_argument("--max-batch", type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_propagate needs a GPU"
    {"batch": mode_batch, "n16": mode_n16, "driver": mode_driver}[a.mode](a)


if __name__ == "__main__":
    main()
