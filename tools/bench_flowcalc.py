"""fresco_amd.flowcalc.FlowCalc at video_blend.py's frame size (512 x 512), closed-form stand-in GMFlow weights
(tests/golden/closed_form.py; the published checkpoint is not needed for timing).

Workload: --frames frames, the pairs video_blend.py's two chains of one key interval request: (k, k + 1) forwards and
(k + 1, k) backwards, 2 (frames - 1) pairs, of which frames - 1 are swaps of others.  Reported per requested pair, median
of --runs timed runs after --warmup (host clock around device-synchronised calls; outputs come back to the host as
get_flow's do, no files):

  loop               get_flow per pair (one bidirectional forward each, batch 1): the reference's call pattern
  batched            get_flows at max_pairs 1 / 4 / 8 / 16, with and without sharing a forward between swapped pairs
  library_ops        the same two forms with FRESCO_GMFLOW_LIBRARY_OPS=1: the network on PyTorch's library ops, the
                     nearest in-tree stand-in for the reference's eager network
  driver             the `flows` phase of fresco_amd.propagate.run_ebsynth on tools/bench_propagate.py --mode driver's
                     sequence (512 x 512, key frames every 10 of 21 frames) with the FlowCalc patched in: before (a
                     flow_calc with get_flow only: the per-pair loop) and after (get_flows); synthesis is the stand-in
                     answer there, it is not what is measured

Every forward's range guard is watched: `library_fallbacks` counts forwards recomputed with library ops.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import closed_form as cf  # noqa: E402
from fresco_amd import flowcalc as FC  # noqa: E402


def stand_in_model():
    import fresco_amd.gmflow as G
    m = G.GMFlow(**FC.CONFIG).eval()
    m.load_state_dict({k: cf.gmflow_param(k, tuple(v.shape)) for k, v in m.state_dict().items()})
    return m.cuda()


def make_frames(n, size):
    return [f.permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).numpy().copy()
            for f in cf.gmflow_frames(n, size, size)]


def chain_pairs(n):
    return [(k, k + 1) for k in range(n - 1)] + [(k + 1, k) for k in reversed(range(n - 1))]


class Fallbacks:
    """counts the range guard's RuntimeWarning (a forward recomputed with library ops)"""

    def __init__(self):
        self.n = 0

    def __enter__(self):
        self._cm = warnings.catch_warnings(record=True)
        self._rec = self._cm.__enter__()
        warnings.simplefilter("always")
        return self

    def __exit__(self, *exc):
        self.n += sum("left the range" in str(w.message) for w in self._rec)
        return self._cm.__exit__(*exc)


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def per_pair_ms(seconds, pairs):
    return round(1e3 * seconds / pairs, 3)


def bench_forms(m, frames, pairs, a, fb, library_ops=False):
    out = {}
    fc = FC.FlowCalc(flow_model=m, max_pairs=1, share=False)

    def loop():
        for i, j in pairs:
            fc.get_flow(frames[i], frames[j])

    with fb:
        out["loop"] = per_pair_ms(timed(loop, a.warmup, a.runs), len(pairs))
        for mp in ((8,) if library_ops else (1, 4, 8, 16)):
            for share in (False, True):
                f = FC.FlowCalc(flow_model=m, max_pairs=mp, share=share)
                out["batched_max%d_%s" % (mp, "shared" if share else "unshared")] = per_pair_ms(
                    timed(lambda: f.get_flows(frames, pairs), a.warmup, a.runs), len(pairs))
    return out


def driver_flows(m, a, fb):
    import video_blend_standins as S
    from fresco_amd import propagate as P
    sys.modules["blender.guide"] = types.SimpleNamespace(read_flow=S.read_flow, read_mask=S.read_mask, flow_calc=None)
    key_ind = [0, 10, 20]
    res = {}
    for form in ("before_get_flow_loop", "after_get_flows"):
        walls = []
        for r in range(1 + a.driver_runs):
            with tempfile.TemporaryDirectory() as tmp, fb:
                S.make_video(tmp, key_ind, h=a.size, w=a.size)
                vs = S.VideoSequence(tmp, key_ind)
                fc = FC.FlowCalc(flow_model=m, max_pairs=a.max_pairs)
                vb = types.SimpleNamespace(cv2=S.cv2, flow_calc=None)
                FC.patch_flow_calc(vb, fc)
                if form.startswith("before"):
                    vb.flow_calc = types.SimpleNamespace(get_flow=fc.get_flow)
                st = {}
                P.run_ebsynth(vb, vs, stats=st, synth=S.answer_all)
                if r:
                    walls.append(st["flows"])
        res[form] = round(statistics.median(walls), 4)
    res["pairs"] = 2 * sum(e - b - 1 for b, e in zip(key_ind[:-1], key_ind[1:]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-pairs", type=int, default=FC.MAX_PAIRS, help="driver: FlowCalc's max_pairs")
    ap.add_argument("--driver-runs", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_flowcalc needs a GPU"
    m = stand_in_model()
    frames = make_frames(a.frames, a.size)
    pairs = chain_pairs(a.frames)
    fb = Fallbacks()
    res = dict(metric="flowcalc_ms_per_pair", size=a.size, frames=a.frames, pairs=len(pairs),
               forwards_shared=len(FC.schedule(pairs, True)[0]), weights="closed-form stand-in")
    res["hip"] = bench_forms(m, frames, pairs, a, fb)
    res["hip"]["ratio_batched_max8_shared_vs_loop"] = round(res["hip"]["batched_max8_shared"] / res["hip"]["loop"], 3)
    hip_fallbacks = fb.n
    os.environ["FRESCO_GMFLOW_LIBRARY_OPS"] = "1"
    try:
        res["library_ops"] = bench_forms(m, frames, pairs, a, Fallbacks(), library_ops=True)
    finally:
        del os.environ["FRESCO_GMFLOW_LIBRARY_OPS"]
    fb_driver = Fallbacks()
    res["driver_flows_s"] = driver_flows(m, a, fb_driver)
    res["library_fallbacks"] = hip_fallbacks + fb_driver.n
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
