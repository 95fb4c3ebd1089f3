#!/usr/bin/env python
"""Key-frame selection's per-frame work on 64 frames of 1080 x 1920 (resized to 512 x 896), the synthetic frames of
tests/keyframe_model.py, in milliseconds per frame:

  resident    fresco_amd.frame_errors on two chunks of 32 frames already on the device, resolution 512: the area resize,
              the blurred squared differences and the one download of the sums
  from_host   the same from the host arrays a decoder hands over (the upload of each chunk is timed)
  keys        get_keyframe_ind on the host arrays, selection included
  reference   only where `import cv2` works: the reference's chain per frame, resize_image -> cv2.GaussianBlur ->
              numpy2tensor(...).cuda() -> F.mse_loss(...).cpu(); otherwise the result says that the baseline is unmeasured
              and no speed-up is claimed

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per mode: warm-up, then the
median of five timed blocks (a host clock around 100 or 20 calls of 64 frames, ended by a device synchronise).

--small runs the three package modes on 64 frames of 480 x 854 instead, a video whose short side is below 512: resize_image
enlarges it to 512 x 896 through INTER_LANCZOS4 (the tap-resize kernel, eight taps per axis).  The 1080p `resident` leg is
timed again in the same run for scale.  The reference's chain on that size is not measured (no cv2 here either).

    python tools/bench_keyframe.py        # writes profiles/keyframe_bench.json (--out FILE: elsewhere)
    python tools/bench_keyframe.py --small   # writes profiles/keyframe_small_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H0, W0, RES = 64, 1080, 1920, 512
SMALL_H0, SMALL_W0 = 480, 854
CHUNK = 32
MODES = ("resident", "from_host", "keys", "reference")
LIMITS = dict(resident=240, from_host=240, keys=240, reference=480)  # seconds per child


def timed(fn, iters, blocks=5, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters)
    return statistics.median(out) * 1e3 / N, [t * 1e3 / N for t in out]


def child(mode, H0=H0, W0=W0):
    import numpy as np
    import torch
    import fresco_amd
    import keyframe_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_keyframe.py needs a GPU")
    dev = "cuda:0"
    host = M.synthetic_frames(1, N, H0, W0, block=48 if H0 >= 1080 else 24)
    chunks = [host[i:i + CHUNK] for i in range(0, N, CHUNK)]
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    if mode == "resident":
        on_dev = [torch.from_numpy(c).to(dev) for c in chunks]
        res["ms_per_frame"], res["blocks_ms_per_frame"] = timed(lambda: fresco_amd.frame_errors(on_dev, RES), 100)
        res["size"] = list(fresco_amd.resize_size(H0, W0, RES)[:2])
        res["curve_head"] = fresco_amd.frame_errors(on_dev, RES)[:4].tolist()
    elif mode == "from_host":
        res["ms_per_frame"], res["blocks_ms_per_frame"] = timed(lambda: fresco_amd.frame_errors(chunks, RES), 20)
    elif mode == "keys":
        res["ms_per_frame"], res["blocks_ms_per_frame"] = timed(lambda: fresco_amd.get_keyframe_ind(host), 20)
        res["keys"] = [int(k) for k in fresco_amd.get_keyframe_ind(host)]
    else:
        try:
            import cv2
        except ImportError:
            res["ms_per_frame"] = None
            res["note"] = "cv2 is not installed here: the reference's per-frame chain is unmeasured, no speed-up is claimed"
            print(json.dumps(res), flush=True)
            return

        def numpy2tensor(img):  # src/utils.py
            x0 = torch.from_numpy(img.copy()).float().cuda() / 255.0 * 2.0 - 1.
            x0 = torch.stack([x0], dim=0)
            return x0.permute(0, 3, 1, 2)

        H, W, _ = fresco_amd.resize_size(H0, W0, RES)

        def loop():  # src/keyframe_selection.py:27-39
            err, pre = [0], None
            for i in range(N):
                img = cv2.resize(host[i], (W, H), interpolation=cv2.INTER_AREA)
                img = cv2.GaussianBlur(img, (9, 9), 0.0)
                cur = numpy2tensor(img)
                if i:
                    err += [float(torch.nn.functional.mse_loss(pre, cur).cpu().numpy())]
                pre = cur
            return err

        res["ms_per_frame"], res["blocks_ms_per_frame"] = timed(loop, 1)
        ours = fresco_amd.frame_errors(chunks, RES)
        res["largest_relative_difference_from_cv2_curve"] = float(np.max(np.abs(ours[1:] - np.array(loop()[1:])) / ours[1:]))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="the result as JSON goes here as well (default: profiles/keyframe_bench.json, "
                    "with --small profiles/keyframe_small_bench.json)")
    ap.add_argument("--small", action="store_true", help="the 480 x 854 legs (see above)")
    ap.add_argument("--mode", choices=MODES, default=None, help="(internal) run one mode in this process")
    ap.add_argument("--size", nargs=2, type=int, default=(H0, W0), help="(internal) the frame size of that mode")
    args = ap.parse_args()
    if args.mode:
        return child(args.mode, *args.size)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "keyframe_small_bench.json" if args.small else "keyframe_bench.json")
    if args.small:
        return main_small(args)
    got = {}
    for mode in MODES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode], stdout=subprocess.PIPE,
                           timeout=LIMITS[mode], text=True)
        if p.returncode != 0:
            sys.exit("bench_keyframe.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    ref = got["reference"]
    result = dict(bench="keyframe_frame_errors", device=got["resident"]["device"], frames=N, chunk=CHUNK, height=H0, width=W0,
                  resized=got["resident"]["size"], resident_ms_per_frame=got["resident"]["ms_per_frame"],
                  from_host_ms_per_frame=got["from_host"]["ms_per_frame"],
                  get_keyframe_ind_ms_per_frame=got["keys"]["ms_per_frame"], keys=got["keys"]["keys"],
                  reference_per_frame_chain_ms_per_frame=ref["ms_per_frame"],
                  timed_blocks_ms_per_frame={m: got[m].get("blocks_ms_per_frame") for m in MODES})
    if ref["ms_per_frame"] is None:
        result["reference_note"] = ref["note"]
    else:
        result["largest_relative_difference_from_cv2_curve"] = ref["largest_relative_difference_from_cv2_curve"]
        result["reference_over_from_host"] = ref["ms_per_frame"] / got["from_host"]["ms_per_frame"]
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def run_mode(mode, size):
    """one mode in a child process of its own under its time limit -> its result; a child that fails ends the run"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--size", str(size[0]), str(size[1])],
                       stdout=subprocess.PIPE, timeout=LIMITS[mode], text=True)
    if p.returncode != 0:
        sys.exit("bench_keyframe.py: mode %s at %d x %d ended with status %d; nothing further is started"
                 % (mode, size[0], size[1], p.returncode))
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(mode, size, res, flush=True)
    return res


def main_small(args):
    small = (SMALL_H0, SMALL_W0)
    got = {mode: run_mode(mode, small) for mode in ("resident", "from_host", "keys")}
    big = run_mode("resident", (H0, W0))
    result = dict(bench="keyframe_frame_errors_small", device=got["resident"]["device"], frames=N, chunk=CHUNK,
                  height=SMALL_H0, width=SMALL_W0, resized=got["resident"]["size"], resize="INTER_LANCZOS4 (frame_resize_u8)",
                  resident_ms_per_frame=got["resident"]["ms_per_frame"],
                  from_host_ms_per_frame=got["from_host"]["ms_per_frame"],
                  get_keyframe_ind_ms_per_frame=got["keys"]["ms_per_frame"], keys=got["keys"]["keys"],
                  area_1080p_resident_ms_per_frame=big["ms_per_frame"], area_1080p_resized=big["size"],
                  runs="per figure: 2 warm-up calls, then the median of 5 timed blocks of 100 (resident) or 20 calls of "
                       "64 frames",
                  reference_note="cv2 is not installed here: the reference's per-frame chain is unmeasured, no speed-up is "
                                 "claimed",
                  timed_blocks_ms_per_frame=dict(resident=got["resident"]["blocks_ms_per_frame"],
                                                 from_host=got["from_host"]["blocks_ms_per_frame"],
                                                 keys=got["keys"]["blocks_ms_per_frame"],
                                                 area_1080p_resident=big["blocks_ms_per_frame"]))
    print(json.dumps(result))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
