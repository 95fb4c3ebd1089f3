#!/usr/bin/env python
"""The Canny annotator on 8 frames of 512 x 512 (one key-frame batch of run_fresco.py), the natural field of
tests/canny_model.py at thresholds 50 / 100:

  native         CannyDetector.detect_batch on this package's kernels (frames already on the device, result left there)
  from_host      the same from the list of host arrays the reference's caller holds (the upload is timed)
  control_image  CannyDetector.control_image(frames, fp16): the edge maps and the doubled condition tensor in one call
  reference      only where `import cv2` works: the reference's chain per frame, cv2.Canny(img, 50, 100) on the host ->
                 numpy2tensor(...) -> .cuda(), then the condition as run_fresco.py:199-202 builds it; otherwise the
                 result says that the baseline is unmeasured

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per mode: warm-up, then the
median of five timed blocks (a host clock around several calls that end in a device synchronise).

    python tools/bench_canny.py        # writes profiles/canny_bench.json (--out FILE: elsewhere)
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

N, H, W = 8, 512, 512
LOW, HIGH = 50, 100
MODES = ("native", "from_host", "control_image", "reference")
LIMITS = dict(native=180, from_host=180, control_image=180, reference=240)  # seconds per child


def timed(fn, iters, blocks=5, warmup=3):
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
    return statistics.median(out) * 1e3, [t * 1e3 for t in out]


def child(mode):
    import torch
    import fresco_amd
    import canny_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_canny.py needs a GPU")
    dev = "cuda:0"
    host = M.natural(N, H, W, 10.0, seed=1)
    lst = [host[i] for i in range(N)]
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    det = fresco_amd.CannyDetector()
    if mode == "native":
        frames = torch.from_numpy(host).to(dev)
        res["ms"], res["blocks_ms"] = timed(lambda: det.detect_batch(frames, LOW, HIGH), 20)
        res["edge_fraction"] = float((det.detect_batch(frames, LOW, HIGH) == 255).float().mean())
    elif mode == "from_host":
        res["ms"], res["blocks_ms"] = timed(lambda: det.detect_batch(lst, LOW, HIGH), 20)
    elif mode == "control_image":
        frames = torch.from_numpy(host).to(dev)
        res["ms"], res["blocks_ms"] = timed(lambda: det.control_image(frames, torch.float16, True, LOW, HIGH), 20)
    else:
        try:
            import cv2
        except ImportError:
            res["ms"] = None
            res["note"] = "cv2 is not installed here: the reference's per-frame chain is unmeasured"
            print(json.dumps(res), flush=True)
            return

        def numpy2tensor(img):  # src/utils.py
            x0 = torch.from_numpy(img.copy()).float().cuda() / 255.0 * 2.0 - 1.
            x0 = torch.stack([x0], dim=0)
            return x0.permute(0, 3, 1, 2)

        def loop():  # run_fresco.py:199-202
            edges = torch.cat([numpy2tensor(cv2.Canny(img, LOW, HIGH)[:, :, None]) for img in lst], dim=0)
            edges = edges.repeat(1, 3, 1, 1).cuda() * 0.5 + 0.5
            return torch.cat([edges.to(torch.float16)] * 2)

        res["ms"], res["blocks_ms"] = timed(loop, 5)
        same = all(bool((det(img, LOW, HIGH) == cv2.Canny(img, LOW, HIGH)).all()) for img in lst)
        res["native_equals_cv2"] = same
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canny_bench.json"),
                    help="the result as JSON goes here as well")
    ap.add_argument("--mode", choices=MODES, default=None, help="(internal) run one mode in this process")
    args = ap.parse_args()
    if args.mode:
        return child(args.mode)
    got = {}
    for mode in MODES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode], stdout=subprocess.PIPE,
                           timeout=LIMITS[mode], text=True)
        if p.returncode != 0:
            sys.exit("bench_canny.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    ref = got["reference"]
    result = dict(bench="canny_detect_batch", device=got["native"]["device"], frames=N, height=H, width=W, low=LOW, high=HIGH,
                  edge_fraction=got["native"]["edge_fraction"], native_ms=got["native"]["ms"],
                  native_from_host_ms=got["from_host"]["ms"], control_image_fp16_ms=got["control_image"]["ms"],
                  reference_per_frame_chain_ms=ref["ms"],
                  timed_blocks_ms={m: got[m].get("blocks_ms") for m in MODES})
    if ref["ms"] is None:
        result["reference_note"] = ref["note"]
    else:
        result["native_equals_cv2"] = ref["native_equals_cv2"]
        result["reference_over_control_image"] = ref["ms"] / got["control_image"]["ms"]
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
