#!/usr/bin/env python
"""The EGNet saliency detector on 8 frames of 512 x 512 (one key-frame batch of run_fresco.py), stand-in weights of
tests/egnet_model.py and frames of tests/hed_model.py:

  native      get_saliency on this package's kernels (frames already on the device, result left there)
  library     the same module with library_ops=True: the live graph on PyTorch's convolutions, pooling and interpolation,
              batched, between this package's input and tail kernels
  per_frame   a restatement of what the reference does (src/utils.py:96-102), one frame at a time: host cv2sod, upload,
              the full forward with every side head, sigmoid, Dilate
  stages      native: the time between the stage marks of TUN_bone._score_native (backbone with convert / merge1 /
              merge2) and the tail kernel, from device events around one batch

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per mode: warm-up, then the
median of five timed blocks (a host clock around several calls that end in a device synchronise).

    python tools/bench_egnet.py [--out profiles/egnet_bench.json]
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
MODES = ("native", "library", "per_frame", "stages")
LIMITS = dict(native=240, library=240, per_frame=300, stages=240)  # seconds per child


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
    return statistics.median(out) * 1e3, [t * 1e3 for t in out]


def child(mode):
    import torch
    import fresco_amd
    import egnet_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_egnet.py needs a GPU")
    dev = "cuda:0"
    net = fresco_amd.TUN_bone(library_ops=mode in ("library", "per_frame"))
    net.load_state_dict(M.standin_state_dict())
    net = net.to(dev).eval()
    host = M.frames((N, H, W))
    frames = torch.from_numpy(host).to(dev)
    dil = fresco_amd.Dilate(kernel_size=7, device=dev)
    res = dict(mode=mode)
    if mode in ("native", "library"):
        res["ms"], res["blocks_ms"] = timed(lambda: fresco_amd.get_saliency(frames, net, dil), 3)
    elif mode == "per_frame":
        ones = torch.ones(1, 1, 7, 7, device=dev)

        def loop():
            out = []
            with torch.no_grad():
                for i in range(N):
                    x = M.cv2sod64(host[i:i + 1], torch.float32).to(dev)  # host cv2sod, then the upload
                    p = torch.nn.functional.pad(torch.sigmoid(net(x)[2][-1]), (3, 3, 3, 3), "replicate")
                    out.append(1 - torch.clamp(torch.nn.functional.conv2d(p, ones), 0, 1))  # utils.Dilate on library ops
            return torch.cat(out, 0)
        res["ms"], res["blocks_ms"] = timed(loop, 1)
    else:
        from fresco_amd import ops
        names = ("backbone", "merge1", "merge2")
        runs = []
        with torch.no_grad():
            for it in range(7):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
                k = [0]

                def mark(stage):
                    k[0] += 1
                    ev[k[0]].record()
                ev[0].record()
                with ops.fn_range_guard(frames.device):
                    score = net._score_native(frames, mark=mark)
                ops.egnet_saliency(score, (H // 2, W // 2), k=7)
                ev[4].record()
                torch.cuda.synchronize()
                runs.append([ev[i].elapsed_time(ev[i + 1]) for i in range(4)])
        runs = runs[2:]  # (warm-up: the weight planes are made on the first pass)
        res["stages_ms"] = {name: statistics.median(r[i] for r in runs) for i, name in enumerate(names + ("tail",))}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the result as JSON here as well")
    ap.add_argument("--mode", choices=MODES, default=None, help="(internal) run one mode in this process")
    args = ap.parse_args()
    if args.mode:
        return child(args.mode)
    got = {}
    for mode in MODES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode], stdout=subprocess.PIPE,
                           timeout=LIMITS[mode], text=True)
        if p.returncode != 0:
            sys.exit("bench_egnet.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    native, library, per_frame = got["native"]["ms"], got["library"]["ms"], got["per_frame"]["ms"]
    result = dict(bench="egnet_get_saliency", device=got["native"]["device"], frames=N, height=H, width=W, native_ms=native,
                  library_batched_ms=library, reference_per_frame_loop_ms=per_frame, library_over_native=library / native,
                  per_frame_over_native=per_frame / native, native_stages_ms=got["stages"]["stages_ms"],
                  timed_blocks_ms={m: got[m]["blocks_ms"] for m in ("native", "library", "per_frame")})
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
