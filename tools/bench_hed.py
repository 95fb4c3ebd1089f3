#!/usr/bin/env python
"""The HED annotator on 8 frames of 512 x 512 (one key-frame batch of run_fresco.py), stand-in weights and frames of
tests/hed_model.py:

  native      HEDdetector.detect_batch on this package's kernels (frames already on the device, result left there)
  library     the same module with library_ops=True: PyTorch's convolutions and pooling, batched, this package's fuse
  per_frame   a restatement of the reference's loop (src/ControlNet/annotator/hed/__init__.py:66-78), one frame at a
              time: host -> device copy, library ops, five maps back to the host, host resize (the stand-in of
              tests/hed_model.py for cv2.resize), float64 sigmoid, uint8 on the host
  from_host   native again, from the list of host arrays the reference's caller holds (the upload is timed)
  blocks      native and library up to block k, k = 1 .. 5: the difference of consecutive figures is block k's time

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per mode: warm-up, then the
median of five timed blocks (a host clock around several calls that end in a device synchronise; per_frame ends on the
host by itself).
FLOPs are counted from the shapes (2 x 9 x cin x cout per output pixel and convolution).

    python tools/bench_hed.py [--out profiles/hed_bench.json]
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
MODES = ("native", "library", "per_frame", "from_host", "blocks")
LIMITS = dict(native=180, library=180, per_frame=240, from_host=180, blocks=300)  # seconds per child


def conv_flops():
    import hed_model as M
    per_block, h, w = [], H, W
    for cin, cout, layers in M.BLOCKS:
        per_block.append(sum(2 * 9 * (cin if j == 0 else cout) * cout * N * h * w for j in range(layers)))
        h, w = h // 2, w // 2
    return per_block


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
    import numpy as np
    import torch
    import fresco_amd
    import hed_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_hed.py needs a GPU")
    dev = "cuda:0"
    net = fresco_amd.ControlNetHED_Apache2(library_ops=mode in ("library", "per_frame"))
    net.load_state_dict(M.standin_state_dict())
    net = net.to(dev).eval()
    det = fresco_amd.HEDdetector(network=net)
    host = M.frames((N, H, W))
    frames = torch.from_numpy(host).to(dev)
    res = dict(mode=mode)
    if mode in ("native", "library"):
        res["ms"], res["blocks_ms"] = timed(lambda: det.detect_batch(frames), 5)
    elif mode == "from_host":
        lst = [host[i] for i in range(N)]
        res["ms"], res["blocks_ms"] = timed(lambda: det.detect_batch(lst), 5)
    elif mode == "per_frame":
        def loop():
            out = []
            with torch.no_grad():
                for i in range(N):
                    x = torch.from_numpy(host[i].copy()).float().to(dev).permute(2, 0, 1)[None]
                    edges = [e.detach().cpu().numpy().astype(np.float32)[0, 0] for e in net(x)]
                    out.append(M.fuse_u8(edges, H, W)[1])
            return out
        res["ms"], res["blocks_ms"] = timed(loop, 2)
    else:
        lib = fresco_amd.ControlNetHED_Apache2(library_ops=True)
        lib.load_state_dict(M.standin_state_dict())
        lib = lib.to(dev).eval()
        res["native_upto_ms"], res["library_upto_ms"] = [], []
        with torch.no_grad():
            for k in range(1, 6):
                res["native_upto_ms"].append(timed(lambda: net._sides_native(frames, k), 5)[0])
                res["library_upto_ms"].append(timed(lambda: lib._sides_library(frames, k), 5)[0])
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
            sys.exit("bench_hed.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    flops = conv_flops()
    diff = lambda v: [v[0]] + [v[k] - v[k - 1] for k in range(1, 5)]  # noqa: E731
    nat_b, lib_b = diff(got["blocks"]["native_upto_ms"]), diff(got["blocks"]["library_upto_ms"])
    native, library, per_frame = got["native"]["ms"], got["library"]["ms"], got["per_frame"]["ms"]
    result = dict(bench="hed_detect_batch", device=got["native"]["device"], frames=N, height=H, width=W,
                  conv_gflop=sum(flops) / 1e9, native_ms=native, library_batched_ms=library,
                  reference_per_frame_loop_ms=per_frame, native_from_host_ms=got["from_host"]["ms"],
                  native_tflops=sum(flops) / native / 1e9, library_over_native=library / native,
                  per_frame_over_native=per_frame / native, per_frame_over_native_from_host=per_frame / got["from_host"]["ms"],
                  timed_blocks_ms={m: got[m]["blocks_ms"] for m in ("native", "library", "per_frame", "from_host")},
                  per_block=[dict(block=k + 1, conv_gflop=flops[k] / 1e9, native_ms=nat_b[k], library_ms=lib_b[k],
                                  native_tflops=flops[k] / nat_b[k] / 1e9) for k in range(5)])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
