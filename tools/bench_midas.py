#!/usr/bin/env python
"""The MiDaS depth annotator on 8 frames of 512 x 512 (one key-frame batch of run_fresco.py), stand-in weights and frames of
tests/midas_model.py:

  native      MidasDetector.detect_batch on this package's kernels (frames already on the device, results left there)
  library     the same module with library_ops=True: PyTorch's own kernels, batched, between this package's input and tail
  per_frame   a restatement of the reference's loop (src/ControlNet/annotator/midas/__init__.py), one frame at a time: host
              -> device copy, an fp32 forward on library ops, two copies back to the host, the numpy tail of
              tests/midas_model.py (its Sobel in cv2.Sobel's place; that host tail is also timed alone and reported, because
              numpy's Sobel is slower than OpenCV's: the loop without it is the figure to hold against the reference)
  from_host   native again, from the list of host arrays the reference's caller holds (the upload is timed)
  parts       native with a device synchronise after the backbone, the transformer and the decoder: where the time goes

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per mode: warm-up, then the
median of five timed blocks (a host clock around several calls that end in a device synchronise; per_frame ends on the
host by itself).

    python tools/bench_midas.py [--out profiles/midas_bench.json]
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
MODES = ("native", "library", "per_frame", "from_host", "parts")
LIMITS = dict(native=240, library=240, per_frame=300, from_host=240, parts=240)  # seconds per child


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
    import midas_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_midas.py needs a GPU")
    dev = "cuda:0"
    net = fresco_amd.DPTDepthModel(library_ops=mode in ("library", "per_frame"))
    net.load_state_dict(M.standin_state_dict(M.module_names_shapes(net)))
    net = net.to(dev).eval()
    det = fresco_amd.MidasDetector(network=net)
    host = M.frames((N, H, W))
    frames = torch.from_numpy(host).to(dev)
    res = dict(mode=mode)
    if mode in ("native", "library"):
        res["ms"], res["blocks_ms"] = timed(lambda: det.detect_batch(frames), 3)
    elif mode == "from_host":
        lst = [host[i] for i in range(N)]
        res["ms"], res["blocks_ms"] = timed(lambda: det.detect_batch(lst), 3)
    elif mode == "per_frame":
        def loop():
            out = []
            with torch.no_grad():
                for i in range(N):
                    x = torch.from_numpy(host[i].copy()).float().to(dev)
                    x = (x / 127.5 - 1.0).permute(2, 0, 1)[None]
                    depth = net(x)[0]
                    pt = depth.clone()
                    pt -= torch.min(pt)
                    pt /= torch.max(pt)
                    pt.cpu().numpy()
                    out.append(M.tail(depth.cpu().numpy()))
            return out
        res["ms"], res["blocks_ms"] = timed(loop, 1)
        # the host tail alone: numpy concatenations where the reference calls cv2.Sobel, so this share of the loop is the
        # stand-in's cost, not the reference's
        with torch.no_grad():
            depths = [net((torch.from_numpy(host[i].copy()).float().to(dev) / 127.5 - 1.0).permute(2, 0, 1)[None])[0].cpu().numpy()
                      for i in range(N)]
        res["tail_ms"] = timed(lambda: [M.tail(d) for d in depths], 3)[0]
    else:
        marks = {}

        def run():
            t0 = time.perf_counter()

            def mark(stage):
                torch.cuda.synchronize()
                marks.setdefault(stage, []).append(time.perf_counter() - t0)
            with torch.no_grad():
                net._depth_native(frames, mark=mark)
        for _ in range(7):
            run()
        med = {k: statistics.median(v[2:]) * 1e3 for k, v in marks.items()}
        res["backbone_ms"], res["transformer_ms"] = med["backbone"], med["transformer"] - med["backbone"]
        res["decoder_ms"] = med["decoder"] - med["transformer"]
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
            sys.exit("bench_midas.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    native, library, per_frame = got["native"]["ms"], got["library"]["ms"], got["per_frame"]["ms"]
    result = dict(bench="midas_detect_batch", device=got["native"]["device"], frames=N, height=H, width=W, native_ms=native,
                  library_batched_ms=library, reference_per_frame_loop_ms=per_frame,
                  per_frame_numpy_tail_ms=got["per_frame"]["tail_ms"],
                  per_frame_loop_without_tail_ms=per_frame - got["per_frame"]["tail_ms"],
                  native_from_host_ms=got["from_host"]["ms"], library_over_native=library / native,
                  per_frame_over_native=per_frame / native,
                  per_frame_without_tail_over_native=(per_frame - got["per_frame"]["tail_ms"]) / native,
                  per_frame_over_native_from_host=per_frame / got["from_host"]["ms"],
                  native_parts_ms={k: got["parts"][k] for k in ("backbone_ms", "transformer_ms", "decoder_ms")},
                  timed_blocks_ms={m: got[m]["blocks_ms"] for m in ("native", "library", "per_frame", "from_host")})
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
