#!/usr/bin/env python
"""What fresco_amd.unet_shell replaces, at the shapes of one SD-1.5 denoising step at 512 x 512, batch 16 (8 frames x
classifier-free guidance), fp16, stand-in weights and the restated modules of tests/unet_shell_model.py:

  native    each drop-in, channels_last in and out: Downsample2D 320 @64 / 640 @32 / 1280 @16, Upsample2D 1280 @8 / 1280 @16 /
            640 @32 (input planes), conv_in 4 -> 320 @64, conv_norm_out + SiLU + conv_out 320 -> 4 @64, the time MLP
            (320 -> 1280 -> 1280), the condition embedding at 512 x 512 -- computed on every call, and answered from its cache
  pytorch   the same nn.Module in fp16 on PyTorch's own kernels on the same GPU, contiguous and channels_last; the faster one
            counts
  kinds     unet_conv3 at stride 2 against vaeenc_conv_down at the same cin, cout and plane, with algorithmic TFLOP/s and the
            share of the 2.5 PFLOP/s dense fp16 MFMA peak

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per measurement: two warm-up
calls, then the median of five timed blocks (a host clock around several calls that end in a device synchronise).  No time
is fixed in advance: the comparison is against the PyTorch fp16 module measured in the same run, and every shape where
PyTorch wins is listed as such.

    python tools/bench_unet_shell.py [--out profiles/unet_shell_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_vae import PEAK_F16_DENSE, timed  # noqa: E402

N = 16
MODES = ("native", "pytorch", "kinds")
LIMITS = dict(native=240, pytorch=420, kinds=240)  # seconds per child
# (kind of tests/unet_shell_model.py, width, side of the input plane, how many the UNet runs, how many the ControlNet runs)
SHAPES = (("down", 320, 64, 1, 1), ("down", 640, 32, 1, 1), ("down", 1280, 16, 1, 1),
          ("up", 1280, 8, 1, 0), ("up", 1280, 16, 1, 0), ("up", 640, 32, 1, 0),
          ("conv_in", 320, 64, 1, 1), ("conv_out", 320, 64, 1, 0), ("time", 320, 1, 1, 1), ("cond", 320, 512, 0, 1))


def _name(kind, c, side):
    return {"down": "Downsample2D %d @%d", "up": "Upsample2D %d @%d", "conv_in": "conv_in 4->%d @%d",
            "conv_out": "conv_norm_out+SiLU+conv_out %d->4 @%d", "time": "time MLP %d->1280->1280, n %d",
            "cond": "condition embedding 3->%d @%d"}[kind] % ((c, N) if kind == "time" else (c, side))


def _iters(side):
    return 3 if side >= 64 else 6


def _input(kind, c, side, g):
    import torch
    if kind == "time":
        return torch.linspace(1.0, 981.0, N).round()
    cin = {"conv_in": 4, "cond": 3}.get(kind, c)
    return torch.randn(N, cin, side, side, generator=g).half()


def child(mode):
    import torch
    import fresco_amd
    from fresco_amd import ops
    import unet_shell_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_unet_shell.py needs a GPU")
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    if mode in ("native", "pytorch"):
        rows = []
        for kind, c, side, _, _ in SHAPES:
            mod = M.build((kind, c, N, side, side), torch.float16).to(dev)
            x = _input(kind, c, side, g).to(dev)
            plain = kind in ("time", "conv_in", "cond")       # what the model hands these is not channels_last
            x_cl = x if plain else x.contiguous(memory_format=torch.channels_last)
            row = dict(shape=_name(kind, c, side))
            it = _iters(side)
            if mode == "native":
                if kind == "time":
                    native = fresco_amd.UNetTimeEmbedding.from_module(mod)
                    fn = lambda: native(native.proj(x))  # noqa: E731
                elif kind == "conv_out":
                    native = fresco_amd.UNetConvOut.from_module(mod)
                    fn = lambda: native(x_cl)  # noqa: E731
                else:
                    cls, m = {"down": (fresco_amd.UNetDownsample, mod), "up": (fresco_amd.UNetUpsample, mod),
                              "conv_in": (fresco_amd.UNetConvIn, getattr(mod, "conv", None)),
                              "cond": (fresco_amd.ControlNetCondEmbedding, mod)}[kind]
                    native = cls.from_module(m)
                    fn = lambda: native(x_cl)  # noqa: E731
                if kind == "cond":
                    native.cache = False
                    row["ms"], row["blocks_ms"] = timed(fn, it)
                    native.cache = True
                    row["cached_ms"], _ = timed(fn, 20)
                else:
                    row["ms"], row["blocks_ms"] = timed(fn, it)
            else:
                with torch.no_grad():
                    if kind == "time":
                        row["contiguous_ms"], _ = timed(lambda: mod(x, dtype=torch.float16), it)
                        row["channels_last_ms"] = row["contiguous_ms"]
                    else:
                        row["contiguous_ms"], _ = timed(lambda: mod(x), it)
                        mod_cl = mod.to(memory_format=torch.channels_last)
                        x_in = x.contiguous(memory_format=torch.channels_last)
                        row["channels_last_ms"], _ = timed(lambda: mod_cl(x_in), it)
                row["ms"] = min(row["contiguous_ms"], row["channels_last_ms"])
            rows.append(row)
            del mod, x, x_cl
        res["rows"] = rows
    else:
        conv = []
        for c, side in ((320, 64), (640, 32), (1280, 16)):
            x = torch.randn(N, side, side, c, generator=g).half().to(dev)
            wt = (torch.randn(c, 9 * c, generator=g) * (9 * c) ** -0.5).half().to(dev)
            b = torch.randn(c, generator=g).to(dev)
            ms, _ = timed(lambda: ops.unet_conv3(x, wt, b, stride=2), 6)
            enc_ms, _ = timed(lambda: ops.vaeenc_conv_down(x, wt, b), 6)
            flop = 2.0 * N * (side // 2) ** 2 * c * 9 * c
            conv.append(dict(form="3x3 stride 2 %d->%d @%d" % (c, c, side), unet_conv3_ms=ms, vaeenc_conv_down_ms=enc_ms,
                             vaeenc_over_unet_conv3=enc_ms / ms, tflops=flop / ms / 1e9,
                             frac_of_mfma_peak=flop / (ms * 1e-3) / PEAK_F16_DENSE))
            del x, wt
        res["conv"] = conv
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
            sys.exit("bench_unet_shell.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    shapes, nat_ms, pt_ms = [], 0.0, 0.0
    for (kind, c, side, u, cn), nat, pt in zip(SHAPES, got["native"]["rows"], got["pytorch"]["rows"]):
        row = dict(shape=nat["shape"], unet_count=u, controlnet_count=cn, native_ms=nat["ms"], pytorch_ms=pt["ms"],
                   pytorch_contiguous_ms=pt["contiguous_ms"], pytorch_channels_last_ms=pt["channels_last_ms"],
                   pytorch_over_native=pt["ms"] / nat["ms"], pytorch_wins=bool(pt["ms"] < nat["ms"]), native_blocks_ms=nat["blocks_ms"])
        if "cached_ms" in nat:
            row["native_cached_ms"] = nat["cached_ms"]
            row["pytorch_over_native_cached"] = pt["ms"] / nat["cached_ms"]
        shapes.append(row)
        nat_ms += (u + cn) * nat["ms"]
        pt_ms += (u + cn) * pt["ms"]
    result = dict(bench="unet_shell", device=got["native"]["device"], batch=N, image=512, dtype="float16", shapes=shapes,
                  per_step_uncached=dict(native_ms=nat_ms, pytorch_ms=pt_ms, pytorch_over_native=pt_ms / nat_ms),
                  shapes_where_pytorch_wins=[s["shape"] for s in shapes if s["pytorch_wins"]],
                  conv3_stride2_vs_vaeenc_conv_down=got["kinds"]["conv"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
