#!/usr/bin/env python
"""The 32 ResnetBlock2D shapes of one SD-1.5 denoising step at 512 x 512 (22 in the UNet, 10 in the ControlNet), batch 16
(8 frames x classifier-free guidance), fp16, stand-in weights and the restated module of tests/unet_resnet_model.py:

  native    fresco_amd.UNetResnet per distinct shape, channels_last in and out
  pytorch   the restated module in fp16 on PyTorch's own kernels, contiguous and channels_last; the faster one counts
  kinds     each launch kind alone: unet_groupnorm at every (C, side) a block runs it, with its bytes/s against the bytes it
            must move (LDS form: one read + one write; three-launch form: two reads + one write) and the 8 TB/s HBM
            specification -- from the call time, and (`queued_us`) from device events around 40 calls queued behind 10 ms of
            matrix products, so that the host is ahead and what is timed is the GPU's work with its dispatch gaps;
            vae_conv 3 x 3 and 1 x 1 at every form, with algorithmic TFLOP/s and the share of the 2.5 PFLOP/s dense fp16
            MFMA peak, summed per resolution -- the 8 x 8 rows priced separately: vae_conv's tile is 8 x 16 pixels, so an
            8 x 8 plane computes half-empty tiles; unet_temb

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per measurement: two warm-up
calls, then the median of five timed blocks (a host clock around several calls that end in a device synchronise).  No time
is fixed in advance: the comparison is against the PyTorch fp16 module measured in the same run, and every shape where
PyTorch wins is listed as such.

    python tools/bench_unet_resnet.py [--out profiles/unet_resnet_bench.json]

--dtype bf16 (--out profiles/unet_resnet_bf16_bench.json): the same 32 blocks with bf16 weights and activations, three
children: the native bf16 blocks (csrc/net_bf16.hip's kernels), the native fp16 blocks of the same run, and PyTorch's bf16
module.  bf16 moves the same bytes as fp16 and the dense MFMA rate is the same for both types, so what is tested is parity:
per shape the bf16 median against the spread (smallest and largest) of the fp16 leg's five timed blocks.  The launch kinds
are not timed again: they are the fp16 kernels' text.
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
HBM_PEAK = 8.0e12  # bytes / s, MI355X specification
MODES = ("native", "pytorch", "kinds")
BF16_MODES = ("native", "native_fp16", "pytorch")  # --dtype bf16
LIMITS = dict(native=240, native_fp16=240, pytorch=420, kinds=240)  # seconds per child
# (cin, cout, side, how many the UNet runs, how many the ControlNet runs)
SHAPES = (
    (320, 320, 64, 2, 2), (320, 640, 32, 1, 1), (640, 640, 32, 1, 1), (640, 1280, 16, 1, 1), (1280, 1280, 16, 1, 1),
    (1280, 1280, 8, 4, 4),                                                 # two in the last down block, two in the mid block
    (2560, 1280, 8, 3, 0), (2560, 1280, 16, 2, 0), (1920, 1280, 16, 1, 0), (1920, 640, 32, 1, 0), (1280, 640, 32, 1, 0),
    (960, 640, 32, 1, 0), (960, 320, 64, 1, 0), (640, 320, 64, 2, 0),
)
assert sum(s[3] for s in SHAPES) == 22 and sum(s[4] for s in SHAPES) == 10


def _name(cin, cout, side):
    return "%d->%d @%d" % (cin, cout, side)


def _iters(cin, cout, side):
    return 3 if side >= 32 else 6


def queued_us(fn, reps=40):
    """microseconds per call on the GPU's own clock: `reps` calls between two events, queued while the device is still busy
    with matrix products, so the host's call time is not in it"""
    import torch
    a = torch.randn(8192, 8192, device="cuda:0", dtype=torch.float16)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    for _ in range(6):
        a @ a
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def child(mode, dtype="fp16"):
    import torch
    import fresco_amd
    from fresco_amd import _lib, ops
    import unet_resnet_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_unet_resnet.py needs a GPU")
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    dt = torch.bfloat16 if dtype == "bf16" and mode != "native_fp16" else torch.float16
    if mode in ("native", "native_fp16", "pytorch"):
        rows = []
        for cin, cout, side, _, _ in SHAPES:
            mod = M.build(cin, cout, dt).to(dev)
            x = torch.randn(N, cin, side, side, generator=g).to(dt).to(dev)
            temb = torch.randn(N, M.TEMB_CHANNELS, generator=g).to(dt).to(dev)
            x_cl = x.contiguous(memory_format=torch.channels_last)
            row = dict(shape=_name(cin, cout, side))
            if mode != "pytorch":
                blk = fresco_amd.UNetResnet.from_module(mod, dtype=dt)
                row["ms"], row["blocks_ms"] = timed(lambda: blk(x_cl, temb), _iters(cin, cout, side))
            else:
                with torch.no_grad():
                    row["contiguous_ms"], _ = timed(lambda: mod(x, temb), _iters(cin, cout, side))
                    mod_cl = mod.to(memory_format=torch.channels_last)
                    row["channels_last_ms"], _ = timed(lambda: mod_cl(x_cl, temb), _iters(cin, cout, side))
                row["ms"] = min(row["contiguous_ms"], row["channels_last_ms"])
            rows.append(row)
            del mod, x, x_cl
        res["rows"] = rows
    else:
        gn_shapes, conv_shapes = {}, {}
        for cin, cout, side, u, c in SHAPES:
            for C, with_addend in ((cin, False), (cout, True)):
                k = (C, side, with_addend)
                gn_shapes[k] = gn_shapes.get(k, 0) + u + c
            conv_shapes[(cin, cout, side, 3)] = conv_shapes.get((cin, cout, side, 3), 0) + u + c
            conv_shapes[(cout, cout, side, 3)] = conv_shapes.get((cout, cout, side, 3), 0) + u + c
            if cin != cout:
                conv_shapes[(cin, cout, side, 1)] = conv_shapes.get((cin, cout, side, 1), 0) + u + c
        lib = _lib.load()
        gn = []
        for (C, side, with_addend), count in sorted(gn_shapes.items()):
            P = side * side
            x = torch.randn(N, side, side, C, generator=g).half().to(dev)
            ga, be = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            ad = torch.randn(N, C, generator=g).to(dev) if with_addend else None
            lds = lib.unet_groupnorm_lds_form(N, P, C) == 1
            ms, _ = timed(lambda: ops.unet_groupnorm(x, ga, be, 1e-5, silu=True, addend=ad), 6)
            us = queued_us(lambda: ops.unet_groupnorm(x, ga, be, 1e-5, silu=True, addend=ad))
            must = N * P * C * 2 * (2 if lds else 3)
            gn.append(dict(form="GroupNorm+SiLU %d @%d%s" % (C, side, " + addend" if with_addend else ""), count=count,
                           lds_form=lds, ms=ms, bytes_moved=must, gbytes_per_s=must / ms / 1e6,
                           frac_of_hbm_peak=must / (ms * 1e-3) / HBM_PEAK, queued_us=us, queued_gbytes_per_s=must / us / 1e3,
                           queued_frac_of_hbm_peak=must / (us * 1e-6) / HBM_PEAK))
            del x
        res["groupnorm"] = gn
        conv = []
        for (cin, cout, side, k), count in sorted(conv_shapes.items()):
            x = torch.randn(N, side, side, cin, generator=g).half().to(dev)
            wt = (torch.randn(cout, k * k * cin, generator=g) * (k * k * cin) ** -0.5).half().to(dev)
            b = torch.randn(cout, generator=g).to(dev)
            r = torch.randn(N, side, side, cout, generator=g).half().to(dev)
            out = torch.empty(N * side * side * cout, dtype=torch.float16, device=dev)
            if k == 3:
                ms, _ = timed(lambda: ops.vae_conv(x, wt, b, N, side, side, cin, cout, 3, residual=r, out=out), 6)
            else:
                ms, _ = timed(lambda: ops.vae_conv(x, wt, b, N, side * side, 1, cin, cout, 1, out=out), 6)
            flop = 2.0 * N * side * side * cout * k * k * cin
            conv.append(dict(form="%dx%d %d->%d @%d" % (k, k, cin, cout, side), side=side, ksize=k, count=count, ms=ms,
                             tflops=flop / ms / 1e9, frac_of_mfma_peak=flop / (ms * 1e-3) / PEAK_F16_DENSE))
            del x, wt, r, out
        res["conv"] = conv
        temb = torch.randn(N, M.TEMB_CHANNELS, generator=g).half().to(dev)
        rows = []
        for cout in (320, 640, 1280):
            wt = (torch.randn(cout, M.TEMB_CHANNELS, generator=g) * M.TEMB_CHANNELS ** -0.5).half().to(dev)
            b = torch.randn(cout, generator=g).to(dev)
            ms, _ = timed(lambda: ops.unet_temb(temb, wt, b, b), 10)
            rows.append(dict(form="unet_temb 1280->%d, n %d" % (cout, N), ms=ms, weight_gbytes_per_s=cout * M.TEMB_CHANNELS * 2 / ms / 1e6))
        res["temb"] = rows
    print(json.dumps(res), flush=True)


def report_bf16(got, out):
    """per shape: native bf16 against PyTorch's bf16 module and against the native fp16 leg's five timed blocks"""
    shapes, tot = [], dict(native_bf16_ms=0.0, native_fp16_ms=0.0, pytorch_bf16_ms=0.0)
    for (cin, cout, side, u, c), nat, f16, pt in zip(SHAPES, got["native"]["rows"], got["native_fp16"]["rows"], got["pytorch"]["rows"]):
        lo, hi = min(f16["blocks_ms"]), max(f16["blocks_ms"])
        shapes.append(dict(shape=nat["shape"], unet_count=u, controlnet_count=c, native_bf16_ms=nat["ms"], native_bf16_blocks_ms=nat["blocks_ms"],
                           native_fp16_ms=f16["ms"], native_fp16_blocks_ms=f16["blocks_ms"], bf16_over_fp16=nat["ms"] / f16["ms"],
                           bf16_within_fp16_spread=bool(lo <= nat["ms"] <= hi), pytorch_bf16_ms=pt["ms"],
                           pytorch_contiguous_ms=pt["contiguous_ms"], pytorch_channels_last_ms=pt["channels_last_ms"],
                           pytorch_over_native=pt["ms"] / nat["ms"], pytorch_wins=bool(pt["ms"] < nat["ms"])))
        tot["native_bf16_ms"] += (u + c) * nat["ms"]
        tot["native_fp16_ms"] += (u + c) * f16["ms"]
        tot["pytorch_bf16_ms"] += (u + c) * pt["ms"]
    tot["pytorch_over_native"] = tot["pytorch_bf16_ms"] / tot["native_bf16_ms"]
    tot["bf16_over_fp16"] = tot["native_bf16_ms"] / tot["native_fp16_ms"]
    result = dict(bench="unet_resnet_bf16", device=got["native"]["device"], batch=N, image=512, dtype="bfloat16", shapes=shapes,
                  all_32_blocks=tot, shapes_where_pytorch_wins=[s["shape"] for s in shapes if s["pytorch_wins"]],
                  shapes_outside_fp16_spread=[s["shape"] for s in shapes if not s["bf16_within_fp16_spread"]])
    print(json.dumps(result))
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the result as JSON here as well")
    ap.add_argument("--mode", choices=MODES + BF16_MODES, default=None, help="(internal) run one mode in this process")
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16", help="bf16: the bf16 blocks against the fp16 leg and PyTorch")
    args = ap.parse_args()
    if args.mode:
        return child(args.mode, args.dtype)
    got = {}
    for mode in (BF16_MODES if args.dtype == "bf16" else MODES):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--dtype", args.dtype],
                           stdout=subprocess.PIPE, timeout=LIMITS[mode], text=True)
        if p.returncode != 0:
            sys.exit("bench_unet_resnet.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    if args.dtype == "bf16":
        return report_bf16(got, args.out)
    shapes, unet_ms, cnet_ms, t_unet_ms, t_cnet_ms = [], 0.0, 0.0, 0.0, 0.0
    for (cin, cout, side, u, c), nat, pt in zip(SHAPES, got["native"]["rows"], got["pytorch"]["rows"]):
        shapes.append(dict(shape=nat["shape"], unet_count=u, controlnet_count=c, native_ms=nat["ms"], pytorch_ms=pt["ms"],
                           pytorch_contiguous_ms=pt["contiguous_ms"], pytorch_channels_last_ms=pt["channels_last_ms"],
                           pytorch_over_native=pt["ms"] / nat["ms"], pytorch_wins=bool(pt["ms"] < nat["ms"]),
                           native_blocks_ms=nat["blocks_ms"]))
        unet_ms += u * nat["ms"]
        cnet_ms += c * nat["ms"]
        t_unet_ms += u * pt["ms"]
        t_cnet_ms += c * pt["ms"]
    kinds = got["kinds"]
    per_side = []
    for side in (64, 32, 16, 8):
        rows = [r for r in kinds["conv"] if r["side"] == side]
        ms = sum(r["ms"] * r["count"] for r in rows)
        flop = sum(r["tflops"] * 1e9 * r["ms"] * r["count"] for r in rows)
        per_side.append(dict(side=side, launches_per_step=sum(r["count"] for r in rows), ms_per_step=ms, tflops=flop / ms / 1e9,
                             frac_of_mfma_peak=flop / (ms * 1e-3) / PEAK_F16_DENSE))
    gn_forms = []
    for lds in (True, False):
        rows = [r for r in kinds["groupnorm"] if r["lds_form"] == lds]
        ms = sum(r["ms"] * r["count"] for r in rows)
        moved = sum(r["bytes_moved"] * r["count"] for r in rows)
        qms = sum(r["queued_us"] * 1e-3 * r["count"] for r in rows)
        gn_forms.append(dict(lds_form=lds, launches_per_step=sum(r["count"] for r in rows), ms_per_step=ms,
                             gbytes_per_s=moved / ms / 1e6, frac_of_hbm_peak=moved / (ms * 1e-3) / HBM_PEAK,
                             queued_ms_per_step=qms, queued_gbytes_per_s=moved / qms / 1e6,
                             queued_frac_of_hbm_peak=moved / (qms * 1e-3) / HBM_PEAK))
    result = dict(bench="unet_resnet", device=got["native"]["device"], batch=N, image=512, dtype="float16", shapes=shapes,
                  unet_22_blocks=dict(native_ms=unet_ms, pytorch_ms=t_unet_ms), controlnet_10_blocks=dict(native_ms=cnet_ms, pytorch_ms=t_cnet_ms),
                  all_32_blocks=dict(native_ms=unet_ms + cnet_ms, pytorch_ms=t_unet_ms + t_cnet_ms,
                                     pytorch_over_native=(t_unet_ms + t_cnet_ms) / (unet_ms + cnet_ms)),
                  shapes_where_pytorch_wins=[s["shape"] for s in shapes if s["pytorch_wins"]],
                  groupnorm=kinds["groupnorm"], groupnorm_by_form=gn_forms, conv=kinds["conv"], conv_by_resolution=per_side,
                  conv_8x8_half_empty_tiles=[r for r in kinds["conv"] if r["side"] == 8], temb=kinds["temb"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
