#!/usr/bin/env python
"""AutoencoderKL.encode of 8 images of 512 x 512 (one key-frame batch of run_fresco.py) plus the distribution's sample, fp16,
stand-in weights and the restated module of tests/vae_encoder_model.py:

  native      VAEEncoder.encode(x).latent_dist.sample() on this package's kernels
  batched     the restated module in fp16 on PyTorch's own kernels, the batch in one call
  per_frame   the same module, one image per call
  layers      each layer form of the encoder at its 8-frame size, alone: the three vaeenc_conv_down forms, conv_in and the
              stride-1 vae_conv forms with time, algorithmic TFLOP/s and share of the 2.5 PFLOP/s dense fp16 MFMA peak; the
              GroupNorm forms and the tail (conv_out in fp32, quant_conv, the sample) with their bytes

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per mode: two warm-up calls,
then the median of five timed blocks (a host clock around several calls that end in a device synchronise).  No time is
fixed in advance: the comparison is against the PyTorch fp16 module measured in the same run.

    python tools/bench_vae_encoder.py [--out profiles/vae_encoder_bench.json]
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

N, H, W = 8, 512, 512
MODES = ("native", "batched", "per_frame", "layers")
LIMITS = dict(native=240, batched=300, per_frame=300, layers=240)  # seconds per child
# (name, input side, cin, cout, how many of them one encode runs)
DOWN_FORMS = (("down 128->128 @512->256", 512, 128, 128, 1), ("down 256->256 @256->128", 256, 256, 256, 1),
              ("down 512->512 @128->64", 128, 512, 512, 1))
# (name, side, cin, cout, ksize, residual, how many of them one encode runs)
CONV_FORMS = (
    ("3x3 conv_in 3(32)->128 @512", 512, 32, 128, 3, False, 1),
    ("3x3 128->128 @512", 512, 128, 128, 3, True, 4),
    ("3x3 128->256 @256", 256, 128, 256, 3, False, 1),
    ("1x1 128->256 @256", 256, 128, 256, 1, False, 1),
    ("3x3 256->256 @256", 256, 256, 256, 3, True, 3),
    ("3x3 256->512 @128", 128, 256, 512, 3, False, 1),
    ("1x1 256->512 @128", 128, 256, 512, 1, False, 1),
    ("3x3 512->512 @128", 128, 512, 512, 3, True, 3),
    ("3x3 512->512 @64", 64, 512, 512, 3, True, 8),
)
GN_FORMS = ((512, 128, 4), (256, 128, 1), (256, 256, 3), (128, 256, 1), (128, 512, 3), (64, 512, 10))  # (side, C, per encode)


def child(mode):
    import torch
    import fresco_amd
    from fresco_amd import _lib, ops
    import vae_encoder_model as EM
    if not torch.cuda.is_available():
        sys.exit("bench_vae_encoder.py needs a GPU")
    dev = "cuda:0"
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    if mode in ("native", "batched", "per_frame"):
        x = EM.images((N, H, W)).to(dev)
        vae = EM.build(torch.float16).to(dev)
        if mode == "native":
            enc = fresco_amd.VAEEncoder.from_vae(vae)
            res["ms"], res["blocks_ms"] = timed(lambda: enc.encode(x).latent_dist.sample(), 2)
        elif mode == "batched":
            with torch.no_grad():
                res["ms"], res["blocks_ms"] = timed(lambda: vae.encode(x).latent_dist.sample(), 2)
        else:
            with torch.no_grad():
                res["ms"], res["blocks_ms"] = timed(lambda: [vae.encode(x[i:i + 1]).latent_dist.sample() for i in range(N)], 1)
    else:
        g = torch.Generator().manual_seed(0)
        conv = lambda flop, ms: dict(ms=ms, tflops=flop / ms / 1e9, frac_of_mfma_peak=flop / (ms * 1e-3) / PEAK_F16_DENSE)  # noqa: E731
        rows = []
        for name, side, cin, cout, count in DOWN_FORMS:
            x = torch.randn(N, side, side, cin, generator=g).half().to(dev)
            wt = (torch.randn(cout, 9 * cin, generator=g) * (9 * cin) ** -0.5).half().to(dev)
            b = torch.randn(cout, generator=g).to(dev)
            ms, _ = timed(lambda: ops.vaeenc_conv_down(x, wt, b), 5)
            rows.append(dict(form=name, count=count, **conv(2.0 * N * (side // 2) ** 2 * cout * 9 * cin, ms)))
            del x, wt
        res["conv_down"] = rows
        rows = []
        for name, side, cin, cout, k, residual, count in CONV_FORMS:
            x = torch.randn(N, side, side, cin, generator=g).half().to(dev)
            wt = (torch.randn(cout, k * k * cin, generator=g) * (k * k * cin) ** -0.5).half().to(dev)
            b = torch.randn(cout, generator=g).to(dev)
            r = torch.randn(N, side, side, cout, generator=g).half().to(dev) if residual else None
            out = torch.empty(N * side * side * cout, dtype=torch.float16, device=dev)
            ms, _ = timed(lambda: ops.vae_conv(x, wt, b, N, side, side, cin, cout, k, residual=r, out=out), 5)
            # (conv_in's algorithmic flop counts its 3 real channels)
            rows.append(dict(form=name, count=count, **conv(2.0 * N * side * side * cout * k * k * (3 if cin == 32 else cin), ms)))
            del x, wt, r, out
        res["conv"] = rows
        gn = []
        for side, c, count in GN_FORMS:
            x = torch.randn(N, side, side, c, generator=g).half().to(dev)
            ga, be = torch.ones(c, device=dev), torch.zeros(c, device=dev)
            ms, _ = timed(lambda: ops.vae_groupnorm(x, ga, be, 1e-6, silu=True), 5)
            gn.append(dict(form="GroupNorm+SiLU %d @%d" % (c, side), count=count, ms=ms, gbytes_per_s=N * side * side * c * 2 * 3 / ms / 1e6))
            del x
        res["groupnorm"] = gn
        # head and tail
        img = torch.randn(N, 3, H, W, generator=g).half().to(dev)
        ms, _ = timed(lambda: ops.vaeenc_input(img), 5)
        tail = [dict(form="vaeenc_input @512", ms=ms, gbytes_per_s=N * H * W * (3 + 32) * 2 / ms / 1e6)]
        del img
        x = torch.randn(N, 64, 64, 512, generator=g).half().to(dev)
        wt = (torch.randn(8, 9 * 512, generator=g) * (9 * 512) ** -0.5).half().to(dev)
        b = torch.randn(8, generator=g).to(dev)
        ms, _ = timed(lambda: ops.vae_conv(x, wt, b, N, 64, 64, 512, 8, 3, out_kind=_lib.VAE_OUT_F32), 5)
        tail.append(dict(form="3x3 conv_out 512->8 @64 (fp32)", **conv(2.0 * N * 64 * 64 * 8 * 9 * 512, ms)))
        h = torch.randn(N, 64, 64, 8, generator=g).to(dev)
        wq, bq = torch.eye(8, device=dev), torch.zeros(8, device=dev)
        ms, _ = timed(lambda: ops.vaeenc_moments(h, wq, bq), 5)
        tail.append(dict(form="vaeenc_moments @64", ms=ms, gbytes_per_s=N * 64 * 64 * 8 * (4 + 2) / ms / 1e6))
        p = ops.vaeenc_moments(h, wq, bq)
        nz = torch.randn(N, 4, 64, 64, generator=g).half().to(dev)
        ms, _ = timed(lambda: ops.vaeenc_sample(p, nz, 0.18215), 5)
        tail.append(dict(form="vaeenc_sample @64", ms=ms, gbytes_per_s=N * 64 * 64 * (8 + 4 + 4) * 2 / ms / 1e6))
        res["tail"] = tail
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
            sys.exit("bench_vae_encoder.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    native, batched, per_frame = got["native"]["ms"], got["batched"]["ms"], got["per_frame"]["ms"]
    lay = got["layers"]
    conv_total = sum(r["ms"] * r["count"] for r in lay["conv"] + lay["conv_down"])
    result = dict(bench="vae_encode", device=got["native"]["device"], images=N, height=H, width=W, dtype="float16",
                  native_ms=native, pytorch_batched_ms=batched, pytorch_per_frame_ms=per_frame,
                  pytorch_batched_over_native=batched / native, pytorch_per_frame_over_native=per_frame / native,
                  native_faster_than_pytorch=bool(native < min(batched, per_frame)),
                  conv_down_forms=lay["conv_down"], conv_layer_forms=lay["conv"], conv_layers_sum_ms=conv_total,
                  groupnorm=lay["groupnorm"], groupnorm_sum_ms=sum(r["ms"] * r["count"] for r in lay["groupnorm"]),
                  head_and_tail=lay["tail"],
                  timed_blocks_ms={m: got[m]["blocks_ms"] for m in ("native", "batched", "per_frame")})
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
