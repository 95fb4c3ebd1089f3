#!/usr/bin/env python
"""AutoencoderKL.decode of 8 latents of 64 x 64 (one key-frame batch of run_fresco.py at 512 x 512), fp16, stand-in weights
and the restated module of tests/vae_model.py:

  native      VAEDecoder.decode on this package's kernels
  batched     the restated module in fp16 on PyTorch's own kernels, the batch in one call
  per_frame   the same module, one latent per call
  layers      each vae_conv layer form of the decoder at its 8-frame size, alone: time, algorithmic TFLOP/s and its share of
              the 2.5 PFLOP/s dense fp16 MFMA peak; the GroupNorm and softmax passes with their bytes

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per mode: warm-up, then the
median of five timed blocks (a host clock around several calls that end in a device synchronise).

    python tools/bench_vae.py [--out profiles/vae_bench.json]
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

N, H, W = 8, 64, 64
PEAK_F16_DENSE = 2.5e15
MODES = ("native", "batched", "per_frame", "layers")
LIMITS = dict(native=240, batched=300, per_frame=300, layers=240)  # seconds per child
# (name, H, W, cin, cout, ksize, up2, residual, how many of them one decode runs)
LAYER_FORMS = (
    ("3x3 512->512 @64", 64, 64, 512, 512, 3, False, True, 10),
    ("3x3 512->512 @128", 128, 128, 512, 512, 3, False, True, 6),
    ("3x3 up2 512->512 @128", 128, 128, 512, 512, 3, True, False, 1),
    ("3x3 up2 512->512 @256", 256, 256, 512, 512, 3, True, False, 1),
    ("3x3 512->256 @256", 256, 256, 512, 256, 3, False, False, 1),
    ("3x3 256->256 @256", 256, 256, 256, 256, 3, False, True, 5),
    ("1x1 512->256 @256", 256, 256, 512, 256, 1, False, False, 1),
    ("3x3 up2 256->256 @512", 512, 512, 256, 256, 3, True, False, 1),
    ("3x3 256->128 @512", 512, 512, 256, 128, 3, False, False, 1),
    ("3x3 128->128 @512", 512, 512, 128, 128, 3, False, True, 5),
    ("1x1 256->128 @512", 512, 512, 256, 128, 1, False, False, 1),
    ("3x3 128->3 @512 (NCHW)", 512, 512, 128, 3, 3, False, False, 1),
)


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
    from fresco_amd import _lib, ops
    import vae_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_vae.py needs a GPU")
    dev = "cuda:0"
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    z = M.latents((N, H, W)).to(dev)
    if mode in ("native", "batched", "per_frame"):
        vae = M.build(torch.float16).to(dev)
        if mode == "native":
            dec = fresco_amd.VAEDecoder.from_vae(vae)
            res["ms"], res["blocks_ms"] = timed(lambda: dec.decode(z).sample, 2)
        elif mode == "batched":
            with torch.no_grad():
                res["ms"], res["blocks_ms"] = timed(lambda: vae.decode(z).sample, 2)
        else:
            with torch.no_grad():
                res["ms"], res["blocks_ms"] = timed(lambda: [vae.decode(z[i:i + 1]).sample for i in range(N)], 1)
    else:
        rows = []
        g = torch.Generator().manual_seed(0)
        for name, h, w, cin, cout, k, up2, residual, count in LAYER_FORMS:
            hs, ws = (h // 2, w // 2) if up2 else (h, w)
            x = torch.randn(N, hs, ws, cin, generator=g).half().to(dev)
            wt = (torch.randn(cout, k * k * cin, generator=g) * (k * k * cin) ** -0.5).half().to(dev)
            b = torch.randn(cout, generator=g).to(dev)
            r = torch.randn(N, h, w, cout, generator=g).half().to(dev) if residual else None
            kind = _lib.VAE_OUT_F16_NCHW if cout == 3 else _lib.VAE_OUT_F16
            out = torch.empty(N * h * w * cout, dtype=torch.float16, device=dev)
            ms, _ = timed(lambda: ops.vae_conv(x, wt, b, N, h, w, cin, cout, k, up2=up2, residual=r, out_kind=kind, out=out), 5)
            flop = 2.0 * N * h * w * cout * k * k * cin
            rows.append(dict(form=name, count=count, ms=ms, tflops=flop / ms / 1e9, frac_of_mfma_peak=flop / (ms * 1e-3) / PEAK_F16_DENSE))
            del x, wt, r, out
        res["conv"] = rows
        # the mid block's attention at 4096 tokens
        L, C = H * W, 512
        q = torch.randn(N, L, C, generator=g).half().to(dev)
        kk = torch.randn(N, L, C, generator=g).half().to(dev)
        sc = torch.empty(N * L, L, dtype=torch.float32, device=dev)
        ms, _ = timed(lambda: ops.vae_conv(q, kk, None, N, L, 1, C, L, 1, out_kind=_lib.VAE_OUT_F32, w_img_stride=L * C, out=sc), 3)
        flop = 2.0 * N * L * L * C
        res["qk"] = dict(ms=ms, tflops=flop / ms / 1e9, frac_of_mfma_peak=flop / (ms * 1e-3) / PEAK_F16_DENSE)
        ms, _ = timed(lambda: ops.vae_softmax(sc, L, C ** -0.5), 3)
        res["softmax"] = dict(ms=ms, gbytes_per_s=N * L * L * (3 * 4 + 2) / ms / 1e6)
        del q, kk, sc
        gn = []
        for hw, c in ((64, 512), (128, 512), (256, 512), (256, 256), (512, 256), (512, 128)):
            x = torch.randn(N, hw, hw, c, generator=g).half().to(dev)
            ga, be = torch.ones(c, device=dev), torch.zeros(c, device=dev)
            ms, _ = timed(lambda: ops.vae_groupnorm(x, ga, be, 1e-6, silu=True), 5)
            gn.append(dict(form="GroupNorm+SiLU %d @%d" % (c, hw), ms=ms, gbytes_per_s=N * hw * hw * c * 2 * 3 / ms / 1e6))
            del x
        res["groupnorm"] = gn
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
            sys.exit("bench_vae.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    native, batched, per_frame = got["native"]["ms"], got["batched"]["ms"], got["per_frame"]["ms"]
    conv_total = sum(r["ms"] * r["count"] for r in got["layers"]["conv"])
    result = dict(bench="vae_decode", device=got["native"]["device"], latents=N, height=H, width=W, dtype="float16",
                  native_ms=native, pytorch_batched_ms=batched, pytorch_per_frame_ms=per_frame,
                  pytorch_batched_over_native=batched / native, pytorch_per_frame_over_native=per_frame / native,
                  native_faster_than_pytorch=bool(native < min(batched, per_frame)),
                  conv_layer_forms=got["layers"]["conv"], conv_layers_sum_ms=conv_total, attention_qk=got["layers"]["qk"],
                  softmax=got["layers"]["softmax"], groupnorm=got["layers"]["groupnorm"],
                  timed_blocks_ms={m: got[m]["blocks_ms"] for m in ("native", "batched", "per_frame")})
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
