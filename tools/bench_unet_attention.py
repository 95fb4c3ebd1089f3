#!/usr/bin/env python
"""The plain attention modules of one SD-1.5 denoising step at 512 x 512, batch 16 (8 frames x classifier-free guidance), fp16,
8 heads, a 77 x 768 text: the stand-in module of tests/unet_attention_model.py with its stand-in weights, self- and
cross-attention at 320 @64, 640 @32, 1280 @16 and 1280 @8.

  native    fresco_amd.UNetAttnProcessor on the module: the cross-attention with the text K | V cache (every step but the first)
            and without it
  pytorch   the module's projections as fp16 Linears around PyTorch's scaled_dot_product_attention (section 20's "attention
            ms" column)
  kernel    unet_attention alone against scaled_dot_product_attention at (16, 8, Lq, Lk, 160), with algorithmic TFLOP/s and
            the share of the 2.5 PFLOP/s dense fp16 MFMA peak

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per measurement: two warm-up
calls, then the median of five timed blocks (a host clock around several calls that end in a device synchronise): `ms`; and
`gpu_us`, device events around calls queued behind 10 ms of matrix products, so that the host is ahead and what is timed is
the GPU's work with its dispatch gaps (tools/bench_unet_resnet.py's measure).  The step total weighs each shape by how many
transformer modules run it: 17 without a FRESCO processor (10 in the UNet, 7 in the ControlNet), self + cross each, and 23
with include_fresco_cross (the cross-attention of up_blocks.2 and up_blocks.3 as well).  No ratio is fixed in advance: every
shape where PyTorch wins is listed as such.

    python tools/bench_unet_attention.py [--out profiles/unet_attention_bench.json]
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

from bench_unet_resnet import queued_us  # noqa: E402
from bench_vae import PEAK_F16_DENSE, timed  # noqa: E402

N, HEADS, TEXT, TEXT_WIDTH = 16, 8, 77, 768
MODES = ("native", "pytorch", "kernel")
LIMITS = dict(native=240, pytorch=240, kernel=240)  # seconds per child
# (channels, side, transformer modules without a FRESCO processor: UNet + ControlNet, modules whose attn2 alone joins with
# include_fresco_cross)
SHAPES = ((320, 64, 2 + 2, 3), (640, 32, 2 + 2, 3), (1280, 16, 5 + 2, 0), (1280, 8, 1 + 1, 0))
assert sum(s[2] for s in SHAPES) == 17 and sum(s[2] + s[3] for s in SHAPES) == 23
KERNEL_SHAPES = ((256, 256), (64, 64), (256, 77), (64, 77))   # (Lq, Lk) at batch 16, 8 heads, head dim 160


def _name(C, side):
    return "%d @%d" % (C, side)


def _iters(side):
    return 4 if side >= 32 else 10


class SdpaProcessor:
    """fp16 Linears around PyTorch's scaled_dot_product_attention"""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        import torch.nn.functional as F
        e = hidden_states if encoder_hidden_states is None else encoder_hidden_states
        n, L, D = hidden_states.shape
        split = lambda t: t.view(n, -1, attn.heads, D // attn.heads).transpose(1, 2)  # noqa: E731
        o = F.scaled_dot_product_attention(split(attn.to_q(hidden_states)), split(attn.to_k(e)), split(attn.to_v(e)))
        return attn.to_out[1](attn.to_out[0](o.transpose(1, 2).reshape(n, L, D)))


def child(mode):
    import torch
    import torch.nn.functional as F
    import fresco_amd
    from fresco_amd import ops
    import unet_attention_model as M
    if not torch.cuda.is_available():
        sys.exit("bench_unet_attention.py needs a GPU")
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    if mode in ("native", "pytorch"):
        rows = []
        text = torch.randn(N, TEXT, TEXT_WIDTH, generator=g).half().to(dev)
        for C, side, _, _ in SHAPES:
            x = torch.randn(N, side * side, C, generator=g).half().to(dev)
            proc = fresco_amd.UNetAttnProcessor() if mode == "native" else SdpaProcessor()
            a1 = M.build(C, HEADS, None, torch.float16, proc).to(dev)
            a2 = M.build(C, HEADS, TEXT_WIDTH, torch.float16, proc).to(dev)
            row = dict(shape=_name(C, side))
            it = _iters(side)
            with torch.no_grad():
                row["self_ms"], _ = timed(lambda: a1(x), it)
                row["self_gpu_us"] = queued_us(lambda: a1(x), 20)
                row["cross_ms"], _ = timed(lambda: a2(x, encoder_hidden_states=text), it)
                row["cross_gpu_us"] = queued_us(lambda: a2(x, encoder_hidden_states=text), 20)
                if mode == "native":
                    a2.set_processor(fresco_amd.UNetAttnProcessor(cache_text_kv=False))
                    row["cross_uncached_ms"], _ = timed(lambda: a2(x, encoder_hidden_states=text), it)
                    row["cross_uncached_gpu_us"] = queued_us(lambda: a2(x, encoder_hidden_states=text), 20)
            rows.append(row)
            del a1, a2, x
        res["rows"] = rows
    else:
        rows = []
        scale = 160 ** -0.5
        for Lq, Lk in KERNEL_SHAPES:
            C = HEADS * 160
            q = torch.randn(N, Lq, C, generator=g).half().to(dev)
            k = torch.randn(N, Lk, C, generator=g).half().to(dev)
            v = torch.randn(N, Lk, C, generator=g).half().to(dev)
            out = torch.empty(N, Lq, C, dtype=torch.float16, device=dev)
            q4, k4, v4 = (t.view(N, -1, HEADS, 160).transpose(1, 2) for t in (q, k, v))
            flop = 4.0 * N * HEADS * Lq * Lk * 160
            ms, _ = timed(lambda: ops.unet_attention(q, k, v, HEADS, scale, out=out), 10)
            us = queued_us(lambda: ops.unet_attention(q, k, v, HEADS, scale, out=out), 40)
            sms, _ = timed(lambda: F.scaled_dot_product_attention(q4, k4, v4), 10)
            sus = queued_us(lambda: F.scaled_dot_product_attention(q4, k4, v4), 40)
            rows.append(dict(shape="(16, 8, %d, %d)" % (Lq, Lk), ms=ms, gpu_us=us, tflops=flop / us / 1e6,
                             frac_of_mfma_peak=flop / (us * 1e-6) / PEAK_F16_DENSE, sdpa_ms=sms, sdpa_gpu_us=sus,
                             sdpa_over_native_gpu=sus / us, pytorch_wins=bool(sus < us)))
        res["rows"] = rows
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
            sys.exit("bench_unet_attention.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    shapes = []
    tot = {k: 0.0 for k in ("native_17", "pytorch_17", "native_23", "pytorch_23", "native_17_uncached")}
    for (C, side, count, extra), nat, pt in zip(SHAPES, got["native"]["rows"], got["pytorch"]["rows"]):
        row = dict(shape=nat["shape"], modules=count, fresco_cross_modules=extra)
        for kind in ("self", "cross"):
            row[kind] = dict(native_ms=nat[kind + "_ms"], native_gpu_us=nat[kind + "_gpu_us"], pytorch_ms=pt[kind + "_ms"],
                             pytorch_gpu_us=pt[kind + "_gpu_us"], pytorch_over_native=pt[kind + "_ms"] / nat[kind + "_ms"],
                             pytorch_over_native_gpu=pt[kind + "_gpu_us"] / nat[kind + "_gpu_us"],
                             pytorch_wins=bool(pt[kind + "_ms"] < nat[kind + "_ms"]))
        row["cross"].update(native_uncached_ms=nat["cross_uncached_ms"], native_uncached_gpu_us=nat["cross_uncached_gpu_us"])
        shapes.append(row)
        both_n, both_p = nat["self_ms"] + nat["cross_ms"], pt["self_ms"] + pt["cross_ms"]
        tot["native_17"] += count * both_n
        tot["pytorch_17"] += count * both_p
        tot["native_17_uncached"] += count * (nat["self_ms"] + nat["cross_uncached_ms"])
        tot["native_23"] += count * both_n + extra * nat["cross_ms"]
        tot["pytorch_23"] += count * both_p + extra * pt["cross_ms"]
    wins = ["%s %s" % (s["shape"], kind) for s in shapes for kind in ("self", "cross") if s[kind]["pytorch_wins"]]
    result = dict(bench="unet_attention", device=got["native"]["device"], batch=N, image=512, dtype="float16", heads=HEADS,
                  text=[TEXT, TEXT_WIDTH], shapes=shapes,
                  step_17_modules=dict(native_ms=tot["native_17"], native_without_text_cache_ms=tot["native_17_uncached"],
                                       pytorch_ms=tot["pytorch_17"], pytorch_over_native=tot["pytorch_17"] / tot["native_17"]),
                  step_23_modules=dict(native_ms=tot["native_23"], pytorch_ms=tot["pytorch_23"],
                                       pytorch_over_native=tot["pytorch_23"] / tot["native_23"]),
                  shapes_where_pytorch_wins=wins, kernel=got["kernel"]["rows"],
                  kernel_shapes_where_pytorch_wins=[r["shape"] for r in got["kernel"]["rows"] if r["pytorch_wins"]])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
