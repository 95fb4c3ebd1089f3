#!/usr/bin/env python
"""The 23 Transformer2DModel shapes of one SD-1.5 denoising step at 512 x 512 (16 in the UNet, 7 in the ControlNet), batch 16
(8 frames x classifier-free guidance), fp16, 8 heads, a 77 x 768 text, stand-in weights and the restated module of
tests/unet_transformer_model.py.  The SAME attention runs in both columns -- the module's projections as fp16 Linears around
PyTorch's scaled_dot_product_attention -- so the difference is the shell this package builds:

  native    fresco_amd.UNetTransformer per distinct shape, channels_last in and out
  pytorch   the restated module in fp16 on PyTorch's own kernels, contiguous and channels_last; the faster one counts
  kinds     unet_geglu alone against vae_conv into a (rows, 2 inner) buffer + torch's chunk / gelu / mul, with algorithmic
            TFLOP/s and the share of the 2.5 PFLOP/s dense fp16 MFMA peak; unet_layernorm alone, plain and with the residual
            and sum_out, against the bytes it must move and the 8 TB/s HBM specification -- from the call time, and
            (`queued_us`) from device events around calls queued behind 10 ms of matrix products, so that the host is
            ahead and what is timed is the GPU's work with its dispatch gaps (tools/bench_unet_resnet.py's measure)

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per measurement: two warm-up
calls, then the median of five timed blocks (a host clock around several calls that end in a device synchronise).  No ratio
is fixed in advance: every shape where PyTorch wins is listed as such.

    python tools/bench_unet_transformer.py [--out profiles/unet_transformer_bench.json]
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
HBM_PEAK = 8.0e12  # bytes / s, MI355X specification
MODES = ("native", "pytorch", "kinds")
LIMITS = dict(native=240, pytorch=300, kinds=240)  # seconds per child
# (channels, side, how many the UNet runs, how many the ControlNet runs)
SHAPES = ((320, 64, 5, 2), (640, 32, 5, 2), (1280, 16, 5, 2), (1280, 8, 1, 1))
assert sum(s[2] for s in SHAPES) == 16 and sum(s[3] for s in SHAPES) == 7


def _name(C, side):
    return "%d @%d" % (C, side)


def _iters(side):
    return 3 if side >= 32 else 6


def _sdpa_module(C, dev):
    """the restated module in fp16 with its attention modules' arithmetic replaced by fp16 Linears + PyTorch's SDPA"""
    import torch
    import torch.nn.functional as F
    import unet_transformer_model as M

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **kwargs):
        e = hidden_states if encoder_hidden_states is None else encoder_hidden_states
        n, L, D = hidden_states.shape
        split = lambda t: t.view(n, -1, self.heads, D // self.heads).transpose(1, 2)  # noqa: E731
        o = F.scaled_dot_product_attention(split(self.to_q(hidden_states)), split(self.to_k(e)), split(self.to_v(e)))
        return self.to_out[0](o.transpose(1, 2).reshape(n, L, D))
    mod = M.build(C, HEADS, TEXT_WIDTH, torch.float16).to(dev)
    for blk in mod.transformer_blocks:
        for a in (blk.attn1, blk.attn2):
            a.forward = forward.__get__(a)
    return mod


def child(mode):
    import torch
    import fresco_amd
    from fresco_amd import ops
    from fresco_amd.unet_transformer import pack_geglu_weight
    if not torch.cuda.is_available():
        sys.exit("bench_unet_transformer.py needs a GPU")
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    if mode in ("native", "pytorch"):
        rows = []
        for C, side, _, _ in SHAPES:
            mod = _sdpa_module(C, dev)
            x = torch.randn(N, C, side, side, generator=g).half().to(dev)
            text = torch.randn(N, TEXT, TEXT_WIDTH, generator=g).half().to(dev)
            x_cl = x.contiguous(memory_format=torch.channels_last)
            row = dict(shape=_name(C, side))
            with torch.no_grad():
                if mode == "native":
                    tf = fresco_amd.UNetTransformer.from_module(mod)
                    row["ms"], row["blocks_ms"] = timed(lambda: tf(x_cl, text, return_dict=False), _iters(side))
                    blk = mod.transformer_blocks[0]
                    y = torch.randn(N, side * side, C, generator=g).half().to(dev)
                    row["attention_ms"], _ = timed(lambda: (blk.attn1(y), blk.attn2(y, encoder_hidden_states=text)), _iters(side))
                else:
                    row["contiguous_ms"], _ = timed(lambda: mod(x, text, return_dict=False), _iters(side))
                    mod_cl = mod.to(memory_format=torch.channels_last)
                    row["channels_last_ms"], _ = timed(lambda: mod_cl(x_cl, text, return_dict=False), _iters(side))
                    row["ms"] = min(row["contiguous_ms"], row["channels_last_ms"])
            rows.append(row)
            del mod, x, x_cl
        res["rows"] = rows
    else:
        geglu, ln = [], []
        for C, side, u, c in SHAPES:
            M_, inner = N * side * side, 4 * C
            x = torch.randn(M_, C, generator=g).half().to(dev)
            w = (torch.randn(2 * inner, C, generator=g) * C ** -0.5).half()
            b = torch.randn(2 * inner, generator=g) * 0.1
            pw, pb = (t.to(dev) for t in pack_geglu_weight(w, b))
            w, b = w.to(dev), b.to(dev)
            out = torch.empty(M_, inner, dtype=torch.float16, device=dev)
            buf = torch.empty(M_ * 2 * inner, dtype=torch.float16, device=dev)

            def unfused():
                p = ops.vae_conv(x, w, b, 1, M_, 1, C, 2 * inner, 1, out=buf).view(M_, 2 * inner)
                value, gate = p.chunk(2, dim=-1)
                return value * torch.nn.functional.gelu(gate)
            ms, _ = timed(lambda: ops.unet_geglu(x, pw, pb, out=out), _iters(side))
            us = queued_us(lambda: ops.unet_geglu(x, pw, pb, out=out), 20)
            cus = queued_us(lambda: ops.vae_conv(x, w, b, 1, M_, 1, C, 2 * inner, 1, out=buf), 20)
            ums, _ = timed(unfused, _iters(side))
            cms, _ = timed(lambda: ops.vae_conv(x, w, b, 1, M_, 1, C, 2 * inner, 1, out=buf), _iters(side))
            flop = 2.0 * M_ * C * 2 * inner
            geglu.append(dict(form="GEGLU %d -> %d, %d rows" % (C, inner, M_), shape=_name(C, side), count=u + c, ms=ms,
                              tflops=flop / ms / 1e9, frac_of_mfma_peak=flop / (ms * 1e-3) / PEAK_F16_DENSE, unfused_ms=ums,
                              unfused_vae_conv_ms=cms, unfused_over_fused=ums / ms, projection_bytes_not_written=M_ * 2 * inner * 2, queued_us=us,
                              queued_frac_of_mfma_peak=flop / (us * 1e-6) / PEAK_F16_DENSE, unfused_vae_conv_queued_us=cus))
            del out, buf, w, pw
            ga, be = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            r = torch.randn(M_, C, generator=g).half().to(dev)
            for with_r in (False, True):
                if with_r:
                    fn = lambda: ops.unet_layernorm(x, ga, be, 1e-5, residual=r, want_sum=True)  # noqa: E731
                else:
                    fn = lambda: ops.unet_layernorm(x, ga, be, 1e-5)  # noqa: E731
                ms, _ = timed(fn, 6)
                us = queued_us(fn)
                must = M_ * C * 2 * (4 if with_r else 2)
                ln.append(dict(form="LayerNorm %d, %d rows%s" % (C, M_, " + r + sum_out" if with_r else ""), shape=_name(C, side),
                               count=(u + c) * (2 if with_r else 1), ms=ms, bytes_moved=must, gbytes_per_s=must / ms / 1e6,
                               frac_of_hbm_peak=must / (ms * 1e-3) / HBM_PEAK, queued_us=us, queued_gbytes_per_s=must / us / 1e3,
                               queued_frac_of_hbm_peak=must / (us * 1e-6) / HBM_PEAK))
            del x, r
        res["geglu"], res["layernorm"] = geglu, ln
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
            sys.exit("bench_unet_transformer.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    shapes, unet_ms, cnet_ms, t_unet_ms, t_cnet_ms = [], 0.0, 0.0, 0.0, 0.0
    for (C, side, u, c), nat, pt in zip(SHAPES, got["native"]["rows"], got["pytorch"]["rows"]):
        shapes.append(dict(shape=nat["shape"], unet_count=u, controlnet_count=c, native_ms=nat["ms"], pytorch_ms=pt["ms"],
                           pytorch_contiguous_ms=pt["contiguous_ms"], pytorch_channels_last_ms=pt["channels_last_ms"],
                           pytorch_over_native=pt["ms"] / nat["ms"], pytorch_wins=bool(pt["ms"] < nat["ms"]),
                           attention_ms=nat["attention_ms"], native_shell_ms=nat["ms"] - nat["attention_ms"],
                           pytorch_shell_ms=pt["ms"] - nat["attention_ms"], native_blocks_ms=nat["blocks_ms"]))
        unet_ms += u * nat["ms"]
        cnet_ms += c * nat["ms"]
        t_unet_ms += u * pt["ms"]
        t_cnet_ms += c * pt["ms"]
    kinds = got["kinds"]
    result = dict(bench="unet_transformer", device=got["native"]["device"], batch=N, image=512, dtype="float16", heads=HEADS,
                  text=[TEXT, TEXT_WIDTH], shapes=shapes,
                  unet_16_modules=dict(native_ms=unet_ms, pytorch_ms=t_unet_ms),
                  controlnet_7_modules=dict(native_ms=cnet_ms, pytorch_ms=t_cnet_ms),
                  all_23_modules=dict(native_ms=unet_ms + cnet_ms, pytorch_ms=t_unet_ms + t_cnet_ms,
                                      pytorch_over_native=(t_unet_ms + t_cnet_ms) / (unet_ms + cnet_ms)),
                  shapes_where_pytorch_wins=[s["shape"] for s in shapes if s["pytorch_wins"]],
                  geglu=kinds["geglu"], layernorm=kinds["layernorm"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
