#!/usr/bin/env python
"""FreeU at the ten sites of SD-1.5's decoder at 512 x 512, batch 16 (8 frames x 2), fp16: this package's site (two
library calls that write straight into the concat tensor, ops.freeu_site) against a torch restatement of the
reference's op sequence (src/free_lunch_utils.py:127-149 with Fourier_filter inlined; its FFT in fp32, as the reference
runs it for planes that are not a power of two -- a half-precision FFT is not probed).

Both forms scale `hidden` in place, so every timed iteration first restores it from a pristine copy; the same copy is
timed on its own and subtracted from both.  Per site and for their sum: the median of five timed blocks (device events,
warm-up first), the algorithmic bytes (hidden read twice, C/2 channels written in place, C + Cs written to the concat,
the skip read once) and the fraction of the HBM peak they amount to at the measured time.

    python tools/bench_freeu.py [--out profiles/freeu_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.fft as fft

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fresco_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X specification
BATCH = 16
# (block, side, hidden channels, skip channels)
SITES = [("up_blocks.0", 8, 1280, 1280)] * 3 + [("up_blocks.1", 16, 1280, 1280)] * 2 + [("up_blocks.1", 16, 1280, 640),
         ("up_blocks.2", 32, 1280, 640), ("up_blocks.2", 32, 640, 640), ("up_blocks.2", 32, 640, 320),
         ("up_blocks.3", 64, 640, 320)]
FACTORS = {1280: (640, 1.2, 0.9), 640: (320, 1.5, 0.2)}  # hidden channels -> (n_scaled, b, s): run_fresco.py's b1, b2


def torch_site(hidden, skip, n, b, s):
    """the reference's op sequence at one site, concat included"""
    m = hidden.mean(1).unsqueeze(1)
    B = m.shape[0]
    hi, _ = torch.max(m.view(B, -1), dim=-1, keepdim=True)
    lo, _ = torch.min(m.view(B, -1), dim=-1, keepdim=True)
    m = (m - lo.unsqueeze(2).unsqueeze(3)) / (hi - lo).unsqueeze(2).unsqueeze(3)
    hidden[:, :n] = hidden[:, :n] * ((b - 1) * m + 1)
    x = skip.to(torch.float32)
    f = fft.fftshift(fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    H, W = x.shape[-2:]
    mask = torch.ones(x.shape, device=x.device)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    f = fft.ifftshift(f * mask, dim=(-2, -1))
    y = fft.ifftn(f, dim=(-2, -1)).real.to(skip.dtype)
    return torch.cat([hidden, y], dim=1)


def timed_blocks(fn, iters, blocks=5, warmup=2):
    for _ in range(warmup):
        for _ in range(max(iters // 4, 2)):
            fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e-3 / iters)
    return statistics.median(out)


def site_bytes(C, Cs, side, esize=2):
    return esize * BATCH * side * side * (2 * C + C // 2 + (C + Cs) + Cs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the result as JSON here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_freeu.py needs a GPU")
    dev = "cuda:0"
    torch.manual_seed(0)
    rows, tot_ours, tot_torch = [], 0.0, 0.0
    for i, (block, side, C, Cs) in enumerate(SITES):
        n, b, s = FACTORS[C]
        ramp = torch.linspace(0, 1, side * side, device=dev).view(1, 1, side, side)
        pristine = (torch.randn(BATCH, C, side, side, device=dev) + ramp).half()
        skip = (0.7 + torch.randn(BATCH, Cs, side, side, device=dev)).half()
        hidden = pristine.clone()

        def restore():
            hidden.copy_(pristine)

        def ours():
            restore()
            return ops.freeu_site(hidden, skip, n, b, s)

        def ref():
            restore()
            return torch_site(hidden, skip, n, b, s)

        with torch.no_grad():
            d = (ours().float() - ref().float()).abs().max().item()
            nbytes = site_bytes(C, Cs, side)
            iters = int(min(400, max(20, 0.02 / (nbytes / 2e12 + 30e-6))))
            t_copy = timed_blocks(restore, iters)
            t_ours = timed_blocks(ours, iters) - t_copy
            t_torch = timed_blocks(ref, iters) - t_copy
        tot_ours += t_ours
        tot_torch += t_torch
        rows.append(dict(site=i, block=block, side=side, hidden_channels=C, skip_channels=Cs, iters=iters,
                         max_abs_diff_vs_torch=d, bytes=nbytes, ours_us=t_ours * 1e6, torch_us=t_torch * 1e6,
                         restore_copy_us=t_copy * 1e6, ours_hbm_fraction=nbytes / t_ours / HBM_PEAK,
                         torch_hbm_fraction=nbytes / t_torch / HBM_PEAK))
        print("site %d %s %dx%d hidden %d skip %d: ours %.1f us (%.1f%% of HBM peak), torch %.1f us (%.1f%%), "
              "%.2f MB, max |ours - torch| %.3g" % (i, block, side, side, C, Cs, t_ours * 1e6,
                                                    100 * rows[-1]["ours_hbm_fraction"], t_torch * 1e6,
                                                    100 * rows[-1]["torch_hbm_fraction"], nbytes / 1e6, d), flush=True)
    nbytes = sum(r["bytes"] for r in rows)
    result = dict(bench="freeu_sites", device=torch.cuda.get_device_name(0), batch=BATCH, dtype="float16",
                  hbm_peak_bytes_per_s=HBM_PEAK, sites=rows, total_bytes=nbytes, total_ours_us=tot_ours * 1e6,
                  total_torch_us=tot_torch * 1e6, total_ours_hbm_fraction=nbytes / tot_ours / HBM_PEAK,
                  speedup=tot_torch / tot_ours)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    if tot_ours > tot_torch:
        sys.exit("FreeU sites: this package (%.1f us) is slower than the torch sequence (%.1f us)"
                 % (tot_ours * 1e6, tot_torch * 1e6))


if __name__ == "__main__":
    main()
