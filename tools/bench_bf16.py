"""Layer-call timing of a bf16 pipeline against the alternatives, on cfg2's attention shapes:
L3 = up_blocks.3 (16, 4096, 320) and L2 = up_blocks.2 (16, 1024, 640), Bernoulli(0.1) occlusions, modes cf / cf_temporal /
full.  Variants, per shape and mode:
  (a) bf16 native   : bf16 module and activations, FRESCOAttnProcessor2_0.native_bf16 = True (the bf16 kernels), the default
                      two-launch K | V path (fresco_linear with x_rows + kv_pack)
  (a') bf16 fused   : the same with fuse_kv_pack_bf16 = True (K | V projected inside the key pack, fresco_attn_fwd_kvproj)
  (b) bf16 rounding : the same with native_bf16 = False (library GEMMs, q / k / v rounded to fp16, cast back)
  (c) fp16          : fp16 module and activations (the headline path, fused K | V pack included)
  (d) torch bf16    : oracle/torch_path.processor_call on bf16 cuda tensors = the reference's op sequence
One process; warm-up, then BLOCKS timed blocks; inside a block the variants ALTERNATE call by call (REPS rounds), each call
bracketed by its own pair of HIP events; per variant the median over blocks of the block means, and min - max over blocks.
On a tree without native_bf16 (the parent commit) setting the attribute is harmless and (a) = (b) = that tree's bf16 time;
likewise (a') = (a) on a tree without fuse_kv_pack_bf16.  f/a compares the fused pack with the same tree's two-launch path.
usage: python tools/bench_bf16.py [reps] [blocks]"""
import copy
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import synth  # noqa: E402
import fresco_amd  # noqa: E402
from oracle import torch_path as TP  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
BLOCKS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
DEV = "cuda"
warnings.simplefilter("ignore", RuntimeWarning)  # (b) says once per processor that it rounds


def variants(case, mode):
    def ours(dtype, native, fused_bf16=False):
        proc = fresco_amd.FRESCOAttnProcessor2_0(2, synth.controller_for(case, mode, DEV, dtype=dtype))
        proc.native_bf16 = native
        proc.fuse_kv_pack_bf16 = fused_bf16
        attn = copy.deepcopy(case["attn"]).to(DEV).to(dtype)
        x = case["hidden"].to(DEV).to(dtype)
        return lambda: proc(attn, x)

    def torch_seq():
        a = copy.deepcopy(case["attn"]).to(DEV).to(torch.bfloat16)
        x = case["hidden"].to(DEV).to(torch.bfloat16)
        kw = dict(use_cf=True, cf_mask=case["cf_mask"].to(DEV))
        if mode in ("full", "cf_temporal"):
            kw.update(fwd_map=case["fwd_map"][:, 0].to(DEV), tmask=case["tmask"][:, 0].to(DEV))
        if mode == "full":
            kw.update(ref=case["ref"].to(DEV).to(torch.bfloat16))
        return lambda: TP.processor_call(x, a.to_q.weight, a.to_k.weight, a.to_v.weight, a.to_out[0].weight,
                                         a.to_out[0].bias, case["heads"], **kw)

    return [("(a) bf16 native", ours(torch.bfloat16, True)), ("(a') bf16 fused", ours(torch.bfloat16, True, True)),
            ("(b) bf16 rounding", ours(torch.bfloat16, False)),
            ("(c) fp16", ours(torch.float16, True)), ("(d) torch bf16", torch_seq())]


def main():
    print("# %s, %s; %d blocks x %d alternating rounds; us per layer call: median of block means [min - max]"
          % (torch.cuda.get_device_name(0), fresco_amd._lib.load().fresco_version().decode(), BLOCKS, REPS))
    for layer, R in (("L3", 512), ("L2", 512)):
        case = synth.make_attention_case(8, R, layer, seed=0)
        for mode in ("cf", "cf_temporal", "full"):
            vs = variants(case, mode)
            with torch.no_grad():
                for _ in range(3):
                    for _, fn in vs:
                        fn()
                torch.cuda.synchronize()
                means = {name: [] for name, _ in vs}
                for _ in range(BLOCKS):
                    ev = {name: [] for name, _ in vs}
                    for _ in range(REPS):
                        for name, fn in vs:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fn()
                            e1.record()
                            ev[name].append((e0, e1))
                    torch.cuda.synchronize()
                    for name in ev:
                        means[name].append(sum(a.elapsed_time(b) for a, b in ev[name]) / REPS * 1e3)
            row = "%s (%d, %d, %d) %-11s" % (layer, 16, case["HW"], case["C"], mode)
            for name, _ in vs:
                m = means[name]
                row += " | %s %7.1f [%7.1f - %7.1f]" % (name, statistics.median(m), min(m), max(m))
            a, f, b, c, d = (statistics.median(means[name]) for name, _ in vs)
            print(row + " | f/a %.3f a/b %.2f a/c %.2f a/d %.2f" % (f / a, a / b, a / c, a / d), flush=True)


if __name__ == "__main__":
    main()
