#!/usr/bin/env python
"""The denoising loop's glue (fresco_amd/loop.py, csrc/loop.hip) beside the route before it, fp16, on one GPU.

  (a) glue      one plain, guided step's glue in propagation mode at B = 8, latents 8 x 4 x 64 x 64, given the UNet's output.
                native: torch.randn + one loop_update (next latents, restored rows, record, both model-input halves).
                before: torch.cat([latents] * 2), the guidance ops (chunk, sub, mul, add), fresco_amd.step (two kernels and
                its randn) and the restore / record ops (index, clone, assign) -- what the reference's loop runs between
                two UNet calls once patch_reference has put fresco_amd.step in.
  (b) frames    fresco_amd.tensor2numpy on 8 x 3 x 512 x 512 and 8 x 3 x 512 x 896 fp16, beside the reference's expression
                (src/utils.py:17-21): clamp on the GPU, a download of fp16, `* 255` and `.round()` in numpy's half arithmetic.
  (c) loop      fresco_amd.inference beside tests/loop_model.py's restated inference() with fresco_amd.step, 20 steps at
                B = 8, with null networks (they return one preallocated tensor): wall time per step.

The two sides alternate inside one process; a figure is the median of five blocks and comes with the smallest and largest
block (the spread).  `host_us` is the time the host needs to enqueue (the clock stops before the synchronise), `wall_us`
includes the synchronise.  Launches are counted, and the kernels' summed time taken, in a pass of their own under
torch.profiler after the timing; with `rocprofv3` on the PATH the summed kernel time also comes from a
`rocprofv3 --kernel-trace --stats` run of each side alone (`--glue SIDE` is that run's workload).  No ratio is fixed in
advance: where the native side loses, the result says so.

    python tools/bench_loop.py [--out profiles/loop_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, SIDE, STEPS, GUIDANCE, T = 8, 64, 20, 7.5, 601
GLUE_ITERS = 200


def alternate(sides, iters, blocks=5, warmup=3):
    """sides: name -> fn.  Per side: median / min / max over the blocks of host and wall microseconds per call."""
    import torch
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: dict(host=[], wall=[]) for k in sides}
    for _ in range(blocks):
        for name, fn in sides.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            got[name]["host"].append((t1 - t0) / iters * 1e6)
            got[name]["wall"].append((t2 - t0) / iters * 1e6)
    return {name: {k + "_us": dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in g.items()}
            for name, g in got.items()}


def profiled(fn):
    """(kernel launches, their summed microseconds) of one call of fn under torch.profiler"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "trace.json")
        prof.export_chrome_trace(path)
        kernels = [e for e in json.load(open(path))["traceEvents"] if e.get("cat") == "kernel"]
    return len(kernels), sum(e.get("dur", 0) for e in kernels)


def verdict(native, before, key="wall_us"):
    """slower only beyond the spread of the blocks: the native median above the other side's largest block"""
    n, b = native[key], before[key]
    return dict(before_over_native=b["median"] / n["median"], native_slower_beyond_spread=bool(n["median"] > b["max"]),
                native_faster_beyond_spread=bool(n["max"] < b["median"]))


def glue_sides():
    import torch
    import fresco_amd
    from fresco_amd import loop
    import loop_model as M
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    mk = lambda *s: torch.randn(*s, generator=g).half().to(dev)  # noqa: E731
    pipe = types.SimpleNamespace(scheduler=M.Scheduler())
    pipe.scheduler.previous_timestep = lambda t: t - 50
    co = loop._coefficients(pipe.scheduler, [T])[0]
    gen = torch.Generator(device=dev).manual_seed(1)
    state = dict(lat=mk(B, 4, SIDE, SIDE), rec=mk(2, 4, SIDE, SIDE), eps=mk(2 * B, 4, SIDE, SIDE))
    model_input = torch.empty(2 * B, 4, SIDE, SIDE, dtype=torch.float16, device=dev)
    n = state["lat"].numel()

    def native():
        lat = state["lat"]
        noise = torch.randn(lat.shape, generator=gen, device=dev, dtype=lat.dtype)
        nxt, record = torch.empty_like(lat), torch.empty_like(state["rec"])
        loop._update(lat, state["eps"], None, noise, state["rec"], nxt, model_input, record, n, 2, GUIDANCE, co)
        return nxt, record

    def before():
        uncond, text = state["eps"].chunk(2)
        noise_pred = uncond + GUIDANCE * (text - uncond)
        lat = fresco_amd.step(pipe, noise_pred, T, state["lat"], gen)[0]
        lat[0:2] = state["rec"].detach().clone()
        record = lat[[0, len(lat) - 1]].detach().clone()
        return lat, record, torch.cat([lat] * 2)

    return dict(native=native, before=before)


def rocprof_kernel_us(side):
    """summed kernel microseconds per iteration of `--glue side` under rocprofv3 --kernel-trace --stats, or None"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                            os.path.abspath(__file__), "--glue", side], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=300, text=True)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not stats:
            sys.exit("bench_loop.py: the rocprofv3 run of the %s side ended with status %d; nothing further is started\n%s"
                     % (side, p.returncode, p.stdout[-2000:]))
        rows = list(csv.DictReader(open(stats[0])))
    return dict(kernel_us=sum(int(r["TotalDurationNs"]) for r in rows) / 1e3 / (GLUE_ITERS + 3),
                launches=sum(int(r["Calls"]) for r in rows) / (GLUE_ITERS + 3))


def bench_frames():
    import torch
    import fresco_amd
    import loop_model as M
    out = []
    for H, W in ((512, 512), (512, 896)):
        img = (torch.rand(8, 3, H, W, generator=torch.Generator().manual_seed(H + W)) * 2.4 - 1.2).half().to("cuda:0")
        assert (fresco_amd.tensor2numpy(img) == M.image_to_frames_model(img)).all()
        sides = dict(native=lambda: fresco_amd.tensor2numpy(img), before=lambda: M.image_to_frames_model(img))
        r = alternate(sides, 3, warmup=1)
        out.append(dict(shape=[8, 3, H, W], native_ms=r["native"]["wall_us"]["median"] / 1e3,
                        before_ms=r["before"]["wall_us"]["median"] / 1e3, blocks=r, **verdict(r["native"], r["before"])))
    return out


def bench_loop():
    import torch
    import fresco_amd
    import loop_model as M
    dev = "cuda:0"
    pipe = M.Pipe(dev, torch.float16)
    pipe.scheduler.timesteps = torch.arange(951, 0, -50)
    pipe.scheduler.previous_timestep = lambda t: t - 50
    eps = torch.randn(2 * B, 4, SIDE, SIDE, generator=torch.Generator().manual_seed(2)).half().to(dev) * 0.1
    res = ([torch.zeros(1, dtype=torch.float16, device=dev)] * 2, torch.zeros(1, dtype=torch.float16, device=dev))
    pipe.unet.forward = lambda *a, **k: (eps,)
    null_controlnet = lambda *a, **k: res  # noqa: E731
    imgs = torch.zeros(B, 3, 8 * SIDE, 8 * SIDE, dtype=torch.float16, device=dev)
    embeds = torch.zeros(2 * B, 77, 768, dtype=torch.float16, device=dev)
    edges = torch.zeros(2 * B, 3, 8 * SIDE, 8 * SIDE, dtype=torch.float16, device=dev)
    timesteps = pipe.scheduler.timesteps.to(dev)
    kw = dict(cond_scale=[0.7] * STEPS, num_inference_steps=STEPS, num_warmup_steps=0, guidance_scale=GUIDANCE, seed=0)
    recs = []
    fresco_amd.inference(pipe, null_controlnet, pipe.frescoProc, imgs, embeds, edges, timesteps, record_latents=recs, **kw)

    def side(fn, extra):
        def call():
            pipe.trace.clear()
            pipe.progress.clear()
            fn(pipe, null_controlnet, pipe.frescoProc, imgs, embeds, edges, timesteps,
               record_latents=[r.clone() for r in recs], propagation_mode=True, **kw, **extra)
        return call

    sides = dict(native=side(fresco_amd.inference, {}), before=side(M.inference_model, dict(step_fn=fresco_amd.step)))
    r = alternate(sides, 2, warmup=1)
    per_step = {k: v["wall_us"]["median"] / STEPS for k, v in r.items()}
    return dict(steps=STEPS, frames=B, native_us_per_step=per_step["native"], before_us_per_step=per_step["before"], blocks=r,
                note="both sides include the SDEdit start (one stand-in VAE encode and add_noise) spread over the steps",
                **verdict(r["native"], r["before"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the result as JSON here as well")
    ap.add_argument("--glue", choices=("native", "before"), default=None, help="run one side of (a) alone and exit")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_loop.py needs a GPU")
    if args.glue:
        fn = glue_sides()[args.glue]
        for _ in range(GLUE_ITERS + 3):
            fn()
        torch.cuda.synchronize()
        return
    sides = glue_sides()
    glue = alternate(sides, 200)
    for name, fn in sides.items():
        launches, us = profiled(fn)
        glue[name].update(launches=launches, profiler_kernel_us=us, rocprofv3="not measured")
    result = dict(bench="loop", device=torch.cuda.get_device_name(0), dtype="float16",
                  glue=dict(frames=B, latents=[B, 4, SIDE, SIDE], sides=glue, host=verdict(glue["native"], glue["before"], "host_us"),
                            wall=verdict(glue["native"], glue["before"])),
                  frames=bench_frames(), loop=bench_loop())

    def write():
        print(json.dumps(result), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    write()  # (before the rocprofv3 children: a failure there leaves the timings written)
    if shutil.which("rocprofv3") is not None:
        for name in sides:
            glue[name]["rocprofv3"] = rocprof_kernel_us(name)
        write()

if __name__ == "__main__":
    main()
