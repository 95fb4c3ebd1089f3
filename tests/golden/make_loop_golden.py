"""Golden record of the denoising loop from the UNMODIFIED reference inference() (src/pipe_FRESCO.py:80-234) on the CPU in
float64, on the stand-ins of tests/loop_model.py -> tests/golden/loop_golden.npz.  Build container only.

Per case of loop_model.CASES: the latents every UNet call saw (`_steps`: frames of the first model-input half) and the
returned latents (`_final`), every record_latents entry after the call (`_rec`; `_rec_in` what a propagation case was handed),
the trace of controller / ControlNet / UNet calls with their timesteps and conditioning scales and the progress bar's
(`_trace`, JSON), every torch.randn draw in order (`_draws`), the largest magnitude of steps and final (`_peak`), and
`_noise`: the largest distance of loop_model.inference_model with every operation rounded to fp16 (the stand-in networks
computing in fp16 tensors) from that float64 record, over the peak.  Asserted: the float64 restatement reproduces the reference to 1e-12 of the peak (1e-5 with smoothing, where
the reference's warp computes in fp32), and the noise is positive.

Also: tensor2numpy's uint8 result for all 65536 fp16 bit patterns (`u8_table`, `u8_nan` marks the NaN patterns, whose cast is
undefined) and the inspect dump of the reference inference()'s signature (`sig_names`, `sig_defaults`).
"""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_harness  # noqa: E402
import loop_model as M  # noqa: E402


def run(fn, name, rec_in, randn, **extra):
    """one case on fresh stand-ins: (pipe, steps, final, records)"""
    pipe = M.Pipe("cpu", torch.float64)
    (imgs, embeds, edges), kw = M.make_inputs(name, "cpu", torch.float64)
    records = [r.clone() for r in rec_in] if rec_in is not None else []
    if extra.get("q") is M.round_half:  # an fp16 run starts from fp16 inputs
        imgs, embeds, edges = M.round_half(imgs), M.round_half(embeds), M.round_half(edges)
        records = [M.round_half(r) for r in records]
    real = torch.randn
    torch.randn = randn
    try:
        final = fn(pipe, pipe.controlnet, pipe.frescoProc, imgs, embeds, edges, pipe.scheduler.timesteps,
                   record_latents=records, **kw, **extra)
    finally:
        torch.randn = real
    B = M.CASES[name][0]
    steps = torch.stack([x[:B] for x in pipe.unet.inputs])
    return pipe, steps, final, records


if __name__ == "__main__":
    _, fu, _, ut = _ref_harness.load_reference()
    os.chdir(_ref_harness.REF_ROOT)
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))  # only used by the debug visualiser
    import src.pipe_FRESCO as pf

    out = {}
    recs = {}
    for name, (B, ckw) in M.CASES.items():
        rec_in = None
        if ckw.get("propagation_mode"):
            pred = M.PREDECESSOR[name]
            if pred is None:  # an unrecorded first batch of B frames
                M.CASES["_pred"] = (B, dict(num_warmup_steps=ckw["num_warmup_steps"], seed=12))
                rec_in = run(pf.inference, "_pred", None, torch.randn)[3]
                del M.CASES["_pred"]
            else:
                rec_in = recs[pred]
        draws = []
        real_randn = torch.randn

        def recording(*a, **k):
            z = real_randn(*a, **k)
            draws.append(z.clone())
            return z

        pipe, steps, final, records = run(pf.inference, name, rec_in, recording)
        recs[name] = records
        trace = M.finish_trace(pipe.trace) + pipe.progress
        peak = float(max(steps.abs().max(), final.abs().max()))
        smooth = "flows" in M.make_inputs(name, "cpu", torch.float64)[1]

        # the restatement in float64 must be the reference; in fp16 it gives the noise the GPU bar rests on
        p2, s2, f2, r2 = run(M.inference_model, name, rec_in, M.replay_randn(draws), warp_tensor=fu.warp_tensor)
        same = float(max((s2 - steps).abs().max(), (f2 - final).abs().max())) / peak
        assert same <= (1e-5 if smooth else 1e-12), (name, same)
        assert M.finish_trace(p2.trace) + p2.progress == trace, name
        assert all(torch.equal(a, b) for a, b in zip(r2, records)) or smooth, name
        p3, s3, f3, r3 = run(M.inference_model, name, rec_in, M.replay_randn(draws), warp_tensor=fu.warp_tensor,
                             q=M.round_half, net_dtype=torch.float16)
        noise = float(max((s3 - steps).abs().max(), (f3 - final).abs().max())) / peak
        assert noise > 0, name

        out[name + "_steps"] = steps.numpy()
        out[name + "_final"] = final.numpy()
        out[name + "_rec"] = torch.stack(records).numpy()
        if rec_in is not None:
            out[name + "_rec_in"] = torch.stack(rec_in).numpy()
        out[name + "_trace"] = np.array(json.dumps(trace))
        out[name + "_draws"] = torch.stack(draws).numpy()
        out[name + "_peak"] = np.array([peak], np.float64)
        out[name + "_noise"] = np.array([noise], np.float64)
        print("%-8s %d UNet calls, %d draws, peak %.3f, restatement %.1e, fp16 noise %.2e" % (name, len(steps), len(draws), peak,
                                                                                         same, noise))

    pat = M.all_half_patterns()
    with np.errstate(invalid="ignore"):
        table = ut.tensor2numpy(pat).reshape(-1)
    out["u8_table"] = table
    out["u8_nan"] = torch.isnan(pat).reshape(-1).numpy()
    assert np.array_equal(M.image_to_frames_model(pat).reshape(-1)[~out["u8_nan"]], table[~out["u8_nan"]])

    sig = inspect.signature(pf.inference)
    out["sig_names"] = np.array(list(sig.parameters))
    out["sig_defaults"] = np.array(["<none>" if p.default is inspect.Parameter.empty else repr(p.default)
                                    for p in sig.parameters.values()])
    path = os.path.join(HERE, M.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
