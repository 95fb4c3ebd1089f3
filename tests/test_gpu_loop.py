"""fresco_amd.inference and fresco_amd.tensor2numpy on the stand-ins of tests/loop_model.py, against the float64 record of the
unmodified reference's inference() (tests/golden/loop_golden.npz), with the recorded draws replayed through torch.randn.

The bar is the project's drop-in bar: the latents every UNet call saw and the returned latents within 4 x noise x peak of
the record, `noise` being the recorded distance of the reference's arithmetic in fp16 from its float64 run.  Beside each
ratio the test prints the ratio of that restatement run with torch ops in fp16 on the same GPU."""
import json
import os

import numpy as np
import pytest
import torch

import loop_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lg():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", M.GOLDEN_FILE)))


def run(lg, name, dtype, monkeypatch, fn=None, on_call=None, setup=None, replay=True, **extra):
    """one case on fresh stand-ins on the GPU: (pipe, steps, final, records, records handed in)"""
    import fresco_amd
    native = fn is None
    pipe = M.Pipe(DEV, dtype)
    pipe.unet.on_call = on_call
    if setup is not None:
        setup(pipe)
    (imgs, embeds, edges), kw = M.make_inputs(name, DEV, dtype)
    rec_in = [torch.from_numpy(r).to(DEV, dtype) for r in lg[name + "_rec_in"]] if name + "_rec_in" in lg else None
    records = [r.clone() for r in rec_in] if rec_in is not None else []
    if replay:  # uploaded before the run: a replayed draw then is no copy at all
        monkeypatch.setattr(torch, "randn", M.replay_randn([torch.from_numpy(z).to(DEV, dtype) for z in lg[name + "_draws"]],
                                                           DEV))
    timesteps = pipe.scheduler.timesteps.to(DEV) if native else pipe.scheduler.timesteps
    final = (fresco_amd.inference if native else fn)(pipe, pipe.controlnet, pipe.frescoProc, imgs, embeds, edges, timesteps,
                                                     record_latents=records, **kw, **extra)
    torch.cuda.synchronize()
    steps = torch.stack([x[:M.CASES[name][0]] for x in pipe.unet.inputs])
    return pipe, steps, final, records, rec_in


def distance(lg, name, steps, final):
    d = max(float((steps.double().cpu() - torch.from_numpy(lg[name + "_steps"])).abs().max()),
            float((final.double().cpu() - torch.from_numpy(lg[name + "_final"])).abs().max()))
    return d / (float(lg[name + "_noise"][0]) * float(lg[name + "_peak"][0]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_inference_against_the_reference(lg, name, dtype, monkeypatch):
    import fresco_amd
    B, ckw = M.CASES[name]
    noise = float(lg[name + "_noise"][0])
    assert noise > 0
    pipe, steps, final, records, rec_in = run(lg, name, dtype, monkeypatch)
    ratio = distance(lg, name, steps, final)
    line = "%s %s: %.3f of noise x peak (noise %.2e, peak %.3g)" % (name, dtype, ratio, noise, float(lg[name + "_peak"][0]))
    if dtype == torch.float16:
        _, s2, f2, _, _ = run(lg, name, dtype, monkeypatch, fn=M.inference_model, warp_tensor=fresco_amd.warp_tensor)
        line += "; the restatement in fp16 torch ops on this GPU: %.3f" % distance(lg, name, s2, f2)
    print(line)
    assert final.dtype == dtype and final.shape == (B, 4, M.SIDE // 8, M.SIDE // 8)
    assert ratio <= 4.0, line

    # what the stand-ins and the controller were called with, in order, and the progress bar
    assert M.finish_trace(pipe.trace) + pipe.progress == json.loads(str(lg[name + "_trace"]))
    assert all(ev[2] for ev in pipe.trace if ev[0] == "unet"), "the UNet receives 0-dim device timesteps"
    # the record entries are the rows they copy (restore first: row 0 of a propagation batch is the restored row)
    assert len(records) == len(pipe.unet.inputs) == len(lg[name + "_rec"])
    for i, (rec, x) in enumerate(zip(records, pipe.unet.inputs)):
        assert rec.shape == (2,) + x.shape[1:] and rec.dtype == dtype
        assert torch.equal(rec[0], x[0]) and torch.equal(rec[1], x[B - 1]), (name, i)
        if rec_in is not None:
            assert torch.equal(x[:2], rec_in[i]), (name, i)
        if ckw.get("do_classifier_free_guidance", True):
            assert x.shape[0] == 2 * B and torch.equal(x[:B], x[B:]), (name, i)
        else:
            assert x.shape[0] == B


def test_omitted_record_latents_is_a_fresh_list(lg, monkeypatch):
    import fresco_amd
    from fresco_amd import loop
    pipe = M.Pipe(DEV, torch.float16)
    (imgs, embeds, edges), kw = M.make_inputs("warm2", DEV, torch.float16)
    for _ in range(2):
        fresco_amd.inference(pipe, pipe.controlnet, pipe.frescoProc, imgs, embeds, edges, pipe.scheduler.timesteps.to(DEV), **kw)
    assert loop._OMITTED == [] and len(pipe.unet.inputs) == 8


def test_hook_follows_the_host_timestep(lg, monkeypatch):
    """apply_FRESCO_opt on the stand-in: state.active follows `t in steps` while the UNet receives device timesteps"""
    import fresco_amd
    from fresco_amd import hook
    seen = []
    box = {}

    def setup(pipe):
        fresco_amd.apply_FRESCO_opt(pipe, steps=[601, 301], layers=[])
        box["state"] = getattr(pipe.unet, hook._STATE)

    def on_call():
        seen.append((box["state"].active, box["state"].host_timestep))

    pipe, steps, final, _, _ = run(lg, "warm2", torch.float16, monkeypatch, on_call=on_call, setup=setup)
    assert seen == [(t in (601, 301), None) for t in M.STEPS[2:]]
    assert all(ev[2] for ev in pipe.trace if ev[0] == "unet")
    assert distance(lg, "warm2", steps, final) <= 4.0


def test_loop_body_does_not_synchronise(lg, monkeypatch):
    """a plain, guided case with everything from the first UNet call on under torch.cuda.set_sync_debug_mode("error")"""
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            raised = False
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")

    def on_call():
        torch.cuda.set_sync_debug_mode("error")

    import fresco_amd
    pipe = M.Pipe(DEV, torch.float16)
    pipe.unet.on_call = on_call
    (imgs, embeds, edges), kw = M.make_inputs("warm2", DEV, torch.float16)
    monkeypatch.setattr(torch, "randn", M.replay_randn([torch.from_numpy(z).to(DEV, torch.float16)
                                                        for z in lg["warm2_draws"]], DEV))
    timesteps = pipe.scheduler.timesteps.to(DEV)
    try:
        final = fresco_amd.inference(pipe, pipe.controlnet, pipe.frescoProc, imgs, embeds, edges, timesteps, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    steps = torch.stack([x[:3] for x in pipe.unet.inputs])
    assert len(pipe.unet.inputs) == 4 and distance(lg, "warm2", steps, final) <= 4.0


def test_a_plain_step_is_one_kernel_beside_randn(lg):
    """under torch.profiler, outside the stand-ins' own ranges: between the UNet call of a step and the next ControlNet call
    (or the return) the device runs exactly one loop_update kernel and what one torch.randn runs; between the ControlNet and
    the UNet of a step it runs nothing.  Each gap is a profiler session of its own, opened and closed at the stand-ins'
    boundaries behind a device synchronise, so that what a session holds is what was launched inside the gap: no
    timestamp of one clock is compared with another's."""
    import fresco_amd
    from torch.profiler import ProfilerActivity, profile
    pipe = M.Pipe(DEV, torch.float16)
    (imgs, embeds, edges), kw = M.make_inputs("warm2", DEV, torch.float16)
    timesteps = pipe.scheduler.timesteps.to(DEV)
    unet_forward, controlnet = pipe.unet.forward, pipe.controlnet
    gaps, session = [], {}

    def open_gap(label):
        if session.get("on"):
            torch.cuda.synchronize()
            session["prof"] = profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA])
            session["prof"].__enter__()
            session["label"] = label

    def close_gap():
        prof = session.pop("prof", None)
        if prof is not None:
            torch.cuda.synchronize()
            prof.__exit__(None, None, None)
            gaps.append((session["label"], sorted(e.name for e in prof.events()
                                                  if e.device_type == torch.autograd.DeviceType.CUDA)))

    def unet_outside(*a, **k):
        close_gap()
        out = unet_forward(*a, **k)
        open_gap("after the UNet")
        return out

    def controlnet_outside(*a, **k):
        close_gap()
        out = controlnet(*a, **k)
        open_gap("after the ControlNet")
        return out

    pipe.unet.forward = unet_outside
    args = (pipe, controlnet_outside, pipe.frescoProc, imgs, embeds, edges, timesteps)
    fresco_amd.inference(*args, **kw)  # (first launches load code objects)
    torch.cuda.synchronize()
    session["on"] = True
    fresco_amd.inference(*args, **kw)
    close_gap()  # the last step's glue ends at the return
    gen = torch.Generator(device=DEV).manual_seed(1)
    open_gap("randn alone")
    torch.randn((3, 4, 8, 8), generator=gen, device=DEV, dtype=torch.float16)
    close_gap()

    randn_kernels = gaps.pop()[1]
    assert randn_kernels and not any("loop_update" in n for n in randn_kernels)
    assert [label for label, _ in gaps] == ["after the ControlNet", "after the UNet"] * 4
    for k, (label, names) in enumerate(gaps):
        ours = [n for n in names if "loop_update_kernel" in n]
        print("step %d, %s: %d on the device, %d of them loop_update, %d of randn"
              % (k // 2, label, len(names), len(ours), len(randn_kernels) if ours else 0))
        if label == "after the ControlNet":
            assert names == [], (k, names)
        else:
            assert len(ours) == 1 and sorted(n for n in names if n not in ours) == randn_kernels, (k, names, randn_kernels)


def test_tensor2numpy_on_a_decoded_batch(lg, monkeypatch):
    import fresco_amd
    _, _, final, _, _ = run(lg, "warm2", torch.float16, monkeypatch)
    img = M.VAE().decode(final / M.VAE.config.scaling_factor).sample
    assert img.shape == (3, 3, M.SIDE, M.SIDE) and img.dtype == torch.float16
    got = fresco_amd.tensor2numpy(img)
    want = M.image_to_frames_model(img)
    assert got.dtype == np.uint8 and got.shape == (3, M.SIDE, M.SIDE, 3) and np.array_equal(got, want)
    assert len(np.unique(got)) > 16
    assert np.array_equal(fresco_amd.tensor2numpy(img.float()), M.image_to_frames_model(img.float()))
    with pytest.raises(TypeError):
        fresco_amd.tensor2numpy(img.bfloat16())
