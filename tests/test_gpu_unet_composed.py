"""The system INTEGRATION.md tells a user to build, on one model: the four patches (recipes N, O, P, Q), the FRESCO processors
on up_blocks.2 / up_blocks.3, the up-block hook and fresco_amd.inference (recipe S) on the composed stand-in UNet + ControlNet
of tests/unet_composed_model.py, against the float64 records of tests/golden/unet_composed_golden.npz.

Every numeric bar is the project's drop-in bar, read from the golden file: |got - record| <= 4 x noise x peak, `noise` being
the recorded distance of the reference arithmetic (fp32, every layer's output rounded to fp16, resp. bf16) from its float64
run.  Each comparison prints its ratio to the bar beside the ratio of the unpatched fp16 model on PyTorch's kernels (for
`fresco` and `bf16`: PyTorch's modules around the native FRESCO sites).  Nothing is compared with the code's own earlier output except
bit for bit.  The models are stand-ins with stand-in weights: diffusers' modules and a checkpoint stay unchecked."""
import os
import types

import numpy as np
import pytest
import torch

import loop_model as L
import unet_attention_model as A
import unet_composed_model as M
from test_gpu_unet_shell import ALLOWED, NOT_OURS, _deterministic, _kernel_names

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOOK_STEP = 451       # call_inputs' timestep: the hook is active on it
ORDERS = ("NOPQ", "QPON", "ONQP")
UNET_COUNTS = dict(N=8, O=6, P=6, P_cross=9,
                   Q={"down": 3, "up": 3, "conv_in": 1, "conv_out": 1, "time": 1, "cond_embedding": 0, "zero_conv": 0})
CN_COUNTS = dict(N=3, O=3, P=6, P_cross=6,
                 Q={"down": 3, "up": 0, "conv_in": 1, "conv_out": 0, "time": 1, "cond_embedding": 1, "zero_conv": 6})


@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


class Rig:
    """the fp16 pair on the GPU with the reference's processor placement, the inputs of the single calls, and the
    controller's parameters"""

    def __init__(self):
        import fresco_amd
        self.unet, self.cn = M.build("unet", torch.float16, DEV), M.build("controlnet", torch.float16, DEV)
        self.ctrl = fresco_amd.AttentionControl()
        self.proc = fresco_amd.FRESCOAttnProcessor2_0(2, self.ctrl)
        self.plain = A.RefProcessor()
        self.place()
        fi = M.fresco_inputs()
        d = lambda ts: [t.to(DEV) for t in ts]  # noqa: E731
        self.flows, self.occs, self.saliency = d(fi["flows"]), d(fi["occs"]), fi["saliency"].to(DEV)
        self.inter = dict(fwd_mappings=d(fi["fwd_maps"]), bwd_mappings=d(fi["bwd_maps"]), interattn_masks=d(fi["tmasks"]))
        self.cf_masks = d(fi["cf_masks"])
        self.pipe = types.SimpleNamespace(unet=self.unet)

    def place(self):
        """apply_FRESCO_attn's rule (diffusion_hacked.py:394-402): the FRESCO processor on up_blocks.2 / up_blocks.3, a plain
        one elsewhere; the ControlNet keeps plain ones"""
        self.unet.set_attn_processor({k: self.proc if k.startswith(("up_blocks.2", "up_blocks.3")) else self.plain
                                      for k in self.unet.attn_processors})
        self.cn.set_attn_processor(self.plain)

    def inputs(self):
        x, t, text, edges = M.call_inputs()
        return x.to(DEV), t.to(DEV), text.to(DEV), edges.to(DEV)

    def fresco_on(self):
        import fresco_amd
        self.ctrl.enable_interattn(self.inter)
        self.ctrl.enable_cfattn(self.cf_masks)
        fresco_amd.apply_FRESCO_opt(self.pipe, steps=[HOOK_STEP], layers=[0, 1, 2, 3], flows=self.flows, occs=self.occs,
                                    correlation_matrix=[], iters=0, saliency=self.saliency)

    def fresco_off(self):
        from fresco_amd import hook
        self.ctrl.disable_controller()
        hook._remove(self.unet)


@pytest.fixture(scope="module")
def rig():
    import time
    t0 = time.time()
    r = Rig()
    torch.cuda.synchronize()
    print("the fp16 pair (%d parameters) built on the GPU in %.1f s" % (M.parameters_of(r.unet) + M.parameters_of(r.cn), time.time() - t0))
    return r


def patch(net, order="NOPQ", cross=True):
    """the four patches on one model in `order` -> {recipe letter: what the patch returned}"""
    import fresco_amd
    fns = {"N": fresco_amd.patch_unet_resnets, "O": fresco_amd.patch_unet_transformers,
           "P": lambda m: fresco_amd.patch_unet_attention(m, include_fresco_cross=cross), "Q": fresco_amd.patch_unet_shell}
    return {k: fns[k](net) for k in order}


def unpatch(net):
    import fresco_amd
    return (fresco_amd.unpatch_unet_attention(net) + fresco_amd.unpatch_unet_transformers(net)
            + fresco_amd.unpatch_unet_resnets(net) + fresco_amd.unpatch_unet_shell(net))


class patched:
    def __init__(self, rig, order="NOPQ", cross=True):
        self.rig, self.order, self.cross = rig, order, cross

    def __enter__(self):
        self.counts = patch(self.rig.unet, self.order, self.cross), patch(self.rig.cn, self.order, self.cross)
        return self.counts

    def __exit__(self, *exc):
        unpatch(self.rig.unet)
        unpatch(self.rig.cn)
        self.rig.fresco_off()
        self.rig.place()


def flat(out):
    o, down, mid = out
    return torch.cat([o.reshape(-1)] + [t.reshape(-1) for t in down] + [mid.reshape(-1)])


def call(rig, inputs=None):
    """(noise prediction, down residuals, mid residual) of one ControlNet + UNet call"""
    with torch.no_grad():
        return M.run_call(rig.unet, rig.cn, *(inputs or rig.inputs()))


def ratios(gold, case, rec):
    """per CALL_KEYS entry |rec - record| / (4 x noise x peak)"""
    return [M.distance(rec[k], gold["%s_%s" % (case, k)]) / (4 * float(gold[case + "_noise"][i]) * float(gold[case + "_peak"][i]))
            for i, k in enumerate(M.CALL_KEYS)]


def report(what, got, own=None, own_label="PyTorch fp16"):
    line = "%s |got - record| / (4 x noise x peak): %s" % (what, "  ".join("%s %.3f" % kv for kv in zip(M.CALL_KEYS, got)))
    if own is not None:
        line += "   (%s: %s)" % (own_label, "  ".join("%s %.3f" % kv for kv in zip(M.CALL_KEYS, own)))
    print(line)
    return line


# ---------------------------------------------------------------------------------------------------------------
# counts, placement and the dispatch
# ---------------------------------------------------------------------------------------------------------------
def test_counts_placement_and_dispatch(rig, monkeypatch):
    import fresco_amd
    from fresco_amd import ops
    fresco_mods = dict(rig.unet._attention_modules())
    fresco_names = M.fresco_names(rig.unet)
    with patched(rig, cross=False) as (uc, cc):
        assert uc == {"N": UNET_COUNTS["N"], "O": UNET_COUNTS["O"], "P": UNET_COUNTS["P"], "Q": UNET_COUNTS["Q"]}
        assert cc == {"N": CN_COUNTS["N"], "O": CN_COUNTS["O"], "P": CN_COUNTS["P"], "Q": CN_COUNTS["Q"]}
        # what the model holds
        assert uc["N"] == sum(1 for m in rig.unet.modules() if isinstance(m, M.R.Resnet))
        assert uc["O"] == sum(1 for m in rig.unet.modules() if isinstance(m, M.T.Transformer))
        assert uc["P"] == len(fresco_mods) - len(fresco_names)
        for name, m in fresco_mods.items():          # the FRESCO modules keep their processor
            assert (m.processor is rig.proc) == (name in fresco_names), name
            assert isinstance(m.processor, fresco_amd.UNetAttnProcessor) == (name not in fresco_names), name
        assert all(isinstance(m.processor, fresco_amd.UNetAttnProcessor) for _, m in rig.cn._attention_modules())
        # include_fresco_cross=True takes exactly their .attn2 modules
        assert fresco_amd.patch_unet_attention(rig.unet, include_fresco_cross=True) == UNET_COUNTS["P_cross"]
        for name, m in fresco_mods.items():
            if name in fresco_names:
                assert (m.processor is rig.proc) == name.endswith(".attn1"), name
                assert isinstance(m.processor, fresco_amd.UNetAttnProcessor) == name.endswith(".attn2"), name

        seen = []

        def spy(name, describe):
            real = getattr(ops, name)

            def wrapper(*a, **k):
                seen.append((name,) + describe(*a, **k))
                return real(*a, **k)
            monkeypatch.setattr(ops, name, wrapper)
        spy("unet_attention", lambda q, k, v, heads, *a, **kw: (q.shape[-1] // heads, k.shape[1]))
        spy("attention", lambda q, k, v, heads, *a, **kw: (q.shape[-1] // heads,))
        spy("linear", lambda x, weights, *a, **kw: (x.shape[-1], len(weights)))
        spy("vae_conv", lambda x, w, bias, n, H, W, cin, cout, ksize, **kw: (cin, cout, ksize, bool(kw.get("up2", False))))
        spy("unet_conv3", lambda x, w, bias, stride=1, silu=False: (x.shape[-1], w.shape[0], stride))
        spy("unet_geglu", lambda x, w, bias, **kw: (x.shape[-1],))
        call(rig)
        monkeypatch.undo()
        # head dim 160: unet_attention on self- (4 keys) and cross-attention (77 keys), q | k | v and to_out through vae_conv
        assert ("unet_attention", 160, 4) in seen and ("unet_attention", 160, M.TEXT_TOKENS) in seen
        assert ("vae_conv", 1280, 3840, 1, False) in seen and ("vae_conv", 1280, 1280, 1, False) in seen
        # head dims 40 and 80: fresco_attn_fwd; q | k | v in one fresco_linear launch, to_q alone for cross-attention
        assert ("attention", 40) in seen and ("attention", 80) in seen
        for K in (320, 640):
            assert ("linear", K, 3) in seen and ("linear", K, 1) in seen
        assert not any(s[0] == "attention" and s[1] == 160 for s in seen)
        assert not any(s[0] == "linear" and s[1] == 1280 for s in seen)
        # the text K | V: one vae_conv 1 x 1 over the stacked (2 C, text width) matrix per width
        for C in (320, 640, 1280):
            assert ("vae_conv", M.TEXT_WIDTH, 2 * C, 1, False) in seen
        # the shell: both Downsample2D widths, both Upsample2D widths (the up2 form), the zero convolutions, conv_in
        assert ("unet_conv3", 320, 320, 2) in seen and ("unet_conv3", 640, 640, 2) in seen
        assert ("vae_conv", 1280, 1280, 3, True) in seen and ("vae_conv", 640, 640, 3, True) in seen
        assert ("vae_conv", 640, 1280, 1, False) in seen          # the mid zero convolution
        assert ("vae_conv", 32, 320, 3, False) in seen            # conv_in on the padded latents
        # the concatenating resnets' first convolutions, and the GEGLU at each width
        for cin, cout in ((640, 320), (960, 320), (960, 640), (1920, 640), (1920, 1280)):
            assert ("vae_conv", cin, cout, 3, False) in seen, (cin, cout)
        assert {s[1] for s in seen if s[0] == "unet_geglu"} == {320, 640, 1280}


# ---------------------------------------------------------------------------------------------------------------
# plain and fresco against the record
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def own(rig):
    """the unpatched fp16 model on PyTorch's kernels: the plain call's record"""
    return M.call_record(rig.unet, rig.cn, torch.float16, device=DEV)


def test_plain_and_fresco_hold_the_bar(rig, gold, own):
    inputs = rig.inputs()
    # PyTorch's modules around the native FRESCO sites
    rig.fresco_on()
    try:
        own_fresco = M.call_record(rig.unet, rig.cn, torch.float16, inputs=inputs)
    finally:
        rig.fresco_off()
    with patched(rig):
        rec = M.call_record(rig.unet, rig.cn, torch.float16, inputs=inputs)
        plain_bits = flat(call(rig, inputs))
        assert torch.equal(flat(call(rig, inputs)), plain_bits)                 # a second call: the same bits
        got = ratios(gold, "plain", rec)
        line = report("plain", got, ratios(gold, "plain", own))
        assert np.isfinite(rec["out"]).all() and max(got) <= 1.0, line

        rig.fresco_on()
        rec_f = M.call_record(rig.unet, rig.cn, torch.float16, inputs=inputs)
        fresco_bits = flat(call(rig, inputs))
        assert torch.equal(flat(call(rig, inputs)), fresco_bits)
        got = ratios(gold, "fresco", rec_f)
        line = report("fresco", got, ratios(gold, "fresco", own_fresco), "PyTorch fp16 around the native FRESCO sites")
        assert np.isfinite(rec_f["out"]).all() and max(got) <= 1.0, line
        # the sites were live: further from plain's record than the bar
        bar = 4 * float(gold["plain_noise"][0]) * float(gold["plain_peak"][0])
        assert M.distance(rec_f["out"], gold["plain_out"]) > bar
        # the controller and the hook off again: plain's bits
        rig.fresco_off()
        assert torch.equal(flat(call(rig, inputs)), plain_bits)


# ---------------------------------------------------------------------------------------------------------------
# native only
# ---------------------------------------------------------------------------------------------------------------
def test_patched_models_run_natively(rig):
    inputs = rig.inputs()
    before = _kernel_names(lambda: call(rig, inputs))
    print("unpatched: %s" % (before,))
    foreign = [k for k in before if "fresco" not in k and any(s in k for s in NOT_OURS)]
    assert foreign, before       # the profiler sees PyTorch's convolutions and GEMMs: the check below is not vacuous
    with patched(rig):
        call(rig, inputs)        # (the caches of the text and of the condition fill: the profiled call is a later step's)
        names = _kernel_names(lambda: call(rig, inputs))
        rig.cn.controlnet_cond_embedding.forward.clear()
        first = _kernel_names(lambda: call(rig, inputs))    # ... and a first step's, with the embedding computed
    print("patched: %s" % (names,))
    for k in sorted(set(names) | set(first)):
        if "fresco" in k:
            continue
        assert any(a in k for a in ALLOWED) and not any(s in k for s in NOT_OURS), k
    assert any("unet_conv3_kernel" in k for k in first) and any("unet_attention" in k or "unet_attn" in k for k in names), names


# ---------------------------------------------------------------------------------------------------------------
# order
# ---------------------------------------------------------------------------------------------------------------
def test_patch_order_and_unpatching(rig):
    inputs = rig.inputs()
    with torch.no_grad():
        own_det = _deterministic(lambda: flat(call(rig, inputs)))
        assert torch.equal(_deterministic(lambda: flat(call(rig, inputs))), own_det)     # what the last assertion stands on
    processors = dict(rig.unet.attn_processors), dict(rig.cn.attn_processors)
    bits = []
    for order in ORDERS:
        for late in (False, True):       # the processors set before patch_unet_transformers, or after it
            if late:                     # every processor plain while N, O and Q go on ...
                rig.unet.set_attn_processor(rig.plain)
            with patched(rig, order.replace("P", "") if late else order):
                if late:                 # ... then apply_FRESCO_attn's placement, and recipe P AFTER it
                    rig.place()
                    assert patch(rig.unet, "P")["P"] == UNET_COUNTS["P_cross"] and patch(rig.cn, "P")["P"] == CN_COUNTS["P_cross"]
                bits.append(flat(call(rig, inputs)))
            assert dict(rig.unet.attn_processors) == processors[0] and dict(rig.cn.attn_processors) == processors[1], (order, late)
            for net in (rig.unet, rig.cn):
                assert not any("forward" in vars(m) for m in net.modules()), (order, late)
                for m in net.modules():
                    assert m.forward.__func__ is type(m).forward
    assert all(torch.equal(b, bits[0]) for b in bits[1:]), [float((b.float() - bits[0].float()).abs().max()) for b in bits]
    with torch.no_grad():
        assert torch.equal(_deterministic(lambda: flat(call(rig, inputs))), own_det)     # the modules' own forwards, bit for bit


# ---------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------
def loop_ratio(gold, steps, final):
    d = max(M.distance(steps.double().cpu().numpy(), gold["loop_steps"]), M.distance(final.double().cpu().numpy(), gold["loop_final"]))
    return d / (4 * float(gold["loop_noise"][0]) * float(gold["loop_peak"][0]))


def loop_setup(rig, gold, monkeypatch):
    """(pipe, (imgs, prompt_embeds, edges)) with the recorded draws uploaded and torch.randn replaying them"""
    pipe = M.Pipe(DEV, torch.float16, rig.unet, rig.cn)
    pipe.frescoProc = types.SimpleNamespace(controller=rig.ctrl)
    monkeypatch.setattr(torch, "randn", L.replay_randn([torch.from_numpy(z).to(DEV, torch.float16) for z in gold["loop_draws"]], DEV))
    return pipe, M.loop_inputs(DEV, torch.float16)


def test_inference_on_the_patched_pipe(rig, gold, monkeypatch):
    import fresco_amd
    from fresco_amd import ops
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            raised = False
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pipe, args = loop_setup(rig, gold, monkeypatch)       # the restated loop in fp16 torch ops on the unpatched models
    f_own = L.inference_model(pipe, pipe.controlnet, pipe.frescoProc, *args, pipe.scheduler.timesteps, **M.LOOP_KW)
    s_own = torch.stack([x[:M.FRAMES] for x in rig.unet.inputs])
    monkeypatch.undo()
    with patched(rig):
        seen = {"cond": 0, "text": 0, "latents": [], "where": set()}
        real_input, real_rows = ops.unet_input, ops.conv_rows

        def unet_input(x, cpad):
            out = real_input(x, cpad)
            if x.shape[1] == 3:
                seen["cond"] += 1
            else:
                seen["latents"].append(out[..., :4].clone())       # what conv_in's convolution reads
                seen["where"].add(x.data_ptr())
            return out

        def conv_rows(x, w, bias=None, residual=None):
            if x.shape[-1] == M.TEXT_WIDTH and x.shape[-2] == M.TEXT_TOKENS:
                seen["text"] += 1
            return real_rows(x, w, bias, residual)
        if raised:     # from the first UNet call on, a host synchronisation raises (tests/test_gpu_loop.py's check)
            rig.unet.on_call = lambda: torch.cuda.set_sync_debug_mode("error")
        try:
            monkeypatch.setattr(ops, "unet_input", unet_input)
            monkeypatch.setattr(ops, "conv_rows", conv_rows)
            pipe, args = loop_setup(rig, gold, monkeypatch)
            final = fresco_amd.inference(pipe, pipe.controlnet, pipe.frescoProc, *args, pipe.scheduler.timesteps.to(DEV),
                                         **M.LOOP_KW)
        finally:
            torch.cuda.set_sync_debug_mode("default")
            rig.unet.on_call = None
            monkeypatch.undo()
        torch.cuda.synchronize()
        assert raised, "torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build"
        steps = torch.stack([x[:M.FRAMES] for x in rig.unet.inputs])
        ratio = loop_ratio(gold, steps, final)
        line = "loop: %.3f of the bar (noise %.2e, peak %.3g); fp16 torch ops on the unpatched model: %.3f" % (
            ratio, float(gold["loop_noise"][0]), float(gold["loop_peak"][0]), loop_ratio(gold, s_own, f_own))
        print(line)
        assert len(rig.unet.inputs) == 3 and final.shape == (M.FRAMES, 4, M.LAT, M.LAT) and ratio <= 1.0, line
        # one condition embedding and one text projection per cross-attention module over the three steps
        n_cross = sum(1 for net in (rig.unet, rig.cn) for name, _ in net._attention_modules() if name.endswith(".attn2"))
        assert seen["cond"] == 1 and seen["text"] == n_cross == 9, seen
        # conv_in ran three times per model on three different inputs: on the VALUES, the tensor object is the same each time
        lat = seen["latents"]
        assert len(lat) == 6 and len(seen["where"]) == 1      # the loop's one model input, rewritten in place
        bar = 4 * float(gold["loop_noise"][0]) * float(gold["loop_peak"][0])
        for i in range(3):
            assert torch.equal(lat[2 * i], lat[2 * i + 1])                          # the ControlNet's and the UNet's of a step
            read = lat[2 * i + 1].permute(0, 3, 1, 2)
            assert torch.equal(read[:M.FRAMES], read[M.FRAMES:])                    # both CFG halves
            assert M.distance(read[:M.FRAMES].double().cpu().numpy(), gold["loop_steps"][i]) <= bar, i
        assert M.distance(gold["loop_steps"][0], gold["loop_steps"][1]) > 2 * bar
        assert M.distance(gold["loop_steps"][1], gold["loop_steps"][2]) > 2 * bar


def test_in_place_edits_recompute_the_caches(rig, gold):
    """edges.mul_() and prompt_embeds.mul_() between two calls: the condition embedding, resp. the text K | V, are computed
    again -- each call against the record of its own inputs"""
    x, t, text, edges = rig.inputs()
    with patched(rig):
        for case, edit in (("plain", None), ("halfedges", lambda: edges.mul_(0.5)), ("plain", lambda: edges.mul_(2.0)),
                           ("halftext", lambda: text.mul_(0.5)), ("plain", lambda: text.mul_(2.0))):
            if edit is not None:
                edit()
            rec = M.call_record(rig.unet, rig.cn, torch.float16, inputs=(x, t, text, edges))
            got = ratios(gold, case, rec)
            line = report("%s, edited in place" % case, got)
            assert max(got) <= 1.0, line


# ---------------------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------------------
def test_bf16_pair(gold):
    """a bf16 pipeline: native resnets and native FRESCO processors around PyTorch's bf16 transformers, plain attention and
    shell.  No second-call bit check here: PyTorch's own bf16 kernels around the native modules gave other last bits on a
    second run on an MI355X (as tests/test_gpu_unet_shell.py notes of its default convolutions)"""
    import fresco_amd
    unet, cn = M.build("unet", torch.bfloat16, DEV), M.build("controlnet", torch.bfloat16, DEV)
    ctrl = fresco_amd.AttentionControl()
    proc, plain = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl), A.RefProcessor()
    unet.set_attn_processor({k: proc if k.startswith(("up_blocks.2", "up_blocks.3")) else plain for k in unet.attn_processors})
    own = M.call_record(unet, cn, torch.bfloat16, device=DEV)
    assert fresco_amd.patch_unet_resnets(unet, dtype=torch.bfloat16) == UNET_COUNTS["N"]
    assert fresco_amd.patch_unet_resnets(cn, dtype=torch.bfloat16) == CN_COUNTS["N"]
    for net in (unet, cn):
        bound = {m for m in net.modules() if "forward" in vars(m)}
        procs = dict(net.attn_processors)
        for fn, why in ((fresco_amd.patch_unet_transformers, "fp16 modules only"), (fresco_amd.patch_unet_attention, "fp16 modules only"),
                        (fresco_amd.patch_unet_shell, "fp16 modules only")):
            with pytest.raises(NotImplementedError, match=why):
                fn(net)
        assert {m for m in net.modules() if "forward" in vars(m)} == bound and dict(net.attn_processors) == procs
        assert all(isinstance(m, M.R.Resnet) for m in bound)
    rec = M.call_record(unet, cn, torch.bfloat16, device=DEV)
    got = ratios(gold, "bf16", rec)
    line = report("bf16", got, ratios(gold, "bf16", own), "PyTorch bf16 around the native FRESCO processors")
    assert np.isfinite(rec["out"]).all() and max(got) <= 1.0, line
