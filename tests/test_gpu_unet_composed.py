"""The system INTEGRATION.md tells a user to build, on one model: the four patches (recipes N, O, P, Q), the FRESCO processors
on up_blocks.2 / up_blocks.3, the up-block hook and fresco_amd.inference (recipe S) on the composed stand-in UNet + ControlNet
of tests/unet_composed_model.py, against the float64 records of tests/golden/unet_composed_golden.npz.

Every numeric bar is the project's drop-in bar, read from the golden file: |got - record| <= 4 x noise x peak, `noise` being
the recorded distance of the reference arithmetic (fp32, every layer's output rounded to fp16, resp. bf16) from its float64
run.  Each comparison prints its ratio to the bar beside the ratio of the unpatched fp16 model on PyTorch's kernels (for
`fresco` and `bf16`: PyTorch's modules around the native FRESCO sites).  Nothing is compared with the code's own earlier output except
bit for bit.  The models are stand-ins with stand-in weights: diffusers' modules and a checkpoint stay unchecked.

The second half drives what a keyframe run does around those calls, against tests/golden/unet_composed_seq_golden.npz:
fresco_amd.get_intraframe_paras (the store pass: one UNet call without residuals), the call with the spatial-guided pass on
top of cross-frame and temporal attention (`full`), and fresco_amd.inference with the real AttentionControl going through the
reference's sequence (`seq`).  What they pin is the order and the number of `attn1` calls under the patches: the store pass
appends one tensor per self-attention call of up_blocks.2 / up_blocks.3 and the cyclic read index advances once per such
call."""
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

    def full_on(self, steps=(HOOK_STEP,), correlation_matrix=()):
        """run_fresco.py:231-234: enable_controller (intra too: it stays off on an empty store) and the hook, iters = 0"""
        import fresco_amd
        self.ctrl.enable_controller(self.inter, self.cf_masks)
        fresco_amd.apply_FRESCO_opt(self.pipe, steps=steps, layers=[0, 1, 2, 3], flows=self.flows, occs=self.occs,
                                    correlation_matrix=list(correlation_matrix), iters=0, saliency=self.saliency)

    def flags(self):
        c = self.ctrl
        return (int(c.use_intraattn), int(c.use_interattn), int(c.use_cfattn), int(c.index))

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


def report(what, got, own=None, own_label="PyTorch fp16", keys=M.CALL_KEYS):
    line = "%s |got - record| / (4 x noise x peak): %s" % (what, "  ".join("%s %.3f" % kv for kv in zip(keys, got)))
    if own is not None:
        line += "   (%s: %s)" % (own_label, "  ".join("%s %.3f" % kv for kv in zip(keys, own)))
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


# ---------------------------------------------------------------------------------------------------------------
# the store pass, the spatial-guided call and the controller as the loop drives it
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seq_gold():
    return M.seq_golden(GOLDEN)


class keyframe:
    """patched(rig, order) -- order None: the unpatched models -- whose exit also empties the controller's store and puts
    the processor's switches back"""

    def __init__(self, rig, order="NOPQ"):
        self.rig, self.inner = rig, None if order is None else patched(rig, order)

    def __enter__(self):
        return None if self.inner is None else self.inner.__enter__()

    def __exit__(self, *exc):
        if self.inner is not None:
            self.inner.__exit__(*exc)
        else:
            self.rig.fresco_off()
            self.rig.place()
        self.rig.ctrl.clear_store()
        self.rig.proc.fuse_kv_pack = self.rig.proc.sparse_kv_projection = True
        self.rig.unet.on_call = None


def device_pipe(rig):
    """unet_composed_model.Pipe around the rig's models with what a diffusers pipeline has and loop_model.Pipe lacks for
    get_intraframe_paras: the scheduler's timesteps on the device (set_timesteps(n, device=...)), the controller"""
    pipe = M.Pipe(DEV, torch.float16, rig.unet, rig.cn)
    pipe.frescoProc = types.SimpleNamespace(controller=rig.ctrl)
    pipe.scheduler.timesteps = pipe.scheduler.timesteps.to(DEV)
    return pipe


def store_pass(rig, seed=M.STORE_SEED):
    """fresco_amd.get_intraframe_paras on the rig's UNet with the record's images and its one draw -> the Gram targets"""
    import fresco_amd
    imgs, draw = M.store_inputs(seed)
    pipe = device_pipe(rig)
    keep, torch.randn = torch.randn, L.replay_randn([draw.to(DEV)], DEV)
    try:
        return fresco_amd.get_intraframe_paras(pipe, imgs.to(DEV), pipe.frescoProc, rig.inputs()[2], seed=0)
    finally:
        torch.randn = keep


def stored(rig):
    return rig.ctrl.stored_attn["decoder_attn"]


def store_ratios(seq_gold, tensors, corr):
    """per STORE_KEYS entry |got - record| / (4 x noise x peak)"""
    got = {"attn%d" % i: M.thin_tokens(t.double().cpu()) for i, t in enumerate(tensors)}
    got.update({"gram%d" % i: M.thin_gram(c.double().cpu()) for i, c in enumerate(corr)})
    return [M.distance(got[k], seq_gold["store_" + k]) / bar for k, bar in zip(M.STORE_KEYS, M.store_bars(seq_gold))]


def test_store_pass_under_the_four_patches(rig, seq_gold):
    ctrl = rig.ctrl
    x, t, text, _ = rig.inputs()
    with keyframe(rig, None):        # PyTorch's modules around the native processor
        corr = store_pass(rig)       # (clear_store() makes a new list: read it after the pass)
        own = store_ratios(seq_gold, stored(rig), corr)
    with keyframe(rig):
        ctrl.enable_interattn(rig.inter)      # the call must switch both off
        ctrl.enable_cfattn(rig.cf_masks)
        corr = store_pass(rig)
        kept = stored(rig)
        assert len(kept) == M.STORED
        n = 2 * M.FRAMES
        assert [tuple(k.shape) for k in kept] == [(n, 64, 640), (n, 256, 320), (n, 256, 320)]
        assert all(k.dtype == torch.float16 and k.is_contiguous() for k in kept)
        assert ctrl.store is False and rig.flags() == (0, 0, 0, 0)
        assert [tuple(c.shape) for c in corr] == [(n, 4, 4), (n, 16, 16), (n, 64, 64), (n, 256, 256)]
        assert all(c.dtype == torch.float32 for c in corr)
        got = store_ratios(seq_gold, kept, corr)
        line = report("store", got, own, "PyTorch fp16 around the native processor", keys=M.STORE_KEYS)
        assert max(got) <= 1.0 and max(own) <= 1.0, line
        # each tensor owns its memory: no two overlap, and further calls (the loop's form with residuals, then the store pass's
        # form without) leave every bit as it was
        spans = sorted((k.data_ptr(), k.data_ptr() + k.numel() * k.element_size()) for k in kept)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
        bits = [k.clone() for k in kept]
        first = call(rig)[0]
        with torch.no_grad():
            second = rig.unet(x, t, encoder_hidden_states=text, cross_attention_kwargs=None, return_dict=False)
        assert len(second) == 5 and len(stored(rig)) == M.STORED     # disable_FRESCO_opt's hook keeps collecting; nothing stored
        assert all(k is s for k, s in zip(kept, stored(rig))) and all(torch.equal(k, b) for k, b in zip(kept, bits))
        assert M.distance(first.double().cpu().numpy(), second[0].double().cpu().numpy()) > 0      # (the residuals were live)


def test_full_holds_the_bar(rig, gold, seq_gold):
    ctrl = rig.ctrl
    inputs = rig.inputs()
    with keyframe(rig, None):
        store_pass(rig)
        rig.full_on()
        own = M.call_record(rig.unet, rig.cn, torch.float16, inputs=inputs)
    with keyframe(rig):
        plain_bits = flat(call(rig, inputs))
        rig.fresco_on()
        fresco_bits = flat(call(rig, inputs))
        rig.fresco_off()
        # enable_intraattn() on an empty store: use_intraattn stays False and the call is `fresco`'s
        assert len(stored(rig)) == 0
        rig.full_on()
        assert rig.flags() == (0, 1, 1, 0)
        assert torch.equal(flat(call(rig, inputs)), fresco_bits)
        rig.fresco_off()
        # the store pass, everything on, the call
        store_pass(rig)
        rig.full_on()
        assert rig.flags() == (1, 1, 1, 0) and len(stored(rig)) == M.STORED
        kept = [k.clone() for k in stored(rig)]
        rec = M.call_record(rig.unet, rig.cn, torch.float16, inputs=inputs)
        assert rig.flags() == (1, 1, 1, 0)                      # three reads: the index is back at 0
        bits = flat(call(rig, inputs))
        assert rig.flags() == (1, 1, 1, 0)
        assert torch.equal(flat(call(rig, inputs)), bits)       # a second call: the same bits
        assert all(torch.equal(k, s) for k, s in zip(kept, stored(rig)))
        got = ratios(seq_gold, "full", rec)
        line = report("full", got, ratios(seq_gold, "full", own), "PyTorch fp16 around the native FRESCO sites")
        assert np.isfinite(rec["out"]).all() and max(got) <= 1.0, line
        bar = 4 * float(seq_gold["full_noise"][0]) * float(seq_gold["full_peak"][0])
        assert M.distance(rec["out"], gold["fresco_out"]) > 2 * bar      # the spatial pass was live
        assert not torch.equal(bits, fresco_bits)
        # the unfused routes behind the spatial pass
        for switch in ("fuse_kv_pack", "sparse_kv_projection"):
            setattr(rig.proc, switch, False)
            r = ratios(seq_gold, "full", M.call_record(rig.unet, rig.cn, torch.float16, inputs=inputs))
            line = report("full, %s off" % switch, r)
            assert max(r) <= 1.0 and rig.flags() == (1, 1, 1, 0), line
        rig.proc.fuse_kv_pack = rig.proc.sparse_kv_projection = True
        assert torch.equal(flat(call(rig, inputs)), bits)
        # the controller and the hook off again, the store still filled: plain's bits
        rig.fresco_off()
        assert len(stored(rig)) == M.STORED and torch.equal(flat(call(rig, inputs)), plain_bits)
    for order in ORDERS[1:]:
        with keyframe(rig, order):
            store_pass(rig)
            rig.full_on()
            assert torch.equal(flat(call(rig, inputs)), bits), order


def test_full_runs_natively(rig):
    inputs = rig.inputs()
    with keyframe(rig):
        store_pass(rig)
        rig.full_on()
        call(rig, inputs)        # (the caches of the text, of the condition and of the index tables fill)
        names = _kernel_names(lambda: call(rig, inputs))
        assert rig.flags() == (1, 1, 1, 0)
    print("full, patched: %s" % (names,))
    for k in names:
        if "fresco" in k:
            continue
        assert any(a in k for a in ALLOWED) and not any(s in k for s in NOT_OURS), k
    assert any("unet_attention" in k or "unet_attn" in k for k in names), names


def seq_ratio(seq_gold, steps, final):
    d = max(M.distance(steps.double().cpu().numpy(), seq_gold["seq_steps"]), M.distance(final.double().cpu().numpy(), seq_gold["seq_final"]))
    return d / (4 * float(seq_gold["seq_noise"][0]) * float(seq_gold["seq_peak"][0]))


def seq_run(rig, seq_gold, loop, on_call=None):
    """the store pass, everything switched on as run_fresco.py does (the hook on timesteps[:END_OPT_STEP] with the store pass's
    Gram targets and iters = 0), then `loop` -- fresco_amd.inference or its restatement -- with the recorded draws replayed
    -> (every UNet input's first half, the final latents, the controller's flags at each UNet call)"""
    corr = store_pass(rig)
    pipe = device_pipe(rig)
    timesteps = pipe.scheduler.timesteps
    if loop is L.inference_model:      # (the restatement indexes the scheduler's host tables)
        timesteps = pipe.scheduler.timesteps = timesteps.cpu()
    rig.full_on(steps=timesteps[:M.END_OPT_STEP], correlation_matrix=corr)
    seen = []

    def observe():
        seen.append(rig.flags())
        if on_call is not None:
            on_call()
    rig.unet.on_call = observe
    keep, torch.randn = torch.randn, L.replay_randn([torch.from_numpy(z).to(DEV, torch.float16) for z in seq_gold["seq_draws"]], DEV)
    try:
        final = loop(pipe, pipe.controlnet, pipe.frescoProc, *M.loop_inputs(DEV, torch.float16), timesteps,
                     flows=rig.flows, occs=rig.occs, saliency=rig.saliency, **M.SEQ_KW)
    finally:
        torch.randn, rig.unet.on_call = keep, None
        torch.cuda.set_sync_debug_mode("default")
    return torch.stack([x[:M.FRAMES] for x in rig.unet.inputs]), final, tuple(seen)


def test_inference_drives_the_real_controller(rig, seq_gold):
    """`seq`: intra + temporal + cross-frame at 601, temporal + cross-frame at 451, cross-frame at 301 and 151.  The index
    tables of the masks and of the trajectory maps are built and checked on the host once per table, at their first use
    (processor._sel_rows, ops._check_once); the restated loop on the unpatched models, which runs first, is that first use,
    and from the first UNet call of fresco_amd.inference on nothing synchronises"""
    import fresco_amd
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            raised = False
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert raised, "torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build"
    ctrl = rig.ctrl
    with keyframe(rig, None):
        s_own, f_own, flags_own = seq_run(rig, seq_gold, L.inference_model)
    with keyframe(rig):
        kept = []

        def on_call():
            if not kept:
                kept.extend((k, k.clone()) for k in stored(rig))
            torch.cuda.set_sync_debug_mode("error")
        steps, final, flags = seq_run(rig, seq_gold, fresco_amd.inference, on_call)
        torch.cuda.synchronize()
        ratio = seq_ratio(seq_gold, steps, final)
        line = "seq: %.3f of the bar (noise %.2e, peak %.3g); fp16 torch ops on the unpatched model: %.3f" % (
            ratio, float(seq_gold["seq_noise"][0]), float(seq_gold["seq_peak"][0]), seq_ratio(seq_gold, s_own, f_own))
        print(line)
        assert steps.shape[0] == len(M.STEPS2) and final.shape == (M.FRAMES, 4, M.LAT, M.LAT) and ratio <= 1.0, line
        bar = 4 * float(seq_gold["seq_noise"][0]) * float(seq_gold["seq_peak"][0])
        for i in range(len(M.STEPS2)):
            assert M.distance(steps[i].double().cpu().numpy(), seq_gold["seq_steps"][i]) <= bar, i
        # the controller went through the reference's sequence, the index back at 0 at every call
        recorded = tuple(map(tuple, seq_gold["seq_flags"].tolist()))
        assert flags == recorded == M.SEQ_FLAGS and flags_own == recorded, (flags, flags_own)
        assert rig.flags() == (0, 0, 1, 0) and ctrl.store is False
        # the store is untouched by the loop
        assert len(kept) == M.STORED == len(stored(rig))
        assert all(k is s and torch.equal(k, b) for (k, b), s in zip(kept, stored(rig)))
