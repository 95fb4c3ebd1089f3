"""Generate tests/golden/unet_composed_golden.npz and tests/golden/unet_composed_seq_golden.npz: float64 records of the
composed stand-in UNet + ControlNet of tests/unet_composed_model.py on the CPU.

Run:  python tests/golden/make_unet_composed_golden.py [calls | seq]     (both files, or one; about a minute; 4 GB of memory)

diffusers is absent, so the record is the restatement's own (see unet_composed_model's docstring for what is unverified).

Cases (unet_composed_model.derive):
  plain      one ControlNet + UNet call on 2 frames x 2 CFG halves, no controller active
  fresco     the same call with cross-frame and temporal attention on `attn1` of up_blocks.2 / up_blocks.3 and the hook
             (AdaIN + warp_tensor, optimize_feature with iters = 0) on the four up blocks; the sites call
             oracle.fresco_oracle's fresco_attention, adain and warp_tensor, all three in float64
  halfedges  plain with the edges x 0.5, halftext: plain with the text x 0.5 -- what a call after an in-place edit of either
             must give (the condition embedding and the text K | V are cached by tensor identity and version)
  loop       three steps of loop_model.inference_model on loop_model.Pipe with the stand-ins as pipe.unet and the ControlNet,
             guidance and ControlNet on, num_warmup_steps = 3 of six steps; `loop_draws` are the draws, for replay_randn
  bf16       plain again with the layers rounding to bf16 for the noise; its float64 run is of the weights and inputs a bf16
             pipeline holds (each rounded to bf16 once, as unet_resnet_bf16_model does), so that the bar measures the
             arithmetic and not the cast of the checkpoint

Recorded per call case: the noise prediction (`*_out`), every ControlNet residual thinned (vae_model.thin) and flattened
(`*_res`), two taps thinned (`*_mid`, `*_up2`), and for each of the four, in that order, the noise of the reference
arithmetic -- the same models in fp32 with every layer's output rounded to fp16, against the float64 run:
max|difference| / max|float64| (`*_noise`) -- and that largest magnitude (`*_peak`).  The loop case keeps every step's UNet
input (`loop_steps`), the returned latents (`loop_final`) and one noise and peak over both, as loop_golden.npz does.

Asserted: both models together hold at most unet_composed_model.PARAM_LIMIT parameters; no activation above 65504 / 8 in
any run; every noise is positive; `fresco`, `halfedges` and `halftext` differ from `plain` by more than twice the bar.

The second file (unet_composed_model.derive_seq) holds what a keyframe run does around those calls:
  store      the pass get_intraframe_paras makes (src/diffusion_hacked.py:842-901 of the reference): ONE UNet call without
             ControlNet and without residuals at the scheduler's last timestep, 151, on latents of its own (store_latents:
             other images than the loop's, another draw), the controller storing, every flag off, the hook collecting the up
             blocks' inputs and optimising nothing.  `store_attn0..2`: the stored tensors in call order -- attn1's input of
             up_blocks.2 (4, 64, 640) and of up_blocks.3's two transformers (4, 256, 320) -- thinned as maps;
             `store_gram0..3`: oracle.gram_target of each up block's input, thinned as a one-channel map
  full       call_inputs() through ControlNet + UNet with intra, cross-frame and temporal attention on and the hook as in
             `fresco`, reading the float64 stored features of `store`; recorded as the call cases above
  seq        four steps (601, 451, 301, 151: num_warmup_steps = 2) of loop_model.inference_model with the restatement's
             controller working: enable_controller and the hook on timesteps[:4] (iters = 0) as run_fresco.py sets them up,
             num_intraattn_steps = 1, step_interattn_end = 350 -- intra + temporal + cross-frame, temporal + cross-frame,
             cross-frame, cross-frame; the hook on 601 and 451.  `seq_steps`, `seq_final`, `seq_draws` as `loop_*`;
             `seq_flags`: (use_intraattn, use_interattn, use_cfattn, index) at each UNet call
The noise of each is derived as above, the store pass included: the fp32 pair with every layer's output rounded to fp16 makes
its own store pass and reads its own, rounded, references.  For a Gram target it is gram_target of that run's features
against the float64 Gram (2.5e-4 .. 5.1e-4 of the diagonal's 1); a Gram without the normalisation lands 3e6 bars away, one
of the pixels in column order 93 (tests/test_unet_composed_cpu.py).

Asserted for the second file: no activation above 65504 / 8, every noise positive, `full` differs from `fresco` and `seq`'s
step inputs from each other by more than twice the bar, the flags are unet_composed_model.SEQ_FLAGS.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import unet_composed_model as M  # noqa: E402


def main_seq(models, watch):
    out = watch(lambda: M.derive_seq(models))
    for case in ("store", "full", "seq"):
        assert (out[case + "_noise"] > 0).all(), case
        print("%s: noise %s of peak %s" % (case, np.array2string(out[case + "_noise"], precision=5),
                                           np.array2string(out[case + "_peak"], precision=4)))
    bar = 4 * out["full_noise"][0] * out["full_peak"][0]
    d = M.distance(out["full_out"], M.load_golden(HERE)["fresco_out"])
    print("full differs from fresco by %.3f = %.1f bars" % (d, d / bar))
    assert d > 2 * bar
    bar = 4 * out["seq_noise"][0] * out["seq_peak"][0]
    s = out["seq_steps"]
    for i in range(len(s)):
        for j in range(i + 1, len(s)):
            d = M.distance(s[i], s[j])
            print("seq: steps %d and %d differ by %.3f = %.1f bars" % (i, j, d, d / bar))
            assert d > 2 * bar, (i, j)
    assert tuple(map(tuple, out["seq_flags"].tolist())) == M.SEQ_FLAGS, out["seq_flags"]
    path = os.path.join(HERE, M.SEQ_GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


def main(which=("calls", "seq")):
    models = M.Models()
    nets = (models.u64, models.c64, models.u32, models.c32)
    params = M.parameters_of(models.u64) + M.parameters_of(models.c64)
    assert params <= M.PARAM_LIMIT, params
    seen = [0.0]

    def see(m, i, o):
        if isinstance(o, torch.Tensor):
            seen[0] = max(seen[0], float(o.detach().abs().max()))

    def watch(fn):
        seen[0] = 0.0
        hooks = [m.register_forward_hook(see) for net in nets for m in net.modules() if not list(m.children())]
        try:
            out = fn()
        finally:
            for h in hooks:
                h.remove()
        assert seen[0] < M.ACT_LIMIT, seen[0]
        print("%d parameters; largest activation %.1f" % (params, seen[0]))
        return out
    if "calls" in which:
        main_calls(models, watch)
    if "seq" in which:
        main_seq(models, watch)


def main_calls(models, watch):
    out = watch(lambda: M.derive(models))
    for case in list(M.CALL_CASES) + ["bf16", "loop"]:
        assert (out[case + "_noise"] > 0).all(), case
        print("%s: noise %s of peak %s" % (case, np.array2string(out[case + "_noise"], precision=5),
                                           np.array2string(out[case + "_peak"], precision=4)))
    bar = 4 * out["plain_noise"][0] * out["plain_peak"][0]
    for case in ("fresco", "halfedges", "halftext"):
        d = M.distance(out[case + "_out"], out["plain_out"])
        print("%s differs from plain by %.3f = %.1f bars" % (case, d, d / bar))
        assert d > 2 * bar, case
    path = os.path.join(HERE, M.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(tuple(sys.argv[1:]) or ("calls", "seq"))
