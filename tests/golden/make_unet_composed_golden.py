"""Generate tests/golden/unet_composed_golden.npz: float64 records of the composed stand-in UNet + ControlNet of
tests/unet_composed_model.py on the CPU.

Run:  python tests/golden/make_unet_composed_golden.py        (about a minute; 4 GB of memory)

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
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import unet_composed_model as M  # noqa: E402


def main():
    models = M.Models()
    nets = (models.u64, models.c64, models.u32, models.c32)
    params = M.parameters_of(models.u64) + M.parameters_of(models.c64)
    assert params <= M.PARAM_LIMIT, params
    seen = [0.0]

    def see(m, i, o):
        if isinstance(o, torch.Tensor):
            seen[0] = max(seen[0], float(o.detach().abs().max()))
    hooks = [m.register_forward_hook(see) for net in nets for m in net.modules() if not list(m.children())]
    out = M.derive(models)
    for h in hooks:
        h.remove()
    assert seen[0] < M.ACT_LIMIT, seen[0]
    print("%d parameters; largest activation %.1f" % (params, seen[0]))
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
    main()
