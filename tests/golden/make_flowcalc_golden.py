"""Generate tests/golden/flowcalc_golden.npz: the UNMODIFIED reference FlowCalc.get_flow (src/ebsynth/flow/flow_utils.py)
on CPU in fp32, with the closed-form stand-in GMFlow weights (closed_form.gmflow_param: the published checkpoint is
absent), on closed-form uint8 frames.  Build container only:  python tests/golden/make_flowcalc_golden.py

In this process only: cv2 is a stub whose imwrite records the array, torch.load returns the closed-form state dict, and
.cuda() / .to('cuda') are identities.  Forward_backward_consistency_check is wrapped (not changed) to record the two
unpadded fields it is given, so the margin of every mask pixel comes from the reference's own geometry functions.

Cases (h, w): a = 96 x 128 (no padding), b = 123 x 171 (replicate pads of 2 / 3 rows and 2 / 3 columns, 128 x 176); each
as the pair (frame 0, frame 1) ("ab") and its swap ("ba").  Stored per case and order:
  flow_<case>_<order>   the .npy get_flow saved: (1, 2, h, w) float32
  mask_<case>_<order>   the array handed to cv2.imwrite ((h, w, 1) int64 0 / 255 in the reference), stored as uint8
  margin_<case>_<order> |bwd + warp(fwd, bwd)| - (0.01 (|fwd| + |bwd|) + 0.5) per pixel, float16
  frames_sha256_<case>  sha256 of the two uint8 (h, w, 3) frames (frames_of rebuilds them; the hash pins them)
and the reference's mask dtype / shape and .npy dtype / shape as strings."""
import hashlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import closed_form as cf  # noqa: E402
from _ref_harness import REF_ROOT  # noqa: E402

REF = os.path.join(REF_ROOT, "src", "ebsynth")
CASES = {"a": (96, 128), "b": (123, 171)}


def frames_of(h, w):
    imgs = cf.gmflow_frames(2, h, w)
    return [f.permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).numpy().copy() for f in imgs]


def main():
    sys.dont_write_bytecode = True
    torch.set_num_threads(8)
    written = {}
    cv2 = types.ModuleType("cv2")
    cv2.imwrite = lambda path, arr: written.__setitem__(path, np.array(arr)) or True
    sys.modules["cv2"] = cv2
    # .cuda() / .to('cuda') are identities in this process
    torch.Tensor.cuda = lambda self, *a, **k: self
    to_t, to_m = torch.Tensor.to, torch.nn.Module.to

    def strip(a, k):
        a = tuple(x for x in a if not (isinstance(x, (str, torch.device)) and str(x).startswith("cuda")))
        k = {n: v for n, v in k.items() if not (n == "device" and str(v).startswith("cuda"))}
        return a, k

    torch.Tensor.to = lambda self, *a, **k: to_t(self, *strip(a, k)[0], **strip(a, k)[1])
    torch.nn.Module.to = lambda self, *a, **k: to_m(self, *strip(a, k)[0], **strip(a, k)[1])

    sys.path.insert(0, os.path.join(REF, "deps", "gmflow"))
    from gmflow.gmflow import GMFlow
    probe = GMFlow(feature_channels=128, num_scales=1, upsample_factor=8, num_head=1, attention_type="swin",
                   ffn_dim_expansion=4, num_transformer_layers=6)
    state = {k: cf.gmflow_param(k, tuple(v.shape)) for k, v in probe.state_dict().items()}
    torch.load = lambda *a, **k: dict(state)
    sys.path.insert(0, REF)
    from flow import flow_utils as fu  # the module builds flow_calc = FlowCalc() on import

    seen = []
    check = fu.forward_backward_consistency_check

    def recording_check(fwd, bwd, *a, **k):
        seen.append((fwd.clone(), bwd.clone()))
        return check(fwd, bwd, *a, **k)

    fu.forward_backward_consistency_check = recording_check
    out = {}
    tmp = tempfile.mkdtemp()
    for tag, (h, w) in CASES.items():
        fr = frames_of(h, w)
        out["frames_sha256_" + tag] = hashlib.sha256(np.stack(fr).tobytes()).hexdigest()
        for order, (i, j) in (("ab", (0, 1)), ("ba", (1, 0))):
            path = os.path.join(tmp, "flow_%s_%s.npy" % (tag, order))
            seen.clear()
            ret = fu.flow_calc.get_flow(fr[i], fr[j], path)
            saved = np.load(path)
            mask = written[os.path.splitext(path)[0] + ".png"]
            fwd, bwd = seen[0]
            diff = torch.norm(bwd + fu.flow_warp(fwd, bwd), dim=1)
            thr = 0.01 * (torch.norm(fwd, dim=1) + torch.norm(bwd, dim=1)) + 0.5
            margin = (diff - thr)[0].numpy()
            assert np.array_equal(ret.numpy(), saved)
            assert np.array_equal(mask[..., 0] != 0, margin > 0)
            key = "%s_%s" % (tag, order)
            out["flow_" + key] = saved
            out["mask_" + key] = mask.astype(np.uint8)
            out["margin_" + key] = margin.astype(np.float16)
            out["mask_dtype"], out["mask_shape_suffix"] = str(mask.dtype), str(mask.shape[2:])
            out["npy_dtype"], out["npy_ndim"] = str(saved.dtype), saved.ndim
            print(key, saved.shape, "mean |flow| %.3f, occluded %.4f, min |margin| %.2e"
                  % (float(np.abs(saved).mean()), float((mask != 0).mean()), float(np.abs(margin).min())))
    path = os.path.join(HERE, "flowcalc_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
