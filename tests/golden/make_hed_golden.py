"""Generate tests/golden/hed_golden.npz (hed_model.CASES) and tests/golden/hed_wide_golden.npz (hed_model.WIDE_CASES): records of the UNMODIFIED reference src/ControlNet/annotator/hed/__init__.py on
the CPU.

Run (build container, where the reference tree is present):  python tests/golden/make_hed_golden.py [file name ...]
(no argument: both files; `hed_wide_golden.npz`: that one alone -- an .npz carries the time it was written, so a file that is
not named keeps its bytes).

The reference module imports cv2 (absent) and annotator.util; stubs for exactly what it touches are registered here:
`cv2.resize` / `cv2.INTER_LINEAR` (hed_model.resize_standin, see its docstring for what the stand-in is) and
`annotator.util.annotator_ckpts_path`.  einops is installed.  `HEDdetector.__init__` (which fetches the checkpoint) is
bypassed with object.__new__, the network gets the stand-in weights of tests/hed_model.py, and Tensor.cuda is the identity
while the detector runs.

Recorded per case and frame f < hed_model.GOLDEN_FRAMES[case]:
  *_p{1..5}_f32   the five projections of ControlNetHED_Apache2 in float32
  *_p{1..5}_d64   (the projections of the same network run in float64) - (the float32 record), as float32
  *_logit_f32     the float32 mean of the five resized maps inside HEDdetector.__call__ (recomputed the same way; the uint8
                  map it gives is asserted equal to the detector's own output)
  *_logit_d64     (the mean of the float64 projections resized and averaged in float64) - (the float32 record), as float32
  *_u8            HEDdetector.__call__'s output
plus the state-dict names and shapes of the reference network and the sha256 of the frames and the weights.
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hed_model as M  # noqa: E402

REF = "/root/reference/src/ControlNet/annotator/hed/__init__.py"
SETS = dict(zip(M.GOLDEN_FILES, (M.CASES, M.WIDE_CASES)))


def load_reference():
    sys.dont_write_bytecode = True
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1
    cv2.resize = lambda e, dsize, interpolation=None: M.resize_standin(e, dsize[0], dsize[1], interpolation)
    ann, util = types.ModuleType("annotator"), types.ModuleType("annotator.util")
    util.annotator_ckpts_path = os.path.join(HERE, "no_such_dir")
    ann.util = util
    for name, mod in (("cv2", cv2), ("annotator", ann), ("annotator.util", util)):
        assert name not in sys.modules, name
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_hed", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(names):
    ref = load_reference()
    for name in names:
        record(ref, SETS[name], os.path.join(HERE, name))


def record(ref, cases, path):
    net = ref.ControlNetHED_Apache2().float().eval()
    net.load_state_dict(M.standin_state_dict())
    net64 = copy.deepcopy(net).double()  # the same weight VALUES: the distance between the runs is arithmetic alone
    det = object.__new__(ref.HEDdetector)
    det.netNetwork = net
    peaks = []
    hooks = [c.register_forward_hook(lambda m, i, o: peaks.append(float(o.abs().max())))
             for b in (net.block1, net.block2, net.block3, net.block4, net.block5) for c in b.convs]
    out = {"param_names": np.array(list(net.state_dict().keys())),
           "param_shapes": np.array(["x".join(map(str, v.shape)) for v in net.state_dict().values()]),
           "weights_sha256": np.array(M.weights_digest())}
    torch.Tensor.cuda, saved = (lambda self, *a, **k: self), torch.Tensor.cuda
    try:
        for case in cases:
            fr = M.frames(case)
            out[M.case_key(case) + "_sha256"] = np.array(M.digest(fr))
            n, H, W = case
            for f in range(M.GOLDEN_FRAMES[case]):
                key = "%s_f%d" % (M.case_key(case), f)
                del peaks[:]
                with torch.no_grad():
                    u8 = det(fr[f])
                    x = torch.from_numpy(fr[f].copy()).float().permute(2, 0, 1)[None]
                    p32 = [p[0, 0].numpy() for p in net(x)]
                    peak = max(peaks)
                    p64 = [p[0, 0].numpy() for p in net64(x.double())]
                l32, u8_again = M.fuse_u8(p32, H, W)
                assert np.array_equal(u8, u8_again), key
                l64 = M.fuse_logit64(p64, H, W)
                for k in range(5):
                    out["%s_p%d_f32" % (key, k + 1)] = p32[k]
                    out["%s_p%d_d64" % (key, k + 1)] = (p64[k] - p32[k].astype(np.float64)).astype(np.float32)
                out[key + "_logit_f32"] = l32
                out[key + "_logit_d64"] = (l64 - l32.astype(np.float64)).astype(np.float32)
                out[key + "_u8"] = u8
                band = M.guard_band(l64)
                print("%s: activation peak %.0f, logit %.2f .. %.2f, |f32 - f64| logit %.2e sides %.2e, %d uint8 levels, "
                      "%.1f %% of pixels in the guard band"
                      % (key, peak, l64.min(), l64.max(), np.abs(l32 - l64).max(),
                         max(np.abs(a - b).max() for a, b in zip(p32, p64)), len(np.unique(u8)), 100 * band.mean()))
                assert band.mean() <= M.GUARD_CAP, key
    finally:
        torch.Tensor.cuda = saved
        for h in hooks:
            h.remove()
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main(sys.argv[1:] or list(M.GOLDEN_FILES))
