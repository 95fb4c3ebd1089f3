"""Generate tests/golden/keyframe_small_golden.npz by running the UNMODIFIED reference `get_keyframe_ind`
(src/keyframe_selection.py) on CPU on videos whose short side is at or below 512, where its resize_image enlarges: through
INTER_LANCZOS4 (k > 1) or through INTER_AREA on a geometry whose rounding to multiples of 64 grows a side.  cv2 is absent: the
stand-in module of tests/resize_model.py serves the synthetic frames and dispatches its resize on the interpolation flag the
reference passes -- so, as with make_keyframe_golden.py, the golden pins what the reference does AROUND cv2's calls (which flag
it picks, the frame loop, numpy2tensor, F.mse_loss in fp32, the greedy selection) on top of the numpy restatements, not
OpenCV itself.  The frames are generated at test time (keyframe_model.synthetic_frames), not stored.  Build container only:
    python tests/golden/make_keyframe_small_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_harness  # noqa: E402
import keyframe_model as KM  # noqa: E402
import resize_model as R  # noqa: E402


def main():
    torch.set_num_threads(8)
    sys.modules.setdefault("cv2", R.standin_cv2(np.zeros((1, 8, 8, 3), np.uint8)))
    _, _, _, ut = _ref_harness.load_reference()
    import src.keyframe_selection as ks
    curve, sizes = [], []

    def recording_mse_loss(a, b):
        loss = torch.nn.functional.mse_loss(a, b)
        assert loss.dtype == torch.float32
        curve.append(float(loss))
        sizes.append(tuple(a.shape[-2:]))
        return loss

    ks.F = types.SimpleNamespace(mse_loss=recording_mse_loss)
    torch.Tensor.cuda, saved = (lambda self, *a, **k: self), torch.Tensor.cuda
    out = dict(names=np.array(sorted(R.SMALL_GOLDEN_CASES)))
    try:
        for name, (seed, n, H0, W0, mininterv, maxinterv) in R.SMALL_GOLDEN_CASES.items():
            frames = KM.synthetic_frames(seed, n, H0, W0)
            ks.cv2 = ut.cv2 = R.standin_cv2(frames)
            del curve[:], sizes[:]
            keys = ks.get_keyframe_ind("synthetic.mp4", 10 ** 10, mininterv, maxinterv)
            err = np.array([0.0] + curve)
            assert len(err) == n and len(set(sizes)) == 1
            # no two competing values within 1e-3 relative: the fp32 summation order of mse_loss cannot change an argmax
            live = np.sort(err[1:])
            assert (np.diff(live) > 1e-3 * live[1:]).all(), (name, live)
            H, W, how = R.dispatch(H0, W0, 512)
            assert sizes[0] == (H, W), (name, sizes[0])
            out[name + "_args"] = np.array([seed, n, H0, W0, mininterv, maxinterv], np.int64)
            out[name + "_size"] = np.array([H, W], np.int64)
            out[name + "_err"] = err
            out[name + "_keys"] = np.array(keys, np.int64)
            print(name, how, (H, W), "keys", list(keys))
    finally:
        torch.Tensor.cuda = saved
    np.savez_compressed(os.path.join(HERE, "keyframe_small_golden.npz"), **out)
    print("wrote keyframe_small_golden.npz", sum(v.nbytes for v in out.values()), "bytes raw")


if __name__ == "__main__":
    main()
