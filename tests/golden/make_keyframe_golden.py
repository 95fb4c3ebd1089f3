"""Generate tests/golden/keyframe_golden.npz by running the UNMODIFIED reference `get_keyframe_ind`
(src/keyframe_selection.py) on CPU.  cv2 is absent: a stand-in module (tests/keyframe_model.py standin_cv2) serves the
synthetic frames through the VideoCapture protocol, and its resize / GaussianBlur are the numpy model's -- so the golden pins
what the reference does AROUND those two calls (the frame loop, numpy2tensor, F.mse_loss in fp32, the greedy selection with
its sentinels) on top of the model, not OpenCV itself.  Tensor.cuda is the identity while it runs; F.mse_loss is wrapped (not
changed) to record the error curve, which the function does not return.  Build container only:
    python tests/golden/make_keyframe_golden.py
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
import keyframe_model as M  # noqa: E402


def main():
    torch.set_num_threads(8)
    frames = M.synthetic_frames(M.GOLDEN_SEED, M.GOLDEN_FRAMES)
    sys.modules.setdefault("cv2", M.standin_cv2(frames))
    _, _, _, ut = _ref_harness.load_reference()
    import src.keyframe_selection as ks
    curve = []

    def recording_mse_loss(a, b):
        loss = torch.nn.functional.mse_loss(a, b)
        assert loss.dtype == torch.float32
        curve.append(float(loss))
        return loss

    ks.F = types.SimpleNamespace(mse_loss=recording_mse_loss)
    torch.Tensor.cuda, saved = (lambda self, *a, **k: self), torch.Tensor.cuda
    out = dict(seed=np.int64(M.GOLDEN_SEED), frames=np.int64(M.GOLDEN_FRAMES), frame_size=np.array(frames.shape[1:3]),
               names=np.array(sorted(M.GOLDEN_CASES)))
    try:
        for name, (served, reported, lastframen, mininterv, maxinterv) in M.GOLDEN_CASES.items():
            ks.cv2 = ut.cv2 = M.standin_cv2(frames[:served], reported)
            del curve[:]
            keys = ks.get_keyframe_ind("synthetic.mp4", lastframen, mininterv, maxinterv)
            err = np.array([0.0] + curve)
            # no two competing values within 1e-3 relative: the fp32 summation order of mse_loss cannot change an argmax
            live = np.sort(err[1:])
            if len(live) > 1:
                assert (np.diff(live) > 1e-3 * live[1:]).all(), (name, live)
            if mininterv != maxinterv:
                assert len(err) == min(served, reported, lastframen), (name, len(err))
            out[name + "_args"] = np.array([served, reported, lastframen, mininterv, maxinterv], np.int64)
            out[name + "_err"] = err
            out[name + "_keys"] = np.array(keys, np.int64)
            print(name, "n =", len(err), "keys", list(keys))
    finally:
        torch.Tensor.cuda = saved
    np.savez_compressed(os.path.join(HERE, "keyframe_golden.npz"), **out)
    print("wrote keyframe_golden.npz", sum(v.nbytes for v in out.values()), "bytes raw")


if __name__ == "__main__":
    main()
