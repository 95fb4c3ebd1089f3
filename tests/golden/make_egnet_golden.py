"""Generate tests/golden/egnet_golden.npz (egnet_model.CASES) and tests/golden/egnet_wide_golden.npz (egnet_model.WIDE_CASES):
records of the UNMODIFIED reference src/EGNet/model.py (+ resnet.py) with src/utils.py's cv2sod and Dilate on the CPU.

Run (build container, where the reference tree is present):  python tests/golden/make_egnet_golden.py [file name ...]
(no argument: both files; an .npz carries the time it was written, so a file that is not named keeps its bytes).

src/utils.py imports cv2 (absent): an empty stub module is registered for it -- nothing this script calls touches it.
Tensor.cuda is the identity while utils.get_saliency runs.  The network gets the stand-in weights of tests/egnet_model.py
and runs in eval mode, once in float32 on utils.cv2sod's tensor and once as a float64 copy (the same weight VALUES) on
egnet_model.cv2sod64's, so the distance between the two runs is the arithmetic of the whole float32 pipeline.
utils.get_saliency squeezes the batch axis away for a single frame, so the saliency map is formed here as its last line
does, with utils.Dilate, and compared with get_saliency's own output where the case has more than one frame.

Recorded per case (all its frames):
  *_logit_f32 / _d64     up_sal_final[-1] at cv2sod's size, (n, h, w): float32, and (float64 - float32) as float32
  *_saliency_f32 / _d64  1 - Dilate(7)(sigmoid(logit)), (n, 1, h, w), likewise
  *_{tap}_f32 / _d64     the taps egnet_model.TAPS as NHWC, every 16th channel: the stem after its ReLU, layer1..4, the five
                         convert outputs, merge1's edge_feature[0] and four sal_feature, merge2's fused tmp_fea
plus the state-dict names and shapes of the reference network and the sha256 of the frames and the weights.

Asserted for every case, on the name-seeded weights: peak activation < 500; at least 10 % of the saliency map exactly 0,
at least 10 % above 0.9, at least 5 % in between.
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
import egnet_model as M  # noqa: E402

REF_ROOT = "/root/reference"
SETS = dict(zip(M.GOLDEN_FILES, (M.CASES, M.WIDE_CASES)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    sys.dont_write_bytecode = True
    assert "cv2" not in sys.modules
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, os.path.join(REF_ROOT, "src", "EGNet"))  # model.py imports its siblings resnet and vgg
    model = _load("reference_egnet_model", os.path.join(REF_ROOT, "src", "EGNet", "model.py"))
    utils = _load("reference_utils", os.path.join(REF_ROOT, "src", "utils.py"))
    return model, utils


class Taps:
    """the tap tensors and the largest |activation| of one forward, by hooks on the unmodified modules"""

    def __init__(self, net):
        self.t, self.peak, self.hooks = {}, 0.0, []
        add = lambda m, fn: self.hooks.append(m.register_forward_hook(fn))  # noqa: E731
        keep = lambda name: (lambda m, i, o: self.t.__setitem__(name, o.detach().clone()))  # noqa: E731
        add(net.base.relu, keep("stem"))
        for k in range(1, 5):
            add(getattr(net.base, "layer%d" % k), keep("layer%d" % k))
        add(net.convert, lambda m, i, o: self.t.update(("convert%d" % k, v.detach().clone()) for k, v in enumerate(o)))

        def merge1(m, i, o):
            self.t["edge_feature"] = o[1][0].detach().clone()
            self.t.update(("sal_feature%d" % k, v.detach().clone()) for k, v in enumerate(o[3]))
        add(net.merge1, merge1)
        self.hooks.append(net.merge2.final_score.register_forward_pre_hook(
            lambda m, i: self.t.__setitem__("tmp_fea", i[0].detach().clone())))

        def peak(m, i, o):
            self.peak = max(self.peak, float(o.detach().abs().max()))
        for m in net.modules():
            if not list(m.children()):
                add(m, peak)

    def remove(self):
        for h in self.hooks:
            h.remove()


def thin(t):
    """NCHW tap -> NHWC numpy, every TAP_STRIDE-th channel"""
    return t[:, ::M.TAP_STRIDE].permute(0, 2, 3, 1).contiguous().numpy()


def record(model, utils, cases, path):
    net = model.build_model("resnet")
    net.load_state_dict(M.standin_state_dict())
    net = net.float().eval()
    net64 = copy.deepcopy(net).double()
    dil, dil64 = utils.Dilate(kernel_size=M.K_DILATE), utils.Dilate(kernel_size=M.K_DILATE)
    dil64.gaussian_filter = dil64.gaussian_filter.double()
    sd = net.state_dict()
    assert list(sd) == list(M.param_shapes()) and all(tuple(v.shape) == M.param_shapes()[k] for k, v in sd.items())
    out = {"param_names": np.array(list(sd.keys())),
           "param_shapes": np.array(["x".join(map(str, v.shape)) for v in sd.values()]),
           "weights_sha256": np.array(M.weights_digest())}
    for case in cases:
        key = M.case_key(case)
        fr = M.frames(case)
        out[key + "_sha256"] = np.array(M.digest(fr))
        with torch.no_grad():
            x32 = torch.cat([utils.cv2sod(f) for f in fr], 0)
            x64 = M.cv2sod64(fr)
            assert torch.equal(x32, M.cv2sod64(fr, torch.float32)) and float((x32.double() - x64).abs().max()) < 1e-4
            taps = Taps(net)
            l32 = net(x32)[2][-1]
            taps.remove()
            taps64 = Taps(net64)
            l64 = net64(x64)[2][-1]
            taps64.remove()
            s32 = 1 - dil(torch.sigmoid(l32))
            s64 = 1 - dil64(torch.sigmoid(l64))
            if case[0] > 1:
                torch.Tensor.cuda, saved = (lambda self, *a, **k: self), torch.Tensor.cuda
                try:
                    own = utils.get_saliency(list(fr), net, dil)
                finally:
                    torch.Tensor.cuda = saved
                assert torch.equal(own, s32), key
        pairs = [("logit", l32[:, 0].numpy(), l64[:, 0].numpy()), ("saliency", s32.numpy(), s64.numpy())]
        pairs += [(t, thin(taps.t[t]), thin(taps64.t[t])) for t in M.TAPS]
        for name, a32, a64 in pairs:
            out["%s_%s_f32" % (key, name)] = a32
            out["%s_%s_d64" % (key, name)] = (a64 - a32.astype(np.float64)).astype(np.float32)
        s = s32.numpy()
        zeros, high = float((s == 0).mean()), float((s > 0.9).mean())
        between = float(((s > 0) & (s <= 0.9)).mean())
        print("%s: activation peak %.0f, logit %.2f .. %.2f (std %.2f), saliency: %.0f %% exactly 0, %.0f %% above 0.9, "
              "%.0f %% in between; |f32 - f64| logit %.2e saliency %.2e, worst tap %.2e"
              % (key, taps.peak, l64.min(), l64.max(), l64.std(), 100 * zeros, 100 * high, 100 * between,
                 float((l32.double() - l64).abs().max()), float((s32.double() - s64).abs().max()),
                 max(float(np.abs(a - b).max()) for _, a, b in pairs[2:])))
        assert taps.peak < 500, (key, taps.peak)
        assert zeros >= 0.10 and high >= 0.10 and between >= 0.05, (key, zeros, high, between)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


def main(names):
    model, utils = load_reference()
    for name in names:
        record(model, utils, SETS[name], os.path.join(HERE, name))


if __name__ == "__main__":
    main(sys.argv[1:] or list(M.GOLDEN_FILES))
