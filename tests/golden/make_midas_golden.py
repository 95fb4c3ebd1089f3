"""Generate tests/golden/midas_golden.npz (midas_model.CASES): records of the reference's MiDaS annotator on the CPU --
src/ControlNet/annotator/midas/midas/dpt_depth.py, blocks.py and vit.py UNMODIFIED, and MidasDetector.__call__ of
src/ControlNet/annotator/midas/__init__.py UNMODIFIED -- around the restated backbone of tests/midas_model.py.

Run (build container, where the reference tree is present):  python tests/golden/make_midas_golden.py

`timm` is absent: a stub module is registered whose create_model("vit_base_resnet50_384") returns
midas_model.VisionTransformer, so the record is the reference's reassemble, decoder and head around a backbone that could not
be compared with the real one.  `cv2` is absent: a stub with midas_model.sobel as Sobel.  `.api` (which needs the annotator
package and a checkpoint) is replaced by a stub; the detector gets its model set by hand.  Tensor.cuda is the identity while
the detector runs.  The network carries the stand-in weights of midas_model and runs in eval mode, in float32 and as a
float64 copy of the same weight VALUES.

Recorded: the reference's state-dict names and shapes; per case the sha256 of the frames, the taps midas_model.TAPS as
midas_model.thin keeps them, the fp32 depth at every DEPTH_STRIDE-th row and column (in full for FULL_DEPTH_CASES), the detector's two uint8 maps in full,
and the reference's own rounding noise: per tap and for the depth max|fp32 - float64| / max|float64| (`*_noise`, in TAPS
order, the depth last; `*_peak`: those largest magnitudes), and for the two uint8 maps the share of values that differ between the runs and the largest
difference (`*_u8_noise`: depth share, depth max, normal share, normal max).

Asserted for every case and frame: min < max; pixels on both sides of bg_th; the depth image is not constant over any quarter
of the frame; no activation above 500 (half of what the planes hold at scale 64 is 507); the two runs' uint8 maps differ in
under 0.5 % of their values, by 1 at most; the restated tail equals the detector's output.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import midas_model as M  # noqa: E402

REF_MIDAS = "/root/reference/src/ControlNet/annotator/midas"


def load_reference():
    """-> (DPTDepthModel, MidasDetector) of the reference, with the stubs described above"""
    sys.dont_write_bytecode = True
    assert "timm" not in sys.modules and "cv2" not in sys.modules
    timm = types.ModuleType("timm")

    def create_model(name, pretrained=False):
        assert name == "vit_base_resnet50_384" and not pretrained
        return M.VisionTransformer()
    timm.create_model = create_model
    sys.modules["timm"] = timm
    cv2 = types.ModuleType("cv2")
    cv2.CV_32F = 5

    def Sobel(src, ddepth, dx, dy, ksize=3):
        assert ddepth == cv2.CV_32F and ksize == 3 and src.dtype in (np.float32, np.float64)
        return M.sobel(src, dx, dy)
    cv2.Sobel = Sobel
    sys.modules["cv2"] = cv2
    for name, path in (("ref_midas_annotator", REF_MIDAS), ("ref_midas_annotator.midas", os.path.join(REF_MIDAS, "midas"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    dpt = importlib.import_module("ref_midas_annotator.midas.dpt_depth")
    api = types.ModuleType("ref_midas_annotator.api")
    api.MiDaSInference = None
    sys.modules["ref_midas_annotator.api"] = api
    spec = importlib.util.spec_from_file_location("ref_midas_annotator.detector", os.path.join(REF_MIDAS, "__init__.py"))
    det = importlib.util.module_from_spec(spec)
    det.__package__ = "ref_midas_annotator"
    spec.loader.exec_module(det)
    return dpt.DPTDepthModel, det.MidasDetector


class Taps:
    """the tap tensors and the largest |activation| of one forward, by hooks on the unmodified modules"""

    def __init__(self, net):
        self.t, self.peak, self.hooks = {}, 0.0, []
        add = lambda m, fn: self.hooks.append(m.register_forward_hook(fn))  # noqa: E731
        nhwc = lambda o: o.detach().permute(0, 2, 3, 1).clone()  # noqa: E731
        keep = lambda name, f=nhwc: (lambda m, i, o: self.t.__setitem__(name, f(o)))  # noqa: E731
        tok = lambda o: o.detach().clone()  # noqa: E731
        vit, bb = net.pretrained.model, net.pretrained.model.patch_embed.backbone
        add(bb.stem.norm, keep("stem"))
        for k in range(3):
            add(bb.stages[k], keep("stage%d" % k))
        for k in (0, 8, 11):
            add(vit.blocks[k], keep("tokens%d" % k, tok))
        add(net.pretrained.act_postprocess3[3], keep("layer3"))
        add(net.pretrained.act_postprocess4[4], keep("layer4"))
        for k in (1, 2, 3, 4):
            add(getattr(net.scratch, "refinenet%d" % k), keep("path_%d" % k))

        def peak(m, i, o):
            self.peak = max(self.peak, float(o.detach().abs().max()))
        for m in net.modules():
            if not list(m.children()):
                add(m, peak)

    def remove(self):
        for h in self.hooks:
            h.remove()


def detect(Detector, net, frame):
    """the reference detector's own __call__ on one frame, on the CPU"""
    det = Detector.__new__(Detector)
    det.model = net
    torch.Tensor.cuda, saved = (lambda self, *a, **k: self), torch.Tensor.cuda
    try:
        return det(frame)
    finally:
        torch.Tensor.cuda = saved


def main():
    DPTDepthModel, Detector = load_reference()
    net = DPTDepthModel(path=None, backbone="vitb_rn50_384", non_negative=True)
    names_shapes = M.module_names_shapes(net)
    net.load_state_dict(M.standin_state_dict(names_shapes))
    net = net.float().eval()
    # (a second instance, not a deep copy: the reference's hooks write into one module-level dict that a copy would not read)
    net64 = DPTDepthModel(path=None, backbone="vitb_rn50_384", non_negative=True)
    net64.load_state_dict(M.standin_state_dict(names_shapes, torch.float64))
    net64 = net64.double().eval()
    out = {"param_names": np.array([k for k, _ in names_shapes]),
           "param_shapes": np.array(["x".join(map(str, s)) for _, s in names_shapes]),
           "weights_sha256": np.array(M.digest(*[v.numpy() for v in net.state_dict().values()]))}
    for case in M.CASES:
        key = M.case_key(case)
        fr = M.frames(case)
        out[key + "_sha256"] = np.array(M.digest(fr))
        # frame by frame, as the reference's detector runs (the CPU kernels' summation order depends on the batch size)
        runs = []
        with torch.no_grad():
            for f in range(case[0]):
                taps = Taps(net)
                a = net(M.network_input(fr[f:f + 1]))
                taps.remove()
                taps64 = Taps(net64)
                b = net64(M.network_input(fr[f:f + 1], torch.float64))
                taps64.remove()
                runs.append((a, b, taps, taps64))
        d32, d64 = torch.cat([r[0] for r in runs]), torch.cat([r[1] for r in runs])
        taps, taps64 = runs[0][2], runs[0][3]
        taps.peak = max(r[2].peak for r in runs)
        for t in M.TAPS:
            taps.t[t] = torch.cat([r[2].t[t] for r in runs])
            taps64.t[t] = torch.cat([r[3].t[t] for r in runs])
        d32, d64 = d32.numpy(), d64.numpy()
        assert taps.peak < 500, (key, taps.peak)
        noise, peaks = [], []
        for t in M.TAPS:
            a32, a64 = taps.t[t].numpy(), taps64.t[t].numpy()
            peaks.append(float(np.abs(a64).max()))
            noise.append(float(np.abs(a32 - a64).max() / peaks[-1]))
            out["%s_%s" % (key, t)] = M.thin(a32)
        peaks.append(float(np.abs(d64).max()))
        noise.append(float(np.abs(d32 - d64).max() / peaks[-1]))
        out[key + "_noise"] = np.array(noise, np.float64)
        out[key + "_peak"] = np.array(peaks, np.float64)
        out[key + "_depth"] = M.thin_depth(d32)
        if case in M.FULL_DEPTH_CASES:
            out[key + "_depth_full"] = d32
        dimgs, nimgs, u8_noise = [], [], np.zeros(4)
        for f in range(case[0]):
            with torch.no_grad():
                dimg, nimg = detect(Detector, net, fr[f])
            own_d, own_n = M.tail(d32[f])
            assert np.array_equal(dimg, own_d) and np.array_equal(nimg, own_n), key
            d64_img, n64_img = M.tail(d64[f].astype(np.float32))
            dd = np.abs(dimg.astype(int) - d64_img.astype(int))
            dn = np.abs(nimg.astype(int) - n64_img.astype(int))
            u8_noise = np.maximum(u8_noise, [(dd > 0).mean(), dd.max(), (dn > 0).mean(), dn.max()])
            H, W = dimg.shape
            pt = (d32[f] - d32[f].min()) / (d32[f].max() - d32[f].min())
            assert d32[f].min() < d32[f].max(), key
            assert (pt < M.BG_TH).any() and (pt >= M.BG_TH).any(), (key, f, float((pt < M.BG_TH).mean()))
            for q in (dimg[:H // 2, :W // 2], dimg[:H // 2, W // 2:], dimg[H // 2:, :W // 2], dimg[H // 2:, W // 2:]):
                assert q.min() < q.max(), (key, f)
            dimgs.append(dimg)
            nimgs.append(nimg)
            print("%s frame %d: depth %.3f .. %.3f, %.1f %% below bg_th" % (key, f, d32[f].min(), d32[f].max(),
                                                                           100 * float((pt < M.BG_TH).mean())))
        out[key + "_u8_noise"] = u8_noise
        out[key + "_depth_image"] = np.stack(dimgs)
        out[key + "_normal_image"] = np.stack(nimgs)
        print("%s: activation peak %.0f; fp32 vs float64: worst tap %.2e (%s), depth %.2e; uint8 maps differ in %.3f %% / "
              "%.3f %% of their values, by at most %d / %d" % (key, taps.peak, max(noise[:-1]), M.TAPS[int(np.argmax(noise[:-1]))],
                                                               noise[-1], 100 * u8_noise[0], 100 * u8_noise[2], u8_noise[1],
                                                               u8_noise[3]))
        assert u8_noise[0] < 0.005 and u8_noise[2] < 0.005 and u8_noise[1] <= 1 and u8_noise[3] <= 1, (key, u8_noise)
    path = os.path.join(HERE, M.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
