"""Generate tests/golden/vae_golden.npz and tests/golden/vae_decoder_names.txt (vae_model.CASES): records of the restated
AutoencoderKL decoder of tests/vae_model.py on the CPU, with its stand-in weights, in float64.

Run:  python tests/golden/make_vae_golden.py

diffusers is absent, so the record is the restatement's own (see vae_model's docstring for what is unverified).

Recorded: the state-dict names and shapes (the text file); per case the float64 taps vae_model.TAPS as vae_model.thin keeps
them, the float64 image at every IMAGE_STRIDE-th row and column, the whole uint8 image of the reference's tensor2numpy, and
the noise of the reference arithmetic: the same module run in fp32 with every layer's output rounded to fp16, against the
float64 run -- per tap and for the image max|difference| / max|float64| (`*_noise`, in TAPS order, the image last; `*_peak`:
those largest magnitudes), and for the uint8 image the share of values one level from the float64 run's (`*_u8_share`).

Asserted for every case: no activation above 65504 / 8 in either run; the two uint8 images are never 2 or more apart; every
noise entry and the uint8 share are positive; the image is not constant and uses both halves of the uint8 range.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vae_model as M  # noqa: E402


class Peak:
    """the largest |output| of any leaf module during a forward"""

    def __init__(self, net):
        self.peak = 0.0
        self.hooks = [m.register_forward_hook(self.see) for m in net.modules() if not list(m.children())]

    def see(self, m, i, o):
        self.peak = max(self.peak, float(o.detach().abs().max()))

    def remove(self):
        for h in self.hooks:
            h.remove()


def record(net64, net32, cases, whole_u8=lambda case: True):
    """the arrays of the module docstring for every case; whole_u8(case) false: without that case's whole uint8 image"""
    out = {}
    for case in cases:
        key = M.case_key(case)
        z = M.latents(case)
        peak = Peak(net64)
        peak32 = Peak(net32)
        t64, t16 = {}, {}
        with torch.no_grad():
            img64 = net64(z.double(), t64)
            img16 = net32(z.float(), t16, M.round16)
        peak.remove()
        peak32.remove()
        assert peak.peak < M.ACT_LIMIT and peak32.peak < M.ACT_LIMIT, (key, peak.peak, peak32.peak)
        noise, peaks = [], []
        for t in M.TAPS:
            a64 = t64[t].numpy()
            peaks.append(float(np.abs(a64).max()))
            noise.append(float(np.abs(t16[t].double().numpy() - a64).max() / peaks[-1]))
            out["%s_%s" % (key, t)] = M.thin(a64)
        peaks.append(float(img64.abs().max()))
        noise.append(float((img16.double() - img64).abs().max() / peaks[-1]))
        u64, u16 = M.tensor2numpy(img64), M.tensor2numpy(img16)
        d = np.abs(u64.astype(int) - u16.astype(int))
        assert d.max() <= 1, (key, d.max())
        share = float((d == 1).mean())
        assert min(noise) > 0 and share > 0, (key, noise, share)
        assert u64.min() < 64 and u64.max() > 192 and u64.std() > 20, (key, u64.min(), u64.max(), u64.std())
        out[key + "_noise"] = np.array(noise, np.float64)
        out[key + "_peak"] = np.array(peaks, np.float64)
        out[key + "_u8_share"] = np.array(share, np.float64)
        out[key + "_image"] = M.thin_image(img64)
        if whole_u8(case):
            out[key + "_image_u8"] = u64
        print("%s: activation peak %.1f; fp16-rounded layers vs float64: worst tap %.2e (%s), image %.2e; uint8 one apart %.3f %%; "
              "clipped %.1f %%" % (key, max(peak.peak, peak32.peak), max(noise[:-1]), M.TAPS[int(np.argmax(noise[:-1]))],
                                   noise[-1], 100 * share, 100 * float(((u64 == 0) | (u64 == 255)).mean())))
    return out


def main():
    net64 = M.build(torch.float64)
    net32 = M.build(torch.float32)
    names_shapes = M.module_names_shapes(net64)
    with open(os.path.join(HERE, M.NAMES_FILE), "w") as f:
        for name, shape in names_shapes:
            f.write("%s %s\n" % (name, "x".join(map(str, shape))))
    out = record(net64, net32, M.CASES)
    path = os.path.join(HERE, M.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
