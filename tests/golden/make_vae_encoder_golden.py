"""Generate tests/golden/vae_encoder_golden.npz and tests/golden/vae_encoder_names.txt (vae_encoder_model.CASES): records of
the restated AutoencoderKL encoder of tests/vae_encoder_model.py on the CPU, with its stand-in weights, in float64.

Run:  python tests/golden/make_vae_encoder_golden.py

diffusers is absent, so the record is the restatement's own (see vae_encoder_model's docstring for what is unverified).

Recorded: the encoder.* and quant_conv.* state-dict names and shapes (the text file); per case the float64 taps
vae_encoder_model.TAPS as vae_model.thin keeps them, the float64 parameters of the distribution, whole, and the noise of
the reference arithmetic: the same module run in fp32 with every layer's output rounded to fp16, against the float64 run
-- per tap and for the parameters max|difference| / max|float64| (`*_noise`, in TAPS order, the parameters last; `*_peak`:
those largest magnitudes).

Asserted for every case: no activation above 65504 / 8 in either run; every noise entry is positive; logvar stays inside
(-30, 20) in both runs, so the clamp decides nothing here (the kernel test has hand-made elements on both sides of it).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vae_encoder_model as EM  # noqa: E402
from make_vae_golden import Peak  # noqa: E402


def record(net64, net32, cases):
    """the arrays of the module docstring for every case"""
    out = {}
    for case in cases:
        key = EM.case_key(case)
        x = EM.images(case)
        peak, peak32 = Peak(net64), Peak(net32)
        t64, t16 = {}, {}
        with torch.no_grad():
            p64 = net64.encode_forward(x.double(), t64)
            p16 = net32.encode_forward(x.float(), t16, EM.round16)
        peak.remove()
        peak32.remove()
        assert peak.peak < EM.ACT_LIMIT and peak32.peak < EM.ACT_LIMIT, (key, peak.peak, peak32.peak)
        noise, peaks = [], []
        for t in EM.TAPS:
            a64 = t64[t].numpy()
            peaks.append(float(np.abs(a64).max()))
            noise.append(float(np.abs(t16[t].double().numpy() - a64).max() / peaks[-1]))
            out["%s_%s" % (key, t)] = EM.thin(a64)
        peaks.append(float(p64.abs().max()))
        noise.append(float((p16.double() - p64).abs().max() / peaks[-1]))
        assert min(noise) > 0, (key, noise)
        for p in (p64, p16):
            assert -30 < float(p[:, 4:].min()) and float(p[:, 4:].max()) < 20, (key, float(p[:, 4:].min()), float(p[:, 4:].max()))
        assert p64.shape == (case[0], 8, case[1] // 8, case[2] // 8), (key, p64.shape)
        out[key + "_noise"] = np.array(noise, np.float64)
        out[key + "_peak"] = np.array(peaks, np.float64)
        out[key + "_parameters"] = p64.numpy()
        print("%s: activation peak %.1f; fp16-rounded layers vs float64: worst tap %.2e (%s), parameters %.2e; logvar in "
              "[%.2f, %.2f]" % (key, max(peak.peak, peak32.peak), max(noise[:-1]), EM.TAPS[int(np.argmax(noise[:-1]))], noise[-1],
                                float(p64[:, 4:].min()), float(p64[:, 4:].max())))
    return out


def main():
    net64 = EM.build(torch.float64)
    net32 = EM.build(torch.float32)
    with open(os.path.join(HERE, EM.NAMES_FILE), "w") as f:
        for name, shape in EM.encoder_names_shapes(net64):
            f.write("%s %s\n" % (name, "x".join(map(str, shape))))
    out = record(net64, net32, EM.CASES)
    path = os.path.join(HERE, EM.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "vae_golden.npz"))


if __name__ == "__main__":
    main()
