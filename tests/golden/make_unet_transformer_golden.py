"""Generate tests/golden/unet_transformer_golden.npz (unet_transformer_model.CASES): records of the restated
Transformer2DModel of tests/unet_transformer_model.py on the CPU, with its stand-in weights and stand-in attention, in float64.

Run:  python tests/golden/make_unet_transformer_golden.py

diffusers is absent, so the record is the restatement's own (see unet_transformer_model's docstring for what is unverified).

Recorded per case, NHWC and thinned as the VAE golden is (vae_model.thin): the float64 GEGLU output of the first block
(`*_tap`, (n, H, W, inner)), the float64 output (`*_out`), and for the two tensors in that order the noise of the reference
arithmetic -- the same module run in fp32 with every layer's output rounded to fp16, against the float64 run:
max|difference| / max|float64| (`*_noise`) -- and those largest magnitudes (`*_peak`).

Asserted for every case: no activation above 65504 / 8 in either run; every noise entry is positive.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import unet_transformer_model as M  # noqa: E402


def main():
    out = {}
    for case in M.CASES:
        key = M.case_key(case)
        tap, o, noise, peaks, act = M.record(case)
        assert act < M.ACT_LIMIT, (key, act)
        assert min(noise) > 0, (key, noise)
        out[key + "_tap"] = M.thin(tap)
        out[key + "_out"] = M.thin(o)
        out[key + "_noise"] = np.array(noise, np.float64)
        out[key + "_peak"] = np.array(peaks, np.float64)
        print("%s: activation peak %.1f; fp16-rounded layers vs float64: tap %.2e of %.3g, output %.2e of %.3g; kept %d + %d values"
              % (key, act, noise[0], peaks[0], noise[1], peaks[1], out[key + "_tap"].size, out[key + "_out"].size))
    path = os.path.join(HERE, M.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
