"""Generate tests/golden/unet_shell_golden.npz (unet_shell_model.CASES): records of the restated modules of
tests/unet_shell_model.py on the CPU, with their stand-in weights, in float64.

Run:  python tests/golden/make_unet_shell_golden.py

diffusers is absent, so the record is the restatement's own (see unet_shell_model's docstring for what is unverified).

Recorded per case, as unet_shell_model.as_record lays it out and thinned as the VAE golden is (vae_model.thin): the float64
output (`*_out`), the noise of the reference arithmetic -- the same module run in fp32 with every layer's output rounded to
fp16, against the float64 run: max|difference| / max|float64| (`*_noise`) -- and that largest magnitude (`*_peak`).

Asserted for every case: no activation above 65504 / 8 in either run; the noise is positive.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import unet_shell_model as M  # noqa: E402


def main():
    out = {}
    for case in M.CASES:
        key = M.case_key(case)
        o, noise, peak, act = M.record(case)
        assert act < M.ACT_LIMIT, (key, act)
        assert noise > 0, (key, noise)
        out[key + "_out"] = M.thin(o)
        out[key + "_noise"] = np.array([noise], np.float64)
        out[key + "_peak"] = np.array([peak], np.float64)
        print("%s: activation peak %.1f; fp16-rounded layers vs float64: %.2e of %.3g; kept %d values"
              % (key, act, noise, peak, out[key + "_out"].size))
    path = os.path.join(HERE, M.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
