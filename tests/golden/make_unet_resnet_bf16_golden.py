"""Generate tests/golden/unet_resnet_bf16_golden.npz (unet_resnet_model.CASES): records of the restated ResnetBlock2D of
tests/unet_resnet_model.py on the CPU, in float64, with its stand-in weights and inputs rounded once to bf16
(tests/unet_resnet_bf16_model.py).

Run:  python tests/golden/make_unet_resnet_bf16_golden.py

Recorded per case, NHWC and thinned with unet_resnet_model.thin: the float64 `conv1 + temb` tap (`*_tap`), the float64 output
(`*_out`), and for the two tensors in that order the noise of the reference arithmetic -- the same module run in fp32 with
every layer's output sent through a bf16 round trip, against the float64 run: max|difference| / max|float64| (`*_noise`) --
and those largest magnitudes (`*_peak`).

Asserted for every case: every noise entry is positive.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import unet_resnet_bf16_model as B  # noqa: E402


def main():
    out = {}
    for case in B.CASES:
        key = B.case_key(case)
        tap, o, noise, peaks = B.record(case)
        assert min(noise) > 0, (key, noise)
        out[key + "_tap"] = B.thin(tap)
        out[key + "_out"] = B.thin(o)
        out[key + "_noise"] = np.array(noise, np.float64)
        out[key + "_peak"] = np.array(peaks, np.float64)
        print("%s: bf16-rounded layers vs float64: tap %.2e of %.3g, output %.2e of %.3g; kept %d + %d values"
              % (key, noise[0], peaks[0], noise[1], peaks[1], out[key + "_tap"].size, out[key + "_out"].size))
    path = os.path.join(HERE, B.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
