"""Generate tests/golden/unet_attention_golden.npz (unet_attention_model.CASES x MODES): what the tests keep of the float64
records of the stand-in attention module of tests/unet_attention_model.py, on the CPU.

Run:  python tests/golden/make_unet_attention_golden.py

diffusers is absent, so the record is the restatement's own (see unet_attention_model's docstring for what is unverified).

Recorded per case and mode (self, cross): `*_noise`, the noise of the reference arithmetic -- the same module run in fp32 with
every Linear's and the attention's output rounded to fp16, against the float64 run: max|difference| / max|float64| --,
`*_peak`, that largest magnitude, `*_sums`, the record's sum and sum of magnitudes, `*_thin`, every 997th value of it, and
`*_logits`, the scaled logits' largest span within a row and the largest probability.  The GPU test derives the float64
record again and checks it against the sums before it compares.

Asserted for every case and mode: the noise is positive; the scaled logits span at least 8 natural-log units within some row
and some row's largest probability exceeds 0.5 (the attention is not a plain average: a wrong running maximum would show).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import unet_attention_model as M  # noqa: E402


def main():
    out = {}
    for case in M.CASES:
        for mode in M.MODES:
            key = "%s_%s" % (M.case_key(case), mode)
            o, noise, peak, span, top = M.record(case, mode)
            assert noise > 0, (key, noise)
            assert span >= M.MIN_LOGIT_SPAN, (key, span)
            assert top > M.MIN_TOP_PROB, (key, top)
            sums, sample = M.checksums(o)
            out[key + "_noise"] = np.array(noise, np.float64)
            out[key + "_peak"] = np.array(peak, np.float64)
            out[key + "_sums"] = sums
            out[key + "_thin"] = sample
            out[key + "_logits"] = np.array([span, top], np.float64)
            print("%s: fp16-rounded layers vs float64 %.2e of %.3g; logit span %.1f, largest probability %.3f; kept %d values"
                  % (key, noise, peak, span, top, sample.size))
    path = os.path.join(HERE, M.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
