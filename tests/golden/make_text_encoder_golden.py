"""Generate tests/golden/text_encoder_golden.npz (clip_text_model.CASES): records of the restated CLIP text model of
tests/clip_text_model.py on the CPU, with its stand-in weights, in float64.

Run:  python tests/golden/make_text_encoder_golden.py

The restatement equals transformers' CLIPTextModel in float64 to 1e-9 (tests/test_text_encoder_cpu.py checks it where
transformers imports), so the records are the real module's on these weights.

Recorded per case, for layer 0's attention output (before out_proj), layer 0's quick_gelu(fc1), hidden_states[-2], the last
hidden state and pooler_output (`*_attn`, `*_fc1`, `*_hidden_m2`, `*_last`, `*_pooled`): the float64 tensor, kept as float32
(2^-24 relative, four orders below the bars the records are used under) and, in case (a), at the whole-width rows of tokens
0, 1, 31, 32, 33, 63, 64, 65, 75, 76 only, so that the file stays under 1 MiB; in that order the noise of the reference
arithmetic -- the same model run in fp32 with every layer's output rounded to fp16, against the float64 run over the WHOLE
tensor: max|difference| / max|float64| (`*_noise`) -- and those largest magnitudes (`*_peak`), both float64.

Asserted for every case: no activation above 65504 / 8 in either run; every noise entry is positive.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_text_model as M  # noqa: E402


def main():
    out = {}
    for case in M.CASES:
        key = M.case_key(case)
        rec, noise, peak, act = M.record(case)
        assert act < M.ACT_LIMIT, (key, act)
        assert min(noise.values()) > 0, (key, noise)
        for n in M.TENSORS:
            out["%s_%s" % (key, n)] = M.thin(case, n, rec[n])
        out[key + "_noise"] = np.array([noise[n] for n in M.TENSORS], np.float64)
        out[key + "_peak"] = np.array([peak[n] for n in M.TENSORS], np.float64)
        print("%s: activation peak %.1f; fp16-rounded layers vs float64: %s; kept %d values"
              % (key, act, ", ".join("%s %.2e of %.3g" % (n, noise[n], peak[n]) for n in M.TENSORS),
                 sum(out["%s_%s" % (key, n)].size for n in M.TENSORS)))
    path = os.path.join(HERE, M.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
