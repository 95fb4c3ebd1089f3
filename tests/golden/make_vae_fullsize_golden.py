"""Generate tests/golden/vae_fullsize_golden.npz (vae_model.FULLSIZE_CASES): make_vae_golden.py's records -- the same float64
run, the same fp32 run with fp16-rounded layers for the noise, the same thinning and the same assertions -- at the sizes
tests/test_gpu_vae_fullsize.py needs: latents (2, 24, 24), a 192 x 192 image with 576 tokens in the mid block, and the real
(1, 64, 64), a 512 x 512 image with 4096 tokens.  The real size keeps the thinned float64 image and the uint8 share, not the
whole uint8 image (786 432 bytes that do not compress).

Run:  python tests/golden/make_vae_fullsize_golden.py     (minutes of CPU time and a few GB of memory; the time is printed)
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vae_model as M  # noqa: E402
from make_vae_golden import record  # noqa: E402

WHOLE_U8_PIXELS = 192 * 192  # per frame: above this the whole uint8 image is left out


def main():
    t0 = time.time()
    out = record(M.build(torch.float64), M.build(torch.float32), M.FULLSIZE_CASES,
                 whole_u8=lambda case: 64 * case[1] * case[2] <= WHOLE_U8_PIXELS)
    path = os.path.join(HERE, M.FULLSIZE_GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays) in %.0f s" % (path, os.path.getsize(path), len(out), time.time() - t0))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
