"""Generate tests/golden/vae_encoder_fullsize_golden.npz (vae_encoder_model.FULLSIZE_CASES): make_vae_encoder_golden.py's
records -- the same float64 run, the same fp32 run with fp16-rounded layers for the noise, the same thinning and the same
assertions -- at the sizes tests/test_gpu_vae_encoder_fullsize.py needs: images (2, 192, 192) and the real (1, 512, 512).

Run:  python tests/golden/make_vae_encoder_fullsize_golden.py     (minutes of CPU time and a few GB of memory; the time is printed)
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vae_encoder_model as EM  # noqa: E402
from make_vae_encoder_golden import record  # noqa: E402


def main():
    t0 = time.time()
    out = record(EM.build(torch.float64), EM.build(torch.float32), EM.FULLSIZE_CASES)
    path = os.path.join(HERE, EM.FULLSIZE_GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays) in %.0f s" % (path, os.path.getsize(path), len(out), time.time() - t0))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
