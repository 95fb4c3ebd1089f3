"""Register / scratch budget of the half-tile flash kernel at head dim 80, read from the hipcc listing (no GPU needed).

attn_flash_kernel<80, 2> holds two query blocks per wave beside a 96-register O: it runs two waves per SIMD only at
<= 256 registers, and its loop has nothing to spare -- a spill there is the 2.7x of DESIGN.md section 4."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _listing, _one

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def test_flash_d80_two_query_blocks_fits_two_waves_per_simd(tmp_path):
    k = _listing("attn.hip", tmp_path)
    r = _one(k, r"attn_flash_kernelILi80ELi2E")   # exactly one such kernel
    assert r["vgpr"] + r["agpr"] <= 256 and r["spill"] == 0 and r["scratch"] == 0, r
