"""Register / scratch budgets of the bf16 instantiations of the fused K | V projection-pack, read from the hipcc listing
(no GPU needed), next to the fp16 ones, which must keep their names: one kernel per pattern.  Five-wave workgroups, one per
CU by LDS at either width: two waves per SIMD at most, so 256 registers and nothing in scratch."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _listing, _one

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def test_bf16_projection_pack_kernels_fit_and_do_not_spill(tmp_path):
    k = _listing("attn.hip", tmp_path)
    for pat in (r"kvproj_pack_bf16_kernelILi320ELi40E", r"kvproj_pack_bf16_kernelILi640ELi80E"):
        r = _one(k, pat)
        print(pat, r)
        assert r["vgpr"] + r["agpr"] <= 256 and r["spill"] == 0 and r["scratch"] == 0, (pat, r)


def test_fp16_projection_pack_kernels_keep_their_names(tmp_path):
    k = _listing("attn.hip", tmp_path)
    for pat in (r"kvproj_pack_kernelILi320ELi40E", r"kvproj_pack_kernelILi640ELi80E"):
        _one(k, pat)
