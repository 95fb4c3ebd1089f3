"""Register / scratch budgets of the bf16 instantiations of the flash, projection and temporal kernels, read from the
hipcc listing (no GPU needed).  The bf16 kernels carry names of their own (attn_flash_bf16_kernel, ...) over bodies shared
with the fp16 ones, so that each name below -- and each fp16 name in test_kernel_resources.py -- matches exactly one kernel."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _listing, _one

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def test_bf16_flash_and_projection_kernels_fit_two_waves_per_simd(tmp_path):
    k = _listing("attn.hip", tmp_path)
    for pat in (r"attn_flash_bf16_kernelILi40ELi2E", r"attn_flash_bf16_kernelILi80ELi1E",
                r"attn_flash_bf16_kernelILi80ELi2E"):
        r = _one(k, pat)
        assert r["vgpr"] + r["agpr"] <= 256 and r["spill"] == 0 and r["scratch"] == 0, (pat, r)
    for pat in (r"kv_pack_bf16_kernelILi40E", r"kv_pack_bf16_kernelILi80E"):
        r = _one(k, pat)
        assert r["spill"] == 0 and r["scratch"] == 0, (pat, r)
    k = _listing("proj.hip", tmp_path)
    for pat in (r"linear_bf16_kernelILi320ELi8E", r"linear_bf16_kernelILi640ELi8E"):
        r = _one(k, pat)
        assert r["vgpr"] + r["agpr"] <= 256 and r["spill"] == 0 and r["scratch"] == 0, (pat, r)


def test_bf16_temporal_kernels_do_not_spill(tmp_path):
    k = _listing("temporal.hip", tmp_path)
    for pat in (r"temporal_mfma_bf16_kernelILi40ELi1E", r"temporal_mfma_bf16_kernelILi80ELi1E",
                r"temporal_mfma_bf16_kernelILi40ELi2E", r"temporal_mfma_bf16_kernelILi80ELi2E",
                r"temporal_attn_bf16_kernelILi40E", r"temporal_attn_bf16_kernelILi80E"):
        r = _one(k, pat)
        assert r["spill"] == 0 and r["scratch"] == 0, (pat, r)


def test_fp16_names_still_match_one_kernel_each(tmp_path):
    """the bf16 kernels must not shadow or duplicate the fp16 ones under the prefixes the fp16 budget tests search for"""
    k = _listing("attn.hip", tmp_path)
    for pat in (r"attn_flash_kernelILi40ELi2E", r"attn_flash_kernelILi80ELi2E", r"kv_pack_kernelILi40E"):
        _one(k, pat)
    _one(_listing("proj.hip", tmp_path), r"linear_kernelILi640ELi8E")
    _one(_listing("temporal.hip", tmp_path), r"temporal_mfma_kernelILi40ELi1E")
