"""Register / scratch / LDS budgets of the VAE encoder's kernels, read from the hipcc listing (no GPU needed) with the flags
fresco_amd/csrc/Makefile builds vae_enc.hip with: the four kernels exist once each, nothing spills, nothing touches scratch
memory, and the LDS is what the stride-2 convolution's comment says: 32 KiB, all dynamic (the launcher passes VD_LDS), below
the 64 KiB every kernel may use without common.h's allow_dyn_lds, so it does not go through it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]  # (-S on the device side alone)
LDS_LIMIT = 64 * 1024  # what a kernel that never calls allow_dyn_lds may use, static + dynamic
KERNELS = ("vaeenc_input_kernel", "vaeenc_conv_down_kernel", "vaeenc_moments_kernel", "vaeenc_sample_kernel")

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vae_enc") / "vae_enc.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "vae_enc.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")))
    return text, kernels


def test_encoder_kernels_exist_once_and_do_not_spill(listing):
    _, kernels = listing
    for pat in KERNELS:
        assert len([n for n in kernels if pat in n]) == 1, (pat, sorted(kernels))
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
    conv = [r for n, r in kernels.items() if "vaeenc_conv_down_kernel" in n][0]
    # four waves per workgroup, one per SIMD; .vgpr_count is the unified file (VGPRs + AGPRs) of 512 per SIMD lane: at most
    # 168 keeps three workgroups on a CU, as the kernel's comment says
    assert conv["agpr"] <= conv["vgpr"] <= 168, conv


def test_lds_is_what_the_comment_says(listing):
    _, kernels = listing
    assert [r["lds"] for r in kernels.values()] == [0, 0, 0, 0]  # no static LDS anywhere; the convolution's is dynamic
    src = open(os.path.join(CSRC, "vae_enc.hip")).read()
    tile = open(os.path.join(CSRC, "conv_tile.h")).read()  # the weight slots are the shared tile's
    consts = dict(re.findall(r"constexpr int (VD_A_BYTES|CT_B_BYTES) = (\d+) \* 1024;", src + tile))
    dyn = 2 * int(consts["VD_A_BYTES"]) * 1024 + 2 * int(consts["CT_B_BYTES"]) * 1024
    assert "constexpr int VD_LDS = 2 * VD_A_BYTES + 2 * CT_B_BYTES;" in src and "LDS (dynamic, 32 KiB)" in src
    assert dyn == 32 * 1024 and dyn <= LDS_LIMIT
    launches = re.findall(r"hipLaunchKernelGGL\((\w+), [^;]*?dim3\(256\), (\w+), as_stream", src)
    assert sorted(launches) == sorted([("vaeenc_conv_down_kernel", "VD_LDS"), ("vaeenc_input_kernel", "0"),
                                       ("vaeenc_moments_kernel", "0"), ("vaeenc_sample_kernel", "0")]), launches
    assert "allow_dyn_lds(" not in src  # needed above LDS_LIMIT only


def test_the_convolution_uses_the_fp16_mfma_and_the_lds_dma(listing):
    text, _ = listing
    assert "v_mfma_f32_32x32x16_f16" in text and "global_load_lds_dwordx4" in text
    assert "global_atomic" not in text and "flat_atomic" not in text  # no float atomics: same inputs, same bits
