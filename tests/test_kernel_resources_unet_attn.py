"""Register / scratch / LDS budget of the head-dim-160 flash attention kernel, read from the hipcc listing's kernel metadata
(no GPU needed) with the flags fresco_amd/csrc/Makefile builds unet_attn.hip with: the kernel exists once, nothing spills,
nothing touches scratch memory, and its registers and LDS are what unet_attn.hip's header comment states -- 81920 bytes of
dynamic LDS (no static LDS in the metadata), half of a CU's 160 KiB, and the stated register count, within the 256 that two
waves per SIMD leave each.  From the listing's text only the MFMA mnemonic is checked."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]  # (-S on the device side alone)

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("unet_attn") / "unet_attn.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "unet_attn.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")),
                                  threads=int(g("max_flat_workgroup_size")))
    return text, kernels


def test_makefile_builds_unet_attn_hip_with_the_plain_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "unet_attn.hip" in srcs
    assert "../../include/fresco_unet_attn.h" in mk
    assert not re.search(r"build/unet_attn\.o[^\n]*EXTRA", mk)  # no per-file flags: FLAGS above is the whole command line
    assert "CXXFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC" in mk


def test_kernel_exists_once_and_does_not_spill(listing):
    _, kernels = listing
    assert len(kernels) == 1 and "unet_attn160_kernel" in list(kernels)[0], sorted(kernels)
    r = list(kernels.values())[0]
    assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["threads"] == 256, r
    # the unified register file is 512 per SIMD lane: a workgroup's four waves must fit one CU's four SIMDs
    assert r["vgpr"] * (r["threads"] // 64) <= 4 * 512, r


def test_registers_and_lds_are_what_the_header_comment_says(listing):
    _, kernels = listing
    r = list(kernels.values())[0]
    src = open(os.path.join(CSRC, "unet_attn.hip")).read()
    m = re.search(r"^// Registers: (\d+) VGPRs \(O\^T in them: no separate accumulation registers\)", src, re.M)
    assert m, "the header comment states the register count"
    assert (r["vgpr"], r["agpr"]) == (int(m.group(1)), 0), (r, m.group(0))
    assert r["vgpr"] <= 256 and "__launch_bounds__(UA_THREADS, 2)" in src     # two waves per SIMD
    m = re.search(r"^// LDS \(dynamic, (\d+) bytes", src, re.M)
    assert m and int(m.group(1)) == 81920
    assert "static_assert(UA_LDS == 81920" in src      # the source's constants add up to the comment's figure
    assert 128 * 160 * 2 + 160 * 128 * 2 == 81920 and 4 * 160 * 32 * 4 == 81920   # K rows + V^T rows; the merge's O^T
    assert r["lds"] == 0                               # all of it dynamic: allow_dyn_lds grants it per device
    assert 2 * 81920 <= 160 * 1024                     # two workgroups per CU


def test_the_mfma_is_the_fp16_32x32x16(listing):
    text, _ = listing
    assert "v_mfma_f32_32x32x16_f16" in text
