"""Register / scratch / LDS budgets of the UNet transformer blocks' kernels, read from the hipcc listing's kernel metadata (no
GPU needed) with the flags fresco_amd/csrc/Makefile builds unet_tf.hip with: the kernels exist in the instantiations the
launcher uses, nothing spills, nothing touches scratch memory, a workgroup's registers fit a CU, and the GEGLU kernel's LDS
is what unet_tf.hip's header comment states: two slots of 8 KiB for the tile's rows and conv_tile.h's two weight slots of
8 KiB, 32 KiB, static."""
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
    out = str(tmp_path_factory.mktemp("unet_tf") / "unet_tf.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "unet_tf.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), threads=int(g("max_flat_workgroup_size")))
    return text, kernels


def test_makefile_builds_unet_tf_hip_with_the_plain_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "unet_tf.hip" in srcs and "unet.hip" in srcs
    assert "../../include/fresco_unet_tf.h" in mk
    assert not re.search(r"build/unet_tf\.o[^\n]*EXTRA", mk)  # no per-file flags: FLAGS above is the whole command line
    assert "CXXFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC" in mk


def test_kernels_exist_and_do_not_spill(listing):
    _, kernels = listing
    assert len([n for n in kernels if "unet_geglu_kernel" in n]) == 1, sorted(kernels)
    ln = sorted(n for n in kernels if "unet_ln_kernel" in n)
    assert len(ln) == 5 and all(any("ILi%dE" % t in n for n in ln) for t in (1, 2, 3, 4, 5)), ln  # 1 .. 5 pieces per lane
    assert len(kernels) == 6, sorted(kernels)
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["threads"] == 256, (n, r)
        # the unified register file is 512 per SIMD lane: a workgroup's waves must fit one CU's four SIMDs
        assert r["vgpr"] * (r["threads"] // 64) <= 4 * 512, (n, r)
    geglu = [r for n, r in kernels.items() if "unet_geglu_kernel" in n][0]
    assert geglu["vgpr"] <= 256   # two workgroups per CU: the next tile's copies fly under this one's epilogue


def test_lds_is_what_the_header_comment_says(listing):
    _, kernels = listing
    lds = lambda pat: [r["lds"] for n, r in kernels.items() if pat in n]  # noqa: E731
    assert lds("unet_geglu_kernel") == [2 * 8 * 1024 + 2 * 8 * 1024]   # two row slots + two weight slots of 8 KiB
    assert lds("unet_ln_kernel") == [0] * 5
    src = open(os.path.join(CSRC, "unet_tf.hip")).read()
    assert "constexpr int UF_LDS = 2 * UF_A_BYTES + 2 * CT_B_BYTES;" in src and "LDS (static, 32 KiB)" in src
    assert "constexpr int UF_A_BYTES = 8 * 1024;" in src


def test_mfma_and_fp64_statistics_without_atomics(listing):
    text, _ = listing
    assert "v_mfma_f32_32x32x16_f16" in text
    assert "v_add_f64" in text and "v_fma_f64" in text
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text   # the norm's 16-byte pieces both ways
    assert "global_store_dwordx2" in text                                     # the GEGLU's four channels as 8 bytes
    assert "global_load_lds_dwordx4" in text
    assert "global_atomic" not in text and "flat_atomic" not in text and "ds_add" not in text  # same inputs, same bits
