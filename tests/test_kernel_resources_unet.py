"""Register / scratch / LDS budgets of the UNet resnet block's kernels, read from the hipcc listing (no GPU needed) with the
flags fresco_amd/csrc/Makefile builds unet.hip with: the kernels exist in the instantiations the launchers use, nothing
spills, nothing touches scratch memory, and static plus dynamic LDS is what unet.hip's header comment states: the LDS form
of the GroupNorm keeps 32 KiB + 512 + 256 bytes static beside a dynamic plane of at most UG_LDS_PLANE_BYTES = 96 KiB
(128.75 KiB together, below the CU's 160 KiB; above 64 KiB it goes through common.h's allow_dyn_lds)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]  # (-S on the device side alone)
CU_LDS = 160 * 1024

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("unet") / "unet.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "unet.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
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


def test_makefile_builds_unet_hip_with_the_plain_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "unet.hip" in srcs
    assert "../../include/fresco_unet.h" in mk
    assert not re.search(r"build/unet\.o[^\n]*EXTRA", mk)  # no per-file flags: FLAGS above is the whole command line
    assert "CXXFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC" in mk


def test_unet_kernels_exist_and_do_not_spill(listing):
    _, kernels = listing
    single = ("unet_gn_lds_kernel", "unet_gn_stats_kernel", "unet_gn_finish_kernel", "unet_gn_apply_kernel")
    for pat in single:
        assert len([n for n in kernels if pat in n]) == 1, (pat, sorted(kernels))
    temb = sorted(n for n in kernels if "unet_temb_kernel" in n)
    assert len(temb) == 4 and all(any("ILi%dE" % t in n for n in temb) for t in (1, 2, 3, 4)), temb  # 16, 32, 48, 64 images
    assert len(kernels) == len(single) + 4, sorted(kernels)
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        # the unified register file is 512 per SIMD lane: a workgroup's waves must fit one CU's four SIMDs
        assert r["vgpr"] * (r["threads"] // 64) <= 4 * 512, (n, r)
    for pat in ("unet_gn_lds_kernel", "unet_gn_stats_kernel", "unet_gn_apply_kernel"):
        r = [r for n, r in kernels.items() if pat in n][0]
        assert r["threads"] == 512 and r["vgpr"] <= 128, (pat, r)   # eight waves: two per SIMD; <= 128 leaves room for four


def test_lds_is_what_the_header_comment_says(listing):
    _, kernels = listing
    lds = lambda pat: [r["lds"] for n, r in kernels.items() if pat in n]  # noqa: E731
    pair_sums = 2 * 512 * 4 * 8           # two fp64 arrays, four pairs per thread
    group_sums = 2 * 32 * 8
    assert lds("unet_gn_lds_kernel") == [pair_sums + group_sums + 2 * 32 * 4]   # + mean and rstd
    assert lds("unet_gn_stats_kernel") == [pair_sums + group_sums]
    assert lds("unet_gn_apply_kernel") == [0] and lds("unet_gn_finish_kernel") == [0]
    assert lds("unet_temb_kernel") == [16 * 512 * 4] * 4                          # SiLU(temb): 16 images x 512 k, fp32
    src = open(os.path.join(CSRC, "unet.hip")).read()
    assert "constexpr int UG_LDS_PLANE_BYTES = 96 * 1024;" in src and "UG_LDS_PLANE_BYTES = 96 KiB" in src
    assert "constexpr int UG_STATIC_LDS = 2 * UG_THREADS * 4 * 8 + 2 * UG_GROUPS * 8 + 2 * UG_GROUPS * 4;" in src
    assert "32 KiB + 512 bytes + 256 bytes of static LDS" in src and "128.75 KiB" in src
    total = 96 * 1024 + lds("unet_gn_lds_kernel")[0]
    assert total == int(128.75 * 1024) and total <= CU_LDS
    # the one dynamic-LDS launch passes the plane; whatever exceeds 64 KiB with the static part goes through allow_dyn_lds
    assert src.count("dim3(UG_THREADS), p.plane, st, a)") == 1
    assert "if (p.plane + UG_STATIC_LDS > 64 * 1024)" in src and src.count("allow_dyn_lds(unet_gn_lds_kernel, p.plane)") == 1


def test_statistics_are_fp64_without_atomics(listing):
    text, _ = listing
    assert "v_add_f64" in text and "v_fma_f64" in text
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text   # 16-byte pieces both ways
    assert "global_atomic" not in text and "flat_atomic" not in text and "ds_add" not in text  # same inputs, same bits
