"""Register / scratch / LDS budgets of the VAE decoder's kernels, read from the hipcc listing (no GPU needed) with the flags
fresco_amd/csrc/Makefile builds vae.hip with: the kernels exist in the instantiations the launchers use, nothing spills,
nothing touches scratch memory, and the LDS is what the kernels' comments say.  The convolution takes its 40 KiB as dynamic
LDS (the launcher passes VC_LDS): that is below the 64 KiB every kernel may use without common.h's allow_dyn_lds, so it does
not go through it; its static LDS is zero."""
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

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vae") / "vae.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "vae.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
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


def test_vae_kernels_exist_and_do_not_spill(listing):
    _, kernels = listing
    # the statistics pass comes from groupnorm_stats.h: fp16 rows (IDF16_E)
    single = ("vae_input_kernel", "gn_stats_kernelIDF16_E", "gn_finish_kernel", "vae_gn_apply_kernel", "vae_softmax_kernel")
    for pat in single:
        assert len([n for n in kernels if pat in n]) == 1, (pat, sorted(kernels))
    conv = sorted(n for n in kernels if "vae_conv_kernel" in n)
    assert len(conv) == 2 and any("ILi9E" in n for n in conv) and any("ILi1E" in n for n in conv), conv  # 3 x 3 and 1 x 1
    assert len(kernels) == len(single) + 2, sorted(kernels)
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] <= LDS_LIMIT, (n, r)
    for n in conv:
        # four waves per workgroup, one per SIMD; .vgpr_count is the unified file (VGPRs + AGPRs) of 512 per SIMD lane: at most
        # 256 keeps two workgroups on a CU, so that one's barrier waits run under the other's MFMAs
        assert kernels[n]["agpr"] <= kernels[n]["vgpr"] <= 256, (n, kernels[n])


def test_lds_is_what_the_comments_say(listing):
    _, kernels = listing
    lds = lambda pat: [r["lds"] for n, r in kernels.items() if pat in n]  # noqa: E731
    assert lds("vae_conv_kernel") == [0, 0]                 # dynamic: VC_LDS below
    assert lds("gn_stats_kernel") == [2 * 512 * 8]          # two fp64 arrays of one entry per half quad
    assert lds("vae_softmax_kernel") == [4 * 4] and lds("vae_gn_apply_kernel") == [0] and lds("vae_input_kernel") == [0]
    src = open(os.path.join(CSRC, "vae.hip")).read()
    tile = open(os.path.join(CSRC, "conv_tile.h")).read()  # the weight slots are the shared tile's
    consts = dict(re.findall(r"constexpr int (VC_A_BYTES|CT_B_BYTES) = (\d+) \* 1024;", src + tile))
    dyn = 2 * int(consts["VC_A_BYTES"]) * 1024 + 2 * int(consts["CT_B_BYTES"]) * 1024
    assert "constexpr int VC_LDS = 2 * VC_A_BYTES + 2 * CT_B_BYTES;" in src and "LDS (dynamic, 40 KiB)" in src
    assert dyn == 40 * 1024 and dyn <= LDS_LIMIT
    assert src.count("VC_LDS, as_stream(stream)") == 2 and "allow_dyn_lds(" not in src


def test_the_convolution_uses_the_fp16_mfma_and_the_lds_dma(listing):
    text, _ = listing
    assert "v_mfma_f32_32x32x16_f16" in text and "global_load_lds_dwordx4" in text
    assert "global_atomic" not in text and "flat_atomic" not in text  # no float atomics: same inputs, same bits
