"""Register / scratch / LDS budgets of csrc/unet_shell.hip's kernels, read from the hipcc listing's metadata (no GPU needed)
with the flags fresco_amd/csrc/Makefile builds the file with: the kernels exist in the instantiations the launchers use,
nothing spills, nothing touches scratch memory, static LDS is what the header comment states and the convolution's dynamic
LDS is the 32 KiB of vaeenc_conv_down_kernel (two pixel slots and two weight slots of 8 KiB), whose register budget it keeps."""
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


def _kernels(tmp, stem):
    out = str(tmp / (stem + ".s"))
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, stem + ".hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", open(out).read(), re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), threads=int(g("max_flat_workgroup_size")))
    return kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return _kernels(tmp_path_factory.mktemp("unet_shell"), "unet_shell")


def test_makefile_builds_unet_shell_hip_with_the_plain_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "unet_shell.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "../../include/fresco_unet_shell.h" in mk
    assert not re.search(r"build/unet_shell\.o[^\n]*EXTRA", mk)  # no per-file flags: FLAGS above is the whole command line
    assert "CXXFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC" in mk


def test_kernels_exist_in_the_launched_instantiations_and_do_not_spill(kernels):
    conv = sorted(n for n in kernels if "unet_conv3_kernel" in n)
    # <STRIDE, ACT>: both strides, with and without SiLU (the down sampler: <2, 0>; the embedding: <1, 1>, <2, 1>, <1, 0>)
    assert len(conv) == 4 and all(any("ILi%dELi%dE" % (s, a) in n for n in conv) for s in (1, 2) for a in (0, 1)), conv
    lin = sorted(n for n in kernels if "unet_time_linear_kernel" in n)
    # <TILES, KIND>: 16, 32, 48, 64 images x (timesteps, SiLU rows)
    assert len(lin) == 8 and all(any("ILi%dELi%dE" % (t, k) in n for n in lin) for t in (1, 2, 3, 4) for k in (0, 1)), lin
    assert len([n for n in kernels if "unet_input_kernel" in n]) == 1
    assert len(kernels) == 4 + 8 + 1, sorted(kernels)
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["threads"] == 256
        # the unified register file is 512 per SIMD lane: a workgroup's waves must fit one CU's four SIMDs
        assert r["vgpr"] * (r["threads"] // 64) <= 4 * 512, (n, r)


def test_lds_is_what_the_source_says(kernels):
    src = open(os.path.join(CSRC, "unet_shell.hip")).read()
    for n, r in kernels.items():
        if "unet_conv3_kernel" in n:
            assert r["lds"] == 0, (n, r)                       # all of it is dynamic
        elif "unet_time_linear_kernel" in n:
            assert r["lds"] == 16 * 512 * 4, (n, r)            # f(src): 16 images x 512 k, fp32
        else:
            assert r["lds"] == 0, (n, r)
    assert "constexpr int UC_A_BYTES = 8 * 1024;" in src and "constexpr int UC_LDS = 2 * UC_A_BYTES + 2 * CT_B_BYTES;  // 32 KiB" in src
    assert "LDS (dynamic, 32 KiB)" in src
    tile = open(os.path.join(CSRC, "conv_tile.h")).read()
    assert "constexpr int CT_B_BYTES = 8 * 1024;" in tile
    assert src.count("dim3(256), UC_LDS, st, a)") == 1       # the one dynamic-LDS launch; below 64 KiB: no allow_dyn_lds
    assert "allow_dyn_lds" not in src
    assert "constexpr int UL_KC = 512, UL_IT = 16, UL_NMAX = 64;" in src


def test_the_convolution_keeps_the_budget_of_the_encoder_down_sampler(kernels, tmp_path):
    """vaeenc_conv_down_kernel's: 32 KiB of dynamic LDS (five workgroups per CU by LDS) and a register count that leaves three
    workgroups of four waves per CU (3 per SIMD: 512 / 3 = 170 registers)"""
    enc = _kernels(tmp_path, "vae_enc")
    down = [r for n, r in enc.items() if "vaeenc_conv_down_kernel" in n]
    assert len(down) == 1
    enc_src = open(os.path.join(CSRC, "vae_enc.hip")).read()
    assert "constexpr int VD_LDS = 2 * VD_A_BYTES + 2 * CT_B_BYTES;" in enc_src and "constexpr int VD_A_BYTES = 8 * 1024;" in enc_src
    for n, r in kernels.items():
        if "unet_conv3_kernel" not in n:
            continue
        assert 512 // r["vgpr"] == 512 // down[0]["vgpr"] == 3, (n, r, down[0])
        if "ELi0EE" in n:                                   # without the activation: the very same count
            assert r["vgpr"] == down[0]["vgpr"], (n, r, down[0])
