"""Register / scratch budget of the denoising loop's two kernels, read from the hipcc listing's kernel metadata (no GPU
needed) with the flags fresco_amd/csrc/Makefile builds loop.hip with: each instantiation (loop_update_kernel for fp16, bf16
and fp32, loop_frames_kernel for fp16 and fp32) exists once, nothing spills, nothing touches scratch memory, no LDS, 256
threads.  Only the metadata is read, nothing of the listing's instructions."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only"]
# mangled element types: _Float16, __bf16, float
KERNELS = {"loop_update_kernel": ("DF16_", "DF16b", "f"), "loop_frames_kernel": ("DF16_", "f")}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("loop") / "loop.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "loop.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = open(out).read()
    found = []
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        found.append(dict(name=g("name"), spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                          scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                          vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")), threads=int(g("max_flat_workgroup_size"))))
    return found


def test_makefile_builds_loop_hip_without_contraction():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "loop.hip" in srcs and srcs.count("loop.hip") == 1
    assert "../../include/fresco_loop.h" in mk and " ddpm_math.h " in mk
    line = re.search(r"^(build/warp\.o[^\n]*): EXTRA := -ffp-contract=off$", mk, re.M)
    assert line and "build/loop.o" in line.group(1).split()
    assert "CXXFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC" in mk


def test_both_files_take_the_formulas_from_the_one_header():
    for name in ("warp.hip", "loop.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert '#include "ddpm_math.h"' in src, name
        assert "ddpm_pred_x0(" in src and "ddpm_posterior(" in src and "ddpm_guided_eps(" in src, name


def test_each_kernel_exists_once_and_does_not_spill(kernels):
    assert len(kernels) == sum(len(v) for v in KERNELS.values()), [k["name"] for k in kernels]
    for kernel, types in KERNELS.items():
        for t in types:
            hits = [k for k in kernels if re.search(r"%d%sI%sE" % (len(kernel), kernel, re.escape(t)), k["name"])]
            assert len(hits) == 1, (kernel, t, [k["name"] for k in kernels])
            r = hits[0]
            assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
            assert r["threads"] == 256 and r["lds"] == 0 and r["agpr"] == 0, r
            assert r["vgpr"] <= 64, r  # elementwise: eight waves per SIMD stay possible
