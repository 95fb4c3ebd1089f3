"""Register / scratch budgets of the key-frame kernels, read from the hipcc listing (no GPU needed) with the flags
fresco_amd/csrc/Makefile builds keyframe.hip with: the four kernels exist, nothing spills, nothing touches scratch memory, and
the blur kernel's static LDS is what its tiles need."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# CXXFLAGS of the Makefile plus the EXTRA of build/keyframe.o
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def test_keyframe_kernels_do_not_spill(tmp_path):
    out = str(tmp_path / "keyframe.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "keyframe.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=600)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")))
    for pat in ("keyframe_resize_box_kernel", "keyframe_resize_table_kernel", "keyframe_blur_diff_kernel",
                "keyframe_sum_kernel"):
        assert len([n for n in kernels if pat in n]) == 1, (pat, sorted(kernels))
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["vgpr"] <= 64, (n, r)  # light kernels: eight waves per SIMD stay possible
    blur = [r for n, r in kernels.items() if "keyframe_blur_diff_kernel" in n][0]
    # two tiles + halo of 40 x 40 x 3 bytes, their horizontal passes of 40 x 96 16-bit words, four partial sums
    assert blur["lds"] == 2 * 40 * 120 + 2 * 40 * 96 * 2 + 16, blur
