"""Register / scratch budgets of the tap-resize kernels, read from the hipcc listing (no GPU needed) with the flags
fresco_amd/csrc/Makefile builds resize.hip with: the two kernels exist, nothing spills, nothing touches scratch memory, and
their static LDS is what the window plan needs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# CXXFLAGS of the Makefile plus the EXTRA of build/resize.o
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def test_resize_kernels_do_not_spill(tmp_path):
    out = str(tmp_path / "resize.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "resize.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=600)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")))
    assert len(kernels) == 2, sorted(kernels)
    for pat in ("frame_resize_kernelILi8E", "frame_resize_kernelILi2E"):
        assert len([n for n in kernels if pat in n]) == 1, (pat, sorted(kernels))
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["vgpr"] <= 64, (n, r)  # light kernels: eight waves per SIMD stay possible
    # a 72 x 72 x 3 byte window, its horizontal pass of 72 x 96 32-bit words, the tile's 2 x 32 first-tap offsets and its
    # 2 x 32 x K 16-bit coefficients: three workgroups fit a CU's 160 KiB
    for pat, K in (("ILi8E", 8), ("ILi2E", 2)):
        r = [r for n, r in kernels.items() if pat in n][0]
        assert r["lds"] == 72 * 216 + 72 * 96 * 4 + 2 * 32 * 4 + 2 * 32 * K * 2, (pat, r)
        assert 3 * r["lds"] <= 160 * 1024
