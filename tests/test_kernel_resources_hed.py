"""Register / scratch budgets of the HED kernels, read from the hipcc listing (no GPU needed) with the flags
fresco_amd/csrc/Makefile builds hed.hip with: the three kernels exist in every instantiation the launchers use, nothing
spills and nothing touches scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# CXXFLAGS of the Makefile plus the EXTRA of build/hed.o
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def test_hed_kernels_do_not_spill(tmp_path):
    out = str(tmp_path / "hed.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "hed.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=600)
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", open(out).read(), re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")))
    # input once; side + pool per channel count (64, 128, 256, 512); fuse per condition type (fp16, bf16, fp32)
    for pat, count in (("hed_input_kernel", 1), ("hed_side_pool_kernel", 4), ("hed_fuse_kernel", 3)):
        assert len([n for n in kernels if pat in n]) == count, (pat, sorted(kernels))
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
