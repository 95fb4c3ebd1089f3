"""Register / scratch budgets of the EGNet kernels, read from the hipcc listing (no GPU needed) with the flags
fresco_amd/csrc/Makefile builds egnet.hip with: the four kernels exist in the instantiations the launchers use (one
each), nothing spills and nothing touches scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# CXXFLAGS of the Makefile (build/egnet.o has no EXTRA)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]  # (-S on the device side alone)

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def test_egnet_kernels_do_not_spill(tmp_path):
    out = str(tmp_path / "egnet.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "egnet.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=600)
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", open(out).read(), re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")))
    # the pool comes from pool3s2.h: the window origin -1 (Lin1E)
    for pat in ("egnet_input_kernel", "pool3s2_kernelILin1EE", "egnet_resize_add_kernel", "egnet_saliency_kernel"):
        assert len([n for n in kernels if pat in n]) == 1, (pat, sorted(kernels))
    assert len(kernels) == 4, sorted(kernels)
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
    tail = [r for n, r in kernels.items() if "egnet_saliency_kernel" in n][0]
    assert tail["lds"] == (16 + 15 - 1) ** 2 * 4  # the sigmoid tile with the widest box's halo
