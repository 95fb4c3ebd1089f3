"""Register / scratch budgets of the FreeU kernels, read from the hipcc listing (no GPU needed) with the flags
fresco_amd/csrc/Makefile builds freeu.hip with: nothing spills and nothing touches scratch memory, in any of the
element types and access widths; the kernels that hold a plane in registers keep four waves per SIMD (<= 128 VGPRs)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BASE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def _listing(src, tmp_path):
    out = str(tmp_path / (src + ".s"))
    subprocess.run([HIPCC] + BASE + [os.path.join(CSRC, src), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=600)
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", open(out).read(), re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")), spill=int(g("vgpr_spill_count")),
                                  sgpr_spill=int(g("sgpr_spill_count")), scratch=int(g("private_segment_fixed_size")))
    return kernels


def test_freeu_kernels_do_not_spill(tmp_path):
    k = _listing("freeu.hip", tmp_path)
    names = [n for n in k if "freeu_" in n]
    # fourier (register form at two widths, two-pass, copy), channel partial, scale + cat: x 3 element types x 2 access
    # widths; min / max once
    for pat, count in (("freeu_fourier_reg_kernel", 12), ("freeu_fourier_two_pass_kernel", 6), ("freeu_copy_kernel", 6),
                       ("freeu_chan_partial_kernel", 6), ("freeu_scale_cat_kernel", 6), ("freeu_minmax_kernel", 1)):
        assert len([n for n in names if pat in n]) == count, (pat, names)
    for n in names:
        r = k[n]
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        if "freeu_fourier_reg_kernel" in n:
            assert r["vgpr"] + r["agpr"] <= 128, (n, r)
