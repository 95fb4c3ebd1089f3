"""Register / scratch budgets of the batched Ebsynth and guide kernels, read from the hipcc listing (no GPU needed),
with the flags fresco_amd/csrc/Makefile builds them with: nothing spills, nothing touches scratch memory, and the
per-pixel search kernels keep at least four waves per SIMD (<= 128 VGPRs)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BASE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]
EXTRA = {"guides.hip": ["-ffp-contract=off"], "blend.hip": ["-ffp-contract=off"]}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def _listing(src, tmp_path):
    out = str(tmp_path / (src + ".s"))
    subprocess.run([HIPCC] + BASE + EXTRA.get(src, []) + [os.path.join(CSRC, src), "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", open(out).read(), re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")), spill=int(g("vgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")),
                                  kernarg=int(g("kernarg_segment_size")))
    return kernels


def test_ebsynth_kernels_do_not_spill(tmp_path):
    k = _listing("ebsynth.hip", tmp_path)
    names = [n for n in k if "eb_" in n]
    assert len(names) >= 25, names
    for n in names:
        r = k[n]
        assert r["spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["kernarg"] <= 1024, (n, r)  # the per-problem seeds: 64 x 8 bytes
        if "eb_propagate" in n or "eb_random_search" in n or "eb_error_pass" in n:
            assert r["vgpr"] + r["agpr"] <= 128, (n, r)


def test_guide_kernels_do_not_spill(tmp_path):
    for src, pats in (("guides.hip", ("guide_edge", "guide_warp_nearest")), ("blend.hip", ("blend_prep",))):
        k = _listing(src, tmp_path)
        for pat in pats:
            hits = [n for n in k if pat in n]
            assert hits, pat
            for n in hits:
                assert k[n]["spill"] == 0 and k[n]["scratch"] == 0, (n, k[n])
