"""Register / scratch / LDS budgets of the MiDaS kernels, read from the hipcc listing (no GPU needed) with the flags
fresco_amd/csrc/Makefile builds midas.hip with: the kernels exist in the instantiations the launchers use, nothing spills,
nothing touches scratch memory, and the static LDS is what the kernels' comments say.  None of them asks for dynamic LDS,
so none goes through common.h's allow_dyn_lds (which raises a kernel's limit per device, and holds no number of its own):
what they may use is the 64 KiB every kernel has without that call.  The stem at the "same" origin is a second
instantiation of flownet.hip's stem kernel and must not cost more than the first."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]  # (-S on the device side alone)
LDS_LIMIT = 64 * 1024  # static LDS of a kernel that never calls allow_dyn_lds

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def _listing(src, tmp_path, extra=()):
    out = str(tmp_path / (src + ".s"))
    subprocess.run([HIPCC] + FLAGS + list(extra) + [os.path.join(CSRC, src), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", open(out).read(), re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")))
    return kernels


def test_midas_kernels_do_not_spill(tmp_path):
    kernels = _listing("midas.hip", tmp_path, ["-ffp-contract=off"])  # (build/midas.o: EXTRA of the Makefile)
    # the statistics pass and the pool come from groupnorm_stats.h / pool3s2.h: fp32 rows, the window origin 0 (Li0E)
    single = ("midas_input_kernel", "gn_stats_kernelIfE", "gn_finish_kernel", "midas_gn_apply_kernel",
              "pool3s2_kernelILi0EE", "midas_layernorm_kernel", "midas_tokens_kernel", "midas_head_merge_kernel",
              "midas_rowbias_gelu_kernel", "midas_minmax_kernel")
    for pat in single:
        assert len([n for n in kernels if pat in n]) == 1, (pat, sorted(kernels))
    assert len([n for n in kernels if "midas_tail_kernel" in n]) == 3  # the condition as fp16, bf16, fp32
    assert len(kernels) == len(single) + 3, sorted(kernels)
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] <= LDS_LIMIT, (n, r)
    lds = lambda pat: [r["lds"] for n, r in kernels.items() if pat in n][0]  # noqa: E731
    assert lds("gn_stats_kernel") == 2 * 512 * 8  # two fp64 arrays of one entry per half quad
    assert lds("midas_minmax_kernel") == 2 * 4 * 4 and lds("midas_tail_kernel") == 2 * 4
    assert lds("midas_layernorm_kernel") == 0 and lds("midas_gn_apply_kernel") == 0


def test_stem_at_the_same_origin_costs_what_the_stem_costs(tmp_path):
    kernels = _listing("flownet.hip", tmp_path)
    stems = {n: r for n, r in kernels.items() if "fn_conv7_rgb_kernel" in n}
    assert len(stems) == 2, sorted(stems)
    (a, ra), (b, rb) = sorted(stems.items())
    for r in (ra, rb):
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0
    assert ra["vgpr"] == rb["vgpr"] and ra["lds"] == rb["lds"]
