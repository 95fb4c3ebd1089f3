"""Register / scratch / LDS budget of the CLIP text model's kernels, read from the hipcc listing's kernel metadata (no GPU
needed) with the flags fresco_amd/csrc/Makefile builds text.hip with: each of the three kernels exists once, nothing spills,
nothing touches scratch memory, and registers and LDS are what text.hip's header comment states -- 32768 bytes of static LDS
for the attention (K and V^T of one (sequence, head)) and for fc1 (conv_tile.h's ring).  From the listing's text only the MFMA
mnemonic is checked."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]  # (-S on the device side alone)
KERNELS = ("clip_embed_kernel", "clip_attn64_kernel", "clip_fc1_kernel")

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("text") / "text.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "text.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")),
                                  threads=int(g("max_flat_workgroup_size")))
    return text, kernels


def _of(kernels, name):
    hits = [v for k, v in kernels.items() if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    return hits[0]


def test_makefile_builds_text_hip_with_the_plain_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "text.hip" in srcs
    assert "../../include/fresco_text.h" in mk
    assert not re.search(r"build/text\.o[^\n]*EXTRA", mk)  # no per-file flags: FLAGS above is the whole command line
    assert "CXXFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC" in mk


def test_each_kernel_exists_once_and_does_not_spill(listing):
    _, kernels = listing
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name in KERNELS:
        r = _of(kernels, name)
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["threads"] == 256, (name, r)
        # the unified register file is 512 per SIMD lane: a workgroup's four waves must fit one CU's four SIMDs
        assert r["vgpr"] * (r["threads"] // 64) <= 4 * 512, (name, r)


def test_registers_and_lds_are_what_the_header_comment_says(listing):
    _, kernels = listing
    src = open(os.path.join(CSRC, "text.hip")).read()
    head = src[:src.index("#include")].replace("\n//", " ")
    regs = re.search(r"Registers \(VGPRs / AGPRs\): (.*?);\s+no\s+spill,\s+no\s+scratch\.", head)
    lds = re.search(r"LDS \(static bytes\): (.*?)\.", head)
    assert regs and lds, "the header comment states registers and LDS"
    stated_regs = {n: (int(v), int(a)) for n, v, a in re.findall(r"(\w+) (\d+) / (\d+)", regs.group(1))}
    stated_lds = {n: int(b) for n, b in re.findall(r"(\w+) (\d+)", lds.group(1))}
    assert sorted(stated_regs) == sorted(stated_lds) == sorted(KERNELS)
    for name in KERNELS:
        r = _of(kernels, name)
        assert (r["vgpr"], r["agpr"]) == stated_regs[name], (name, r, stated_regs[name])
        assert r["lds"] == stated_lds[name], (name, r, stated_lds[name])
    # the attention: K rows + V^T rows of one (sequence, head) at L <= 128, D = 64; two workgroups per SIMD set fit the registers
    assert stated_lds["clip_attn64_kernel"] == 128 * 64 * 2 + 64 * 128 * 2 == 32768
    assert "static_assert(CA_LDS == 32768" in src and "static_assert(CF_LDS == 32768" in src
    assert stated_regs["clip_attn64_kernel"][0] <= 256 and "__launch_bounds__(CA_THREADS, 2)" in src
    assert stated_lds["clip_fc1_kernel"] == 2 * 8192 + 2 * 8192


def test_the_mfma_is_the_fp16_32x32x16(listing):
    text, _ = listing
    assert "v_mfma_f32_32x32x16_f16" in text
    assert not re.search(r"v_mfma_(?!f32_32x32x16_f16)", text)
