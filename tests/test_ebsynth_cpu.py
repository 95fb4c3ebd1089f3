"""Ebsynth backend, host side (no GPU): pyramid level count, the command line of the reference binary (flags, channel
counting, default weights, the .bin error file), argument checks, and the register budget of ebsynth.hip."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from fresco_amd import FrescoHipError, ebsynth_run
from fresco_amd import ebsynth as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def ref_max_levels(source_hw, target_hw, patch):
    """ebsynth.cpp main(): levels 32..0, the first whose min(source, target) size, scaled by 2^-level and truncated,
    keeps its smaller side >= 2 * patch + 1."""
    m = (min(source_hw[0], target_hw[0]), min(source_hw[1], target_hw[1]))
    for level in range(32, -1, -1):
        f = np.float32(2.0) ** np.float32(-level)
        if min(int(np.float32(m[0]) * f), int(np.float32(m[1]) * f)) >= 2 * patch + 1:
            return level + 1
    return 0


@pytest.mark.parametrize("src,tgt,patch", [
    ((512, 512), (512, 512), 5), ((64, 64), (64, 64), 5), ((96, 128), (96, 128), 5), ((11, 11), (11, 11), 5),
    ((10, 40), (10, 40), 5), ((720, 1280), (720, 1280), 5), ((720, 1280), (360, 1280), 7), ((23, 23), (22, 50), 5),
    ((512, 512), (512, 512), 3), ((7, 7), (7, 7), 3), ((1, 1), (1, 1), 3), ((1000, 999), (999, 1000), 9)])
def test_max_levels_matches_reference_formula(src, tgt, patch):
    assert E.max_pyramid_levels(src, tgt, patch) == ref_max_levels(src, tgt, patch)


VIDEO_BLEND_CMD = ("-style /k/0001.png -guide /g/c0.png /g/c1.png -weight 6 -guide /g/e0.png /g/e1.png -weight 0.5 "
                   "-guide /g/t0.png /g/t1.png -weight 0.5 -guide /g/p0.png /g/p1.png -weight 2 "
                   "-output /o/0002.png -searchvoteiters 12 -patchmatchiters 6")


def test_cli_parses_video_blend_command():
    cfg = E.parse_cli(VIDEO_BLEND_CMD.split())
    assert cfg["style"] == "/k/0001.png" and cfg["output"] == "/o/0002.png"
    assert [g[2] for g in cfg["guides"]] == [6.0, 0.5, 0.5, 2.0]
    assert cfg["guides"][1][:2] == ["/g/e0.png", "/g/e1.png"]
    assert (cfg["searchvoteiters"], cfg["patchmatchiters"]) == (12, 6)
    # the binary's defaults for everything else
    assert (cfg["uniformity"], cfg["patchsize"], cfg["pyramidlevels"], cfg["stopthreshold"], cfg["extrapass3x3"],
            cfg["style_weight"]) == (3500.0, 5, -1, 5, False, -1.0)


def test_cli_flags_and_errors():
    cfg = E.parse_cli("-style s.png -weight 2 -guide a b -uniformity 500 -patchsize 7 -pyramidlevels 3 "
                      "-stopthreshold 0 -extrapass3x3 -backend cuda".split())
    assert (cfg["style_weight"], cfg["guides"][0][2], cfg["uniformity"], cfg["patchsize"], cfg["pyramidlevels"],
            cfg["stopthreshold"], cfg["extrapass3x3"]) == (2.0, -1.0, 500.0, 7, 3, 0, True)
    for bad in ("-style s -guide a b -patchsize 4", "-style s -guide a b -patchsize 1", "-weight 1 -style s",
                "-style s -guide a b -weight -1", "-style s -guide a", "-style s -guide a b -bogus",
                "-style s -guide a b -searchvoteiters x", "-style s -guide a b -pyramidlevels 0", "-guide a b",
                "-style s"):
        with pytest.raises(E.CliError):
            E.parse_cli(bad.split())


def _rgba(rgb, alpha=None):
    a = np.full(rgb.shape[:2] + (1,), 255, np.uint8) if alpha is None else alpha[..., None]
    return np.concatenate([rgb, a], -1)


def test_channel_counting_and_default_weights():
    rng = np.random.default_rng(0)
    g = rng.integers(0, 256, (6, 5, 1), dtype=np.uint8)
    gray = _rgba(np.repeat(g, 3, -1))
    rgb = _rgba(rng.integers(0, 256, (6, 5, 3), dtype=np.uint8))
    alpha = rng.integers(0, 255, (6, 5), dtype=np.uint8)
    assert E.num_channels(gray) == 1 and E.num_channels(rgb) == 3
    assert E.num_channels(_rgba(np.repeat(g, 3, -1), alpha)) == 2
    assert E.num_channels(_rgba(rgb[..., :3], alpha)) == 4
    ga = _rgba(np.repeat(g, 3, -1), alpha)
    np.testing.assert_array_equal(E.pick_channels(ga, 2), np.stack([g[..., 0], alpha], -1))
    # style RGB; guides: gray/gray, gray/RGB (counted as the larger, 3), RGB+alpha
    st, sg, tg, sw, gw = E.pack_inputs(rgb, [(gray, gray), (gray, rgb), (_rgba(rgb[..., :3], alpha), rgb)])
    assert st.shape == (6, 5, 3) and sg.shape == tg.shape == (6, 5, 1 + 3 + 4)
    np.testing.assert_allclose(sw, [1 / 3] * 3, rtol=1e-7)
    np.testing.assert_allclose(gw, [1 / 3] + [1 / 9] * 3 + [1 / 12] * 4, rtol=1e-7)
    np.testing.assert_array_equal(sg[..., 0], g[..., 0])
    np.testing.assert_array_equal(tg[..., 1:4], rgb[..., :3])
    # explicit weights: divided by the image's channel count
    _, _, _, sw, gw = E.pack_inputs(rgb, [(gray, gray), (rgb, rgb)], style_weight=3.0, guide_weights=[6.0, -1.0])
    np.testing.assert_allclose(sw, [1.0] * 3, rtol=1e-7)
    np.testing.assert_allclose(gw, [6.0] + [0.5 / 3] * 3, rtol=1e-7)


def load_error(bin_path, img_shape):
    """video_blend.py's load_error, restated."""
    img_size = img_shape[0] * img_shape[1]
    with open(bin_path, "rb") as fp:
        data = fp.read()
    assert struct.unpack("q", data[:8])[0] == img_size
    return np.array(struct.unpack("f" * img_size, data[8:]), dtype=np.float32).reshape(img_shape[0], img_shape[1])


def test_bin_writer_round_trips_through_load_error(tmp_path):
    err = np.random.default_rng(1).uniform(0, 1e5, (7, 9)).astype(np.float32)
    p = str(tmp_path / "out.bin")
    E.write_error_bin(p, err)
    assert os.path.getsize(p) == 8 + 4 * err.size
    np.testing.assert_array_equal(load_error(p, err.shape), err)
    assert E.bin_path("/a/b/0002.png") == "/a/b/0002.bin" and E.bin_path("out") == "out.bin"


def test_python_argument_checks_need_no_gpu():
    s = torch.zeros(32, 32, 3, dtype=torch.uint8)
    g = torch.zeros(32, 32, 2, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ebsynth_run(s.float(), g, g)
    with pytest.raises(ValueError):
        ebsynth_run(s, g, torch.zeros(32, 32, 3, dtype=torch.uint8))   # guide channel mismatch
    with pytest.raises(ValueError):
        ebsynth_run(s, g[:16], g)                                      # source guide size != style size
    with pytest.raises(ValueError):
        ebsynth_run(s, g, g, vote_mode="median")
    with pytest.raises(ValueError):
        ebsynth_run(s, g, g, search_vote_iters=[1, 2, 3, 4])           # 32x32, patch 5: 2 levels
    with pytest.raises(ValueError):
        ebsynth_run(s, g, g, style_weights=[1.0])
    with pytest.raises(ValueError):
        ebsynth_run(s, g, g, pyramid_levels=0)
    with pytest.raises(FrescoHipError):                                # no CPU fallback
        ebsynth_run(s, g, g)


def test_host_queries():
    from fresco_amd import _lib
    lib = _lib.load()
    r256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    S = T = 64 * 64
    # 3 + 10 channels fit one 16-byte record; 2 source + 3 target record images, 2 NNFs, E, 2 masks, 2 Omegas
    want = 2 * r256(S * 16) + 3 * r256(T * 16) + 2 * r256(T * 8) + r256(T * 4) + 2 * r256(T) + 2 * r256(S * 4)
    assert lib.fresco_ebsynth_workspace_bytes(3, 10, 64, 64, 64, 64, 5, -1, 0) == want
    assert lib.fresco_ebsynth_workspace_bytes(3, 10, 64, 64, 64, 64, 5, -1, 1) == want + 2 * r256(T * 16)
    assert lib.fresco_ebsynth_workspace_bytes(8, 24, 64, 64, 64, 64, 5, -1, 0) > want  # 32-byte records
    assert lib.fresco_ebsynth_workspace_bytes(9, 10, 64, 64, 64, 64, 5, -1, 0) == 0
    assert lib.fresco_ebsynth_workspace_bytes(3, 10, 64, 64, 64, 64, 4, -1, 0) == 0


@pytest.mark.parametrize("ns,ng,rec", [(3, 13, 16), (3, 14, 32)])
@pytest.mark.parametrize("with_mod", [0, 1])
def test_workspace_bytes_at_the_record_width_boundary(ns, ng, rec, with_mod):
    """16 style + guide channels fit one 16-byte record per pixel, 17 take two; a source 45x67 and a target 81x53 (sizes
    whose byte counts are not multiples of the 256-byte alignment) give these exact byte counts."""
    from fresco_amd import _lib
    r256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    S, T = 67 * 45, 53 * 81
    want = (2 * r256(S * rec) + 3 * r256(T * rec) + 2 * r256(T * 8) + r256(T * 4) + 2 * r256(T) + 2 * r256(S * 4)
            + with_mod * 2 * r256(T * rec))
    assert _lib.load().fresco_ebsynth_workspace_bytes(ns, ng, 67, 45, 53, 81, 5, -1, with_mod) == want


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_ebsynth_kernels_have_no_spills_or_scratch(tmp_path):
    """The method of tests/test_kernel_resources.py on ebsynth.hip: no kernel spills or uses scratch memory."""
    out = str(tmp_path / "ebsynth.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "fresco_amd", "csrc", "ebsynth.hip"), "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", open(out).read(), re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = (int(g("vgpr_spill_count")), int(g("private_segment_fixed_size")))
    names = [n for n in kernels if re.search(r"eb_(propagate|random_search|error_pass|vote|resample)", n)]
    assert len(names) >= 16, sorted(kernels)
    assert all(v == (0, 0) for v in kernels.values()), kernels
