"""The MiDaS depth detector without a GPU: the restatement of tests/midas_model.py against the record of the reference's
code (tests/golden/midas_golden.npz), the state-dict names of both module trees against the reference's list, the folded
standardised weights, the tail against the reference detector's recorded maps (and cv2.Sobel where cv2 is installed), and the public
surface: the exported names, patch_midas, check_frames."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import midas_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


def _recorded_list(gold):
    shapes = [tuple(int(v) for v in s.split("x")) if s else () for s in gold["param_shapes"]]
    return list(zip(gold["param_names"].tolist(), shapes))


@pytest.fixture(scope="module")
def restated():
    return M.build()


def test_public_names_without_a_gpu():
    import fresco_amd
    for name in ("MidasDetector", "patch_midas", "DPTDepthModel"):
        assert name in fresco_amd.__all__ and hasattr(fresco_amd, name), name
    from fresco_amd import _lib
    assert set(_lib.MIDAS_SIGNATURES) == {
        "midas_input", "midas_stem_conv", "midas_groupnorm_workspace_bytes", "midas_groupnorm_stats", "midas_groupnorm_apply",
        "midas_pool", "midas_layernorm", "midas_tokens", "midas_head_merge", "midas_rowbias_gelu",
        "midas_tail_workspace_bytes", "midas_tail"}
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "fresco_midas.h")).read()
    for name in _lib.MIDAS_SIGNATURES:
        assert "%s(" % name in header, name


def test_state_dict_names_equal_the_reference_list(gold, restated):
    import fresco_amd
    want = _recorded_list(gold)
    assert M.module_names_shapes(restated) == want
    ours = M.module_names_shapes(fresco_amd.DPTDepthModel())
    assert sorted(ours) == sorted(want)
    names = dict(want)
    for name, shape in (("pretrained.model.patch_embed.backbone.stem.conv.weight", (64, 3, 7, 7)),
                        ("pretrained.model.blocks.11.attn.qkv.weight", (2304, 768)),
                        ("pretrained.model.pos_embed", (1, 577, 768)),
                        ("pretrained.act_postprocess3.0.project.0.weight", (768, 1536)),
                        ("pretrained.act_postprocess4.4.weight", (768, 768, 3, 3)),
                        ("scratch.refinenet4.resConfUnit1.conv1.weight", (256, 256, 3, 3)),
                        ("scratch.output_conv.4.bias", (1,))):
        assert names[name] == shape, name


def test_module_loads_a_checkpoint_file_strictly(gold, tmp_path):
    import fresco_amd
    from fresco_amd import midas
    sd = M.standin_state_dict(_recorded_list(gold))
    plain, wrapped = str(tmp_path / "plain.pt"), str(tmp_path / "wrapped.pt")
    torch.save(sd, plain)
    torch.save({"optimizer": {}, "model": sd}, wrapped)
    for path in (plain, wrapped):
        net = midas.load_checkpoint(fresco_amd.DPTDepthModel(), path)
        got = net.state_dict()
        assert all(torch.equal(got[k], v) for k, v in sd.items())
    bad = dict(sd)
    bad.pop("scratch.output_conv.4.bias")
    torch.save(bad, plain)
    with pytest.raises(RuntimeError):
        midas.load_checkpoint(fresco_amd.DPTDepthModel(), plain)
    with pytest.raises(FileNotFoundError, match="downloads nothing"):
        fresco_amd.MidasDetector(model_path=str(tmp_path / "missing.pt"))


@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_restatement_reproduces_the_record(case, gold, restated):
    """frame by frame, as the record was made.  PyTorch's CPU kernels sum in an order that depends on the machine's thread count, so another machine
    reproduces the record to the rounding noise, not to the bit: the bars are those of the GPU tests -- 4 x the reference's
    recorded fp32-vs-float64 noise per tensor, uint8 values at most 1 apart in at most 2 %."""
    key = M.case_key(case)
    fr = M.frames(case)
    assert M.digest(fr) == str(gold[key + "_sha256"])
    taps, depth = {t: [] for t in M.TAPS}, []
    with torch.no_grad():
        for f in range(case[0]):
            t = {}
            depth.append(restated(M.network_input(fr[f:f + 1]), t))
            for name in M.TAPS:
                taps[name].append(t[name])
    depth = torch.cat(depth).numpy()
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    for i, name in enumerate(M.TAPS):
        got = M.thin(torch.cat(taps[name]))
        rec = gold["%s_%s" % (key, name)]
        assert got.shape == rec.shape and np.abs(got - rec).max() <= 4 * noise[i] * peak[i], name
    assert np.abs(M.thin_depth(depth) - gold[key + "_depth"]).max() <= 4 * noise[-1] * peak[-1]
    for f in range(case[0]):
        dimg, nimg = M.tail(depth[f])
        for got, rec in ((dimg, gold[key + "_depth_image"][f]), (nimg, gold[key + "_normal_image"][f])):
            diff = np.abs(got.astype(int) - rec.astype(int))
            assert diff.max() <= 1 and (diff > 0).mean() <= 0.02


def test_the_record_holds_what_the_gpu_tests_rely_on(gold):
    for case in M.CASES:
        key = M.case_key(case)
        assert gold[key + "_noise"].shape == gold[key + "_peak"].shape == (len(M.TAPS) + 1,)
        assert 0 < gold[key + "_noise"].max() < 1e-4
        share_d, max_d, share_n, max_n = gold[key + "_u8_noise"]
        assert share_d < 0.005 and share_n < 0.005 and max_d <= 1 and max_n <= 1
        dimg = gold[key + "_depth_image"]
        assert dimg.shape == case and gold[key + "_normal_image"].shape == case + (3,)
        for f in range(case[0]):
            assert dimg[f].min() == 0 and dimg[f].max() == 255
            assert (dimg[f] < 25).any() and (dimg[f] > 26).any()  # both sides of bg_th = 0.1
    d = gold[M.case_key(M.CASES[0]) + "_depth"]
    assert d[0].min() != d[1].min() and d[0].max() != d[1].max()


def test_folded_standardised_weights_equal_stdconv_arithmetic():
    from fresco_amd import midas
    w = torch.randn(64, 32, 3, 3, generator=torch.Generator().manual_seed(0)) * 0.3 + 0.05
    got = midas.standardise(w.double())
    # StdConv2dSame.forward: F.batch_norm over the (1, cout, fan_in) view in training mode = per-row mean / biased variance
    want = F.batch_norm(w.double().reshape(1, 64, -1), None, None, training=True, momentum=0.0, eps=1e-8).reshape_as(w)
    assert float((got - want).abs().max()) < 1e-12
    assert float(got.mean(dim=(1, 2, 3)).abs().max()) < 1e-12
    assert float((got.var(dim=(1, 2, 3), unbiased=False) - 1).abs().max()) < 1e-6
    assert torch.equal(midas.standardise(w), M.standardise(w))
    for size, k, s, want_pad in ((64, 7, 2, (2, 3)), (64, 3, 2, (0, 1)), (63, 3, 2, (1, 1)), (64, 3, 1, (1, 1)), (64, 1, 2, (0, 0))):
        assert midas.same_padding(size, k, s) == want_pad == M.same_pad(size, k, s)


def test_pos_embed_is_resized_once_per_geometry():
    from fresco_amd import midas
    net = midas.DPTDepthModel()
    with torch.no_grad():
        net.pretrained.model.pos_embed.normal_()
    p = net.pos_embed_for(4, 6)
    assert p.shape == (25, 768) and net.pos_embed_for(4, 6) is p
    assert torch.equal(p, M.resize_pos_embed(net.pretrained.model.pos_embed.detach(), 4, 6)[0])
    assert torch.equal(net.pos_embed_for(24, 24), net.pretrained.model.pos_embed.detach()[0])
    with torch.no_grad():
        net.pretrained.model.pos_embed.mul_(2.0)
    assert torch.equal(net.pos_embed_for(4, 6), 2.0 * p)


def test_tail_model_equals_the_detector_on_the_recorded_depth(gold):
    """the golden maker ran the reference's own MidasDetector.__call__ and recorded its two maps; on the recorded fp32 depth
    of the same frames the restated tail gives those maps, value for value"""
    for case in M.FULL_DEPTH_CASES:
        key = M.case_key(case)
        depth = gold[key + "_depth_full"]
        assert depth.shape == case and depth.dtype == np.float32
        assert np.array_equal(M.thin_depth(depth), gold[key + "_depth"])
        for f in range(case[0]):
            dimg, nimg = M.tail(depth[f])
            assert np.array_equal(dimg, gold[key + "_depth_image"][f]) and np.array_equal(nimg, gold[key + "_normal_image"][f])


def test_tail_model_masks_flat_regions_and_sobel_is_the_3x3_correlation():
    rs = np.random.RandomState(11)
    depth = (3.0 + 40.0 * rs.rand(36, 52)).astype(np.float32)
    depth[4:14, 6:20] = 3.0
    d1, n1 = M.tail(depth)
    assert (n1[6:12, 8:18] == (127, 127, 255)).all() and d1.min() == 0 and d1.max() == 255
    flat_d, flat_n = M.tail(np.full((8, 8), 2.5, np.float32))
    assert not flat_d.any() and (flat_n == (127, 127, 255)).all()
    # the Sobel restatement against its definition as a full 3 x 3 correlation in float64
    p = np.pad(depth.astype(np.float64), 1, mode="reflect")
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float64)
    full = lambda k: sum(k[i, j] * p[i:i + 36, j:j + 52] for i in range(3) for j in range(3))  # noqa: E731
    assert np.abs(M.sobel(depth, 1, 0) - full(kx)).max() < 1e-3 and np.abs(M.sobel(depth, 0, 1) - full(kx.T)).max() < 1e-3
    try:
        import cv2
    except ImportError:
        return
    assert np.array_equal(M.sobel(depth, 1, 0), cv2.Sobel(depth, cv2.CV_32F, 1, 0, ksize=3))
    assert np.array_equal(M.sobel(depth, 0, 1), cv2.Sobel(depth, cv2.CV_32F, 0, 1, ksize=3))


def test_patch_midas_rebinds_a_module():
    import fresco_amd
    mod = types.ModuleType("annotator_midas_standin")
    mod.MidasDetector = object
    assert fresco_amd.patch_midas(mod) is mod and mod.MidasDetector is fresco_amd.MidasDetector


def test_check_frames_refuses_bad_sizes():
    from fresco_amd import midas
    ok = np.zeros((64, 96, 3), np.uint8)
    assert tuple(midas.check_frames(ok).shape) == (1, 64, 96, 3)
    assert tuple(midas.check_frames([ok, ok]).shape) == (2, 64, 96, 3)
    for H, W in ((48, 64), (64, 80), (72, 88), (16, 64)):
        with pytest.raises(ValueError, match="multiples of 32"):
            midas.check_frames(np.zeros((H, W, 3), np.uint8))
    with pytest.raises(ValueError, match="share a size"):
        midas.check_frames([ok, np.zeros((64, 64, 3), np.uint8)])
    with pytest.raises(TypeError):
        midas.check_frames(np.zeros((64, 96, 3), np.float32))
    with pytest.raises(ValueError):
        midas.check_frames(torch.zeros(1, 64, 96, 4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        midas.condition_dtype(torch.float64)
    with pytest.raises(fresco_amd_error()):
        midas.DPTDepthModel().depth(torch.zeros(1, 64, 96, 3, dtype=torch.uint8))  # CPU frames: no fallback


def fresco_amd_error():
    import fresco_amd
    return fresco_amd.FrescoHipError
