"""The oracle against the unmodified reference on seeded RANDOM inputs (the goldens of tests/golden/ reference_outputs.npz are
closed-form inputs at one shape each; this widens the pin to random flows, occlusions, features and several sizes).  What the
reference returned for these inputs is stored in tests/golden/oracle_vs_reference_golden.npz (written by
tests/golden/make_oracle_vs_reference_golden.py, which also builds the inputs from their seeds)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_oracle_vs_reference_golden as G  # noqa: E402
from oracle import fresco_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def stored():
    """(arrays, {key: q / 2}): outputs kept on a grid of step q are within q / 2 of the reference's, so each bound below on
    |oracle - stored| is the original tolerance minus q / 2 (see make_oracle_vs_reference_golden.py)"""
    torch.set_num_threads(8)
    return G.load()


@pytest.fixture(scope="module")
def gold(stored):
    return stored[0]


@pytest.fixture(scope="module")
def half(stored):
    return stored[1]


def _inputs_match(gold, key, *tensors):
    """the seeded inputs are the ones the reference saw (a changed random stream would fail every comparison below)"""
    np.testing.assert_allclose(G.fingerprint(*tensors), gold["inputs/" + key].numpy(), rtol=1e-6, err_msg=key)


_video = G.video


def _maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("N,R,seed", G.FLOW_WARP_CASES)
def test_flow_warp_and_warp_tensor(gold, half, N, R, seed):
    key = "%d-%d-%d" % (N, R, seed)
    v = _video(N, R, seed)
    x = torch.randn(N, 5, R, R, generator=v["g"])
    fp = [x]
    with torch.no_grad():
        assert _maxdiff(O.flow_warp(x, v["bwd"]), gold["flow_warp/" + key]) < 2e-5 - half["flow_warp/" + key]
        for (C, h, chunk) in G.WARP_TENSOR_FORMS(R):
            s = torch.randn(chunk * N, C, h, h, generator=v["g"])
            fp.append(s)
            wkey = "warp_tensor/%s/%d-%d-%d" % (key, C, h, chunk)
            got = O.warp_tensor(s, [v["fwd"], v["bwd"]], [v["fo"], v["bo"]], v["sal"], chunk)
            assert _maxdiff(got, gold[wkey]) < 5e-5 - half[wkey]
    _inputs_match(gold, "flow_warp/" + key, v["fwd"], v["bwd"], v["sal"], *fp)


@pytest.mark.parametrize("N,R,seed,scale", G.MAPPING_CASES)
def test_mapping_ind_is_bit_exact(gold, N, R, seed, scale):
    key = "%d-%d-%d-%g" % (N, R, seed, scale)
    v = _video(N, R, seed)
    _inputs_match(gold, "mapping/" + key, v["bwd"], v["bo"], v["imgs"])
    want = [gold["mapping/%s/%d" % (key, j)] for j in range(3)]
    got = O.mapping_ind(v["bwd"], v["bo"], v["imgs"], scale=scale)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a.to(b.dtype), b)


@pytest.mark.parametrize("heads,C,seed", G.PROCESSOR_CASES)
@pytest.mark.parametrize("mode", G.PROCESSOR_MODES)
def test_processor(gold, half, heads, C, seed, mode):
    key = "%d-%d-%d" % (heads, C, seed)
    p = G.processor_inputs(heads, C, seed)
    v, W, hs, rf, cfm = p["v"], p["W"], p["hs"], p["rf"], p["cfm"]
    _inputs_match(gold, "processor/" + key, v["bwd"], v["bo"], v["imgs"], *W, hs, rf)
    # the reference's own fu.get_mapping_ind on these flows (test_mapping_ind_is_bit_exact pins the oracle's against it)
    fm, tm = gold["processor/%s/fwd_map" % key], gold["processor/%s/tmask" % key]
    with torch.no_grad():
        assert torch.equal(O.cross_frame_masks(v["bo"], scales=(p["scale"],))[0], cfm)
        kw = {}
        if mode == "full":
            kw = dict(ref=rf, use_cf=True, cf_mask=cfm, fwd_map=fm[:, 0], tmask=tm[:, 0])
        elif mode == "cf_temporal":
            kw = dict(use_cf=True, cf_mask=cfm, fwd_map=fm[:, 0], tmask=tm[:, 0])
        elif mode == "cf":
            kw = dict(use_cf=True, cf_mask=cfm)
        elif mode == "temporal":
            kw = dict(fwd_map=fm[:, 0], tmask=tm[:, 0])
        pkey = "processor/%s/%s" % (key, mode)
        want, h = gold[pkey], half[pkey]
        got = O.fresco_attention(hs, W[0], W[1], W[2], W[3], torch.zeros(C), heads, **kw)
        # the op-for-op port that bench.py times as `torch_gpu_baseline` (the "reference PyTorch path")
        from oracle import torch_path as TP
        got_tp = TP.processor_call(hs, W[0], W[1], W[2], W[3], torch.zeros(C), heads, **kw)
    tol = 1e-4 * max(1.0, float(want.abs().max()) - h)  # (<= the tolerance from the reference's own max)
    assert _maxdiff(got, want) < tol - h
    assert _maxdiff(got_tp, want) < tol - h


@pytest.mark.parametrize("C,h,seed", G.OPT_CASES)
def test_optimize_feature_one_and_three_iterations(gold, half, C, h, seed):
    key = "%d-%d-%d" % (C, h, seed)
    N, R = 4, 8 * h
    v = _video(N, R, seed)
    g = v["g"]
    x = torch.randn(2 * N, C, h, h, generator=g)
    t = torch.randn(2 * N, C, h, h, generator=g)
    _inputs_match(gold, "optimize/" + key, v["fwd"], v["bwd"], v["fo"], v["bo"], x, t)
    with torch.no_grad():
        vv = t.reshape(2 * N, C, h * h).transpose(1, 2)
        vv = vv / ((vv ** 2).sum(dim=2, keepdims=True) ** 0.5)
        corr = [torch.bmm(vv, vv.transpose(-1, -2)).float()]
        fl, oc = [v["fwd"], v["bwd"]], [v["fo"], v["bo"]]
        for iters in (1, 3):
            okey = "optimize/%s/%d" % (key, iters)
            want, q2 = gold[okey], half[okey]
            got = O.optimize_feature(x, fl, oc, corr, iters=iters)
            # L1 losses + Adam: a sign flip at a near-tie moves single elements by up to lr per iteration; the bulk agrees
            err = (got - want).abs()
            assert float(err.median()) < 1e-5 - q2 and float((err > 1e-3 - q2).float().mean()) < 0.01 * iters
            # the autograd + Adam port that bench.py times as cfg3's `torch_gpu_baseline`: the reference's own op sequence
            from oracle import torch_opt_path as TOP
            got_tp = TOP.optimize_feature(x, fl, oc, corr, iters=iters)
            err = (got_tp - want).abs()
            assert float(err.median()) < 1e-5 - q2 and float((err > 1e-3 - q2).float().mean()) < 0.01 * iters


@pytest.mark.parametrize("seed", G.ADAIN_SEEDS)
def test_adain_dilate_and_forward_backward_check(gold, seed):
    v = _video(4, 32, seed)
    g = v["g"]
    with torch.no_grad():
        a, b = torch.randn(6, 7, 9, 5, generator=g), 2.0 * torch.randn(6, 7, 9, 5, generator=g) + 0.5
        assert _maxdiff(O.adain(a, b), gold["adain/%d" % seed]) < 2e-5
        fp = [v["fwd"], v["bwd"], a, b]
        for k in G.DILATE_KERNELS:
            m = (torch.rand(3, 1, 32, 32, generator=g) < 0.05).float()
            fp.append(m)
            assert torch.equal(O.dilate(m, k), gold["dilate/%d/%d" % (seed, k)].float())
        fo, bo = gold["fbcheck/%d/fwd_occ" % seed], gold["fbcheck/%d/bwd_occ" % seed]
        fo2, bo2 = O.fb_consistency_check(v["fwd"], v["bwd"])
        assert torch.equal(fo2.float(), fo.float()) and torch.equal(bo2.float(), bo.float())
    _inputs_match(gold, "adain/%d" % seed, *fp)
