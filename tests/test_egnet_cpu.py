"""fresco_amd.egnet without a GPU: the module tree against the reference's recorded state dict, the library-ops forward and
its live-graph restatement against the records of the unmodified reference network (tests/golden/egnet_golden.npz), the
float64 BatchNorm folding, the argument checks of get_saliency, the rebinding of patch_saliency, and the new C entry
points on the header / binding surface of the library."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import egnet_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("fresco_egnet_input", "fresco_egnet_pool", "fresco_egnet_resize_add", "fresco_egnet_saliency")


@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def net():
    from fresco_amd import egnet
    net = egnet.build_model("resnet")
    net.load_state_dict(M.standin_state_dict(), strict=True)
    return net.float().eval()


def test_state_dict_names_and_shapes_are_the_reference_s(gold):
    from fresco_amd import egnet
    sd = egnet.build_model("resnet").state_dict()
    assert list(sd.keys()) == list(gold["param_names"])
    assert ["x".join(map(str, v.shape)) for v in sd.values()] == list(gold["param_shapes"])
    assert list(M.param_shapes()) == list(gold["param_names"])
    assert str(gold["weights_sha256"]) == M.weights_digest()
    with pytest.raises(NotImplementedError):
        egnet.build_model("vgg")


def test_default_build_is_the_resnet_and_exports():
    import fresco_amd
    from fresco_amd import egnet
    assert isinstance(fresco_amd.build_model(), fresco_amd.TUN_bone)
    assert fresco_amd.get_saliency is egnet.get_saliency and fresco_amd.patch_saliency is egnet.patch_saliency
    assert sum(isinstance(m, torch.nn.Conv2d) for m in fresco_amd.build_model().modules()) == 103


@pytest.mark.parametrize("case", M.CASES + M.WIDE_CASES, ids=M.case_key)
def test_forward_and_live_graph_reproduce_the_reference_records(gold, net, case):
    """library ops on the CPU: the logit, the saliency map and every tap within the fp32 record's own distance e_ref from the
    float64 one, at the bar the GPU tests hold the native path to, 8 e_ref + 1e-7 (saliency + 1e-6) -- the same weights
    and input in the same precision, but another thread count blocks the convolutions' sums differently, which is another
    sample of the same rounding noise (in one process with the recording script the results are equal bit for bit); the
    live graph EQUAL to forward's up_sal_final[-1]"""
    key = M.case_key(case)
    fr = M.frames(case)
    assert str(gold[key + "_sha256"]) == M.digest(fr)
    x = M.cv2sod64(fr, torch.float32)
    taps = {}
    with torch.no_grad():
        up_edge, up_sal, up_sal_final = net(x)
        live = net.live_logit(x, taps)
    assert len(up_edge) == 1 and len(up_sal) == 4 and len(up_sal_final) == 5
    assert all(t.shape == (case[0], 1) + tuple(x.shape[2:]) for t in up_edge + up_sal + up_sal_final)
    assert torch.equal(live, up_sal_final[-1])
    l32, l64 = M.golden_pair(gold, key + "_logit")
    e_ref = np.abs(l32 - l64).max()
    got = live[:, 0].double().numpy()
    print("%s: logit |got - f64| %.2e, record's own %.2e" % (key, np.abs(got - l64).max(), e_ref))
    assert np.abs(got - l64).max() <= 8 * e_ref + 1e-7
    s32, s64 = M.golden_pair(gold, key + "_saliency")
    sal = M.saliency_from_logit(live).double().numpy()
    assert np.abs(sal - s64).max() <= 8 * np.abs(s32 - s64).max() + 1e-6
    assert list(taps) == list(M.TAPS)
    for name in M.TAPS:
        t32, t64 = M.golden_pair(gold, "%s_%s" % (key, name))
        t = taps[name][:, ::M.TAP_STRIDE].permute(0, 2, 3, 1).double().numpy()
        assert t.shape == t64.shape, name
        assert np.abs(t - t64).max() <= 8 * np.abs(t32 - t64).max() + 1e-7, name


def test_golden_saliency_is_not_trivial(gold):
    for case in M.CASES + M.WIDE_CASES:
        s = gold[M.case_key(case) + "_saliency_f32"]
        assert (s == 0).mean() >= 0.10 and (s > 0.9).mean() >= 0.10 and ((s > 0) & (s <= 0.9)).mean() >= 0.05


def test_batchnorm_folding_in_float64_equals_conv_then_bn(net):
    """weight rows x gamma / sqrt(var + eps), bias = beta - mean gamma / sqrt(var + eps): the folded convolution against
    conv + BatchNorm in float64, for a plain, a strided, a dilated and the stem convolution"""
    base = net.base
    pairs = [(base.layer1[0].conv1, base.layer1[0].bn1), (base.layer2[0].downsample[0], base.layer2[0].downsample[1]),
             (base.layer4[1].conv2, base.layer4[1].bn2), (base.conv1, base.bn1)]
    g = torch.Generator().manual_seed(5)
    for conv, bn in pairs:
        x = torch.randn(2, conv.in_channels, 9, 11, generator=g, dtype=torch.float64)
        kw = dict(stride=conv.stride, padding=conv.padding, dilation=conv.dilation)
        want = F.batch_norm(F.conv2d(x, conv.weight.double(), None, **kw), bn.running_mean.double(), bn.running_var.double(),
                            bn.weight.double(), bn.bias.double(), False, 0.0, bn.eps)
        scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w = conv.weight.double() * scale.view(-1, 1, 1, 1)
        b = bn.bias.double() - bn.running_mean.double() * scale
        got = F.conv2d(x, w, b, **kw)
        assert float((got - want).detach().abs().max()) <= 1e-12 * max(1.0, float(want.detach().abs().max()))


def test_folded_cache_key_covers_the_batchnorm_tensors(net, monkeypatch):
    """WeightPlanes.get_folded makes new planes when a BatchNorm tensor changes, not only when the weight does (the split
    pass itself needs the GPU: stubbed here by one that keeps the fp32 matrix)"""
    from fresco_amd import fnweights, ops

    class Guard:
        def __init__(self, device):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def tripped(self):
            return False

    monkeypatch.setattr(ops, "fn_range_guard", Guard)
    monkeypatch.setattr(ops, "fn_prep", lambda w, scale: (None, (w.clone(), None)))
    import copy
    blk = copy.deepcopy(net.base.layer1[1])
    wts = fnweights.WeightPlanes()
    (w0, _), b0 = wts.get_folded(blk.conv1.weight, blk.bn1, "conv")
    (w1, _), b1 = wts.get_folded(blk.conv1.weight, blk.bn1, "conv")
    assert w1 is w0 and b1 is b0  # served from the cache
    s = (blk.bn1.weight.double() / torch.sqrt(blk.bn1.running_var.double() + blk.bn1.eps))
    assert torch.equal(w0, (blk.conv1.weight.double() * s.view(-1, 1, 1, 1)).float().reshape(w0.shape))
    assert torch.equal(b0, (blk.bn1.bias.double() - blk.bn1.running_mean.double() * s).float())
    with torch.no_grad():
        blk.bn1.running_var.mul_(4.0)
    (w2, _), b2 = wts.get_folded(blk.conv1.weight, blk.bn1, "conv")
    assert w2 is not w0 and torch.allclose(w2, w0 / 2, rtol=1e-4) and not torch.equal(b2, b0)
    with torch.no_grad():
        blk.bn1.bias.add_(1.0)
    assert torch.allclose(wts.get_folded(blk.conv1.weight, blk.bn1, "conv")[1], b2 + 1.0)


def test_get_saliency_argument_errors(net):
    from fresco_amd import egnet

    class Dil:
        kernel_size = 7

    ok = [np.zeros((64, 64, 3), np.uint8)] * 2
    foreign = torch.nn.Sequential(torch.nn.Conv2d(3, 1, 1))
    with pytest.raises(TypeError, match="no fallback"):
        egnet.get_saliency(ok, foreign, Dil())
    with pytest.raises(ValueError, match="share a size"):
        egnet.get_saliency([np.zeros((64, 64, 3), np.uint8), np.zeros((64, 66, 3), np.uint8)], net, Dil())
    for shape in ((31, 64, 3), (64, 30, 3)):
        with pytest.raises(ValueError, match="at least 32"):
            egnet.get_saliency([np.zeros(shape, np.uint8)], net, Dil())
    with pytest.raises(TypeError):
        egnet.get_saliency([np.zeros((64, 64, 3), np.float32)], net, Dil())
    with pytest.raises(TypeError):
        egnet.get_saliency(torch.zeros(1, 64, 64, 3), net, Dil())
    with pytest.raises(ValueError):
        egnet.get_saliency([], net, Dil())
    with pytest.raises(ValueError):
        egnet.TUN_bone(split_scales=(64.0,) * 5)
    with pytest.raises(ValueError):
        egnet.TUN_bone(split_scales=(48.0,) * len(egnet.STAGES))
    with pytest.raises(ValueError):
        egnet.TUN_bone(max_frames=0)


def test_patch_saliency_rebinds_the_names(monkeypatch):
    from fresco_amd import egnet
    star = types.ModuleType("run_fresco_standin")  # a module that star-imported src.utils and imported build_model
    star.get_saliency = star.build_model = lambda *a: None
    assert egnet.patch_saliency(star) is star
    assert star.get_saliency is egnet.get_saliency and star.build_model is egnet.build_model
    # the defaults: src.utils and the reference's EGNet `model` module (run_fresco puts src/EGNet on sys.path)
    src, utils, model = types.ModuleType("src"), types.ModuleType("src.utils"), types.ModuleType("model")
    src.utils = utils
    utils.get_saliency = lambda *a: None
    model.TUN_bone, model.build_model = object, lambda *a: None
    for name, mod in (("src", src), ("src.utils", utils), ("model", model)):
        monkeypatch.setitem(sys.modules, name, mod)
    assert egnet.patch_saliency() is utils
    assert utils.get_saliency is egnet.get_saliency and not hasattr(utils, "build_model")
    assert model.build_model is egnet.build_model


def test_new_entry_points_are_on_the_c_abi_surface():
    """The four entry points are part of libfresco_hip.so and include/fresco_hip.h (section m), which
    tests/test_capi_surface_cpu.py compares as whole sets: header prototypes == binding == exported functions.  Per new
    symbol here: the header's argument list is the binding's, the return type is int, the symbol is exported -- and
    fresco_fn_gemm carries its dilation argument."""
    import ctypes
    import test_capi_surface_cpu as surface
    from fresco_amd import _lib
    protos = surface._prototypes()
    exported = surface._exported_fresco_functions(_lib.LIB_PATH)
    assert {n for n in protos if "egnet" in n} == set(NEW_SYMBOLS)
    assert {n for n in exported if "egnet" in n} == set(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert protos[name][0] is ctypes.c_int, name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and list(_lib.SIGNATURES[name][1]) == protos[name][1], name
    surface.test_binding_matches_the_header_prototypes()
    gemm = protos["fresco_fn_gemm"][1]
    assert len(gemm) == 33 and gemm[17:25] == [ctypes.c_int] * 8  # n_img, H, W, kh, kw, stride, pad, dilation


def test_entry_points_check_their_arguments_before_any_launch():
    from fresco_amd import _lib
    lib = _lib.load()
    p = 4096  # fake, aligned, never touched
    EINVAL, EUNSUPPORTED = -1, -2
    assert lib.fresco_egnet_input(None, p, 1, 64, 64, None) == EINVAL
    assert lib.fresco_egnet_input(p, p, 1, 1, 64, None) == EUNSUPPORTED
    assert lib.fresco_egnet_input(p, p, 0, 64, 64, None) == EINVAL
    assert lib.fresco_egnet_pool(p, None, p, None, 1, 16, 16, 64, 64.0, None, None) == EINVAL
    assert lib.fresco_egnet_pool(p, None, p, p, 1, 16, 16, 128, 64.0, None, None) == EUNSUPPORTED
    assert lib.fresco_egnet_pool(p + 4, None, p, p, 1, 16, 16, 64, 64.0, None, None) == EINVAL
    assert lib.fresco_egnet_pool(p, None, p, p, 1, 16, 16, 64, 0.0, None, None) == EINVAL
    assert lib.fresco_egnet_resize_add(p, None, None, None, None, 1, 3, 3, 5, 5, 128, 0, 64.0, None, None) == EINVAL
    assert lib.fresco_egnet_resize_add(p, None, p, p, None, 1, 3, 3, 5, 5, 128, 0, 64.0, None, None) == EINVAL
    assert lib.fresco_egnet_resize_add(p, None, p, None, None, 1, 3, 3, 5, 5, 48, 0, 64.0, None, None) == EUNSUPPORTED
    assert lib.fresco_egnet_resize_add(p, None, p, None, None, 1, 3, 3, 5, 5, 544, 0, 64.0, None, None) == EUNSUPPORTED
    assert lib.fresco_egnet_resize_add(p, p + 8, p, None, None, 1, 3, 3, 5, 5, 128, 0, 64.0, None, None) == EINVAL
    assert lib.fresco_egnet_saliency(p, None, None, 1, 8, 8, 32, 32, 7, None) == EINVAL
    assert lib.fresco_egnet_saliency(p, p, None, 1, 8, 8, 32, 32, 6, None) == EUNSUPPORTED
    assert lib.fresco_egnet_saliency(p, p, None, 1, 8, 8, 32, 32, 17, None) == EUNSUPPORTED
    assert lib.fresco_egnet_saliency(p, p, None, 1, 8, 0, 32, 32, 7, None) == EINVAL
    # the GEMM's dilation: checked like stride and pad
    gemm = lambda dil, M_=25: lib.fresco_fn_gemm(p, p, 64, p, p, None, p, None, None, 64, 64, M_, 64, 9 * 64, 0, 1.0, 64.0,  # noqa: E731
                                                1, 5, 5, 3, 3, 1, 2, dil, None, p, None, None, None, 0, 0, None)
    assert gemm(0) == EINVAL
    assert gemm(3) == EINVAL      # 5 + 4 - 6 - 1 + 1 = 3 x 3 outputs, not M = 25
    assert gemm(5) == EINVAL      # a window wider than the padded map
