"""The UNet resnet block without a GPU: the restatement of tests/unet_resnet_model.py against torch's functional operators
composed directly, the golden file against a fresh derivation, patch_unet_resnets / unpatch_unet_resnets on a stand-in tree
(count, restored forwards, every refusal), and the argument checks of unet_groupnorm and unet_temb with fake pointers
(every check answers before any HIP call)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import unet_resnet_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 64)])
def test_restatement_is_the_functional_composition(cin, cout):
    net = M.build(cin, cout, torch.float64)
    sd = net.state_dict()
    gen = torch.Generator().manual_seed(cin)
    x = torch.randn(2, cin, 5, 7, generator=gen, dtype=torch.float64)
    temb = torch.randn(2, M.TEMB_CHANNELS, generator=gen, dtype=torch.float64)
    taps = {}
    with torch.no_grad():
        got = net(x, temb, taps=taps)
    h = F.conv2d(F.silu(F.group_norm(x, 32, sd["norm1.weight"], sd["norm1.bias"], M.EPS)), sd["conv1.weight"], sd["conv1.bias"],
                 padding=1)
    h = h + F.linear(F.silu(temb), sd["time_emb_proj.weight"], sd["time_emb_proj.bias"])[:, :, None, None]
    assert torch.allclose(taps["tap"], h.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    h = F.conv2d(F.silu(F.group_norm(h, 32, sd["norm2.weight"], sd["norm2.bias"], M.EPS)), sd["conv2.weight"], sd["conv2.bias"],
                 padding=1)
    skip = F.conv2d(x, sd["conv_shortcut.weight"], sd["conv_shortcut.bias"]) if cin != cout else x
    assert ("conv_shortcut.weight" in sd) == (cin != cout)
    assert torch.allclose(got, skip + h, rtol=0, atol=1e-12)
    # the rounded run rounds: it differs from the float64 one, by fp16-class noise
    with torch.no_grad():
        r = net(x, temb, M.round16)
    d = float((r - got).abs().max() / got.abs().max())
    assert 0 < d < 1e-2


def test_golden_file_is_current():
    gold = M.load_golden(GOLDEN)
    assert sorted(gold) == sorted(M.case_key(c) + s for c in M.CASES for s in ("_tap", "_out", "_noise", "_peak"))
    case = M.CASES[-1]  # (640, 1280, 1, 4, 4): the cheapest to derive again
    key = M.case_key(case)
    tap, out, noise, peaks, act = M.record(case)
    assert act < M.ACT_LIMIT
    np.testing.assert_allclose(gold[key + "_tap"], M.thin(tap), rtol=0, atol=1e-9)
    np.testing.assert_allclose(gold[key + "_out"], M.thin(out), rtol=0, atol=1e-9)
    np.testing.assert_allclose(gold[key + "_noise"], noise, rtol=1e-3)
    np.testing.assert_allclose(gold[key + "_peak"], peaks, rtol=1e-9)
    for c in M.CASES:
        k = M.case_key(c)
        assert gold[k + "_tap"].shape == gold[k + "_out"].shape and gold[k + "_tap"].shape[0] == c[2]
        assert gold[k + "_noise"].shape == (2,) and (gold[k + "_noise"] > 0).all() and (gold[k + "_noise"] < 2e-3).all()
        x, temb = M.inputs(c)
        assert x.shape == (c[2], c[0], c[3], c[4]) and temb.shape == (c[2], M.TEMB_CHANNELS)
    x, _ = M.inputs(M.CASES[0])  # the last image differs in offset
    assert abs(float(x[0].float().mean())) < 0.1 and abs(float(x[-1].float().mean()) - 1.0) < 0.1


# ---------------------------------------------------------------------------------------------------------------------
# patching (packing the weights needs no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _tree():
    return M.build_tree(torch.float16, c=64)


def test_patch_and_unpatch_on_a_standin_tree():
    from fresco_amd import UNetResnet, patch_unet_resnets, unpatch_unet_resnets
    tree = _tree()
    blocks = [m for m in tree.modules() if isinstance(m, M.Resnet)]
    assert len(blocks) == 2
    assert patch_unet_resnets(tree) == 2
    for b in blocks:
        native = vars(b)["forward"]
        assert isinstance(native, UNetResnet) and native.memory_format == torch.channels_last
        assert (native.cin, native.cout) == (b.conv1.in_channels, b.conv1.out_channels)
        assert (native.ws is not None) == (b.conv_shortcut is not None)
        assert native.w1.shape == (native.cout, 9 * native.cin) and native.w1.dtype == torch.float16
        # k = (ky, kx, ci): the packed matrix is the weight with the input channels last
        assert torch.equal(native.w1.view(native.cout, 3, 3, native.cin), b.conv1.weight.permute(0, 2, 3, 1))
        assert native.cb1.dtype == torch.float32 and torch.equal(native.cb1, b.conv1.bias.float())
    assert "forward" not in vars(tree) and "forward" not in vars(tree.proj)
    assert patch_unet_resnets(tree, memory_format=torch.contiguous_format) == 2   # patching again replaces, it does not stack
    assert vars(blocks[0])["forward"].memory_format == torch.contiguous_format
    assert unpatch_unet_resnets(tree) == 2
    for b in blocks:
        assert "forward" not in vars(b) and b.forward.__func__ is M.Resnet.forward
    assert unpatch_unet_resnets(tree) == 0
    x, temb = torch.randn(1, 64, 4, 4), torch.randn(1, M.TEMB_CHANNELS)
    with torch.no_grad():
        assert tree.float()(x, temb).shape == (1, 16, 64)   # the module's own forwards run again
    with pytest.raises(ValueError, match="memory_format"):
        patch_unet_resnets(tree, memory_format=torch.preserve_format)


def _refused(change, match):
    from fresco_amd import patch_unet_resnets
    tree = _tree()
    change(tree.up["resnets"][0])
    with pytest.raises(NotImplementedError, match=match) as e:
        patch_unet_resnets(tree)
    assert "up.resnets.0" in str(e.value)           # refused by name ...
    assert not any("forward" in vars(m) for m in tree.modules())   # ... before anything is patched


def test_refusals():
    _refused(lambda b: b.float(), "fp16 blocks only")
    _refused(lambda b: b.bfloat16(), "fp16 blocks only")
    _refused(lambda b: setattr(b, "time_embedding_norm", "scale_shift"), "time_embedding_norm")
    _refused(lambda b: setattr(b, "up", True), "samples up or down")
    _refused(lambda b: setattr(b, "down", True), "samples up or down")
    _refused(lambda b: setattr(b, "output_scale_factor", 2.0), "output_scale_factor")

    def groups16(b):
        b.norm2 = nn.GroupNorm(16, 64).half()
    _refused(groups16, "GroupNorm of 16 groups")

    def narrow(b):     # 32 channels: below the kernel's range
        b.conv1 = nn.Conv2d(128, 32, 3, 1, 1).half()
    _refused(narrow, "128 -> 32 channels")

    def wide(b):       # 2624 = 41 x 64: above it
        b.conv1 = nn.Conv2d(2624, 64, 3, 1, 1).half()
    _refused(wide, "2624 -> 64 channels")

    def odd(b):        # 96: not a multiple of 64
        b.conv1 = nn.Conv2d(96, 64, 3, 1, 1).half()
    _refused(odd, "96 -> 64 channels")
    _refused(lambda b: setattr(b, "time_emb_proj", None), "has no time_emb_proj")
    _refused(lambda b: setattr(b, "nonlinearity", nn.GELU()), "only swish")


def test_constructor_checks_the_state_dict():
    from fresco_amd import UNetResnet
    net = M.build(64, 128, torch.float16)
    sd = {"mid.resnets.0." + k: v for k, v in net.state_dict().items()}
    r = UNetResnet(sd, "mid.resnets.0", 64, 128)
    assert r.ws.shape == (128, 64) and r.wt.shape == (128, M.TEMB_CHANNELS) and r.eps == 1e-5
    with pytest.raises(ValueError, match="conv_shortcut present"):
        UNetResnet(sd, "mid.resnets.0", 128, 128)
    with pytest.raises(ValueError, match="conv1.weight"):
        UNetResnet(sd, "mid.resnets.0", 64, 192)
    with pytest.raises(ValueError, match="missing"):
        UNetResnet(sd, "mid.resnets.1", 64, 128)
    with pytest.raises(ValueError, match="conv_shortcut missing"):
        UNetResnet({k: v for k, v in sd.items() if "shortcut" not in k}, "mid.resnets.0", 64, 128)
    with pytest.raises(TypeError, match="fp16"):
        UNetResnet({k: v.float() for k, v in sd.items()}, "mid.resnets.0", 64, 128)
    with pytest.raises(TypeError, match="fp16 x only"):
        r(torch.zeros(1, 64, 4, 4), torch.zeros(1, M.TEMB_CHANNELS, dtype=torch.float16))
    from fresco_amd import FrescoHipError
    with pytest.raises(FrescoHipError, match="GPU only"):   # no fallback on CPU tensors
        r(torch.zeros(1, 64, 4, 4, dtype=torch.float16), torch.zeros(1, M.TEMB_CHANNELS, dtype=torch.float16))


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points' argument checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


def test_groupnorm_argument_checks(lib):
    p = 4096  # fake, aligned, never touched
    n, P, C = 2, 4096, 320       # the three-launch form: a workspace of partial sums
    need = lib.unet_groupnorm_workspace_bytes(n, P, C)
    assert lib.unet_groupnorm_lds_form(n, P, C) == 0
    assert need >= n * (P // 64) * 32 * 2 * 8 + n * 32 * 2 * 4

    def call(x=p, addend=None, gamma=p, beta=p, y=p, ws=p, wsb=need, n=n, P=P, C=C, eps=1e-5):
        return lib.unet_groupnorm(x, addend, gamma, beta, y, ws, wsb, n, P, C, eps, 1, None)

    for C_bad in (96, 2624, 32, 2500):
        assert call(C=C_bad) == EUNSUPPORTED
        assert lib.unet_groupnorm_workspace_bytes(n, P, C_bad) == 0 and lib.unet_groupnorm_lds_form(n, P, C_bad) == -1
    assert call(wsb=need - 1) == EWORKSPACE
    assert call(wsb=0) == EWORKSPACE
    for null in ("x", "gamma", "beta", "y", "ws"):
        assert call(**{null: None}) == EINVAL
    assert call(n=0) == EINVAL and call(P=0) == EINVAL and call(C=-64) == EINVAL and call(eps=-1.0) == EINVAL
    assert call(eps=float("nan")) == EINVAL
    assert call(x=p + 8) == EINVAL and call(addend=p + 4) == EINVAL and call(y=p + 2) == EINVAL
    assert call(n=65536, wsb=1 << 40) == EUNSUPPORTED
    assert call(n=1024, P=1 << 21, wsb=1 << 40) == EUNSUPPORTED      # n P = 2^31 pixels
    assert lib.unet_groupnorm_workspace_bytes(0, P, C) == 0 and lib.unet_groupnorm_workspace_bytes(n, 0, C) == 0
    # the LDS form takes a nominal workspace: the size is never 0 for a shape that is accepted
    assert lib.unet_groupnorm_lds_form(n, 64, C) == 1 and lib.unet_groupnorm_workspace_bytes(n, 64, C) > 0
    assert call(P=64, wsb=0) == EWORKSPACE


def test_the_switch_between_the_two_forms(lib):
    """the plane of one slab (G groups, the fewest whose bytes are a multiple of 16) against UG_LDS_PLANE_BYTES = 96 KiB"""
    slab_bytes = {320: 80, 640: 80, 960: 240, 1280: 80, 1920: 240, 2560: 160, 64: 16, 128: 16, 192: 48}
    for C, b in slab_bytes.items():
        pmax = 96 * 1024 // b
        assert lib.unet_groupnorm_lds_form(2, pmax, C) == 1 and lib.unet_groupnorm_lds_form(2, pmax + 1, C) == 0, C
    # the SD-1.5 shapes: every 8 x 8 and 16 x 16 plane and 32 x 32 at 640 and 1280 take the LDS form
    for C in (320, 640, 960, 1280, 1920, 2560):
        assert lib.unet_groupnorm_lds_form(16, 64, C) == 1 and lib.unet_groupnorm_lds_form(16, 256, C) == 1
        assert lib.unet_groupnorm_lds_form(16, 1024, C) == (1 if C in (320, 640, 1280) else 0)
        assert lib.unet_groupnorm_lds_form(16, 4096, C) == 0


def test_temb_argument_checks(lib):
    p = 4096

    def call(temb=p, w=p, bias=p, cbias=p, out=p, n=16, K=1280, cout=320):
        return lib.unet_temb(temb, w, bias, cbias, out, n, K, cout, None)

    assert call(n=65) == EUNSUPPORTED
    assert call(K=1284) == EUNSUPPORTED
    for null in ("temb", "w", "bias", "cbias", "out"):
        assert call(**{null: None}) == EINVAL
    assert call(n=0) == EINVAL and call(K=0) == EINVAL and call(cout=0) == EINVAL
    assert call(temb=p + 8) == EINVAL and call(w=p + 2) == EINVAL and call(out=p + 2) == EINVAL
