"""What is left of the UNet and the ControlNet, without a GPU: header == binding == exported symbols for the three entry points
of include/fresco_unet_shell.h, every argument check with fake pointers (each answers before any HIP call), the weight
packing (the 4 -> 32 and 16 -> 32 paddings included) against F.conv2d in float64 on the packed matrices, the golden file
against a fresh derivation, patch_unet_shell / unpatch_unet_shell on the two stand-in skeletons (counts, restored forwards,
every refusal by name), and the condition embedding's cache."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import unet_shell_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL, EUNSUPPORTED = -1, -2
NAMES = ("UNetDownsample", "UNetUpsample", "UNetConvIn", "UNetConvOut", "UNetTimeEmbedding", "ControlNetCondEmbedding",
         "UNetZeroConv", "patch_unet_shell", "unpatch_unet_shell")


# ---------------------------------------------------------------------------------------------------------------------
# the C surface
# ---------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    import fresco_amd
    from fresco_amd import _lib, unet_shell
    hdr = open(os.path.join(ROOT, "include", "fresco_unet_shell.h")).read()
    protos = re.findall(r"^(?:int|size_t)\s+(\w+)\(", hdr, re.M)
    assert sorted(protos) == sorted(_lib.UNET_SHELL_SIGNATURES) == ["unet_conv3", "unet_input", "unet_time_linear"]
    lib = _lib.load()
    others = [_lib.SIGNATURES, _lib.VAE_SIGNATURES, _lib.VAE_ENC_SIGNATURES, _lib.UNET_SIGNATURES, _lib.UNET_TF_SIGNATURES,
              _lib.UNET_ATTN_SIGNATURES]
    for name in protos:
        assert not name.startswith("fresco_") and not any(name in o for o in others)
        res, argtypes = _lib.UNET_SHELL_SIGNATURES[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res  # (getattr: it is exported)
        args = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1).split(",")
        kinds = ["p" if "*" in a else a.split()[0] for a in args]
        bound = [{"c_void_p": "p", "c_int": "int"}[t.__name__] for t in argtypes]
        assert kinds == bound, (name, kinds, bound)
    for macro, value in (("UNET_ACT_NONE", _lib.UNET_ACT_NONE), ("UNET_ACT_SILU", _lib.UNET_ACT_SILU),
                         ("UNET_SRC_TIMESTEPS", _lib.UNET_SRC_TIMESTEPS), ("UNET_SRC_SILU_ROWS", _lib.UNET_SRC_SILU_ROWS)):
        assert re.search(r"^#define %s %d$" % (macro, value), hdr, re.M), macro
    mk = open(os.path.join(ROOT, "fresco_amd", "csrc", "Makefile")).read()
    assert " unet_shell.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1) and "include/fresco_unet_shell.h" in mk
    for name in NAMES:
        assert name in fresco_amd.__all__ and getattr(fresco_amd, name) is getattr(unet_shell, name)


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


def test_conv3_argument_checks(lib):
    p = 4096  # fake, aligned, never touched: every call below fails a check
    base = dict(x=p, w=p, bias=p, out=p, n=2, H=18, W=34, cin=128, cout=128, stride=2, act=0, st=0)

    def conv(**k):
        return lib.unet_conv3(*dict(base, **k).values())
    for null in ("x", "w", "bias", "out"):
        assert conv(**{null: 0}) == EINVAL
    for size in ("n", "H", "W", "cin", "cout"):
        assert conv(**{size: 0}) == EINVAL and conv(**{size: -2}) == EINVAL
    assert conv(x=p + 8) == EINVAL and conv(w=p + 2) == EINVAL and conv(bias=p + 4) == EINVAL and conv(out=p + 4) == EINVAL
    assert conv(stride=0) == EUNSUPPORTED and conv(stride=3) == EUNSUPPORTED
    assert conv(act=2) == EUNSUPPORTED and conv(act=-1) == EUNSUPPORTED
    assert conv(cin=4) == EUNSUPPORTED and conv(cin=144) == EUNSUPPORTED
    assert conv(n=65536) == EUNSUPPORTED
    assert conv(n=1, H=65536, W=32768) == EUNSUPPORTED                             # 2^31 pixels
    assert conv(n=1, H=32768, W=32768, stride=1, cout=1 << 20) == EUNSUPPORTED     # 2^34 workgroups
    assert conv(x=0, stride=5) == EINVAL      # a null pointer answers first


def test_input_argument_checks(lib):
    p = 4096
    ui = lambda x=p, o=p, n=2, c=4, h=8, w=12, cpad=32: lib.unet_input(x, o, n, c, h, w, cpad, 0)  # noqa: E731
    assert ui(x=0) == EINVAL and ui(o=0) == EINVAL
    assert ui(n=0) == EINVAL and ui(c=0) == EINVAL and ui(h=0) == EINVAL and ui(w=-1) == EINVAL
    assert ui(cpad=4) == EINVAL and ui(cpad=36) == EINVAL and ui(cpad=128) == EINVAL and ui(c=9, cpad=8) == EINVAL
    assert ui(o=p + 8) == EINVAL and ui(x=p + 1) == EINVAL
    assert ui(n=1, h=65536, w=32768) == EUNSUPPORTED


def test_time_linear_argument_checks(lib):
    p = 4096
    base = dict(src=p, kind=0, w=p, bias=p, out=p, sin=0, n=16, K=320, cout=1280, st=0)

    def tl(**k):
        return lib.unet_time_linear(*dict(base, **k).values())
    for null in ("src", "w", "bias", "out"):
        assert tl(**{null: 0}) == EINVAL
    assert tl(n=0) == EINVAL and tl(K=0) == EINVAL and tl(cout=-1) == EINVAL
    assert tl(kind=2) == EUNSUPPORTED and tl(kind=-1) == EUNSUPPORTED
    assert tl(n=65) == EUNSUPPORTED and tl(K=324) == EUNSUPPORTED
    assert tl(kind=1, sin=p) == EUNSUPPORTED                     # the sinusoid tap goes with the timesteps
    assert tl(src=p + 2) == EINVAL and tl(src=p + 4, kind=1) == EINVAL      # fp32 timesteps; fp16 rows in 16-byte pieces
    assert tl(w=p + 8) == EINVAL and tl(bias=p + 2) == EINVAL and tl(out=p + 1) == EINVAL and tl(sin=p + 8) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# the golden file
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_file_is_current():
    gold = M.load_golden(GOLDEN)
    assert sorted(gold) == sorted(M.case_key(c) + s for c in M.CASES for s in ("_out", "_noise", "_peak"))
    for case in (M.CASES[1], M.CASES[6], M.CASES[8]):     # down at 4 x 4, the time MLP, the zero convolution: the cheapest
        key = M.case_key(case)
        out, noise, peak, act = M.record(case)
        assert act < M.ACT_LIMIT
        np.testing.assert_allclose(gold[key + "_out"], M.thin(out), rtol=0, atol=1e-9)
        # the noise is a maximum over an fp32 run whose sums depend on the CPU's order of additions: another CPU flips a few
        # fp16 roundings and moves the maximum by some per cent (seen: 1.3 %); the tests use it under a margin of 4
        np.testing.assert_allclose(gold[key + "_noise"], [noise], rtol=0.25)
        np.testing.assert_allclose(gold[key + "_peak"], [peak], rtol=1e-9)
    for c in M.CASES:
        k = M.case_key(c)
        assert 0 < gold[k + "_noise"][0] < 2e-3 and gold[k + "_out"].shape[0] == c[2]


def test_restatements_are_the_functional_compositions():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 5, 7, generator=gen, dtype=torch.float64)
    down, up = M.Downsample2D(64).double(), M.Upsample2D(64).double()
    with torch.no_grad():
        assert torch.equal(down(x), F.conv2d(x, down.conv.weight, down.conv.bias, stride=2, padding=1))
        assert down(x).shape == (2, 64, 3, 4)
        rep = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        assert torch.equal(up(x), F.conv2d(rep, up.conv.weight, up.conv.bias, padding=1))
        assert torch.equal(up(x, output_size=(10, 14)), up(x))
        # Timesteps(320, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin] of t exp(-ln(10000) i / 160)
        t = torch.tensor([0.0, 1.0, 251.0, 999.0], dtype=torch.float64)
        emb = M.Timesteps(320)(t)
        w = torch.exp(-np.log(10000.0) * torch.arange(160, dtype=torch.float64) / 160)
        assert torch.allclose(emb, torch.cat([torch.cos(t[:, None] * w), torch.sin(t[:, None] * w)], 1), rtol=0, atol=1e-12)
        e = M.CondEmbedding(320).double()
        assert [tuple(c.stride) for c in e.blocks] == [(1, 1), (2, 2)] * 3 and len(e.blocks) == 6
        assert e(torch.zeros(1, 3, 32, 48, dtype=torch.float64)).shape == (1, 320, 4, 6)


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
def _conv_from_packed(x, w, b, stride):
    """F.conv2d in float64 from a packed (cout, 9 cin) matrix with k = (ky, kx, ci) on x (n, cin, H, W)"""
    cout, cin = w.shape[0], w.shape[1] // 9
    return F.conv2d(x, w.double().view(cout, 3, 3, cin).permute(0, 3, 1, 2), b.double(), stride=stride, padding=1)


def test_packing_matches_conv2d_in_float64():
    from fresco_amd import ControlNetCondEmbedding, UNetConvIn, UNetDownsample, UNetZeroConv
    mod = M.build(("cond", 64, 1, 16, 24), torch.float16)
    native = ControlNetCondEmbedding.from_module(mod)
    convs = [mod.conv_in] + list(mod.blocks) + [mod.conv_out]
    assert [tuple(w.shape) for w, _, _, _ in native.layers] == [
        (32, 288), (32, 288), (32, 288), (32, 288), (96, 288), (96, 864), (256, 864), (64, 2304)]
    assert [(s, a) for _, _, s, a in native.layers] == [(1, True), (1, True), (2, True), (1, True), (2, True), (1, True),
                                                        (2, True), (1, False)]
    x = torch.rand(1, 3, 16, 24, generator=torch.Generator().manual_seed(5)).half().double()
    h, ref = F.pad(x, (0, 0, 0, 0, 0, 29)), x          # the padded run on 32 channels beside the module's own layers
    with torch.no_grad():
        for i, ((w, b, stride, silu), c) in enumerate(zip(native.layers, convs)):
            assert w.dtype == torch.float16 and b.dtype == torch.float32 and w.is_contiguous()
            h, ref = _conv_from_packed(h, w, b, stride), F.conv2d(ref, c.weight.double(), c.bias.double(), stride=stride, padding=1)
            if silu:
                h, ref = F.silu(h), F.silu(ref)
            assert torch.allclose(h[:, :c.out_channels], ref, rtol=0, atol=1e-12), i   # the padding adds exact zeros
            assert float(h[:, c.out_channels:].abs().max() if h.shape[1] > c.out_channels else 0.0) == 0.0, i  # SiLU(0) = 0
    # the 16-channel layers: 16 zero output rows with zero biases, 16 zero input columns per tap
    w0, b0 = native.layers[0][:2]
    assert float(w0[16:].abs().max()) == 0 and float(b0[16:].abs().max()) == 0
    assert float(w0.view(32, 9, 32)[:, :, 3:].abs().max()) == 0 and float(native.layers[1][0].view(32, 9, 32)[:, :, 16:].abs().max()) == 0
    assert torch.equal(w0.view(32, 3, 3, 32)[:16, :, :, :3], mod.conv_in.weight.permute(0, 2, 3, 1))

    cin = UNetConvIn.from_module(M.build(("conv_in", 64, 1, 4, 4), torch.float16).conv)
    assert cin.w.shape == (64, 288) and float(cin.w.view(64, 9, 32)[:, :, 4:].abs().max()) == 0
    dn_mod = M.build(("down", 64, 1, 4, 4), torch.float16)
    dn = UNetDownsample.from_module(dn_mod)
    assert torch.equal(dn.w.view(64, 3, 3, 64), dn_mod.conv.weight.permute(0, 2, 3, 1)) and torch.equal(dn.b, dn_mod.conv.bias.float())
    z_mod = M.build(("zero", 64, 1, 4, 4), torch.float16)
    z = UNetZeroConv.from_module(z_mod.conv)
    assert torch.equal(z.w, z_mod.conv.weight.view(64, 64)) and z.b.dtype == torch.float32
    # the weights are copies: the module may change afterwards
    dn_mod.conv.weight.data.zero_()
    assert float(dn.w.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# patching (packing the weights needs no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _skeleton(kind):
    return M.build_skeleton(kind, torch.float16, c=64)


def test_patch_and_unpatch_counts():
    from fresco_amd import (ControlNetCondEmbedding, UNetConvIn, UNetConvOut, UNetDownsample, UNetTimeEmbedding, UNetUpsample,
                            UNetZeroConv, patch_unet_shell, unpatch_unet_shell)
    unet = _skeleton("unet")
    counts = patch_unet_shell(unet)
    assert counts == {"down": 3, "up": 3, "conv_in": 1, "conv_out": 1, "time": 1, "cond_embedding": 0, "zero_conv": 0}
    assert all(isinstance(vars(m)["forward"], UNetDownsample) for m in unet.downsamplers)
    assert all(isinstance(vars(m)["forward"], UNetUpsample) for m in unet.upsamplers)
    assert isinstance(vars(unet.conv_in)["forward"], UNetConvIn)
    end = vars(unet.conv_norm_out)["_fresco_unet_shell"]
    assert isinstance(end, UNetConvOut) and vars(unet.conv_act)["_fresco_unet_shell"] is end
    assert vars(unet.conv_out)["forward"] == end.conv and vars(unet.conv_norm_out)["forward"] == end.norm
    marker = torch.zeros(3)
    assert unet.conv_act(marker) is marker                 # under the patch conv_act returns its argument
    tm = vars(unet.time_embedding)["forward"]
    assert isinstance(tm, UNetTimeEmbedding) and vars(unet.time_proj)["forward"] == tm.proj
    assert (tm.K, tm.inner, tm.cout) == (64, 256, 256) and tm.w1.dtype == torch.float16 and tm.b2.dtype == torch.float32
    assert not any("forward" in vars(m) for m in list(unet.down_resnets) + list(unet.up_resnets))   # the resnets are not ours
    assert "forward" not in vars(unet)
    fmt = patch_unet_shell(unet, memory_format=torch.contiguous_format)   # patching again replaces, it does not stack
    assert fmt == counts and vars(unet.downsamplers[0])["forward"].memory_format == torch.contiguous_format
    assert unpatch_unet_shell(unet) == 3 + 3 + 1 + 3 + 2   # modules restored: the output end is three, the time MLP two
    assert not any("forward" in vars(m) or "_fresco_unet_shell" in vars(m) for m in unet.modules())
    assert unpatch_unet_shell(unet) == 0
    x, t, _ = M.skeleton_inputs(1, 8, 8)
    with torch.no_grad():
        assert unet.float()(x.float(), t[:1]).shape == (1, 4, 8, 8)      # the modules' own forwards run again

    cn = _skeleton("controlnet")
    counts = patch_unet_shell(cn, cache=False)
    assert counts == {"down": 3, "up": 0, "conv_in": 1, "conv_out": 0, "time": 1, "cond_embedding": 1, "zero_conv": 13}
    emb = vars(cn.controlnet_cond_embedding)["forward"]
    assert isinstance(emb, ControlNetCondEmbedding) and emb.cache is False and len(emb.layers) == 8
    assert "forward" not in vars(cn.controlnet_cond_embedding.conv_in)     # the embedding's own conv_in is not the model's
    assert all(isinstance(vars(m)["forward"], UNetZeroConv) for m in list(cn.controlnet_down_blocks) + [cn.controlnet_mid_block])
    assert unpatch_unet_shell(cn) == 3 + 1 + 2 + 1 + 13
    with pytest.raises(ValueError, match="memory_format"):
        patch_unet_shell(cn, memory_format=torch.preserve_format)


def _refused(kind, change, name, match):
    from fresco_amd import patch_unet_shell
    net = _skeleton(kind)
    change(net)
    with pytest.raises(NotImplementedError, match=match) as e:
        patch_unet_shell(net)
    assert name in str(e.value) and "no fallback" in str(e.value)            # refused by name ...
    assert not any("forward" in vars(m) for m in net.modules())             # ... before anything is patched


def test_refusals_by_name():
    u, c = "unet", "controlnet"
    _refused(u, lambda n: setattr(n.downsamplers[1], "use_conv", False), "downsamplers.1", "use_conv=False")
    _refused(u, lambda n: setattr(n.downsamplers[2], "padding", 0), "downsamplers.2", "padding 0")
    _refused(u, lambda n: setattr(n.downsamplers[0], "conv", nn.Conv2d(64, 64, 3, 1, 1).half()), "downsamplers.0", "stride 1")
    _refused(u, lambda n: setattr(n.downsamplers[0], "conv", nn.Conv2d(64, 64, 5, 2, 1).half()), "downsamplers.0", "5 x 5")
    _refused(u, lambda n: n.downsamplers[0].float(), "downsamplers.0", "fp16 modules only")
    _refused(u, lambda n: n.upsamplers[1].bfloat16(), "upsamplers.1", "fp16 modules only")
    _refused(u, lambda n: setattr(n.upsamplers[1], "use_conv_transpose", True), "upsamplers.1", "use_conv_transpose")
    _refused(u, lambda n: setattr(n.upsamplers[2], "use_conv", False), "upsamplers.2", "use_conv=False")
    _refused(u, lambda n: setattr(n, "conv_in", nn.Conv2d(4, 64, 3, 1, 0).half()), "conv_in", "padding")
    _refused(u, lambda n: setattr(n, "conv_in", nn.Conv2d(40, 64, 3, 1, 1).half()), "conv_in", "40 channels")
    _refused(u, lambda n: setattr(n, "conv_act", nn.GELU()), "conv_out", "conv_act is GELU")
    _refused(u, lambda n: setattr(n, "conv_norm_out", nn.GroupNorm(32, 96).half()), "conv_out", "96 channels")
    _refused(u, lambda n: setattr(n, "conv_norm_out", nn.GroupNorm(16, 64).half()), "conv_out", "32 groups")
    _refused(u, lambda n: setattr(n.time_embedding, "cond_proj", nn.Linear(8, 64).half()), "time_embedding", "cond_proj")
    _refused(u, lambda n: setattr(n.time_embedding, "post_act", nn.SiLU()), "time_embedding", "post_act")
    _refused(u, lambda n: setattr(n.time_embedding, "act", nn.GELU()), "time_embedding", "only SiLU")
    _refused(u, lambda n: setattr(n.time_proj, "flip_sin_to_cos", False), "time_embedding", "flip_sin_to_cos=False")
    _refused(u, lambda n: setattr(n.time_proj, "downscale_freq_shift", 1), "time_embedding", "downscale_freq_shift 1")
    _refused(c, lambda n: n.time_embedding.float(), "time_embedding", "fp16 modules only")
    _refused(c, lambda n: n.controlnet_cond_embedding.blocks.__setitem__(2, nn.Conv2d(16, 32, 3, 4, 1).half()),
             "controlnet_cond_embedding", "blocks.2")
    _refused(c, lambda n: n.controlnet_cond_embedding.blocks.__setitem__(3, nn.Conv2d(48, 32, 3, 1, 1).half()),
             "controlnet_cond_embedding", "blocks.3 reads 48 channels behind 32")
    _refused(c, lambda n: n.controlnet_down_blocks.__setitem__(7, nn.Conv2d(64, 64, 3, 1, 1).half()),
             "controlnet_down_blocks.7", "3 x 3")
    _refused(c, lambda n: setattr(n, "controlnet_mid_block", nn.Conv2d(48, 64, 1).half()), "controlnet_mid_block", "48 channels")


def test_calls_refuse_what_they_do_not_compute():
    from fresco_amd import FrescoHipError, UNetDownsample, UNetTimeEmbedding, UNetUpsample
    up = UNetUpsample.from_module(M.build(("up", 64, 1, 4, 4), torch.float16), name="up_blocks.0.upsamplers.0")
    with pytest.raises(TypeError, match="fp16 only"):
        up(torch.zeros(1, 64, 4, 4))
    with pytest.raises(ValueError, match=r"\(n, 64, H, W\)"):
        up(torch.zeros(1, 32, 4, 4, dtype=torch.float16))
    with pytest.raises(FrescoHipError, match="GPU only"):                  # no fallback on CPU tensors
        up(torch.zeros(1, 64, 4, 4, dtype=torch.float16))
    dn = UNetDownsample.from_module(M.build(("down", 64, 1, 4, 4), torch.float16))
    with pytest.raises(FrescoHipError, match="GPU only"):
        dn(torch.zeros(1, 64, 4, 4, dtype=torch.float16))
    tm = UNetTimeEmbedding.from_module(M.build(("time", 64, 1, 1, 1), torch.float16), name="time_embedding")
    with pytest.raises(NotImplementedError, match="time_embedding.*sinusoid computed elsewhere"):
        tm(torch.zeros(2, 64, dtype=torch.float16))
    with pytest.raises(NotImplementedError, match="condition"):
        tm(torch.zeros(2), torch.zeros(2, 8))


def test_upsample_output_size(monkeypatch):
    from fresco_amd import UNetUpsample, ops
    up = UNetUpsample.from_module(M.build(("up", 64, 1, 4, 4), torch.float16), name="up_blocks.1.upsamplers.0")
    monkeypatch.setattr(ops, "_need_gpu", lambda *t: None)
    seen = []
    monkeypatch.setattr(ops, "vae_conv", lambda x, w, b, n, H, W, cin, cout, k, up2=False, **kw:
                        seen.append((H, W, up2)) or torch.zeros(n, H, W, cout, dtype=torch.float16))
    x = torch.zeros(1, 64, 4, 6, dtype=torch.float16)
    assert up(x).shape == (1, 64, 8, 12) and up(x, (8, 12)).shape == (1, 64, 8, 12) and up(x, output_size=[8, 12]).shape == (1, 64, 8, 12)
    assert seen == [(8, 12, True)] * 3          # the up2 form: the 2x plane is never written
    with pytest.raises(NotImplementedError, match=r"up_blocks.1.upsamplers.0.*output_size \(9, 12\)"):
        up(x, output_size=(9, 12))


def test_condition_cache(monkeypatch):
    """hit on the same tensor object at the same version; miss on a new tensor, after an in-place edit, after clear(), and
    always with cache=False.  The kernels are replaced by counters: what is tested is which calls reach them."""
    from fresco_amd import ControlNetCondEmbedding, ops
    mod = M.build(("cond", 64, 1, 16, 24), torch.float16)
    calls = []
    monkeypatch.setattr(ops, "_need_gpu", lambda *t: None)
    monkeypatch.setattr(ops, "unet_input", lambda x, cpad: calls.append("input") or torch.zeros(x.shape[0], x.shape[2], x.shape[3], cpad, dtype=torch.float16))

    def conv3(x, w, b, stride=1, silu=False):
        calls.append("conv")
        return torch.zeros(x.shape[0], (x.shape[1] - 1) // stride + 1, (x.shape[2] - 1) // stride + 1, w.shape[0], dtype=torch.float16)
    monkeypatch.setattr(ops, "unet_conv3", conv3)
    emb = ControlNetCondEmbedding.from_module(mod)
    assert emb.cache is True
    cond = torch.rand(1, 3, 16, 24).half()
    one = emb(cond)
    assert one.shape == (1, 64, 2, 3) and calls == ["input"] + ["conv"] * 8
    assert emb(cond) is one and len(calls) == 9                      # hit
    twin = cond.clone()
    assert emb(twin) is not one and len(calls) == 18                 # a new tensor of equal values: miss
    assert emb(twin) is not one and len(calls) == 18                 # ... which is now the cached one
    twin.mul_(0.5)
    emb(twin)
    assert len(calls) == 27                                          # edited in place: its version moved
    emb.clear()
    emb(twin)
    assert len(calls) == 36
    off = ControlNetCondEmbedding(mod, cache=False)
    off(cond)
    off(cond)
    assert len(calls) == 54
