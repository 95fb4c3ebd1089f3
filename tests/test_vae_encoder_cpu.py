"""The VAE encoder without a GPU: the restated module's parameter list, the old attention spelling, the downsample index rule
against torch in float64, the constructor's and encode()'s refusals, patching, the vaeenc_* entry points on the header /
binding / export surface and their argument checks (fake pointers: every check answers before any HIP call), and what the
GPU tests rely on in the golden record."""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_encoder_model as EM
import vae_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def net():
    return EM.build(torch.float64)


def test_public_names_without_a_gpu():
    import fresco_amd
    from fresco_amd import ops, vae
    for name in ("VAEEncoder", "patch_vae_encode", "unpatch_vae_encode", "patch_vae", "unpatch_vae"):
        assert name in fresco_amd.__all__ and getattr(fresco_amd, name) is getattr(vae, name)
    assert vae.VAEEncoder.TAPS == EM.TAPS
    for name in ("vaeenc_input", "vaeenc_conv_down", "vaeenc_moments", "vaeenc_sample"):
        assert callable(getattr(ops, name))


def test_the_two_halves_share_their_layer_code():
    from fresco_amd.vae import VAEDecoder, VAEEncoder
    for name in ("_conv", "_resnet", "_attention", "_mid"):
        assert getattr(VAEEncoder, name) is getattr(VAEDecoder, name), name


def test_state_dict_names_and_shapes_equal_the_committed_list(net):
    listed = EM.read_names_shapes(GOLDEN)
    assert EM.encoder_names_shapes(net) == listed
    names = [k for k, _ in listed]
    shapes = dict(listed)
    assert len(names) == len(set(names)) == 108
    assert all(k.startswith(EM.PREFIXES) for k in names)
    assert shapes["encoder.conv_in.weight"] == (128, 3, 3, 3)
    assert shapes["encoder.conv_out.weight"] == (8, 512, 3, 3)
    assert shapes["quant_conv.weight"] == (8, 8, 1, 1) and shapes["quant_conv.bias"] == (8,)
    assert shapes["encoder.down_blocks.2.downsamplers.0.conv.weight"] == (512, 512, 3, 3)
    assert sorted(k for k in names if "conv_shortcut.weight" in k) == ["encoder.down_blocks.1.resnets.0.conv_shortcut.weight",
                                                                       "encoder.down_blocks.2.resnets.0.conv_shortcut.weight"]
    assert not any(k.startswith("encoder.down_blocks.3.downsamplers") for k in names)
    assert not any("resnets.2" in k for k in names)
    for must in ("encoder.mid_block.attentions.0.to_out.0.bias", "encoder.mid_block.attentions.0.group_norm.weight",
                 "encoder.conv_norm_out.weight", "encoder.down_blocks.0.downsamplers.0.conv.bias"):
        assert must in names, must


def test_old_attention_spelling_loads_to_the_same_tensors(net):
    from fresco_amd.vae import VAEEncoder
    sd = net.state_dict()
    old = M.old_spelling(sd)
    assert sum(k.startswith("encoder.") and (".query." in k or ".key." in k or ".value." in k or ".proj_attn." in k)
               for k in old) == 8
    a, b = VAEEncoder(sd), VAEEncoder(old)
    for k in a.attn:
        assert torch.equal(a.attn[k].w, b.attn[k].w) and torch.equal(a.attn[k].b, b.attn[k].b)
    assert torch.equal(a.down[1][1].w, b.down[1][1].w) and torch.equal(a.q_w, b.q_w)
    assert a.conv_in.w.shape == (128, 9 * 32) and a.conv_out.w.shape == (8, 9 * 512) and a.q_w.shape == (8, 8)
    assert [d is not None for _, d in a.down] == [True, True, True, False]


def test_encoder_refuses_another_architecture(net):
    from fresco_amd.vae import VAEEncoder
    sd = dict(net.state_dict())
    with pytest.raises(ValueError, match="conv_shortcut"):    # a missing parameter
        VAEEncoder({k: v for k, v in sd.items() if "down_blocks.2.resnets.0.conv_shortcut" not in k})
    extra = dict(sd)
    extra["encoder.down_blocks.3.downsamplers.0.conv.weight"] = sd["encoder.down_blocks.2.downsamplers.0.conv.weight"]
    extra["encoder.down_blocks.3.downsamplers.0.conv.bias"] = sd["encoder.down_blocks.2.downsamplers.0.conv.bias"]
    with pytest.raises(ValueError, match="last down block"):  # a downsampler on the last block
        VAEEncoder(extra)
    third = dict(sd)
    third["encoder.down_blocks.0.resnets.2.norm1.weight"] = sd["encoder.down_blocks.0.resnets.1.norm1.weight"]
    with pytest.raises(ValueError, match="resnets.2.norm1"):  # an extra parameter
        VAEEncoder(third)
    narrow = dict(sd)
    narrow["encoder.conv_in.weight"] = sd["encoder.conv_in.weight"][:64]
    narrow["encoder.conv_in.bias"] = sd["encoder.conv_in.bias"][:64]
    with pytest.raises(ValueError, match="conv_in"):          # a wrong shape
        VAEEncoder(narrow)
    wide = dict(sd)
    wide["encoder.conv_out.weight"] = sd["encoder.conv_out.weight"][:4]
    wide["encoder.conv_out.bias"] = sd["encoder.conv_out.bias"][:4]
    with pytest.raises(ValueError, match="conv_out"):
        VAEEncoder(wide)
    quant = dict(sd)
    quant["quant_conv.weight"] = sd["quant_conv.weight"][:4, :4]
    with pytest.raises(ValueError, match="quant_conv"):
        VAEEncoder(quant)
    with pytest.raises(ValueError, match="quant_conv"):
        VAEEncoder({k: v for k, v in sd.items() if not k.startswith("quant_conv.")})
    with pytest.raises(ValueError, match="no encoder"):
        VAEEncoder({k: v for k, v in sd.items() if k.startswith("decoder.")})


def _gather(x):
    """x (n, H, W, C) numpy -> (n, H // 2, W // 2, 9 C) rows in k = (ky, kx, ci) order, by the kernel's index rule"""
    from fresco_amd.vae import down_source_index
    n, H, W, C = x.shape
    out = np.zeros((n, H // 2, W // 2, 9 * C))
    for yo in range(H // 2):
        for xo in range(W // 2):
            for ky in range(3):
                for kx in range(3):
                    src = down_source_index(yo, xo, ky, kx, H, W)
                    if src is not None:
                        out[:, yo, xo, (ky * 3 + kx) * C:(ky * 3 + kx + 1) * C] = x[:, src[0], src[1]]
    return out


@pytest.mark.parametrize("size", [(5, 7), (2, 2), (3, 2), (8, 16)], ids=lambda s: "%dx%d" % s)
def test_down_index_rule_equals_pad_then_strided_conv(size):
    from fresco_amd.vae import down_source_index, pack_conv_weight
    g = torch.Generator().manual_seed(sum(size))
    x = torch.randn(2, size[0], size[1], 4, generator=g, dtype=torch.float64)
    w = torch.randn(5, 4, 3, 3, generator=g, dtype=torch.float64).half().double()
    ref = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1)), w, stride=2).permute(0, 2, 3, 1).numpy()
    got = _gather(x.numpy()) @ pack_conv_weight(w).double().numpy().T
    assert got.shape == ref.shape == (2, size[0] // 2, size[1] // 2, 5) and np.abs(got - ref).max() < 1e-12
    H, W = size
    # the pad is read on an even side only, by the last output row / column's third tap
    assert (down_source_index(H // 2 - 1, 0, 2, 0, H, W) is None) == (H % 2 == 0)
    assert (down_source_index(0, W // 2 - 1, 0, 2, H, W) is None) == (W % 2 == 0)
    assert down_source_index(0, 0, 0, 0, H, W) == (0, 0)


def test_encode_refuses_what_is_out_of_scope():
    from fresco_amd import FrescoHipError
    from fresco_amd.vae import VAEEncoder
    vae = EM.build(torch.float16)
    enc = VAEEncoder.from_vae(vae)
    x = EM.images(EM.CASES[0])
    for dt in (torch.float32, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError):
            enc.encode(x.to(dt))
    with pytest.raises(TypeError):
        enc.encode(x.numpy())
    with pytest.raises(ValueError):
        enc.encode(x[:, :2])
    with pytest.raises(ValueError):
        enc.encode(x[0])
    with pytest.raises(ValueError):
        enc.encode(x[:, :, :7])
    for flag in ("use_slicing", "use_tiling"):
        setattr(vae, flag, True)
        with pytest.raises(NotImplementedError):
            enc.encode(x)
        setattr(vae, flag, False)
    with pytest.raises(FrescoHipError):  # a CPU tensor: no fallback
        enc.encode(x)


def test_patch_rebinds_and_unpatch_restores():
    from fresco_amd.vae import (VAEDecoder, VAEEncoder, patch_vae, patch_vae_decode, patch_vae_encode, unpatch_vae,
                                unpatch_vae_decode, unpatch_vae_encode)
    vae = EM.build(torch.float16)
    pipe = types.SimpleNamespace(vae=vae)
    own_enc, own_dec = vae.encode, vae.decode
    enc = patch_vae_encode(pipe)
    assert isinstance(enc, VAEEncoder) and pipe.vae.encode == enc.encode and "encode" in vars(vae) and "decode" not in vars(vae)
    enc2 = patch_vae_encode(pipe)  # patching twice replaces, it does not stack
    assert pipe.vae.encode == enc2.encode
    unpatch_vae_encode(pipe)
    assert "encode" not in vars(vae) and pipe.vae.encode == own_enc
    unpatch_vae_encode(pipe)  # and is idempotent
    dec, enc = patch_vae(pipe)
    assert isinstance(dec, VAEDecoder) and isinstance(enc, VAEEncoder)
    assert pipe.vae.decode == dec.decode and pipe.vae.encode == enc.encode
    unpatch_vae_decode(pipe)       # the halves come off one at a time as well
    assert pipe.vae.decode == own_dec and pipe.vae.encode == enc.encode
    patch_vae_decode(pipe)
    unpatch_vae(pipe)
    assert "encode" not in vars(vae) and "decode" not in vars(vae)
    assert pipe.vae.encode == own_enc and pipe.vae.decode == own_dec
    assert type(vae).encode is EM.VAE.encode and type(vae).decode is M.VAE.decode  # the class's methods were never touched
    unpatch_vae(pipe)


def _lib():
    from fresco_amd import _lib
    return _lib.load()


def test_header_binding_and_exports_agree():
    from fresco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fresco_vae_enc.h")).read()
    protos = re.findall(r"^(?:int|size_t)\s+(\w+)\(", hdr, re.M)
    assert sorted(protos) == sorted(_lib.VAE_ENC_SIGNATURES) and len(protos) == 4
    assert all(p.startswith("vaeenc_") for p in protos)
    lib = _lib.load()
    for name in protos:
        assert getattr(lib, name).argtypes == _lib.VAE_ENC_SIGNATURES[name][1]  # (getattr: the symbol is exported)
        assert getattr(lib, name).restype is _lib.VAE_ENC_SIGNATURES[name][0]
        assert name not in _lib.SIGNATURES and name not in _lib.VAE_SIGNATURES
        # the header's argument list, type by type, against the bound argtypes
        args = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1).split(",")
        kinds = ["p" if "*" in a else a.split()[0] for a in args]
        bound = [{"c_void_p": "p", "c_int": "int", "c_float": "float", "c_int64": "int64_t", "c_long": "int64_t",
                  "c_size_t": "size_t", "c_ulong": "size_t"}[t.__name__] for t in _lib.VAE_ENC_SIGNATURES[name][1]]
        assert kinds == bound, (name, kinds, bound)
    for name in protos:  # the names stay clear of the patterns the other surfaces are counted by
        assert not name.startswith(("fresco_", "vae_", "frame_"))
        assert not any(s in name for s in ("keyframe", "canny", "egnet", "midas"))
    mk = open(os.path.join(ROOT, "fresco_amd", "csrc", "Makefile")).read()
    assert " vae_enc.hip" in mk and "include/fresco_vae_enc.h" in mk


def test_argument_checks_answer_before_any_hip_call():
    lib = _lib()
    p = 4096  # fake, aligned, never touched
    # (each base case is valid and therefore never called: every call below fails a check)
    base = dict(x=p, w=p, bias=p, out=p, n=2, H=18, W=34, cin=128, cout=128, st=0)

    def down(**k):
        return lib.vaeenc_conv_down(*dict(base, **k).values())
    assert down(x=0) == EINVAL and down(w=0) == EINVAL and down(bias=0) == EINVAL and down(out=0) == EINVAL
    assert down(n=0) == EINVAL and down(H=0) == EINVAL and down(W=-2) == EINVAL and down(cin=0) == EINVAL and down(cout=0) == EINVAL
    assert down(x=p + 8) == EINVAL and down(w=p + 2) == EINVAL and down(bias=p + 4) == EINVAL and down(out=p + 4) == EINVAL
    assert down(cin=4) == EUNSUPPORTED and down(cin=144) == EUNSUPPORTED
    assert down(H=1) == EUNSUPPORTED and down(W=1) == EUNSUPPORTED
    assert down(n=65536) == EUNSUPPORTED
    assert down(n=1, H=65536, W=32768) == EUNSUPPORTED                 # 2^31 pixels
    assert down(n=1, H=32768, W=32768, cout=1 << 20) == EUNSUPPORTED   # 2^34 workgroups

    vi = lambda im=p, o=p, n=2, h=8, ww=12, cpad=32: lib.vaeenc_input(im, o, n, h, ww, cpad, 0)  # noqa: E731
    assert vi(im=0) == EINVAL and vi(o=0) == EINVAL and vi(n=0) == EINVAL and vi(h=0) == EINVAL and vi(ww=-1) == EINVAL
    assert vi(cpad=4) == EINVAL and vi(cpad=36) == EINVAL and vi(cpad=128) == EINVAL
    assert vi(o=p + 8) == EINVAL and vi(im=p + 1) == EINVAL
    assert vi(n=1, h=65536, ww=32768) == EUNSUPPORTED

    mo = lambda h=p, w=p, b=p, o=p, n=2, hh=8, ww=12: lib.vaeenc_moments(h, w, b, o, n, hh, ww, 0)  # noqa: E731
    assert mo(h=0) == EINVAL and mo(w=0) == EINVAL and mo(b=0) == EINVAL and mo(o=0) == EINVAL
    assert mo(n=0) == EINVAL and mo(hh=0) == EINVAL and mo(ww=0) == EINVAL
    assert mo(h=p + 8) == EINVAL and mo(w=p + 2) == EINVAL and mo(b=p + 2) == EINVAL and mo(o=p + 1) == EINVAL
    assert mo(n=1, hh=65536, ww=32768) == EUNSUPPORTED

    sa = lambda pa=p, no=p, o=p, n=2, hh=8, ww=12, sc=1.0: lib.vaeenc_sample(pa, no, o, n, hh, ww, sc, 0)  # noqa: E731
    assert sa(pa=0) == EINVAL and sa(no=0) == EINVAL and sa(o=0) == EINVAL
    assert sa(n=0) == EINVAL and sa(hh=-1) == EINVAL and sa(ww=0) == EINVAL and sa(sc=float("nan")) == EINVAL
    assert sa(pa=p + 1) == EINVAL and sa(no=p + 1) == EINVAL and sa(o=p + 1) == EINVAL
    assert sa(n=1, hh=65536, ww=32768) == EUNSUPPORTED


def test_the_record_holds_what_the_gpu_tests_rely_on():
    gold = EM.load_golden(GOLDEN)
    assert os.path.getsize(os.path.join(GOLDEN, EM.GOLDEN_FILE)) <= 476194  # no larger than vae_golden.npz was when this was added
    for case in EM.CASES:
        key = EM.case_key(case)
        n, H, W = case
        noise, peak = gold[key + "_noise"], gold[key + "_peak"]
        assert noise.shape == peak.shape == (len(EM.TAPS) + 1,)
        assert (noise > 0).all() and (noise < 0.01).all() and (peak > 0).all() and (peak < EM.ACT_LIMIT).all()
        params = gold[key + "_parameters"]
        assert params.dtype == np.float64 and params.shape == (n, 8, H // 8, W // 8)
        assert -30 < params[:, 4:].min() and params[:, 4:].max() < 20
        for t in EM.TAPS:
            assert gold["%s_%s" % (key, t)].dtype == np.float64 and gold["%s_%s" % (key, t)].shape[0] == n
        img = EM.images(case)
        assert img.shape == (n, 3, H, W) and img.dtype == torch.float16 and float(img.abs().max()) < 1.6
        assert float(img.float().std()) > 0.2
    assert (68 // 4, 100 // 4) == (17, 25)  # the last case's third level: odd sides, no multiple of the 8 x 16 tile


def test_restatement_reproduces_the_record_on_the_smallest_case(net):
    gold = EM.load_golden(GOLDEN)
    case = min(EM.CASES, key=lambda c: c[0] * c[1] * c[2])
    key = EM.case_key(case)
    taps = {}
    with torch.no_grad():
        params = net.encode_forward(EM.images(case).double(), taps)
    for t in EM.TAPS:
        assert np.abs(EM.thin(taps[t]) - gold["%s_%s" % (key, t)]).max() <= 1e-9 * gold[key + "_peak"].max()
    assert np.abs(params.numpy() - gold[key + "_parameters"]).max() <= 1e-9 * gold[key + "_peak"].max()
    dist = EM.DiagonalGaussianDistribution(params)
    assert torch.equal(dist.mode(), params[:, :4]) and torch.equal(dist.std, torch.exp(0.5 * params[:, 4:]))
