"""The VAE decoder without a GPU: the restated module's parameter list, the old attention spelling, the host weight packing
and the `up2` index rule against torch in float64, decode()'s refusals, the vae_* entry points on the header / binding /
export surface and their argument checks (fake pointers: every check answers before any HIP call), and what the GPU tests
rely on in the golden record."""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def net():
    return M.build(torch.float64)


def test_public_names_without_a_gpu():
    import fresco_amd
    from fresco_amd import vae
    for name in ("VAEDecoder", "patch_vae_decode", "unpatch_vae_decode"):
        assert name in fresco_amd.__all__ and getattr(fresco_amd, name) is getattr(vae, name)
    assert vae.TAPS == M.TAPS and vae.BLOCK_CHANNELS == M.BLOCK_CHANNELS


def test_state_dict_names_and_shapes_equal_the_committed_list(net):
    listed = M.read_names_shapes(GOLDEN)
    assert M.module_names_shapes(net) == listed
    names = [k for k, _ in listed]
    assert len(names) == len(set(names)) == 140
    for must in ("post_quant_conv.weight", "decoder.conv_in.weight", "decoder.mid_block.attentions.0.to_out.0.bias",
                 "decoder.mid_block.attentions.0.group_norm.weight", "decoder.up_blocks.2.resnets.0.conv_shortcut.weight",
                 "decoder.up_blocks.3.resnets.0.conv_shortcut.weight", "decoder.up_blocks.2.upsamplers.0.conv.weight",
                 "decoder.up_blocks.3.resnets.2.norm2.bias", "decoder.conv_norm_out.weight", "decoder.conv_out.bias"):
        assert must in names, must
    assert not any(k.startswith("decoder.up_blocks.3.upsamplers") for k in names)
    assert not any("conv_shortcut" in k for k in names if "up_blocks.0" in k or "up_blocks.1" in k or "mid_block" in k)
    assert dict(listed)["decoder.conv_in.weight"] == (512, 4, 3, 3) and dict(listed)["decoder.conv_out.weight"] == (3, 128, 3, 3)


def test_old_attention_spelling_loads_to_the_same_tensors(net):
    from fresco_amd.vae import VAEDecoder, canonical_state_dict
    sd = net.state_dict()
    old = M.old_spelling(sd)
    assert sum(".query." in k or ".key." in k or ".value." in k or ".proj_attn." in k for k in old) == 8
    assert not any(".to_q." in k or ".to_out." in k for k in old)
    canon = canonical_state_dict(old)
    assert list(canon) == list(canonical_state_dict(sd))
    a, b = VAEDecoder(sd), VAEDecoder(old)
    for k in a.attn:
        assert torch.equal(a.attn[k].w, b.attn[k].w) and torch.equal(a.attn[k].b, b.attn[k].b)
    # the oldest checkpoints carry the projections as 1 x 1 convolutions
    conv = {k: (v[:, :, None, None] if ".attentions." in k and k.endswith("weight") and v.dim() == 2 else v) for k, v in old.items()}
    c = VAEDecoder(conv)
    assert all(torch.equal(a.attn[k].w, c.attn[k].w) for k in a.attn)


def test_decoder_refuses_another_architecture(net):
    from fresco_amd.vae import VAEDecoder
    sd = dict(net.state_dict())
    with pytest.raises(ValueError):
        VAEDecoder({k: v for k, v in sd.items() if "up_blocks.2.resnets.0.conv_shortcut" not in k})
    extra = dict(sd)
    extra["decoder.up_blocks.3.upsamplers.0.conv.weight"] = sd["decoder.up_blocks.2.upsamplers.0.conv.weight"]
    extra["decoder.up_blocks.3.upsamplers.0.conv.bias"] = sd["decoder.up_blocks.2.upsamplers.0.conv.bias"]
    with pytest.raises(ValueError):
        VAEDecoder(extra)
    narrow = dict(sd)
    narrow["decoder.conv_in.weight"] = sd["decoder.conv_in.weight"][:256]
    narrow["decoder.conv_in.bias"] = sd["decoder.conv_in.bias"][:256]
    with pytest.raises(ValueError):
        VAEDecoder(narrow)
    with pytest.raises(ValueError):
        VAEDecoder({k: v for k, v in sd.items() if k.startswith("encoder.")})


def _im2col(x, up2=False):
    """x (n, Hs, Ws, C) numpy -> (n, H, W, 9 C) rows in k = (ky, kx, ci) order, by the kernel's index rule"""
    from fresco_amd.vae import up2_source_index
    n, Hs, Ws, C = x.shape
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    out = np.zeros((n, H, W, 9 * C))
    for y in range(H):
        for xx in range(W):
            for ky in range(3):
                for kx in range(3):
                    ty, tx = y + ky - 1, xx + kx - 1
                    if up2:
                        src = up2_source_index(ty, tx, H, W)
                    else:
                        src = (ty, tx) if 0 <= ty < H and 0 <= tx < W else None
                    if src is not None:
                        out[:, y, xx, (ky * 3 + kx) * C:(ky * 3 + kx + 1) * C] = x[:, src[0], src[1]]
    return out


def test_packed_weights_multiplied_out_equal_conv2d():
    from fresco_amd.vae import pack_conv_weight
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 7, 6, generator=g, dtype=torch.float64)
    w = torch.randn(10, 6, 3, 3, generator=g, dtype=torch.float64).half().double()  # (the packing rounds to fp16 once)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).numpy()
    wp = pack_conv_weight(w).double().numpy()
    assert wp.shape == (10, 54)
    assert np.abs(_im2col(x.numpy()) @ wp.T - ref).max() < 1e-12
    # padded input channels: zero columns after each tap's real ones
    wpad = pack_conv_weight(w, cin_pad=8).double().numpy().reshape(10, 9, 8)
    assert not wpad[:, :, 6:].any() and np.array_equal(wpad[:, :, :6].reshape(10, 54), wp)
    # 1 x 1 and linear spellings
    w1 = torch.randn(10, 6, generator=g, dtype=torch.float64).half().double()
    assert torch.equal(pack_conv_weight(w1), pack_conv_weight(w1[:, :, None, None])) and pack_conv_weight(w1).shape == (10, 6)
    assert pack_conv_weight(w1).dtype == torch.float16


@pytest.mark.parametrize("size", [(5, 7), (3, 1), (1, 4)], ids=lambda s: "%dx%d" % s)
def test_up2_index_rule_equals_interpolate_then_conv(size):
    from fresco_amd.vae import pack_conv_weight
    g = torch.Generator().manual_seed(sum(size))
    x = torch.randn(2, size[0], size[1], 4, generator=g, dtype=torch.float64)
    w = torch.randn(5, 4, 3, 3, generator=g, dtype=torch.float64).half().double()
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = F.conv2d(up, w, padding=1).permute(0, 2, 3, 1).numpy()
    got = _im2col(x.numpy(), up2=True) @ pack_conv_weight(w).double().numpy().T
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-12


def test_decode_refuses_what_is_out_of_scope(net):
    from fresco_amd import FrescoHipError
    from fresco_amd.vae import VAEDecoder
    vae = M.build(torch.float16)
    dec = VAEDecoder.from_vae(vae)
    z = M.latents(M.CASES[0])
    for dt in (torch.float32, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError):
            dec.decode(z.to(dt))
    with pytest.raises(ValueError):
        dec.decode(z[:, :3])
    for flag in ("use_slicing", "use_tiling"):
        setattr(vae, flag, True)
        with pytest.raises(NotImplementedError):
            dec.decode(z)
        setattr(vae, flag, False)
    with pytest.raises(FrescoHipError):  # a CPU tensor: no fallback
        dec.decode(z)


def test_patch_rebinds_and_unpatch_restores():
    from fresco_amd.vae import patch_vae_decode, unpatch_vae_decode
    vae = M.build(torch.float16)
    pipe = types.SimpleNamespace(vae=vae)
    own = vae.decode
    dec = patch_vae_decode(pipe)
    assert pipe.vae.decode == dec.decode and "decode" in vars(vae)
    dec2 = patch_vae_decode(pipe)  # patching twice replaces, it does not stack
    assert pipe.vae.decode == dec2.decode
    unpatch_vae_decode(pipe)
    assert "decode" not in vars(vae) and pipe.vae.decode == own
    unpatch_vae_decode(pipe)  # and is idempotent


def _lib():
    from fresco_amd import _lib
    return _lib.load()


def test_header_binding_and_exports_agree():
    from fresco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fresco_vae.h")).read()
    protos = re.findall(r"^(?:int|size_t)\s+(vae_\w+)\(", hdr, re.M)
    assert sorted(protos) == sorted(_lib.VAE_SIGNATURES) and len(protos) == 5
    lib = _lib.load()
    for name in protos:
        assert getattr(lib, name).argtypes == _lib.VAE_SIGNATURES[name][1]
    assert not any(k.startswith("vae_") for k in _lib.SIGNATURES)
    for k, v in (("VAE_OUT_F16", 0), ("VAE_OUT_F32", 1), ("VAE_OUT_F16_NCHW", 2)):
        assert re.search(r"#define %s %d\b" % (k, v), hdr) and getattr(_lib, k) == v
    mk = open(os.path.join(ROOT, "fresco_amd", "csrc", "Makefile")).read()
    assert " vae.hip" in mk and "include/fresco_vae.h" in mk


def test_argument_checks_answer_before_any_hip_call():
    lib = _lib()
    p = 4096  # fake, aligned, never touched
    base = dict(x=p, xs=10 * 14 * 128, w=p, ws=0, bias=p, res=0, out=p, n=2, H=10, W=14, cin=128, cout=128, k=3, up2=0, kind=0,
                brows=0, ldo=128, st=0)

    def conv(**k):
        return lib.vae_conv(*dict(base, **k).values())
    # (the base case itself is valid and therefore never called: every call below fails a check)
    assert conv(x=0) == EINVAL and conv(w=0) == EINVAL and conv(out=0) == EINVAL
    assert conv(n=0) == EINVAL and conv(H=0) == EINVAL and conv(cout=0) == EINVAL and conv(cin=-32) == EINVAL
    assert conv(kind=3) == EINVAL and conv(ldo=64) == EINVAL
    assert conv(x=p + 8) == EINVAL and conv(w=p + 2) == EINVAL and conv(out=p + 4) == EINVAL and conv(bias=p + 4) == EINVAL
    assert conv(res=p + 2) == EINVAL and conv(res=p, kind=1) == EINVAL
    assert conv(xs=128) == EINVAL                        # a 3 x 3 plane stride that is not the plane
    assert conv(brows=1) == EINVAL and conv(k=1, up2=1) == EINVAL
    assert conv(ws=-8) == EINVAL and conv(ws=12) == EINVAL
    assert conv(kind=2, ldo=256) == EINVAL
    assert conv(k=5) == EUNSUPPORTED and conv(k=2) == EUNSUPPORTED
    assert conv(cin=4, xs=10 * 14 * 4) == EUNSUPPORTED and conv(cin=144, xs=10 * 14 * 144) == EUNSUPPORTED
    assert conv(up2=1, H=9, xs=4 * 7 * 128) == EUNSUPPORTED
    assert conv(n=65536) == EUNSUPPORTED
    assert conv(n=1, H=65536, W=32768, xs=65536 * 32768 * 128) == EUNSUPPORTED      # 2^31 pixels
    assert conv(n=1, H=(1 << 31) - 1, W=1, k=1, xs=0, cout=1 << 20, ldo=1 << 20) == EUNSUPPORTED  # 2^37 workgroups

    assert lib.vae_groupnorm_workspace_bytes(2, 540, 256) == 2 * 3 * 32 * 2 * 8 + 2 * 32 * 2 * 4
    assert lib.vae_groupnorm_workspace_bytes(2, 540, 64) == 0 and lib.vae_groupnorm_workspace_bytes(0, 540, 128) == 0
    gn = lambda x=p, g=p, b=p, y=p, ws=p, nb=1 << 20, n=2, P=540, C=256, eps=1e-6: lib.vae_groupnorm(x, g, b, y, ws, nb, n, P, C,  # noqa: E731
                                                                                                     eps, 1, 0)
    assert gn(x=0) == EINVAL and gn(g=0) == EINVAL and gn(y=0) == EINVAL and gn(ws=0) == EINVAL and gn(P=0) == EINVAL
    assert gn(eps=-1.0) == EINVAL and gn(x=p + 8) == EINVAL and gn(ws=p + 4) == EINVAL
    assert gn(C=64) == EUNSUPPORTED and gn(C=1024) == EUNSUPPORTED and gn(C=130) == EUNSUPPORTED and gn(n=65536) == EUNSUPPORTED
    assert gn(nb=100) == EWORKSPACE

    sm = lambda s=p, o=p, rows=10, Lk=70, ldi=96, ldo=96, scale=0.04: lib.vae_softmax(s, o, rows, Lk, ldi, ldo, scale, 0)  # noqa: E731
    assert sm(s=0) == EINVAL and sm(o=0) == EINVAL and sm(rows=0) == EINVAL and sm(Lk=0) == EINVAL
    assert sm(ldi=64) == EINVAL and sm(ldo=64) == EINVAL and sm(scale=0.0) == EINVAL and sm(scale=-1.0) == EINVAL
    assert sm(s=p + 2) == EINVAL and sm(o=p + 1) == EINVAL
    assert sm(rows=1 << 31) == EUNSUPPORTED

    vi = lambda z=p, w=p, b=p, o=p, n=2, h=8, ww=12, cpad=32: lib.vae_input(z, w, b, o, n, h, ww, cpad, 0)  # noqa: E731
    assert vi(z=0) == EINVAL and vi(w=0) == EINVAL and vi(b=0) == EINVAL and vi(o=0) == EINVAL and vi(n=0) == EINVAL
    assert vi(cpad=4) == EINVAL and vi(cpad=36) == EINVAL and vi(cpad=128) == EINVAL and vi(o=p + 8) == EINVAL
    assert vi(n=1, h=65536, ww=32768) == EUNSUPPORTED


def test_the_record_holds_what_the_gpu_tests_rely_on():
    gold = M.load_golden(GOLDEN)
    for case in M.CASES:
        key = M.case_key(case)
        n, h, w = case
        noise, peak = gold[key + "_noise"], gold[key + "_peak"]
        assert noise.shape == peak.shape == (len(M.TAPS) + 1,)
        assert (noise > 0).all() and (noise < 0.01).all() and (peak > 0).all() and (peak < M.ACT_LIMIT).all()
        assert 0 < float(gold[key + "_u8_share"]) < 0.25
        assert gold[key + "_image_u8"].shape == (n, 8 * h, 8 * w, 3) and gold[key + "_image_u8"].dtype == np.uint8
        assert gold[key + "_image"].dtype == np.float64 and gold[key + "_image"].shape[:2] == (n, 3)
        for t in M.TAPS:
            assert gold["%s_%s" % (key, t)].dtype == np.float64 and gold["%s_%s" % (key, t)].shape[0] == n


def test_restatement_reproduces_the_record_on_the_smallest_case(net):
    gold = M.load_golden(GOLDEN)
    case = M.CASES[0]
    key = M.case_key(case)
    taps = {}
    with torch.no_grad():
        img = net(M.latents(case).double(), taps)
    for t in M.TAPS:
        assert np.abs(M.thin(taps[t]) - gold["%s_%s" % (key, t)]).max() <= 1e-9 * gold[key + "_peak"].max()
    assert np.abs(M.thin_image(img) - gold[key + "_image"]).max() <= 1e-9 * gold[key + "_peak"].max()
    d = np.abs(M.tensor2numpy(img).astype(int) - gold[key + "_image_u8"].astype(int))
    assert d.max() <= 1 and (d > 0).mean() < 1e-4  # (a value within 1e-12 of a rounding boundary may flip across thread counts)
