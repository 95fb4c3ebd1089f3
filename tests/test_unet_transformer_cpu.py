"""The UNet transformer without a GPU: the restatement of tests/unet_transformer_model.py against torch's functional
operators composed directly, the golden file against a fresh derivation, pack_geglu_weight's order,
patch_unet_transformers / unpatch_unet_transformers on a stand-in tree (count, restored forwards, every refusal), the
call-time refusals, return_dict, and the argument checks of unet_layernorm and unet_geglu with fake pointers (every check
answers before any HIP call)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import unet_transformer_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL, EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("C,heads,layers", [(64, 2, 1), (128, 4, 2)])
def test_restatement_is_the_functional_composition(C, heads, layers):
    net = M.build(C, heads, 48, torch.float64, layers)
    sd = net.state_dict()
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(2, C, 5, 7, generator=gen, dtype=torch.float64)
    text = torch.randn(2, 6, 48, generator=gen, dtype=torch.float64)
    taps = {}
    with torch.no_grad():
        got = net(x, text, return_dict=False, taps=taps)[0]
        h = F.conv2d(F.group_norm(x, 32, sd["norm.weight"], sd["norm.bias"], M.GN_EPS), sd["proj_in.weight"], sd["proj_in.bias"])
        h = h.permute(0, 2, 3, 1).reshape(2, 35, C)
        for i, blk in enumerate(net.transformer_blocks):
            p = "transformer_blocks.%d." % i
            ln = lambda t, nm: F.layer_norm(t, (C,), sd[p + nm + ".weight"], sd[p + nm + ".bias"], M.LN_EPS)  # noqa: E731
            h = h + blk.attn1(ln(h, "norm1"))
            h = h + blk.attn2(ln(h, "norm2"), encoder_hidden_states=text)
            proj = F.linear(ln(h, "norm3"), sd[p + "ff.net.0.proj.weight"], sd[p + "ff.net.0.proj.bias"])
            g = proj[..., :4 * C] * F.gelu(proj[..., 4 * C:])     # the exact (erf) GELU: rows 0 .. inner - 1 are the value
            if i == 0:
                assert torch.allclose(taps["tap"], g, rtol=0, atol=1e-12)
            h = h + F.linear(g, sd[p + "ff.net.2.weight"], sd[p + "ff.net.2.bias"])
        assert torch.allclose(taps["tokens"], h, rtol=0, atol=1e-12)
        ref = x + F.conv2d(h.reshape(2, 5, 7, C).permute(0, 3, 1, 2), sd["proj_out.weight"], sd["proj_out.bias"])
    assert torch.allclose(got, ref, rtol=0, atol=1e-12)
    # the rounded run rounds: it differs from the float64 one, by fp16-class noise
    with torch.no_grad():
        r = net(x, text, q=M.round16).sample
    d = float((r - got).abs().max() / got.abs().max())
    assert 0 < d < 1e-2


def test_standin_attention_is_softmax_attention():
    attn = M.build(64, 2, 48, torch.float64).transformer_blocks[0].attn2
    gen = torch.Generator().manual_seed(3)
    x, e = torch.randn(2, 9, 64, generator=gen, dtype=torch.float64), torch.randn(2, 6, 48, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        q, k, v = (t.view(2, -1, 2, 32).transpose(1, 2) for t in (attn.to_q(x), attn.to_k(e), attn.to_v(e)))
        ref = attn.to_out[0](F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(2, 9, 64))
        assert torch.allclose(attn(x, encoder_hidden_states=e), ref, rtol=0, atol=1e-12)
        half = attn.half()(x.half(), encoder_hidden_states=e.half())     # fp32 inside, one rounding
    assert half.dtype == torch.float16 and float((half.double() - ref).abs().max()) < 2e-3


def test_golden_file_is_current():
    gold = M.load_golden(GOLDEN)
    assert sorted(gold) == sorted(M.case_key(c) + s for c in M.CASES for s in ("_tap", "_out", "_noise", "_peak"))
    case = M.CASES[0]  # (320, 8, 2, 8, 12, 7, 64): the fewest weights, the cheapest to derive again
    key = M.case_key(case)
    tap, out, noise, peaks, act = M.record(case)
    assert act < M.ACT_LIMIT
    np.testing.assert_allclose(gold[key + "_tap"], M.thin(tap), rtol=0, atol=1e-9)
    np.testing.assert_allclose(gold[key + "_out"], M.thin(out), rtol=0, atol=1e-9)
    np.testing.assert_allclose(gold[key + "_noise"], noise, rtol=1e-3)
    np.testing.assert_allclose(gold[key + "_peak"], peaks, rtol=1e-9)
    for c in M.CASES:
        k = M.case_key(c)
        assert gold[k + "_tap"].shape[0] == c[2] and gold[k + "_out"].shape[0] == c[2]
        assert gold[k + "_noise"].shape == (2,) and (gold[k + "_noise"] > 0).all() and (gold[k + "_noise"] < 2e-3).all()
        x, text = M.inputs(c)
        assert x.shape == (c[2], c[0], c[3], c[4]) and text.shape == (c[2], c[5], c[6])
    x, _ = M.inputs(M.CASES[0])  # the last image differs in offset
    assert abs(float(x[0].float().mean())) < 0.1 and abs(float(x[-1].float().mean()) - 1.0) < 0.1


# ---------------------------------------------------------------------------------------------------------------------
# pack_geglu_weight
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_geglu_weight_order():
    from fresco_amd.unet_transformer import pack_geglu_weight
    inner, K = 96, 64
    gen = torch.Generator().manual_seed(1)
    w, b = torch.randn(2 * inner, K, generator=gen).half(), torch.randn(2 * inner, generator=gen).half()
    pw, pb = pack_geglu_weight(w, b)
    assert pw.shape == (2 * inner, K) and pw.dtype == torch.float16 and pw.is_contiguous()
    assert pb.shape == (2 * inner,) and pb.dtype == torch.float32
    for c in range(inner):
        row = 64 * (c // 32) + c % 32
        assert torch.equal(pw[row], w[c]) and torch.equal(pw[row + 32], w[inner + c]), c
        assert pb[row] == b[c].float() and pb[row + 32] == b[inner + c].float(), c
    with pytest.raises(ValueError, match="multiples of 32"):
        pack_geglu_weight(torch.zeros(2 * 48, 64).half(), torch.zeros(2 * 48).half())
    with pytest.raises(ValueError, match="multiples of 32"):
        pack_geglu_weight(torch.zeros(2 * 32, 48).half(), torch.zeros(2 * 32).half())
    with pytest.raises(ValueError, match="2 inner"):
        pack_geglu_weight(torch.zeros(65, 64).half(), torch.zeros(65).half())


# ---------------------------------------------------------------------------------------------------------------------
# patching (packing the weights needs no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _tree():
    return M.build_tree(torch.float16, c=64, heads=2, cross_dim=48)


def test_patch_and_unpatch_on_a_standin_tree():
    from fresco_amd import UNetTransformer, patch_unet_transformers, unpatch_unet_transformers
    tree = _tree()
    tfs = [m for m in tree.modules() if isinstance(m, M.Transformer)]
    assert len(tfs) == 1
    assert patch_unet_transformers(tree) == 1
    tf = tfs[0]
    native = vars(tf)["forward"]
    assert isinstance(native, UNetTransformer) and native.memory_format == torch.channels_last
    assert (native.channels, native.width, native.inner) == (64, 64, 256) and len(native.blocks) == 1
    assert native.norm_eps == M.GN_EPS and native.ln_eps == M.LN_EPS
    blk = native.blocks[0]
    assert blk.attn1 is tf.transformer_blocks[0].attn1 and blk.attn2 is tf.transformer_blocks[0].attn2   # the MODULES
    assert native.w_in.shape == (64, 64) and torch.equal(native.w_in, tf.proj_in.weight[:, :, 0, 0])
    assert torch.equal(native.b_out, tf.proj_out.bias.float())
    proj = tf.transformer_blocks[0].ff.net[0].proj
    assert blk.w_ff1.shape == (512, 64) and torch.equal(blk.w_ff1[:32], proj.weight[:32])
    assert torch.equal(blk.w_ff1[32:64], proj.weight[256:288]) and torch.equal(blk.b_ff1[32:64], proj.bias[256:288].float())
    assert torch.equal(blk.w_ff2, tf.transformer_blocks[0].ff.net[2].weight)
    assert "forward" not in vars(tree) and "forward" not in vars(tree.resnets[0]) and "forward" not in vars(tf.transformer_blocks[0])
    assert patch_unet_transformers(tree, memory_format=torch.contiguous_format) == 1   # patching again replaces, it does not stack
    assert vars(tf)["forward"] is not native and vars(tf)["forward"].memory_format == torch.contiguous_format
    assert unpatch_unet_transformers(tree) == 1
    assert "forward" not in vars(tf) and tf.forward.__func__ is M.Transformer.forward
    assert unpatch_unet_transformers(tree) == 0
    x, temb, text = torch.randn(1, 64, 4, 4), torch.randn(1, M.R.TEMB_CHANNELS), torch.randn(1, 5, 48)
    with torch.no_grad():
        assert tree.float()(x, temb, text).shape == (1, 16, 64)   # the module's own forwards run again
    with pytest.raises(ValueError, match="memory_format"):
        patch_unet_transformers(tree, memory_format=torch.preserve_format)


def _refused(change, match):
    from fresco_amd import patch_unet_transformers
    tree = _tree()
    tree.mid = M.build(64, 2, 48, torch.float16)      # a second transformer, in order: it must not be patched either
    change(tree.attentions[0])
    with pytest.raises(NotImplementedError, match=match) as e:
        patch_unet_transformers(tree)
    assert "attentions.0" in str(e.value)            # refused by name ...
    assert not any("forward" in vars(m) for m in tree.modules())   # ... before anything is patched


def test_refusals():
    blk = lambda tf: tf.transformer_blocks[0]  # noqa: E731
    _refused(lambda tf: tf.float(), "fp16 modules only")
    _refused(lambda tf: tf.bfloat16(), "fp16 modules only")
    _refused(lambda tf: setattr(tf, "use_linear_projection", True), "use_linear_projection")
    _refused(lambda tf: setattr(tf, "proj_in", nn.Linear(64, 64).half()), "use_linear_projection")
    _refused(lambda tf: setattr(tf, "proj_in", nn.Conv2d(64, 64, 3, 1, 1).half()), "only 1 x 1 convolutions")
    _refused(lambda tf: setattr(tf, "norm", nn.GroupNorm(16, 64, eps=1e-6).half()), "GroupNorm of 16 groups")

    class AdaLayerNorm(nn.LayerNorm):
        pass
    _refused(lambda tf: setattr(blk(tf), "norm1", AdaLayerNorm(64).half()), "norm1 is AdaLayerNorm")
    _refused(lambda tf: setattr(blk(tf), "norm3", nn.LayerNorm(64, elementwise_affine=False).half()), "norm3 is LayerNorm, only a plain")
    _refused(lambda tf: setattr(blk(tf), "use_ada_layer_norm", True), "only a plain nn.LayerNorm")
    _refused(lambda tf: setattr(blk(tf), "only_cross_attention", True), "only_cross_attention")
    _refused(lambda tf: setattr(blk(tf), "attn2", None), "attn2 is None")

    def gelu_ff(tf):           # diffusers' GELU / ApproximateGELU feed-forward: a proj of the inner width, no gate
        class GELU(nn.Module):
            def __init__(self):
                super().__init__()
                self.proj = nn.Linear(64, 256)
        blk(tf).ff.net[0] = GELU().half()
    _refused(gelu_ff, "not a GEGLU|only GEGLU")

    def no_proj(tf):
        blk(tf).ff.net[0] = nn.Linear(64, 512).half()
    _refused(no_proj, "has no proj")
    _refused(lambda tf: setattr(blk(tf).ff.net[1], "p", 0.1), "dropout 0.1")
    _refused(lambda tf: setattr(blk(tf), "_chunk_size", 2), "_chunk_size")

    def rebuild(C, heads):
        def change(tf):
            with torch.device("meta"):     # shapes and dtypes are all a refusal reads
                new = M.Transformer(C, heads, 48).half()
            for part in ("norm", "proj_in", "transformer_blocks", "proj_out"):
                setattr(tf, part, getattr(new, part))
        return change
    _refused(rebuild(32, 1), "32 channels")           # below the kernels' range
    _refused(rebuild(2624, 41), "2624 channels")      # 41 x 64: above it
    _refused(rebuild(96, 3), "96 channels")           # not a multiple of 64

    def narrow_ff(tf):        # inner = 48: not a multiple of 32
        blk(tf).ff.net[0] = M.GEGLU(64, 48).half()
        blk(tf).ff.net[2] = nn.Linear(48, 64).half()
    _refused(narrow_ff, "feed-forward 48 wide")


def test_call_time_refusals_and_return_dict():
    from fresco_amd import FrescoHipError, UNetTransformer
    net = M.build(64, 2, 48, torch.float16)
    native = UNetTransformer.from_module(net)
    x = torch.zeros(1, 64, 4, 4, dtype=torch.float16)
    for name in ("timestep", "class_labels", "attention_mask", "encoder_attention_mask"):
        with pytest.raises(NotImplementedError, match=name):
            native(x, None, **{name: torch.zeros(1)})
    with pytest.raises(NotImplementedError, match="timestep"):
        native(x, None, torch.zeros(1))                 # diffusers' positional order
    with pytest.raises(TypeError, match="fp16 hidden_states only"):
        native(x.float())
    with pytest.raises(ValueError, match=r"\(n, 64, H, W\)"):
        native(torch.zeros(1, 32, 4, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="memory_format"):
        native(x, memory_format=torch.preserve_format)
    with pytest.raises(FrescoHipError, match="GPU only"):   # no fallback on CPU tensors
        native(x, torch.zeros(1, 5, 48, dtype=torch.float16), return_dict=False)
    # return_dict both ways, with the kernels stood in for by the module's own arithmetic: what comes back is the wrapping
    import fresco_amd.unet_transformer as T
    calls = []

    class Ops:
        @staticmethod
        def _need_gpu(*a):
            pass

        @staticmethod
        def unet_groupnorm(xn, g, b, eps, silu=False):
            calls.append("groupnorm")
            return xn

        @staticmethod
        def conv_rows(x, w, bias=None, residual=None):
            calls.append("conv")
            return torch.zeros(x.shape[:-1] + (w.shape[0],), dtype=torch.float16)

        @staticmethod
        def unet_layernorm(x, g, b, eps, residual=None, want_sum=False):
            calls.append("layernorm")
            return (x, x) if want_sum else x

        @staticmethod
        def unet_geglu(y, w, b):
            calls.append("geglu")
            return torch.zeros(y.shape[:-1] + (w.shape[0] // 2,), dtype=torch.float16)
    real = T.ops
    T.ops = Ops
    try:
        text = torch.zeros(1, 5, 48, dtype=torch.float16)
        as_tuple = native(x, text, return_dict=False)
        assert isinstance(as_tuple, tuple) and len(as_tuple) == 1 and as_tuple[0].shape == (1, 64, 4, 4)
        assert as_tuple[0].is_contiguous(memory_format=torch.channels_last)
        as_object = native(x, encoder_hidden_states=text)
        assert not isinstance(as_object, tuple) and as_object.sample.shape == (1, 64, 4, 4)
        assert native(x, text, memory_format=torch.contiguous_format).sample.is_contiguous()
        assert calls[:8] == ["groupnorm", "conv", "layernorm", "layernorm", "layernorm", "geglu", "conv", "conv"]
    finally:
        T.ops = real


def test_constructor_takes_a_state_dict_and_the_attention_modules():
    from fresco_amd import UNetTransformer
    net = M.build(64, 2, 48, torch.float16, layers=2)
    sd = {"mid.attentions.0." + k: v for k, v in net.state_dict().items()}
    pairs = [(b.attn1, b.attn2) for b in net.transformer_blocks]
    t = UNetTransformer(sd, "mid.attentions.0", pairs)
    assert len(t.blocks) == 2 and t.blocks[1].attn2 is pairs[1][1] and (t.channels, t.width, t.inner) == (64, 64, 256)
    with pytest.raises(ValueError, match="missing"):
        UNetTransformer(sd, "mid.attentions.1", pairs)
    with pytest.raises(ValueError, match="missing"):
        UNetTransformer(sd, "mid.attentions.0", pairs + pairs[:1])     # a third block the state dict does not have
    with pytest.raises(ValueError, match="one pair per block"):
        UNetTransformer(sd, "mid.attentions.0", [])
    with pytest.raises(TypeError, match="fp16"):
        UNetTransformer({k: v.float() for k, v in sd.items()}, "mid.attentions.0", pairs)
    lin = dict(sd)
    lin["mid.attentions.0.proj_in.weight"] = lin["mid.attentions.0.proj_in.weight"][:, :, 0, 0]
    with pytest.raises(NotImplementedError, match="1 x 1 convolution"):
        UNetTransformer(lin, "mid.attentions.0", pairs)


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points' argument checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


def test_version_and_binding(lib):
    from fresco_amd import _lib
    assert _lib.VERSION == "0.5.0.4" and "0.5.0.4" in lib.fresco_version().decode()
    assert sorted(_lib.UNET_TF_SIGNATURES) == ["unet_geglu", "unet_layernorm"]
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "fresco_unet_tf.h")).read()
    for name in _lib.UNET_TF_SIGNATURES:
        assert "int %s(" % name in header and getattr(lib, name).argtypes == _lib.UNET_TF_SIGNATURES[name][1]


def test_layernorm_argument_checks(lib):
    p = 4096  # fake, aligned, never touched

    def call(x=p, ldx=320, r=None, ldr=0, gamma=p, beta=p, y=p, ldy=320, s=None, lds=0, rows=192, C=320, eps=1e-5):
        return lib.unet_layernorm(x, ldx, r, ldr, gamma, beta, y, ldy, s, lds, rows, C, eps, None)

    for C_bad in (56, 2568, 324, 4096):
        assert call(C=C_bad, ldx=4096, ldy=4096) == EUNSUPPORTED
    assert call(rows=1 << 31) == EUNSUPPORTED
    for null in ("x", "gamma", "beta", "y"):
        assert call(**{null: None}) == EINVAL
    assert call(rows=0) == EINVAL and call(C=0) == EINVAL and call(C=-64) == EINVAL
    assert call(eps=-1.0) == EINVAL and call(eps=float("nan")) == EINVAL
    assert call(ldx=312) == EINVAL and call(ldx=324) == EINVAL and call(ldy=312) == EINVAL and call(ldy=324) == EINVAL
    assert call(r=p, ldr=0) == EINVAL and call(r=p, ldr=324) == EINVAL
    assert call(s=p, lds=0) == EINVAL and call(s=p, lds=324) == EINVAL
    assert call(x=p + 8) == EINVAL and call(y=p + 8) == EINVAL and call(gamma=p + 4) == EINVAL and call(beta=p + 8) == EINVAL
    assert call(r=p + 8, ldr=320) == EINVAL and call(s=p + 2, lds=320) == EINVAL


def test_geglu_argument_checks(lib):
    p = 4096

    def call(x=p, w=p, bias=p, out=p, M=192, K=320, inner=1280, ldo=1280):
        return lib.unet_geglu(x, w, bias, out, M, K, inner, ldo, None)

    assert call(K=328) == EUNSUPPORTED and call(K=16) == EUNSUPPORTED
    assert call(inner=48, ldo=48) == EUNSUPPORTED and call(inner=1296, ldo=1296) == EUNSUPPORTED
    assert call(M=1 << 31) == EUNSUPPORTED and call(M=1 << 40) == EUNSUPPORTED
    for null in ("x", "w", "bias", "out"):
        assert call(**{null: None}) == EINVAL
    assert call(M=0) == EINVAL and call(K=0) == EINVAL and call(inner=0) == EINVAL and call(M=-1) == EINVAL
    assert call(ldo=1276) == EINVAL            # ldo < inner
    assert call(ldo=1282) == EINVAL            # ldo % 4
    assert call(x=p + 8) == EINVAL and call(w=p + 8) == EINVAL and call(out=p + 4) == EINVAL and call(bias=p + 4) == EINVAL


def test_ops_check_before_the_library_is_asked():
    from fresco_amd import FrescoHipError, ops
    x = torch.zeros(4, 320, dtype=torch.float16)
    g = torch.ones(320)
    with pytest.raises(FrescoHipError, match="GPU only"):
        ops.unet_layernorm(x, g, g)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.unet_layernorm(torch.zeros(4, 60, dtype=torch.float16), g, g)
    with pytest.raises(TypeError, match="float16"):
        ops.unet_layernorm(x.float(), g, g)
    with pytest.raises(ValueError, match="uniformly strided"):
        ops.unet_layernorm(torch.zeros(320, 4, dtype=torch.float16).t(), g, g)
    with pytest.raises(ValueError, match="residual of 2 rows"):
        ops.unet_layernorm(x, g, g, residual=x[:2])
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.unet_layernorm(torch.zeros(4, 324, dtype=torch.float16)[:, :320], g, g)
    # three dimensions whose leading two do not nest: images 512 apart, 3 rows of 128 each.  (The whole [:, ::2] of the same
    # tensor DOES nest, 4 x 128 = 512: it is 8 uniformly strided rows and passes this check.)
    g64 = torch.ones(64)
    with pytest.raises(ValueError, match="uniformly strided"):
        ops.unet_layernorm(torch.zeros(2, 8, 64, dtype=torch.float16)[:, :6:2], g64, g64)
    with pytest.raises(ValueError, match="uniformly strided"):
        ops.unet_layernorm(torch.zeros(2, 8, 64, dtype=torch.float16)[:, :3], g64, g64)
    with pytest.raises(FrescoHipError, match="GPU only"):
        ops.unet_layernorm(torch.zeros(2, 8, 64, dtype=torch.float16)[:, ::2], g64, g64)
    # an expanded dimension: strides (256, 0, 1) over 512 elements.  Eight rows 256 apart would leave the storage
    wide = torch.zeros(2, 1, 256, dtype=torch.float16)
    expanded = wide[..., :64].expand(2, 4, 64)
    assert expanded.stride() == (256, 0, 1)
    with pytest.raises(ValueError, match="uniformly strided"):
        ops.unet_layernorm(expanded, g64, g64)
    with pytest.raises(ValueError, match="uniformly strided"):
        ops.unet_layernorm(torch.zeros(2, 4, 64, dtype=torch.float16), g64, g64, residual=expanded)
    with pytest.raises(ValueError, match="at least 64 apart"):          # every row the same row
        ops.unet_layernorm(wide[0, :, :64].expand(4, 64), g64, g64)
    with pytest.raises(ValueError, match="at least 64 apart"):
        ops.unet_layernorm(torch.zeros(2, 1, 64, dtype=torch.float16).expand(2, 4, 64)[:1], g64, g64)
    with pytest.raises(FrescoHipError, match="GPU only"):     # a 3-D column slice passes every check: only the GPU is missing
        ops.unet_layernorm(torch.zeros(2, 5, 192, dtype=torch.float16)[..., 64:128], g64, g64)
    w, b = torch.zeros(128, 320, dtype=torch.float16), torch.zeros(128)
    with pytest.raises(FrescoHipError, match="GPU only"):
        ops.unet_geglu(x, w, b)
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.unet_geglu(x, torch.zeros(96, 320, dtype=torch.float16), torch.zeros(96))
    with pytest.raises(ValueError, match="2 inner, K"):
        ops.unet_geglu(x, torch.zeros(128, 64, dtype=torch.float16), b)
    with pytest.raises(ValueError, match=r"out must be a fp16 \(4, 64\)"):
        ops.unet_geglu(x, w, b, out=torch.zeros(4, 32, dtype=torch.float16))


def test_uniform_rows_is_its_definition():
    """accepted exactly where row i starts i ld elements after the first, ld >= C and a multiple of 8, the values dense: over
    every (a, b, 64) view of one buffer with these strides, a stride of 0 (an expanded dimension) among them"""
    import itertools
    from fresco_amd import ops
    C, buf, accepted = 64, torch.zeros(1 << 13, dtype=torch.float16), 0
    for shape in itertools.product((1, 2, 3), (1, 2, 4)):
        for st in itertools.product((0, 64, 128, 256, 384, 512, 1024), (0, 8, 64, 72, 128, 256), (1, 2)):
            starts = [a * st[0] + b * st[1] for a in range(shape[0]) for b in range(shape[1])]
            ld = starts[1] - starts[0] if len(starts) > 1 else C
            want = st[2] == 1 and starts == [i * ld for i in range(len(starts))] and ld >= C and ld % 8 == 0
            try:
                got = ops._uniform_rows(buf.as_strided(shape + (C,), st), "t", C)
            except ValueError:
                got = None
            assert got == ((ld, len(starts)) if want else None), (shape, st, got)
            accepted += want
    assert accepted == 182


def test_conv_rows_asks_vae_conv_for_one_run_of_rows(monkeypatch):
    """the flat-row form: n, H, W, cin, cout, ksize = 1, rows, 1, K, N, 1, whatever the leading shape"""
    from fresco_amd import _lib, ops
    asked = []

    class Lib:
        @staticmethod
        def vae_conv(x, x_img_stride, w, w_img_stride, bias, residual, out, n, H, W, cin, cout, ksize, up2, out_kind,
                     bias_rows, ldo, stream):
            asked.append((n, H, W, cin, cout, ksize, x_img_stride, w_img_stride, bool(bias), bool(residual), up2, out_kind,
                          bias_rows, ldo))
            return 0
    monkeypatch.setattr(_lib, "load", lambda: Lib)
    monkeypatch.setattr(ops, "_need_gpu", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    x, w = torch.zeros(2, 3, 64, dtype=torch.float16), torch.zeros(96, 64, dtype=torch.float16)
    out = ops.conv_rows(x, w)
    assert out.shape == (2, 3, 96) and out.dtype == torch.float16 and out.is_contiguous()
    assert asked == [(1, 6, 1, 64, 96, 1, 6 * 64, 0, False, False, 0, _lib.VAE_OUT_F16, 0, 96)]
    r = torch.zeros(2, 3, 96, dtype=torch.float16)
    assert ops.conv_rows(x, w, torch.zeros(96), residual=r).shape == (2, 3, 96)
    assert asked[1] == (1, 6, 1, 64, 96, 1, 6 * 64, 0, True, True, 0, _lib.VAE_OUT_F16, 0, 96)
    assert ops.conv_rows(x.view(6, 64), w).shape == (6, 96) and asked[2] == asked[0]
    with pytest.raises(ValueError, match="conv_rows"):
        ops.conv_rows(x, torch.zeros(96, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="conv_rows"):
        ops.conv_rows(x, torch.zeros(96 * 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="contiguous"):
        ops.conv_rows(torch.zeros(2, 3, 128, dtype=torch.float16)[..., :64], w)
    assert len(asked) == 3
