"""The plain attention processor without a GPU: the binding of unet_attention against its header and the unchanged fresco_*
surface, every host refusal of the entry point with fake pointers (each answers before any HIP call), what ops.unet_attention
raises on before it asks the library, the golden file against a fresh derivation, the processor's and the patch's refusals
with their messages, patch / unpatch on a stand-in tree, and the text K | V cache's key logic with the kernels stood in for."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import unet_attention_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL, EUNSUPPORTED = -1, -2
F16, F32, BF16 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------------------------------
def _ctype(arg):
    if "*" in arg:
        return ctypes.c_void_p
    if "int64_t" in arg:
        return ctypes.c_int64
    if re.search(r"\bfloat\b", arg):
        return ctypes.c_float
    assert re.search(r"\bint\b", arg), arg
    return ctypes.c_int


def test_binding_is_the_headers_prototype(lib):
    from fresco_amd import _lib
    header = open(os.path.join(ROOT, "include", "fresco_unet_attn.h")).read()
    protos = dict(re.findall(r"^int (\w+)\(([^;]*)\);", header, re.M | re.S))
    assert sorted(protos) == sorted(_lib.UNET_ATTN_SIGNATURES) == ["unet_attention"]
    for name, args in protos.items():
        res, argtypes = _lib.UNET_ATTN_SIGNATURES[name]
        assert res is ctypes.c_int and [_ctype(a) for a in args.split(",")] == list(argtypes), name
        assert getattr(lib, name).argtypes == argtypes            # exported, and bound on the library's one handle
    mk = open(os.path.join(ROOT, "fresco_amd", "csrc", "Makefile")).read()
    assert "unet_attn.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "../../include/fresco_unet_attn.h" in mk


def test_fresco_surface_and_version_are_unchanged(lib):
    import fresco_amd
    from fresco_amd import _lib
    from test_capi_surface_cpu import _exported_fresco_functions
    exported = _exported_fresco_functions(fresco_amd.LIB_PATH)
    assert exported == set(_lib.SIGNATURES) and len(exported) == 78
    assert _lib.VERSION == "0.5.0.4" and "0.5.0.4" in lib.fresco_version().decode()
    assert not any(n.startswith("fresco_") for n in _lib.UNET_ATTN_SIGNATURES)
    for name in ("UNetAttnProcessor", "patch_unet_attention", "unpatch_unet_attention"):
        assert name in fresco_amd.__all__ and hasattr(fresco_amd, name)


def test_host_refusals_answer_before_any_hip_call(lib):
    p = 4096  # fake, aligned, never touched

    def call(q=p, q_ld=3840, k=p, v=p, kv_ld=3840, out=p, out_ld=1280, B=2, H=8, Lq=64, Lk=77, D=160, scale=0.079, dtype=F16):
        return lib.unet_attention(q, q_ld, k, v, kv_ld, out, out_ld, B, H, Lq, Lk, D, scale, dtype, None)

    for null in ("q", "k", "v", "out"):
        assert call(**{null: None}) == EINVAL, null
    for size in ("B", "H", "Lq", "Lk", "D"):
        assert call(**{size: 0}) == EINVAL and call(**{size: -1}) == EINVAL, size
    for ld in ("q_ld", "kv_ld", "out_ld"):
        assert call(**{ld: 1272}) == EINVAL      # below H * D
        assert call(**{ld: 1284}) == EINVAL      # not a multiple of 8
        assert call(**{ld: 0}) == EINVAL and call(**{ld: -1280}) == EINVAL
    assert call(scale=0.0) == EINVAL and call(scale=-0.1) == EINVAL and call(scale=float("nan")) == EINVAL
    for ptr in ("q", "k", "v", "out"):
        assert call(**{ptr: p + 8}) == EINVAL, ptr   # 16-byte pieces
    for D in (40, 80, 128, 152, 168, 320):
        assert call(D=D, H=8, q_ld=8 * 320, kv_ld=8 * 320, out_ld=8 * 320) == EUNSUPPORTED, D
    assert call(dtype=BF16) == EUNSUPPORTED          # bf16 is not built
    assert call(dtype=F32) == EINVAL and call(dtype=7) == EINVAL
    assert call(B=65536) == EUNSUPPORTED
    assert call(kv_ld=1 << 22) == EUNSUPPORTED       # 128 rows of a tile stay inside 32-bit byte offsets
    assert call(Lq=32 * 65535 + 1) == EUNSUPPORTED


def test_flash_entry_point_still_refuses_head_dim_160(lib):
    p = 4096
    rc = lib.fresco_attn_fwd(p, p, p, None, p, p, 1 << 20, 1, 8, 64, 160, 1, 64, 64, 0.079, 0.0, 1280, 1280, F16, None)
    assert rc == EUNSUPPORTED


def test_ops_check_before_the_library_is_asked():
    from fresco_amd import FrescoHipError, ops
    q = torch.zeros(2, 5, 320, dtype=torch.float16)
    with pytest.raises(FrescoHipError, match="GPU only"):
        ops.unet_attention(q, q, q, 2, 0.1)
    with pytest.raises(NotImplementedError, match="head dim 40"):
        ops.unet_attention(q, q, q, 8, 0.1)
    with pytest.raises(TypeError, match="bf16 is not built"):
        ops.unet_attention(q.bfloat16(), q.bfloat16(), q.bfloat16(), 2, 0.1)
    with pytest.raises(TypeError, match="float16"):
        ops.unet_attention(q, q.float(), q, 2, 0.1)
    with pytest.raises(ValueError, match="scale"):
        ops.unet_attention(q, q, q, 2, 0.0)
    with pytest.raises(ValueError, match="one row stride"):
        ops.unet_attention(q, q, torch.zeros(2, 5, 640, dtype=torch.float16)[..., :320], 2, 0.1)
    with pytest.raises(ValueError, match="one row stride"):
        ops.unet_attention(q, q, q[:, :4].contiguous(), 2, 0.1)     # Lk of k and of v
    with pytest.raises(ValueError, match="uniformly strided"):
        ops.unet_attention(torch.zeros(5, 2, 320, dtype=torch.float16).transpose(0, 1), q, q, 2, 0.1)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.unet_attention(torch.zeros(2, 5, 324, dtype=torch.float16)[..., 4:], q, q, 2, 0.1)
    with pytest.raises(ValueError, match="out must be"):
        ops.unet_attention(q, q, q, 2, 0.1, out=torch.zeros(2, 4, 320, dtype=torch.float16))
    # an expanded dimension: strides (640, 0, 1) over 1280 elements.  Ten rows 640 apart would leave the storage -- as `out`,
    # in a write
    expanded = torch.zeros(2, 1, 640, dtype=torch.float16)[..., :320].expand(2, 5, 320)
    assert expanded.stride() == (640, 0, 1)
    for bad in ((expanded, q, q), (q, expanded, q), (q, q, expanded)):
        with pytest.raises(ValueError, match="uniformly strided"):
            ops.unet_attention(*bad, 2, 0.1)
    with pytest.raises(ValueError, match="out: rows must be dense and uniformly strided"):
        ops.unet_attention(q, q, q, 2, 0.1, out=expanded)
    with pytest.raises(ValueError, match="at least 320 apart"):         # every row the same row
        ops.unet_attention(expanded[:1], q[:1], q[:1], 2, 0.1)
    # slices of one (rows, 3 C) buffer pass every check: only the GPU is missing
    qkv = torch.zeros(2, 5, 960, dtype=torch.float16)
    with pytest.raises(FrescoHipError, match="GPU only"):
        ops.unet_attention(qkv[..., :320], qkv[..., 320:640], qkv[..., 640:], 2, 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# the golden file
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_file_is_current():
    gold = M.load_golden(GOLDEN)
    keys = ["%s_%s" % (M.case_key(c), m) for c in M.CASES for m in M.MODES]
    assert sorted(gold) == sorted(k + s for k in keys for s in ("_noise", "_peak", "_sums", "_thin", "_logits"))
    for k in keys:
        assert 0 < float(gold[k + "_noise"]) < 2e-3 and float(gold[k + "_peak"]) > 0
        assert gold[k + "_logits"][0] >= M.MIN_LOGIT_SPAN and gold[k + "_logits"][1] > M.MIN_TOP_PROB
    case, mode = M.CASES[2], "cross"       # the cheapest 1280-wide case to derive again
    o, noise, peak, span, top = M.record(case, mode)
    k = "%s_%s" % (M.case_key(case), mode)
    sums, sample = M.checksums(o)
    np.testing.assert_allclose(gold[k + "_sums"], sums, rtol=1e-9)
    np.testing.assert_allclose(gold[k + "_thin"], sample, rtol=0, atol=1e-9)
    np.testing.assert_allclose(gold[k + "_noise"], noise, rtol=1e-3)
    np.testing.assert_allclose(gold[k + "_peak"], peak, rtol=1e-9)


def test_restated_processor_is_sdpa():
    case = M.CASES[0]
    x, text = M.inputs(case)
    for mode in M.MODES:
        e = text.double() if mode == "cross" else None
        with torch.no_grad():
            a = M.build_case(case, mode, torch.float64)(x.double(), e)
            b = M.build_case(case, mode, torch.float64, M.RefProcessor(sdpa=True))(x.double(), e)
        assert a.shape == x.shape and torch.allclose(a, b, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# the processor's refusals
# ---------------------------------------------------------------------------------------------------------------------
def _attn(C=160, heads=4, cross=None, dtype=torch.float16):
    """head dim 40; 160 = 5 x 32"""
    return M.build(C, heads, cross, dtype)


def _refused(match, change=None, x=None, **kw):
    from fresco_amd import UNetAttnProcessor
    attn = _attn(heads=kw.pop("heads", 4), cross=kw.pop("cross", None))
    if change:
        change(attn)
    x = torch.zeros(1, 4, 160, dtype=torch.float16) if x is None else x
    with pytest.raises(NotImplementedError, match=match) as e:
        UNetAttnProcessor()(attn, x, **kw)
    assert "no fallback" in str(e.value)


def test_processor_refusals_name_their_cause():
    _refused("attention_mask", attention_mask=torch.zeros(1, 4))
    _refused("4-D input", x=torch.zeros(1, 160, 2, 2, dtype=torch.float16))
    _refused("has a spatial_norm", lambda a: setattr(a, "spatial_norm", nn.Identity()))
    _refused("has a group_norm", lambda a: setattr(a, "group_norm", nn.GroupNorm(2, 160)))
    _refused("has norm_cross", lambda a: setattr(a, "norm_cross", nn.LayerNorm(160)))
    _refused("added_kv_proj_dim", lambda a: setattr(a, "added_kv_proj_dim", 32))
    for name in ("to_q", "to_k", "to_v"):
        _refused("%s has a bias" % name, lambda a, n=name: setattr(a, n, nn.Linear(160, 160).half()))

        class LoRALinear(nn.Linear):
            pass
        _refused("%s is LoRALinear, not a plain nn.Linear" % name,
                 lambda a, n=name: setattr(a, n, LoRALinear(160, 160, bias=False).half()))
    _refused("to_out\\[0\\] has no bias", lambda a: a.to_out.__setitem__(0, nn.Linear(160, 160, bias=False).half()))
    _refused("hidden_states are torch.float32, fp16 only", x=torch.zeros(1, 4, 160))
    _refused("torch.float32 weights, fp16 modules only", lambda a: a.float())
    _refused("torch.bfloat16 weights, fp16 modules only", lambda a: a.bfloat16(), x=torch.zeros(1, 4, 160, dtype=torch.bfloat16))
    _refused("encoder_hidden_states are torch.float32", cross=32, encoder_hidden_states=torch.zeros(1, 3, 32))
    _refused("hidden_states are on cpu, GPU tensors only")                      # everything else in order: only the GPU is missing
    _refused("on cpu, GPU tensors only", cross=32, encoder_hidden_states=torch.zeros(1, 3, 32, dtype=torch.float16))
    _refused("head dim 32 .*only 40/80/160", heads=5)
    _refused("is 48 wide, the projection kernels take multiples of 32", cross=48,
             encoder_hidden_states=torch.zeros(1, 3, 48, dtype=torch.float16))
    _refused("inputs 32 / 32 wide", x=torch.zeros(1, 4, 32, dtype=torch.float16))


def test_supported_modules_pass_the_module_check():
    from fresco_amd import UNetAttnProcessor
    for C, heads in ((320, 8), (640, 8), (1280, 8)):
        with torch.device("meta"):
            a1, a2 = M.Attention(C, heads).half(), M.Attention(C, heads, 768).half()
        assert UNetAttnProcessor.refusal(a1) is None and UNetAttnProcessor.refusal(a2) is None
    with torch.device("meta"):
        assert "head dim 96" in UNetAttnProcessor.refusal(M.Attention(768, 8).half())


# ---------------------------------------------------------------------------------------------------------------------
# patch / unpatch
# ---------------------------------------------------------------------------------------------------------------------
def _fresco_tree():
    """the stand-in tree as apply_FRESCO_attn leaves it: one FRESCO processor on up_blocks.2, the reference's on the rest"""
    from fresco_amd import FRESCOAttnProcessor2_0
    tree = M.build_tree()
    fresco = FRESCOAttnProcessor2_0(2, None)
    before = {}
    for name, m in M.attention_modules(tree):
        if name.startswith("up_blocks.2"):
            m.set_processor(fresco)
        before[name] = m.processor
    return tree, fresco, before


def test_patch_and_unpatch_on_a_standin_tree():
    from fresco_amd import UNetAttnProcessor, patch_unet_attention, unpatch_unet_attention
    tree, fresco, before = _fresco_tree()
    assert len(before) == 6
    assert patch_unet_attention(tree) == 4
    procs = {name: m.processor for name, m in M.attention_modules(tree)}
    shared = procs["mid_block.transformer_blocks.0.attn1"]
    assert isinstance(shared, UNetAttnProcessor) and shared.cache_text_kv
    for name, p in procs.items():
        assert (p is fresco) if name.startswith("up_blocks.2") else (p is shared), name     # ONE shared processor
    assert not hasattr(tree.proj, "processor")
    assert patch_unet_attention(tree) == 4                                  # patching again replaces, it does not stack
    assert unpatch_unet_attention(tree) == 4
    assert {name: m.processor for name, m in M.attention_modules(tree)} == before
    assert unpatch_unet_attention(tree) == 0
    # with the option, the FRESCO processor's cross-attention modules are taken too; its self-attention never
    assert patch_unet_attention(tree, include_fresco_cross=True) == 5
    procs = {name: m.processor for name, m in M.attention_modules(tree)}
    assert procs["up_blocks.2.transformer_blocks.0.attn1"] is fresco
    assert isinstance(procs["up_blocks.2.transformer_blocks.0.attn2"], UNetAttnProcessor)
    assert unpatch_unet_attention(tree) == 5
    assert {name: m.processor for name, m in M.attention_modules(tree)} == before
    # a module without set_processor gets the attribute
    for _, m in M.attention_modules(tree):
        m.set_processor = None
        del m.set_processor
    own = UNetAttnProcessor(cache_text_kv=False)
    assert patch_unet_attention(tree, processor=own) == 4 and tree.mid_block.transformer_blocks[0].attn2.processor is own
    assert unpatch_unet_attention(tree) == 4


def test_patch_refuses_by_name_before_it_patches_anything():
    from fresco_amd import patch_unet_attention
    tree, _, before = _fresco_tree()
    tree.mid_block.transformer_blocks[0].attn2.to_k = nn.Linear(64, 320).half()      # a bias; the modules in front are fine
    with pytest.raises(NotImplementedError, match="mid_block.transformer_blocks.0.attn2 to_k has a bias") as e:
        patch_unet_attention(tree)
    assert "no fallback" in str(e.value)
    assert {name: m.processor for name, m in M.attention_modules(tree)} == before
    tree, _, before = _fresco_tree()
    tree.up_blocks[2].transformer_blocks[0].attn2.norm_cross = nn.LayerNorm(64)
    assert patch_unet_attention(tree) == 4                                  # not chosen, not checked
    with pytest.raises(NotImplementedError, match="up_blocks.2.transformer_blocks.0.attn2 has norm_cross"):
        patch_unet_attention(tree, include_fresco_cross=True)
    assert {name: m.processor for name, m in M.attention_modules(tree)} == before    # the earlier patch is undone first


# ---------------------------------------------------------------------------------------------------------------------
# the text K | V cache and the packed copies: key logic, the kernels stood in for
# ---------------------------------------------------------------------------------------------------------------------
class _Ops:
    from fresco_amd.ops import Workspace

    def __init__(self):
        self.convs = []

    def conv_rows(self, x, w, bias=None, residual=None):
        cin, cout = x.shape[-1], w.shape[0]
        self.convs.append((x.data_ptr(), w.data_ptr(), x.numel() // cin, cin, cout))
        return (x.reshape(-1, cin).float() @ w.float().t()).half().view(x.shape[:-1] + (cout,))


@pytest.fixture
def fake_ops(monkeypatch):
    import fresco_amd.unet_attention as U
    fake = _Ops()
    monkeypatch.setattr(U, "ops", fake)
    return fake


def test_text_cache_key_is_the_tensor_object_and_its_version(fake_ops):
    from fresco_amd import UNetAttnProcessor
    attn = _attn(cross=32)
    text = torch.randn(2, 3, 32).half()
    proc = UNetAttnProcessor()
    kv = proc._text_kv(attn, text)
    assert kv.shape == (2, 3, 320) and len(fake_ops.convs) == 1 and fake_ops.convs[0][2:] == (6, 32, 320)
    assert proc._text_kv(attn, text) is kv and len(fake_ops.convs) == 1            # the same object: reused
    clone = text.clone()
    kv2 = proc._text_kv(attn, clone)                                               # a clone at the same values: projected again
    assert kv2 is not kv and len(fake_ops.convs) == 2 and torch.equal(kv2, kv)
    assert proc._text_kv(attn, clone) is kv2 and len(fake_ops.convs) == 2
    clone.mul_(1)                                                                  # a version bump: projected again
    assert proc._text_kv(attn, clone) is not kv2 and len(fake_ops.convs) == 3
    other = _attn(cross=32)                                                        # kept PER MODULE
    proc._text_kv(other, clone)
    assert len(fake_ops.convs) == 4 and proc._text_kv(attn, clone) is not None and len(fake_ops.convs) == 4
    proc.clear()
    proc._text_kv(attn, clone)
    assert len(fake_ops.convs) == 5
    never = UNetAttnProcessor(cache_text_kv=False)
    a, b = never._text_kv(attn, text), never._text_kv(attn, text)
    assert a is not b and len(fake_ops.convs) == 7 and not never._text


def test_packed_copies_follow_their_parameters_versions(fake_ops):
    from fresco_amd import UNetAttnProcessor
    attn = _attn(cross=32)
    proc = UNetAttnProcessor()
    w = proc._stacked(attn, ("to_k", "to_v"))
    assert w.shape == (320, 32) and torch.equal(w[:160], attn.to_k.weight) and torch.equal(w[160:], attn.to_v.weight)
    assert w.data_ptr() not in (attn.to_k.weight.data_ptr(), attn.to_v.weight.data_ptr())   # a COPY
    assert proc._stacked(attn, ("to_k", "to_v")) is w
    text = torch.randn(1, 3, 32).half()
    kv = proc._text_kv(attn, text)
    with torch.no_grad():
        attn.to_v.weight.mul_(2)                                                   # an in-place update is seen ...
    w2 = proc._stacked(attn, ("to_k", "to_v"))
    assert w2 is not w and torch.equal(w2[160:], attn.to_v.weight)
    assert proc._text_kv(attn, text) is not kv                                     # ... by the cached text projection too
    attn.to_k.weight = nn.Parameter(attn.to_k.weight.detach().clone())             # a replaced Parameter as well
    assert proc._stacked(attn, ("to_k", "to_v")) is not w2
    qkv = proc._stacked(_attn(), ("to_q", "to_k", "to_v"))
    assert qkv.shape == (480, 160)
