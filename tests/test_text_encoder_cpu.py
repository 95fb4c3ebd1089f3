"""The CLIP text encoder without a GPU: header == binding == exported symbols for the three entry points of
include/fresco_text.h, every argument check with fake pointers (each answers before any HIP call), every Python refusal, both
parameter layouts, patch_text_encoder / unpatch_text_encoder on a stand-in pipe, the package's exports, the restated model of
tests/clip_text_model.py against the real transformers.CLIPTextModel in float64, and the golden file against a fresh
derivation."""
import os
import re
import types

import numpy as np
import pytest
import torch

import clip_text_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL, EUNSUPPORTED = -1, -2
NAMES = ("CLIPTextEncoder", "patch_text_encoder", "unpatch_text_encoder")
F16, F32, BF16 = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------
# the C surface
# ---------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    import fresco_amd
    from fresco_amd import _lib, text_encoder
    hdr = open(os.path.join(ROOT, "include", "fresco_text.h")).read()
    protos = re.findall(r"^(?:int|size_t)\s+(\w+)\(", hdr, re.M)
    assert sorted(protos) == sorted(_lib.TEXT_SIGNATURES) == ["clip_attention", "clip_embed", "clip_fc1"]
    lib = _lib.load()
    others = [_lib.SIGNATURES, _lib.VAE_SIGNATURES, _lib.VAE_ENC_SIGNATURES, _lib.UNET_SIGNATURES, _lib.UNET_TF_SIGNATURES,
              _lib.UNET_ATTN_SIGNATURES, _lib.UNET_SHELL_SIGNATURES]
    for name in protos:
        assert not name.startswith("fresco_") and not any(name in o for o in others)
        res, argtypes = _lib.TEXT_SIGNATURES[name]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res  # (getattr: it is exported)
        args = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1).split(",")
        kinds = ["p" if "*" in a else a.split()[0] for a in args]
        bound = [{"c_void_p": "p", "c_int": "int", "c_long": "int64_t", "c_float": "float"}[t.__name__] for t in argtypes]
        assert kinds == bound, (name, kinds, bound)
    mk = open(os.path.join(ROOT, "fresco_amd", "csrc", "Makefile")).read()
    assert " text.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1) and "include/fresco_text.h" in mk
    assert not re.search(r"build/text\.o[^\n]*EXTRA", mk)
    for name in NAMES:
        assert name in fresco_amd.__all__ and getattr(fresco_amd, name) is getattr(text_encoder, name)


def test_version_and_the_pinned_surface_are_unchanged():
    from fresco_amd import _lib
    lib = _lib.load()
    assert _lib.VERSION == "0.5.0.4" and lib.fresco_version().decode().split()[1] == "0.5.0.4"
    assert len(_lib.SIGNATURES) == 78 and all(n.startswith("fresco_") for n in _lib.SIGNATURES)
    assert not any(n.startswith("fresco_") for n in _lib.TEXT_SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "fresco_hip.h")).read()
    assert not re.search(r"\bclip_", hdr)


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


def test_embed_argument_checks(lib):
    p = 4096  # fake, aligned, never touched: every call below fails a check
    base = dict(tok=p, pos=p, ids=p, out=p, B=2, L=77, C=768, vocab=1000, st=0)

    def emb(**k):
        return lib.clip_embed(*dict(base, **k).values())
    for null in ("tok", "pos", "ids", "out"):
        assert emb(**{null: 0}) == EINVAL
    for size in ("B", "L", "C", "vocab"):
        assert emb(**{size: 0}) == EINVAL and emb(**{size: -3}) == EINVAL
    assert emb(C=12) == EUNSUPPORTED and emb(C=770) == EUNSUPPORTED
    assert emb(B=1 << 20, L=1 << 11) == EUNSUPPORTED                              # 2^31 rows
    assert emb(tok=p + 8) == EINVAL and emb(pos=p + 2) == EINVAL and emb(out=p + 8) == EINVAL and emb(ids=p + 4) == EINVAL
    assert emb(tok=0, C=12) == EINVAL       # a null pointer answers first


def test_attention_argument_checks(lib):
    p = 4096
    base = dict(q=p, k=p + 1536, v=p + 3072, ld=2304, out=p, out_ld=768, B=2, H=12, L=77, D=64, scale=0.125, dtype=F16, st=0)

    def att(**k):
        return lib.clip_attention(*dict(base, **k).values())
    for null in ("q", "k", "v", "out"):
        assert att(**{null: 0}) == EINVAL
    for size in ("B", "H", "L", "D"):
        assert att(**{size: 0}) == EINVAL and att(**{size: -1}) == EINVAL
    assert att(scale=0.0) == EINVAL and att(scale=-1.0) == EINVAL and att(scale=float("nan")) == EINVAL
    assert att(dtype=F32) == EINVAL and att(dtype=7) == EINVAL
    assert att(ld=760) == EINVAL and att(ld=2308) == EINVAL and att(out_ld=767) == EINVAL and att(out_ld=772) == EINVAL
    assert att(q=p + 8) == EINVAL and att(k=p + 2) == EINVAL and att(v=p + 4) == EINVAL and att(out=p + 8) == EINVAL
    assert att(L=129) == EUNSUPPORTED and att(L=1 << 20) == EUNSUPPORTED
    assert att(D=80, ld=2880, out_ld=960) == EUNSUPPORTED and att(D=160, H=8, ld=3840, out_ld=1280) == EUNSUPPORTED
    assert att(D=32, H=24) == EUNSUPPORTED
    assert att(dtype=BF16) == EUNSUPPORTED
    assert att(B=65536) == EUNSUPPORTED and att(H=65536, ld=3 << 22, out_ld=1 << 22) == EUNSUPPORTED
    assert att(q=0, L=129) == EINVAL        # a null pointer answers first


def test_fc1_argument_checks(lib):
    p = 4096
    base = dict(x=p, w=p, bias=p, out=p, M=154, K=768, N=3072, ldo=3072, st=0)

    def fc1(**k):
        return lib.clip_fc1(*dict(base, **k).values())
    for null in ("x", "w", "bias", "out"):
        assert fc1(**{null: 0}) == EINVAL
    for size in ("M", "K", "N"):
        assert fc1(**{size: 0}) == EINVAL and fc1(**{size: -64}) == EINVAL
    assert fc1(K=760) == EUNSUPPORTED and fc1(K=16) == EUNSUPPORTED               # K % 32
    assert fc1(N=3104, ldo=3104) == EUNSUPPORTED and fc1(N=32, ldo=32) == EUNSUPPORTED    # N % 64
    assert fc1(M=1 << 31) == EUNSUPPORTED and fc1(N=1 << 30, ldo=1 << 30) == EUNSUPPORTED
    assert fc1(ldo=3071) == EINVAL and fc1(ldo=3074) == EINVAL and fc1(ldo=64) == EINVAL
    assert fc1(x=p + 8) == EINVAL and fc1(w=p + 2) == EINVAL and fc1(bias=p + 4) == EINVAL and fc1(out=p + 4) == EINVAL
    assert fc1(x=0, K=760) == EINVAL        # a null pointer answers first


def test_attention_128_tokens_is_within_the_checks():
    """L = 128 is the largest length taken: the constant the Python layer refuses above"""
    from fresco_amd import ops
    src = open(os.path.join(ROOT, "fresco_amd", "csrc", "text.hip")).read()
    assert re.search(r"constexpr int CA_LMAX = 128;", src) and "L > CA_LMAX" in src
    assert ops.CLIP_ATTN_MAX_L == 128 and ops.CLIP_ATTN_HEAD_DIM == 64


# ---------------------------------------------------------------------------------------------------------------------
# Python: refusals, layouts, patch / unpatch
# ---------------------------------------------------------------------------------------------------------------------
CASE_B = M.CASES[1]


def _half_model(case=CASE_B):
    return M.build(case, torch.float16)


def test_ops_refuse_what_the_kernels_would():
    from fresco_amd import FrescoHipError, ops
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)  # noqa: E731
    ids = torch.zeros(2, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="int64"):
        ops.clip_embed(ids.int(), h(10, 64), h(77, 64))
    with pytest.raises(ValueError, match="int64"):
        ops.clip_embed(ids[0], h(10, 64), h(77, 64))
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.clip_embed(ids, h(10, 60), h(77, 60))
    with pytest.raises(ValueError, match="position table"):
        ops.clip_embed(ids, h(10, 64), h(4, 64))
    with pytest.raises(TypeError):
        ops.clip_embed(ids, h(10, 64).float(), h(77, 64))
    with pytest.raises(ValueError, match="contiguous"):
        ops.clip_embed(ids, h(10, 128)[:, :64], h(77, 64))
    with pytest.raises(FrescoHipError, match="GPU"):
        ops.clip_embed(ids, h(10, 64), h(77, 64))
    q = h(2, 5, 128)
    with pytest.raises(NotImplementedError, match="head dim 32"):
        ops.clip_attention(q, q, q, 4, 0.125)
    with pytest.raises(NotImplementedError, match="129 tokens"):
        ops.clip_attention(h(1, 129, 64), h(1, 129, 64), h(1, 129, 64), 1, 0.125)
    with pytest.raises(ValueError, match="scale"):
        ops.clip_attention(q, q, q, 2, 0.0)
    with pytest.raises(ValueError, match="one row stride"):
        ops.clip_attention(q, h(2, 5, 256)[..., :128], q, 2, 0.125)
    with pytest.raises(TypeError, match="bf16 is not built"):
        ops.clip_attention(q.bfloat16(), q.bfloat16(), q.bfloat16(), 2, 0.125)
    with pytest.raises(ValueError, match="uniformly strided"):
        ops.clip_attention(h(5, 2, 128).transpose(0, 1), q, q, 2, 0.125)
    with pytest.raises(FrescoHipError, match="GPU"):
        ops.clip_attention(q, q, q, 2, 0.125)
    b = torch.zeros(128)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.clip_fc1(h(3, 48), h(128, 48), b)
    with pytest.raises(ValueError, match="of 64"):
        ops.clip_fc1(h(3, 64), h(96, 64), torch.zeros(96))
    with pytest.raises(TypeError):
        ops.clip_fc1(h(3, 64), h(128, 64), b.half())
    with pytest.raises(ValueError, match="out must be"):
        ops.clip_fc1(h(3, 64), h(128, 64), b, out=h(3, 64))
    with pytest.raises(FrescoHipError, match="GPU"):
        ops.clip_fc1(h(3, 64), h(128, 64), b)


def _config(**changes):
    c = M.make_config(CASE_B)
    for k, v in changes.items():
        setattr(c, k, v)
    return c


def test_module_refusals_each_name_their_cause():
    from fresco_amd import CLIPTextEncoder
    net = _half_model()
    sd = net.state_dict()
    # (the parameters are on the CPU: from_state_dict and from_module refuse that LAST, so every other cause is seen first)
    with pytest.raises(NotImplementedError, match="GPU tensors only.*no fallback"):
        CLIPTextEncoder.from_state_dict(sd, net.config)
    with pytest.raises(NotImplementedError, match="GPU modules only"):
        CLIPTextEncoder.from_module(net)
    for changes, cause in ((dict(hidden_act="gelu"), "hidden_act 'gelu', only quick_gelu"),
                           (dict(num_attention_heads=4), "head dim 32"),
                           (dict(num_attention_heads=3), r"head dim \?"),
                           (dict(hidden_size=96, num_attention_heads=1), "head dim 96"),
                           (dict(intermediate_size=480), "multiples of 64"),
                           (dict(hidden_size=2624, num_attention_heads=41), "multiples of 64")):
        with pytest.raises(NotImplementedError, match=cause):
            CLIPTextEncoder(sd, _config(**changes))
        net.config = _config(**changes)
        assert re.search(cause, CLIPTextEncoder.refusal(net))
    net.config = _config()
    for dtype, name in ((torch.bfloat16, "bfloat16"), (torch.float32, "float32")):
        other = M.build(CASE_B, dtype)
        assert name in CLIPTextEncoder.refusal(other) and "fp16 modules only" in CLIPTextEncoder.refusal(other)
        with pytest.raises(NotImplementedError, match="fp16 only"):
            CLIPTextEncoder(other.state_dict(), other.config)
    with pytest.raises(ValueError, match="missing parameters"):
        CLIPTextEncoder({k: v for k, v in sd.items() if "layers.1.mlp.fc2" not in k}, net.config)
    with pytest.raises(ValueError, match="expected"):
        CLIPTextEncoder(dict(sd, **{"final_layer_norm.bias": sd["final_layer_norm.bias"][:64]}), net.config)
    assert CLIPTextEncoder.refusal(types.SimpleNamespace()) == "has no config"


def test_call_refusals_come_before_any_kernel():
    from fresco_amd import CLIPTextEncoder
    net = _half_model()
    enc = CLIPTextEncoder(net.state_dict(), net.config)      # (the constructor does not ask where the parameters live)
    ids = M.input_ids(CASE_B)
    for kwargs, cause in ((dict(attention_mask=torch.ones_like(ids)), "attention_mask"),
                          (dict(position_ids=torch.arange(ids.shape[1])[None]), "position_ids"),
                          (dict(output_attentions=True), "output_attentions")):
        with pytest.raises(NotImplementedError, match=cause + ".*no fallback"):
            enc(ids, **kwargs)
    for bad in (ids.int(), ids[0], ids.float(), ids[:, :0], None, ids.tolist()):
        with pytest.raises(NotImplementedError, match=r"int64 \(B, L\)"):
            enc(bad)
    with pytest.raises(NotImplementedError, match="78 tokens, at most 77"):
        enc(torch.zeros(1, 78, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="GPU tensors only"):
        enc(ids)
    long_cfg = M.make_config(CASE_B)
    long_cfg.max_position_embeddings = 200
    sd = dict(net.state_dict())
    sd["embeddings.position_embedding.weight"] = torch.zeros(200, 128, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="129 tokens, at most 128"):
        CLIPTextEncoder(sd, long_cfg)(torch.zeros(1, 129, dtype=torch.int64))


def test_both_parameter_layouts_and_a_prefix():
    from fresco_amd import CLIPTextEncoder
    net = _half_model()
    flat = net.state_dict()
    a = CLIPTextEncoder(flat, net.config)
    nested = CLIPTextEncoder({"text_model." + k: v for k, v in flat.items()}, net.config)
    both = CLIPTextEncoder({"cond.text_model." + k: v for k, v in flat.items()}, net.config, prefix="cond")
    as_dict = CLIPTextEncoder({"te." + k: v for k, v in flat.items()}, vars(net.config), prefix="te.")
    for enc in (nested, both, as_dict):
        assert sorted(enc._sd) == sorted(a._sd) == sorted(flat)
        assert all(enc._sd[k] is flat[k] for k in flat)               # read where they live: no copy at intake
    assert (a.width, a.inner, a.layers, a.heads, a.vocab, a.max_positions) == (128, 512, 2, 2, 60, 77)
    with pytest.raises(ValueError, match="missing parameters"):
        CLIPTextEncoder({"other." + k: v for k, v in flat.items()}, net.config)


def test_packed_copies_follow_the_parameters_version():
    from fresco_amd import CLIPTextEncoder
    net = _half_model()
    enc = CLIPTextEncoder(net.state_dict(keep_vars=True), net.config)
    name = "encoder.layers.0.self_attn.q_proj.weight"
    first = enc._f32(name)
    assert first.dtype == torch.float32 and enc._f32(name) is first
    w = net.encoder.layers[0].self_attn.q_proj.weight
    with torch.no_grad():
        w.mul_(2.0)
    second = enc._f32(name)
    assert second is not first and torch.equal(second, w.detach().float())
    assert enc._in_place("encoder.layers.0.mlp.fc1.weight").data_ptr() == net.encoder.layers[0].mlp.fc1.weight.data_ptr()


def test_patch_and_unpatch_on_a_stand_in_pipe(monkeypatch):
    import fresco_amd
    from fresco_amd import CLIPTextEncoder, text_encoder
    net = _half_model()
    pipe = types.SimpleNamespace(text_encoder=net)
    with pytest.raises(NotImplementedError, match="pipe.text_encoder has parameters on cpu"):
        fresco_amd.patch_text_encoder(pipe)
    assert "forward" not in vars(net)                                    # refused before anything was patched
    monkeypatch.setattr(CLIPTextEncoder, "refusal", staticmethod(lambda m: None))   # (as if the module were on the GPU)
    assert fresco_amd.patch_text_encoder(pipe) == 1
    native = vars(net)["forward"]
    assert isinstance(native, CLIPTextEncoder) and vars(net)[text_encoder._ATTR] is native
    assert pipe.text_encoder is net and net.dtype == torch.float16 and net.config.hidden_size == 128
    assert str(net.device) == "cpu"
    with pytest.raises(NotImplementedError, match="attention_mask"):     # the module's __call__ reaches the native forward
        net(M.input_ids(CASE_B), attention_mask=torch.ones(2, 20))
    assert fresco_amd.patch_text_encoder(pipe) == 1 and vars(net)["forward"] is not native     # patching again replaces it
    assert fresco_amd.unpatch_text_encoder(pipe) == 1
    assert "forward" not in vars(net) and text_encoder._ATTR not in vars(net)
    assert fresco_amd.unpatch_text_encoder(pipe) == 0
    with torch.no_grad():
        out = net.float()(M.input_ids(CASE_B))                           # the module's own forward again
    assert out.last_hidden_state.shape == (2, 20, 128)
    with pytest.raises(TypeError, match="must be a module"):
        fresco_amd.patch_text_encoder(types.SimpleNamespace(text_encoder=None))


# ---------------------------------------------------------------------------------------------------------------------
# the restated model is the real module; the golden file is the maker's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_restated_model_is_transformers_clip_text_model(case):
    transformers = pytest.importorskip("transformers")
    c = M.make_config(case)
    cfg = transformers.CLIPTextConfig(vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                                      num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                                      max_position_embeddings=c.max_position_embeddings, hidden_act=c.hidden_act,
                                      layer_norm_eps=c.layer_norm_eps, eos_token_id=c.eos_token_id, bos_token_id=c.bos_token_id,
                                      pad_token_id=c.pad_token_id)
    real = transformers.CLIPTextModel(cfg).double().eval()
    net = M.build(case, torch.float64)
    names = list(real.state_dict())
    nested = names[0].startswith("text_model.")                       # transformers 4.x
    real.load_state_dict({("text_model." + k if nested else k): v for k, v in net.state_dict().items()}, strict=True)
    ids = M.input_ids(case)
    with torch.no_grad():
        theirs, ours = real(ids, output_hidden_states=True), net(ids, output_hidden_states=True)
    assert float((theirs.last_hidden_state - ours.last_hidden_state).abs().max()) <= 1e-9
    assert float((theirs.pooler_output - ours.pooler_output).abs().max()) <= 1e-9
    assert len(theirs.hidden_states) == len(ours.hidden_states) == case[1] + 1
    for a, b in zip(theirs.hidden_states, ours.hidden_states):
        assert float((a - b).abs().max()) <= 1e-9
    # the pooled rows are the FIRST EOS of every sequence under both rules
    for b, e in enumerate(M.eos_positions(case)):
        assert torch.equal(ours.pooler_output[b], ours.last_hidden_state[b, e])
    # what the native class reads from the real module: its config's attributes and its parameter names
    from fresco_amd import CLIPTextEncoder
    from fresco_amd.text_encoder import _CONFIG
    assert all(hasattr(real.config, n) for n in _CONFIG)
    enc = CLIPTextEncoder(real.half().state_dict(keep_vars=True), real.config)
    assert sorted(enc._sd) == sorted(net.state_dict()) and enc.eos_token_id == case[8]
    assert "is torch.float64" not in (CLIPTextEncoder.refusal(real) or "") and "GPU modules only" in CLIPTextEncoder.refusal(real)


def test_golden_file_is_current():
    gold = M.load_golden(GOLDEN)
    assert sorted(gold) == sorted(M.case_key(c) + "_" + s for c in M.CASES for s in M.TENSORS + ("noise", "peak"))
    assert os.path.getsize(os.path.join(GOLDEN, M.GOLDEN_FILE)) < (1 << 20)
    for case in M.CASES:
        key = M.case_key(case)
        noise = gold[key + "_noise"]
        assert noise.shape == (len(M.TENSORS),) and bool((noise > 0).all()) and bool((noise < 5e-3).all())
        B, L, C, inner = case[6], case[7], case[2], case[4]
        rows = len(M.KEPT_TOKENS) if case[0] == "a" else L
        assert gold[key + "_attn"].shape == (B, rows, C) and gold[key + "_fc1"].shape == (B, rows, inner)
        assert gold[key + "_hidden_m2"].shape == gold[key + "_last"].shape == (B, rows, C) and gold[key + "_pooled"].shape == (B, C)
    for case in M.CASES:        # both cases are derived again ((a): 24 forward layers on the CPU, some ten seconds)
        key = M.case_key(case)
        rec, noise, peak, act = M.record(case)
        assert act < M.ACT_LIMIT
        for i, n in enumerate(M.TENSORS):
            np.testing.assert_allclose(gold["%s_%s" % (key, n)], M.thin(case, n, rec[n]), rtol=0, atol=1e-6 * peak[n])
            # the noise is a maximum over an fp32 run whose sums depend on the CPU's order of additions: another CPU flips a
            # few fp16 roundings and moves the maximum by some per cent; the tests use it under a margin of 4
            np.testing.assert_allclose(gold[key + "_noise"][i], noise[n], rtol=0.25)
            np.testing.assert_allclose(gold[key + "_peak"][i], peak[n], rtol=1e-9)
