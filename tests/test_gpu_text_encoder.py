"""The CLIP text encoder on the GPU: the kernels of csrc/text.hip against exact references on the same operands, the native
module against the float64 records of the restated one (tests/golden/text_encoder_golden.npz; stand-in weights,
tests/clip_text_model.py, which test_text_encoder_cpu.py ties to transformers' CLIPTextModel), and patch_text_encoder on a
stand-in pipe.

Bars (e = 2^-24, one fp32 rounding):
  * clip_embed: bit-equal to (tok[ids] + pos[:L]) computed in fp16 on the device; an id of -1 or of `vocab` gives a NaN row
    and leaves every other row as it was;
  * clip_attention: the project's attention bar, |got - ref| <= 1e-3 + 2e-3 |ref| (tests/test_gpu_attention.py), against a
    float64 causal softmax on the same fp16 operands; q | k | v are column slices of one buffer whose other rows and columns
    are NaN, the output lies inside a band that must stay NaN; CAUSALITY IS EXACT: overwriting the keys and values after
    token t leaves rows <= t with the same bits; a second run gives the same bits;
  * clip_fc1: with g the exact pre-activation and Bg = K e (sum |x| |W| + |b|) (vae_conv's accumulation bar),
    1.10 Bg + 16 e max(|g|, 1) + 2^-11 |ref| + 1e-6: 1.10 bounds |quick_gelu'| (its maximum is 1.0998 at g = 1.41), 16 e
    max(|g|, 1) covers the fp32 evaluation of g / (1 + exp(-1.702 g)), 2^-11 |ref| the one rounding to fp16;
  * the module: |got - record| <= 4 x the recorded noise of the reference arithmetic for that tensor x its largest magnitude
    (DESIGN.md sections 16, 17 and 19's margin).
Every comparison prints its ratio to the bar; the module's beside the ratio of PyTorch's own fp16 kernels on the restated
model.
"""
import os
import types

import numpy as np
import pytest
import torch

import clip_text_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = 2.0 ** -24
H11 = 2.0 ** -11
D = 64
GUARD_ROWS, GUARD_COLS = 3, 8          # (8 fp16 columns: the tensors stay 16-byte aligned)


def _bits(t):
    return t.view(torch.int16)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# clip_embed
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(1, 1), (2, 77)])
@pytest.mark.parametrize("C", [64, 768])
def test_embed_is_the_fp16_sum_and_guards_its_ids(C, B, L):
    from fresco_amd import ops
    vocab = 50
    g = _gen(C + L)
    tok = (torch.randn(vocab, C, generator=g) * 2.0).half().to(DEV)
    pos = torch.randn(77, C, generator=g).half().to(DEV)
    tok[3, :8] = 60000.0
    pos[0, :8] = 60000.0                           # a sum beyond fp16: +inf, as torch gives
    keep_tok, keep_pos = tok.clone(), pos.clone()
    for first, last in ((0, vocab - 1), (vocab - 1, 0), (3, 3)):
        ids = torch.randint(0, vocab, (B, L), generator=g)
        ids.view(-1)[-1] = last
        ids.view(-1)[0] = first
        ids = ids.to(DEV)
        keep_ids = ids.clone()
        out = ops.clip_embed(ids, tok, pos)
        ref = tok[ids] + pos[:L]
        assert out.shape == (B, L, C) and out.dtype == torch.float16 and out.is_contiguous()
        assert torch.equal(_bits(out), _bits(ref))
        assert torch.equal(_bits(ops.clip_embed(ids, tok, pos)), _bits(out))
        for bad in (-1, vocab, 1 << 40, -(1 << 40)):
            at = (B * L) // 2
            wrong = ids.clone()
            wrong.view(-1)[at] = bad
            got = ops.clip_embed(wrong, tok, pos).view(B * L, C)
            assert bool(torch.isnan(got[at]).all())                                     # the guarded row shows downstream
            rest = [r for r in range(B * L) if r != at]
            assert torch.equal(_bits(got[rest]), _bits(out.view(B * L, C)[rest]))       # every other row is unchanged
        assert torch.equal(ids, keep_ids)
    assert torch.equal(_bits(tok), _bits(keep_tok)) and torch.equal(_bits(pos), _bits(keep_pos))


# ---------------------------------------------------------------------------------------------------------------------
# clip_attention
# ---------------------------------------------------------------------------------------------------------------------
def _embed_qkv(q, k, v):
    """one ((B L) + 2 GUARD_ROWS, 3 C + 2 GUARD_COLS) NaN buffer with q | k | v as its inner column blocks -> (buffer, views)"""
    B, L, C = q.shape
    buf = torch.full((B * L + 2 * GUARD_ROWS, 3 * C + 2 * GUARD_COLS), float("nan"), dtype=torch.float16, device=DEV)
    views = []
    for i, p in enumerate((q, k, v)):
        view = buf[GUARD_ROWS:GUARD_ROWS + B * L, GUARD_COLS + i * C:GUARD_COLS + (i + 1) * C].unflatten(0, (B, L))
        view.copy_(p)
        views.append(view)
    return buf, views


def _out_band(B, L, C):
    obuf = torch.full((B * L + 2 * GUARD_ROWS, C + 2 * GUARD_COLS), float("nan"), dtype=torch.float16, device=DEV)
    return obuf, obuf[GUARD_ROWS:GUARD_ROWS + B * L, GUARD_COLS:GUARD_COLS + C].unflatten(0, (B, L))


def _causal_reference(q, k, v, H):
    """float64 causal softmax attention on the GPU from the fp16 operands -> (out (B, L, C), scaled logits (B, H, L, L))"""
    B, L, C = q.shape
    split = lambda t: t.double().view(B, L, H, D).transpose(1, 2)  # noqa: E731
    logits = split(q) @ split(k).transpose(-1, -2) * D ** -0.5
    future = torch.ones(L, L, dtype=torch.bool, device=q.device).triu(1)
    p = torch.softmax(logits.masked_fill(future, float("-inf")), -1)
    return (p @ split(v)).transpose(1, 2).reshape(B, L, C), logits


def _run_attention(name, q, k, v, H):
    """clip_attention on q | k | v inside NaN bands into an output inside a NaN band; -> (the result, its worst error / bar)"""
    from fresco_amd import ops
    B, L, C = q.shape
    buf, (qv, kv, vv) = _embed_qkv(q, k, v)
    keep = buf.clone()
    obuf, out = _out_band(B, L, C)
    got = ops.clip_attention(qv, kv, vv, H, D ** -0.5, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (B, L, C)
    res = got.clone()
    again = ops.clip_attention(qv, kv, vv, H, D ** -0.5)          # a second run, into a dense tensor of its own: the same bits
    assert again.is_contiguous() and torch.equal(_bits(again), _bits(res)), name
    assert torch.equal(_bits(buf), _bits(keep)), name             # the inputs (NaN bands included) are unchanged
    out.fill_(float("nan"))
    assert bool(torch.isnan(obuf).all()), name                    # nothing was stored around the output
    assert bool(torch.isfinite(res).all()), name                  # no NaN of the bands reached a sum
    ref, logits = _causal_reference(q, k, v, H)
    ratio = float(((res.double() - ref).abs() / (1e-3 + 2e-3 * ref.abs())).max())
    print("clip_attention %s: worst error / bar %.3f" % (name, ratio))
    assert ratio <= 1.0, (name, ratio)
    return res, logits


def _operands(B, H, L, seed):
    g = _gen(seed)
    return tuple(torch.randn(B, L, H * D, generator=g).half().to(DEV) for _ in range(3))


@pytest.mark.parametrize("B,H,L", [(1, 1, 1), (2, 3, 31), (2, 3, 32), (1, 2, 33), (1, 2, 64), (1, 2, 65), (2, 12, 77), (1, 1, 128)])
def test_attention_matches_float64_causal_softmax(B, H, L):
    """one token; one ragged query block; exactly one; one token in the second; two whole blocks (a whole 64-key step); one
    token in the third; the model's own 77 on its 12 heads; every wave busy, every key block whole"""
    q, k, v = _operands(B, H, L, seed=1000 * L + H)
    _run_attention("(B %d, H %d, L %d)" % (B, H, L), q, k, v, H)


def test_attention_large_logits():
    q, k, v = _operands(2, 12, 77, seed=7)
    q = (q.float() * 7.0).half()
    _, logits = _causal_reference(q, k, v, 12)
    seen = logits.masked_fill(torch.ones(77, 77, dtype=torch.bool, device=DEV).triu(1), 0.0).abs().max()
    assert 25.0 < float(seen) < 40.0
    _run_attention("(B 2, H 12, L 77), |scale q.k| up to %.1f" % float(seen), q, k, v, 12)


def test_attention_causality_is_exact():
    """the keys after token t are overwritten so that their logits would be every earlier row's largest, the values after t
    with +-60000 (finite on purpose: 0 x NaN is NaN in an MFMA, and real future tokens are finite): rows <= t keep their bits"""
    from fresco_amd import ops
    B, H, L = 2, 12, 77
    q, k, v = _operands(B, H, L, seed=11)
    q = (q.float() + 0.75).half()           # a common direction: a key of +6 in every component has a logit of about +36
    base, logits = _run_attention("causality, the run before", q, k, v, H)
    row_max = logits.masked_fill(torch.ones(L, L, dtype=torch.bool, device=DEV).triu(1), float("-inf")).max(-1).values
    for t in (0, 31, 32, 76):
        k2, v2 = k.clone(), v.clone()
        k2[:, t + 1:] = 6.0
        sign = torch.ones(L, H * D, dtype=torch.float16, device=DEV)
        sign[::2, ::2] = -1.0
        sign[1::2, 1::2] = -1.0
        v2[:, t + 1:] = (60000.0 * sign)[t + 1:]
        if t + 1 < L:
            fut = (q.double().view(B, L, H, D).transpose(1, 2)[:, :, :t + 1] * 6.0).sum(-1) * D ** -0.5   # their logits
            assert bool((fut > row_max[:, :, :t + 1] + 4.0).all()), t                  # ... would be each row's largest
        buf, (qv, kv, vv) = _embed_qkv(q, k2, v2)
        got = ops.clip_attention(qv, kv, vv, H, D ** -0.5)
        assert torch.equal(_bits(got[:, :t + 1]), _bits(base[:, :t + 1])), t
        if t + 1 < L:
            assert not torch.equal(_bits(got[:, t + 1:]), _bits(base[:, t + 1:]))      # the later rows do see them
        ref = _causal_reference(q, k2, v2, H)[0]
        assert bool(torch.isfinite(got).all())
        assert bool(((got.double() - ref).abs() <= 1e-3 + 2e-3 * ref.abs())[:, :t + 1].all())


# ---------------------------------------------------------------------------------------------------------------------
# clip_fc1
# ---------------------------------------------------------------------------------------------------------------------
def _fc1_case(M_, K, N, seed):
    g = _gen(seed)
    x = torch.randn(M_, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    b = torch.rand(N, generator=g) * 16.0 - 8.0           # the pre-activations cover [-8, 8]
    b[:4] = torch.tensor([-8.0, 8.0, -7.5, 7.5])
    return x, w, b


def _fc1_ref_and_bar(x, w, b, K):
    xd, wd, bd = x.double(), w.double(), b.double()
    g = xd @ wd.t() + bd
    Bg = K * E * (xd.abs() @ wd.abs().t() + bd.abs())
    ref = g * torch.sigmoid(1.702 * g)
    bar = 1.10 * Bg + 16 * E * g.abs().clamp(min=1.0) + H11 * ref.abs() + 1e-6
    return ref, bar, g


@pytest.mark.parametrize("K,N", [(768, 3072), (96, 128)], ids=["768to3072", "96to128"])
@pytest.mark.parametrize("M_", [1, 77, 154, 257], ids=lambda m: "M%d" % m)
def test_fc1_matches_float64(M_, K, N):
    """one row; one sequence (a ragged tile); two sequences (a second, ragged row tile); 257: one row in the third tile.
    768 -> 3072 is the model's; 96 -> 128 has three K steps and one column tile"""
    from fresco_amd import ops
    x, w, b = _fc1_case(M_, K, N, seed=M_ + K + N)
    xg, wg, bg = x.to(DEV), w.to(DEV), b.to(DEV)
    keep = [t.clone() for t in (xg, wg, bg)]
    out = ops.clip_fc1(xg, wg, bg)
    assert out.shape == (M_, N) and out.dtype == torch.float16
    ref, bar, g = _fc1_ref_and_bar(xg, wg, bg, K)
    assert float(g.min()) < -7.0 and float(g.max()) > 7.0
    err = (out.double() - ref).abs()
    print("clip_fc1 M=%d K=%d N=%d: worst error / bound %.3f" % (M_, K, N, float((err / bar).max())))
    assert bool(torch.isfinite(out).all()) and bool((err <= bar).all())
    assert torch.equal(_bits(out), _bits(ops.clip_fc1(xg, wg, bg)))                    # a second run: the same bits
    assert all(torch.equal(a, b_) for a, b_ in zip((xg, wg, bg), keep))
    # ldo > N: the columns beyond N are left untouched; (n, L, K) rows flat
    buf = torch.full((M_, N + 8), 7.0, dtype=torch.float16, device=DEV)
    got = ops.clip_fc1(xg, wg, bg, out=buf[:, :N])
    assert got.data_ptr() == buf.data_ptr() and torch.equal(_bits(buf[:, :N]), _bits(out)) and bool((buf[:, N:] == 7.0).all())
    if M_ == 154:
        both = ops.clip_fc1(xg.view(2, 77, K), wg, bg)
        assert both.shape == (2, 77, N) and torch.equal(_bits(both.view(M_, N)), _bits(out))


# ---------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_key)
def test_module_matches_the_record(case, gold):
    from fresco_amd import CLIPTextEncoder, ops
    key = M.case_key(case)
    _, layers, C, heads, inner, vocab, B, L, eos = case
    mod = M.build(case, torch.float16).to(DEV)          # the restated model in fp16 on the GPU, with the stand-in weights
    native = CLIPTextEncoder.from_state_dict(mod.state_dict(), mod.config)
    ids = M.input_ids(case).to(DEV)
    taps, ttaps = {}, {}
    res = native(ids, output_hidden_states=True, taps=taps)
    with torch.no_grad():
        theirs = mod(ids, output_hidden_states=True, taps=ttaps)   # PyTorch's own fp16 kernels: printed for context only
    last, pooled, hidden = res.last_hidden_state, res.pooler_output, res.hidden_states
    assert res[0] is last and last.shape == (B, L, C) and last.dtype == torch.float16 and pooled.shape == (B, C)
    assert len(hidden) == layers + 1 and all(h.shape == (B, L, C) and h.dtype == torch.float16 for h in hidden)
    try:
        from transformers.modeling_outputs import BaseModelOutputWithPooling
        assert isinstance(res, BaseModelOutputWithPooling)
    except ImportError:
        assert isinstance(res, tuple) and res._fields == ("last_hidden_state", "pooler_output", "hidden_states")
    ours = dict(attn=taps["attn"], fc1=taps["fc1"], hidden_m2=hidden[-2], last=last, pooled=pooled)
    base = dict(attn=ttaps["attn"], fc1=ttaps["fc1"], hidden_m2=theirs.hidden_states[-2], last=theirs.last_hidden_state,
                pooled=theirs.pooler_output)
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    worst = []
    for i, t in enumerate(M.TENSORS):
        rec = gold["%s_%s" % (key, t)].astype(np.float64)
        a, b = M.thin(case, t, ours[t].double()).astype(np.float64), M.thin(case, t, base[t].double()).astype(np.float64)
        assert a.shape == rec.shape, (t, a.shape, rec.shape)
        bar = 4 * noise[i] * peak[i]
        ratio, tratio = float(np.abs(a - rec).max() / bar), float(np.abs(b - rec).max() / bar)
        print("%s %-9s |got - record| / (4 x reference noise %.2e x peak %.3g) = %.3f   (PyTorch fp16 model: %.3f)"
              % (key, t, noise[i], peak[i], ratio, tratio))
        assert np.isfinite(a).all()
        worst.append((ratio, t))
    assert max(worst)[0] <= 1.0, max(worst)
    # hidden_states[-1] is the stream BEFORE final_layer_norm, and [0] is final_layer_norm of it
    sd = mod.state_dict()
    again = ops.unet_layernorm(hidden[-1], sd["final_layer_norm.weight"].float(), sd["final_layer_norm.bias"].float(), M.LN_EPS)
    assert torch.equal(_bits(again), _bits(last))
    assert torch.equal(_bits(hidden[0]), _bits(sd["embeddings.token_embedding.weight"][ids]
                                               + sd["embeddings.position_embedding.weight"][:L]))
    for b_, e in enumerate(M.eos_positions(case)):                 # pooler_output rows are the (first) EOS rows
        assert torch.equal(_bits(pooled[b_]), _bits(last[b_, e]))
    # without hidden states, as a plain tuple, from a second call: the same bits
    plain = native(ids)
    assert plain.hidden_states is None and torch.equal(_bits(plain[0]), _bits(last))
    as_tuple = native(ids, return_dict=False)
    assert type(as_tuple) is tuple and len(as_tuple) == 2 and torch.equal(_bits(as_tuple[0]), _bits(last)) \
        and torch.equal(_bits(as_tuple[1]), _bits(pooled))
    with_hidden = native(ids, output_hidden_states=True, return_dict=False)
    assert type(with_hidden) is tuple and len(with_hidden) == 3 and len(with_hidden[2]) == layers + 1
    # one sequence alone: the same bits as inside the batch (no kernel mixes sequences)
    assert torch.equal(_bits(native(ids[1:2].contiguous())[0]), _bits(last[1:2]))


# what torch.profiler may record under the patch beside this library's kernels (namespace fresco): the pooling rule's boundary
# copy -- the ids' cast and comparison (elementwise), their argmax (a reduce kernel over B x L ints), arange and the row
# gather (index) -- and copies
ALLOWED = ("elementwise_kernel", "reduce_kernel", "index", "Memcpy", "Memset", "CatArrayBatchedCopy")
NOT_OURS = ("gemm", "Cijk", "oftmax", "ayer_norm", "LayerNorm", "attention", "attn", "fmha", "flash", "sigmoid", "gelu",
            "mbedding", "gemv")


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
    return sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})


def test_patched_pipe_runs_natively_and_follows_its_weights():
    from fresco_amd import CLIPTextEncoder, patch_text_encoder, unpatch_text_encoder
    case = M.CASES[1]
    mod = M.build(case, torch.float16).to(DEV)
    pipe = types.SimpleNamespace(text_encoder=mod)
    ids = M.input_ids(case).to(DEV)
    with torch.no_grad():
        own = mod(ids)[0].clone()                                   # the module's own forward: PyTorch's fp16 kernels
    before = _kernel_names(lambda: mod(ids))
    print("unpatched text model: %s" % before)
    foreign = [k for k in before if "fresco" not in k and any(s in k for s in NOT_OURS)]
    assert foreign, before       # the profiler sees PyTorch's GEMMs: the check below is not vacuous
    native = CLIPTextEncoder.from_module(mod)(ids)[0]
    assert patch_text_encoder(pipe) == 1
    try:
        assert pipe.text_encoder is mod and mod.dtype == torch.float16 and mod.config.hidden_size == case[2]
        assert str(mod.device) == DEV
        got = pipe.text_encoder(ids)[0]
        assert torch.equal(_bits(got), _bits(native))
        assert torch.equal(_bits(pipe.text_encoder(ids, attention_mask=None)[0]), _bits(native))   # as _encode_prompt calls it
        names = _kernel_names(lambda: pipe.text_encoder(ids))
        print("patched text model: %s" % names)
        for want in ("clip_embed_kernel", "clip_attn64_kernel", "clip_fc1_kernel", "unet_ln_kernel", "vae_conv_kernel"):
            assert any("fresco" in k and want in k for k in names), (want, names)
        for k in names:
            if "fresco" in k:
                continue
            assert any(a in k for a in ALLOWED) and not any(s in k for s in NOT_OURS), k
        # the weight-version rule: an in-place change of q_proj.weight is seen on the next call
        wq, b1 = mod.encoder.layers[0].self_attn.q_proj.weight, mod.encoder.layers[1].mlp.fc1.bias
        keep_wq, keep_b1 = wq.detach().clone(), b1.detach().clone()
        with torch.no_grad():
            wq.mul_(-1.5)
        changed = pipe.text_encoder(ids)[0]
        assert not torch.equal(_bits(changed), _bits(native))
        assert torch.equal(_bits(changed), _bits(CLIPTextEncoder.from_module(mod)(ids)[0]))
        with torch.no_grad():
            wq.copy_(keep_wq)
            b1.add_(1.0)                                            # an fp32 bias copy follows its parameter too
        assert not torch.equal(_bits(pipe.text_encoder(ids)[0]), _bits(native))
        with torch.no_grad():
            b1.copy_(keep_b1)
        assert torch.equal(_bits(pipe.text_encoder(ids)[0]), _bits(native))
    finally:
        assert unpatch_text_encoder(pipe) == 1
    assert "forward" not in vars(mod)
    with torch.no_grad():
        back = mod(ids)[0]
    # the module's own output again (PyTorch's kernels: compared under the module bar, not bit for bit)
    gold = M.load_golden(GOLDEN)
    i = M.TENSORS.index("last")
    bar = 4 * float(gold[M.case_key(case) + "_noise"][i]) * float(gold[M.case_key(case) + "_peak"][i])
    assert float((back.double() - own.double()).abs().max()) <= bar
    assert float((back.double() - native.double()).abs().max()) <= 2 * bar      # each within its bar of the float64 run
