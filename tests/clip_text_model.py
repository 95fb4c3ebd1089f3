"""The restated CLIP text model shared by tests/golden/make_text_encoder_golden.py, tests/test_text_encoder_cpu.py and
tests/test_gpu_text_encoder.py.

A torch restatement of transformers' `CLIPTextModel` as SD-1.5 configures it -- token + position embedding, pre-LayerNorm
layers of causal self-attention (q / k / v / out projections with biases) and a quick-GELU MLP, a final LayerNorm, the pooled
EOS row -- under transformers 5.x's flat parameter names:

  embeddings.{token_embedding, position_embedding}, encoder.layers.N.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2,
  mlp.{fc1, fc2}}, final_layer_norm

test_text_encoder_cpu.py checks it against the real `transformers.CLIPTextModel` in float64 where transformers imports, so
the records below are the real module's to 1e-9.

  * weights: closed-form stand-ins seeded by (tag, parameter name), drawn in float64 and rounded to fp16 once.  They are NOT
    transformers' 0.02 initialisation, which leaves the embeddings at 0.13 where nothing can go wrong: the token table is
    N(0, 1), the position table 0.5 N(0, 1), the projections sqrt(1 / fan_in) N(0, 1) (out_proj and fc2 half of that), so the
    residual stream is O(1 - 10) as a trained CLIP's is.  The golden maker asserts every activation below 65504 / 8;
  * `forward(..., q)`: q is applied to every layer's output -- the identity for the float64 record, a round trip through fp16
    for the reference arithmetic's noise (the model run in fp32 with every layer's output rounded to fp16);
  * in fp16 on the GPU the attention is `scaled_dot_product_attention(is_causal=True)`: PyTorch's own kernels, the baseline the
    GPU tests print beside ours and the bench tool times where transformers is absent.
"""
import math
import os
import types
import zlib
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

# (key, layers, width, heads, intermediate, vocabulary, sequences, tokens, eos_token_id): (a) SD-1.5's shape with the vocabulary
# cut, the legacy pooling rule (eos_token_id == 2: argmax of the ids); (b) small, the first-EOS rule
CASES = [("a", 12, 768, 12, 3072, 1000, 3, 77, 2),
         ("b", 2, 128, 2, 512, 60, 2, 20, 59)]
GOLDEN_FILE = "text_encoder_golden.npz"
TENSORS = ("attn", "fc1", "hidden_m2", "last", "pooled")   # layer 0's attention output (before out_proj) and quick_gelu(fc1),
#                                                            hidden_states[-2], the last hidden state, pooler_output
KEPT_TOKENS = (0, 1, 31, 32, 33, 63, 64, 65, 75, 76)       # case (a): whole-width rows at these tokens
MAX_POSITIONS = 77
LN_EPS = 1e-5
ACT_LIMIT = 65504.0 / 8

_ident = lambda t: t  # noqa: E731
Output = namedtuple("Output", ["last_hidden_state", "pooler_output", "hidden_states"])


def round16(t):
    return t.to(torch.float16).to(t.dtype)


def case_key(case):
    return "text_%s_l%dw%dh%di%dv%d_%dx%d" % tuple(case[:8])


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN_FILE)))


def make_config(case):
    _, layers, C, heads, inner, vocab, _, _, eos = case
    return types.SimpleNamespace(vocab_size=vocab, hidden_size=C, intermediate_size=inner, num_hidden_layers=layers,
                                 num_attention_heads=heads, max_position_embeddings=MAX_POSITIONS, hidden_act="quick_gelu",
                                 layer_norm_eps=LN_EPS, eos_token_id=eos, bos_token_id=vocab - 2, pad_token_id=1,
                                 attention_dropout=0.0)


def input_ids(case):
    """(B, L) int64: BOS (vocab - 2), words below it, ONE EOS (vocab - 1, the largest id) at a different position per sequence --
    the last token of the last sequence -- and padding after it: the EOS again in sequence 0 (what SD's tokenizer pads with: the
    pooling rules then take the FIRST), 0 in the others"""
    _, _, _, _, _, vocab, B, L, _ = case
    rs = np.random.RandomState(zlib.crc32(case_key(case).encode()) & 0x7FFFFFFF)
    ids = rs.randint(0, vocab - 2, size=(B, L))
    ids[:, 0] = vocab - 2
    ids[0, 1], ids[-1, 1] = 0, vocab - 3
    for b in range(B):
        e = L - 1 if b == B - 1 else max(2, ((b + 1) * L) // (B + 1) - 3)
        ids[b, e] = vocab - 1
        ids[b, e + 1:] = vocab - 1 if b == 0 else 0
    return torch.from_numpy(ids.astype(np.int64))


def eos_positions(case):
    ids = input_ids(case)
    return [int((ids[b] == case[5] - 1).nonzero()[0]) for b in range(ids.shape[0])]


def thin(case, name, t):
    """a (B, L, width) or (B, width) tensor as the golden file keeps it: float32; case (a)'s token rows at KEPT_TOKENS only"""
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if case[0] == "a" and t.ndim == 3:
        t = t[:, list(KEPT_TOKENS)]
    return np.ascontiguousarray(t.astype(np.float32))


class Attention(nn.Module):
    def __init__(self, C, heads):
        super().__init__()
        self.heads = heads
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(C, C) for _ in range(4))

    def forward(self, y, q=_ident, taps=None):
        B, L, C = y.shape
        D = C // self.heads
        split = lambda t: t.view(B, L, self.heads, D).transpose(1, 2)  # noqa: E731
        qq, kk, vv = split(q(self.q_proj(y))), split(q(self.k_proj(y))), split(q(self.v_proj(y)))
        if y.dtype == torch.float16:
            o = F.scaled_dot_product_attention(qq, kk, vv, is_causal=True, scale=D ** -0.5)
        else:
            s = qq @ kk.transpose(-1, -2) * D ** -0.5
            future = torch.ones(L, L, dtype=torch.bool, device=y.device).triu(1)
            o = torch.softmax(s.masked_fill(future, float("-inf")), dim=-1) @ vv
        o = q(o.transpose(1, 2).reshape(B, L, C))
        if taps is not None and "attn" not in taps:
            taps["attn"] = o
        return q(self.out_proj(o))


class MLP(nn.Module):
    def __init__(self, C, inner):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, inner), nn.Linear(inner, C)

    def forward(self, y, q=_ident, taps=None):
        g = q(self.fc1(y))
        g = q(g * torch.sigmoid(1.702 * g))
        if taps is not None and "fc1" not in taps:
            taps["fc1"] = g
        return q(self.fc2(g))


class Layer(nn.Module):
    def __init__(self, C, heads, inner):
        super().__init__()
        self.self_attn = Attention(C, heads)
        self.layer_norm1 = nn.LayerNorm(C, eps=LN_EPS)
        self.mlp = MLP(C, inner)
        self.layer_norm2 = nn.LayerNorm(C, eps=LN_EPS)

    def forward(self, h, q=_ident, taps=None):
        h = q(h + self.self_attn(q(self.layer_norm1(h)), q, taps))
        return q(h + self.mlp(q(self.layer_norm2(h)), q, taps))


class Embeddings(nn.Module):
    def __init__(self, vocab, C):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, C)
        self.position_embedding = nn.Embedding(MAX_POSITIONS, C)


class Encoder(nn.Module):
    def __init__(self, layers, C, heads, inner):
        super().__init__()
        self.layers = nn.ModuleList([Layer(C, heads, inner) for _ in range(layers)])


class TextModel(nn.Module):
    """CLIPTextModel, restated; `config`, `dtype` and `device` as the pipeline reads them"""

    def __init__(self, config):
        super().__init__()
        self.config = config
        C = config.hidden_size
        self.embeddings = Embeddings(config.vocab_size, C)
        self.encoder = Encoder(config.num_hidden_layers, C, config.num_attention_heads, config.intermediate_size)
        self.final_layer_norm = nn.LayerNorm(C, eps=config.layer_norm_eps)

    @property
    def dtype(self):
        return self.final_layer_norm.weight.dtype

    @property
    def device(self):
        return self.final_layer_norm.weight.device

    def forward(self, input_ids, attention_mask=None, position_ids=None, output_attentions=None, output_hidden_states=None,
                return_dict=None, q=_ident, taps=None):
        assert attention_mask is None and position_ids is None and not output_attentions
        B, L = input_ids.shape
        h = q(self.embeddings.token_embedding(input_ids) + self.embeddings.position_embedding.weight[:L])
        streams = [h]
        for layer in self.encoder.layers:
            h = layer(h, q, taps)
            streams.append(h)
        last = q(self.final_layer_norm(h))
        eos = self.config.eos_token_id
        at = input_ids.argmax(-1) if eos == 2 else (input_ids == eos).int().argmax(-1)
        pooled = last[torch.arange(B, device=last.device), at]
        hidden = tuple(streams) if output_hidden_states else None
        if return_dict is not None and not return_dict:
            return (last, pooled) + ((hidden,) if hidden is not None else ())
        return Output(last, pooled, hidden)


# ---------------------------------------------------------------------------------------------------------------------
# stand-in weights
# ---------------------------------------------------------------------------------------------------------------------
def standin_value(seed_name, name, shape):
    rs = np.random.RandomState(zlib.crc32(seed_name.encode()) & 0x7FFFFFFF)
    if name.endswith("token_embedding.weight"):
        return rs.standard_normal(shape)
    if name.endswith("position_embedding.weight"):
        return 0.5 * rs.standard_normal(shape)
    leaf = name.rsplit(".", 2)[-2]
    if "norm" in leaf and name.endswith(".weight"):
        return rs.uniform(0.75, 1.25, shape)
    if name.endswith(".bias"):
        return 0.1 * rs.standard_normal(shape)
    gain = 0.5 if leaf in ("out_proj", "fc2") else 1.0
    return gain * math.sqrt(1.0 / shape[1]) * rs.standard_normal(shape)


def standin_state_dict(module, tag, dtype=torch.float64):
    """every value is rounded to fp16 once, here: the float64, fp32 and fp16 runs carry the same VALUES"""
    return OrderedDict((name, torch.from_numpy(np.asarray(standin_value("%s.%s" % (tag, name), name, tuple(v.shape)), np.float64)
                                               .astype(np.float16).astype(np.float64)).to(dtype))
                       for name, v in module.state_dict().items())


def build(case, dtype=torch.float32):
    """the restated model of a case with its stand-in weights, in eval mode"""
    net = TextModel(make_config(case))
    net.load_state_dict(standin_state_dict(net, "clip_" + case[0]))
    return net.to(dtype).eval()


def record(case):
    """({name: float64 tensor} for TENSORS, {name: noise}, {name: peak}, the largest activation): the float64 run of the case,
    and the reference arithmetic's noise against it = max|difference| / max|float64| of the fp32 run with every layer's output
    rounded to fp16"""
    ids = input_ids(case)
    net64, net32 = build(case, torch.float64), build(case, torch.float32)
    seen = [0.0]

    def see(m, i, o):
        if isinstance(o, torch.Tensor):
            seen[0] = max(seen[0], float(o.detach().abs().max()))
    hooks = [m.register_forward_hook(see) for net in (net64, net32) for m in net.modules() if not list(m.children())]
    t64, t16 = {}, {}
    with torch.no_grad():
        o64 = net64(ids, output_hidden_states=True, taps=t64)
        o16 = net32(ids, output_hidden_states=True, q=round16, taps=t16)
    for h in hooks:
        h.remove()
    for t, o in ((t64, o64), (t16, o16)):
        t.update(hidden_m2=o.hidden_states[-2], last=o.last_hidden_state, pooled=o.pooler_output)
        seen[0] = max([seen[0]] + [float(s.abs().max()) for s in o.hidden_states] + [float(t["attn"].abs().max())])
    peak = {n: float(t64[n].abs().max()) for n in TENSORS}
    noise = {n: float((t16[n].double() - t64[n]).abs().max() / peak[n]) for n in TENSORS}
    return {n: t64[n] for n in TENSORS}, noise, peak, seen[0]
