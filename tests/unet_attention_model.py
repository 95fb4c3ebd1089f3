"""Stand-ins and restatements shared by tests/golden/make_unet_attention_golden.py, tests/test_unet_attention_cpu.py and
tests/test_gpu_unet_attention.py.

`Attention` restates what fresco_amd.unet_attention reads from diffusers 0.19.3's `Attention` module
(models/attention_processor.py): the attributes `heads`, `to_q`, `to_k`, `to_v` (no bias), `to_out` = [Linear with a bias,
Dropout], `spatial_norm`, `group_norm`, `norm_cross`, `added_kv_proj_dim`, `residual_connection`, `rescale_output_factor`,
`processor`, `set_processor`, and a `forward` that hands the module and its arguments to the processor.  diffusers is NOT
installed where these tests run: the names and the call come from its published source and are UNVERIFIED against the real
module.

`RefProcessor` restates `AttnProcessor2_0` for a 3-D input without a mask -- three Linears, softmax(q k^T / sqrt(d)) v over
`heads` heads, `to_out[0]` with its bias, `to_out[1]` -- in the dtype of what it is given (float64 for the record, fp32 for
the noise run), with `q` applied to every Linear's and the attention's output: the identity for the record, a round trip
through fp16 for the reference arithmetic's own noise.

Weights are closed-form stand-ins in the style of unet_transformer_model.standin_value, seeded by (tag, parameter name), drawn
in float64 and rounded to fp16 once.  to_q and to_k carry a gain of QK_GAIN each, so the scaled logits are about
QK_GAIN^2 N(0, 1): the attention is NOT a plain average (the golden maker asserts a logit span of at least 8 natural-log
units within some row and a largest probability above 0.5), otherwise a wrong running maximum could not show.  The logit
range of trained weights at head dim 160 is not known here.
"""
import os
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from unet_transformer_model import standin_value
from vae_model import round16  # noqa: F401  (the fp16 round trip)

# (C, heads, n, tokens, text tokens, text width)
CASES = [(320, 8, 2, 96, 7, 64),       # head dim 40: fresco_linear + fresco_attn_fwd
         (640, 8, 1, 128, 77, 96),     # head dim 80
         (1280, 8, 2, 16, 5, 64),      # head dim 160: vae_conv + unet_attention; half a query block, a ragged key block
         (1280, 8, 1, 64, 77, 96)]     # two query blocks; the text's 77 keys: three waves' key blocks, the last ragged
MODES = ("self", "cross")
GOLDEN_FILE = "unet_attention_golden.npz"
QK_GAIN = 1.5
MIN_LOGIT_SPAN, MIN_TOP_PROB = 8.0, 0.5

_ident = lambda t: t  # noqa: E731


def case_key(case):
    return "attention_%dh%d_%dx%d_t%dx%d" % tuple(case)


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN_FILE)))


def inputs(case):
    """the case's hidden states (n, tokens, C) and text (n, text tokens, width): N(0, 1) in float64 (what a LayerNorm hands an
    attention module), rounded to fp16"""
    C, _, n, L, T, TW = case
    rs = np.random.RandomState(zlib.crc32(case_key(case).encode()) & 0x7FFFFFFF)
    x = rs.standard_normal((n, L, C))
    t = rs.standard_normal((n, T, TW))
    return torch.from_numpy(x).to(torch.float16), torch.from_numpy(t).to(torch.float16)


class RefProcessor:
    """AttnProcessor2_0, restated (3-D input, no mask); `stats` receives the scaled logits' largest span within a row and the
    largest probability"""

    def __init__(self, q=_ident, stats=None, sdpa=False):
        self.q, self.stats, self.sdpa = q, stats, sdpa

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        assert attention_mask is None and hidden_states.dim() == 3
        q_ = self.q
        x = hidden_states
        e = x if encoder_hidden_states is None else encoder_hidden_states
        n, L, _ = x.shape
        query, key, value = q_(attn.to_q(x)), q_(attn.to_k(e)), q_(attn.to_v(e))
        d = query.shape[-1] // attn.heads
        split = lambda t: t.view(n, -1, attn.heads, d).transpose(1, 2)  # noqa: E731
        query, key, value = split(query), split(key), split(value)
        if self.sdpa:
            o = torch.nn.functional.scaled_dot_product_attention(query, key, value)
        else:
            logits = query @ key.transpose(-1, -2) * d ** -0.5
            p = torch.softmax(logits, dim=-1)
            if self.stats is not None:
                self.stats["span"] = float((logits.max(-1).values - logits.min(-1).values).max())
                self.stats["top"] = float(p.max())
            o = p @ value
        o = q_(o.transpose(1, 2).reshape(n, L, attn.heads * d))
        o = attn.to_out[1](q_(attn.to_out[0](o)))
        if attn.residual_connection:
            o = o + hidden_states
        if attn.rescale_output_factor != 1.0:
            o = o / attn.rescale_output_factor
        return o


class Attention(nn.Module):
    """what the processors read of diffusers' Attention, and its forward -> processor call"""

    def __init__(self, dim, heads, cross_dim=None, processor=None):
        super().__init__()
        self.heads = heads
        self.spatial_norm = None
        self.group_norm = None
        self.norm_cross = None
        self.added_kv_proj_dim = None
        self.residual_connection = False
        self.rescale_output_factor = 1.0
        self.to_q = nn.Linear(dim, dim, bias=False)
        self.to_k = nn.Linear(cross_dim or dim, dim, bias=False)
        self.to_v = nn.Linear(cross_dim or dim, dim, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])
        self.processor = processor if processor is not None else RefProcessor()

    def set_processor(self, processor):
        self.processor = processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **cross_attention_kwargs):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask,
                              **cross_attention_kwargs)


def standin_state_dict(module, tag, dtype=torch.float64):
    """unet_transformer_model's closed forms, to_q and to_k times QK_GAIN; every value is rounded to fp16 once, here"""
    sd = OrderedDict()
    for name, v in module.state_dict().items():
        val = np.asarray(standin_value("%s.%s" % (tag, name), name, tuple(v.shape)), np.float64)
        if name in ("to_q.weight", "to_k.weight"):
            val = val * QK_GAIN
        sd[name] = torch.from_numpy(val.astype(np.float16).astype(np.float64)).to(dtype)
    return sd


def build(C, heads, cross_dim=None, dtype=torch.float32, processor=None):
    """the stand-in module with its stand-in weights, in eval mode; cross_dim None: a self-attention module"""
    net = Attention(C, heads, cross_dim, processor)
    net.load_state_dict(standin_state_dict(net, "attn%dh%dx%s" % (C, heads, cross_dim)))
    return net.to(dtype).eval()


def build_case(case, mode, dtype=torch.float32, processor=None):
    C, heads, _, _, _, TW = case
    return build(C, heads, TW if mode == "cross" else None, dtype, processor)


def record(case, mode):
    """(float64 output (n, tokens, C), noise, peak, logit span, largest probability) of the case's self- or cross-attention:
    the float64 run, and the REFERENCE ARITHMETIC'S OWN NOISE against it = max|difference| / max|float64| of the same module in
    fp32 with every Linear's and the attention's output rounded to fp16"""
    x, text = inputs(case)
    stats = {}
    net64 = build_case(case, mode, torch.float64, RefProcessor(stats=stats))
    net32 = build_case(case, mode, torch.float32, RefProcessor(q=round16))
    with torch.no_grad():
        o64 = net64(x.double(), text.double() if mode == "cross" else None)
        o16 = net32(x.float(), text.float() if mode == "cross" else None)
    peak = float(o64.abs().max())
    noise = float((o16.double() - o64).abs().max() / peak)
    return o64.contiguous(), noise, peak, stats["span"], stats["top"]


def checksums(out64):
    """what the golden file keeps of a record: its sum, its sum of magnitudes, and a thin sample (every 997th value)"""
    flat = out64.reshape(-1).numpy()
    return np.array([flat.sum(), np.abs(flat).sum()]), flat[::997].copy()


# ---------------------------------------------------------------------------------------------------------------------
# a stand-in tree for patch_unet_attention: names as the UNet has them
# ---------------------------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self, dim, heads, cross_dim):
        super().__init__()
        self.attn1 = Attention(dim, heads)
        self.attn2 = Attention(dim, heads, cross_dim)


class _Stage(nn.Module):
    def __init__(self, dim, heads, cross_dim):
        super().__init__()
        self.transformer_blocks = nn.ModuleList([_Block(dim, heads, cross_dim)])


class Tree(nn.Module):
    """down_blocks.0 / mid_block / up_blocks.2, one transformer block each: 6 attention modules, and a Linear that is none"""

    def __init__(self, dim=320, heads=8, cross_dim=64):
        super().__init__()
        self.down_blocks = nn.ModuleList([_Stage(dim, heads, cross_dim)])
        self.mid_block = _Stage(dim, heads, cross_dim)
        self.up_blocks = nn.ModuleList([nn.Identity(), nn.Identity(), _Stage(dim, heads, cross_dim)])
        self.proj = nn.Linear(dim, dim)


def build_tree(dtype=torch.float16, dim=320, heads=8, cross_dim=64):
    return Tree(dim, heads, cross_dim).to(dtype).eval()


def attention_modules(tree):
    return [(n, m) for n, m in tree.named_modules() if isinstance(m, Attention)]
