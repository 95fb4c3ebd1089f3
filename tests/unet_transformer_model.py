"""Stand-ins and restatements shared by tests/golden/make_unet_transformer_golden.py, tests/test_unet_transformer_cpu.py and
tests/test_gpu_unet_transformer.py.

A torch restatement of diffusers 0.19.3's `Transformer2DModel` (models/transformer_2d.py) with its `BasicTransformerBlock`,
`FeedForward` and `GEGLU` (models/attention.py) as the SD-1.5 UNet and ControlNet configure them -- a continuous input,
GroupNorm(32, eps 1e-6), 1 x 1 convolutions as proj_in / proj_out, three plain LayerNorms, attn2 present, a GEGLU
feed-forward of 4 x the width, no dropout -- under diffusers' parameter names:

  norm, proj_in, transformer_blocks.N.{norm1, attn1, norm2, attn2, norm3, ff.net.0.proj, ff.net.2}, proj_out

and its forward: x + proj_out(blocks(proj_in(norm(x)) as tokens)), a block being h += attn1(norm1(h)); h += attn2(norm2(h),
text); h += ff(norm3(h)), ff = net.2(value * gelu(gate)) with (value, gate) = net.0.proj(.).chunk(2).

diffusers is NOT installed where these tests run: the names, the attributes (`use_linear_projection`, `only_cross_attention`,
`use_ada_layer_norm`, `_chunk_size`) and the forwards come from its published source and are UNVERIFIED against the real
modules.

  * the attention modules are STAND-INS (`Attention`: to_q / to_k / to_v without a bias, to_out.0 with one, plain softmax
    attention over `heads` heads): they compute in fp32 (float64 where they are given float64) from whatever they are given
    and round their output once, so that a comparison of the shell around them does not compare PyTorch's SDPA;
  * weights: closed-form stand-ins seeded by (tag, parameter name), drawn in float64 and rounded to fp16 once, scaled so that
    every activation stays below 65504 / 8 (the golden maker asserts it);
  * `forward(..., q)`: q is applied to every layer's output -- the identity for the float64 record, a round trip through fp16
    for the reference arithmetic's noise (the module run in fp32 with every layer's output rounded to fp16);
  * `Tree`: a resnet (unet_resnet_model.Resnet), a transformer and a consumer that does permute(0, 2, 3, 1).reshape: what
    patch_unet_resnets + patch_unet_transformers are tried on.
"""
import math
import os
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import unet_resnet_model as R
from vae_model import round16, thin  # noqa: F401  (the VAE golden's thinning rule and fp16 round trip)

# (C, heads, n, H, W, text tokens, text width)
CASES = [(320, 8, 2, 8, 12, 7, 64),      # 192 rows: two row tiles, the second ragged
         (640, 8, 1, 16, 8, 77, 96),
         (1280, 8, 2, 4, 4, 5, 64)]      # 32 rows, a quarter of a tile; inner 5120, K = 5120 in ff.net.2
GOLDEN_FILE = "unet_transformer_golden.npz"
GN_EPS, LN_EPS = 1e-6, 1e-5
ACT_LIMIT = 65504.0 / 8
TENSORS = ("tap", "out")  # the order of a case's *_noise and *_peak entries: the first block's GEGLU output, the module's output

_ident = lambda t: t  # noqa: E731


def case_key(case):
    return "transformer_%dh%d_%dx%dx%d_t%dx%d" % tuple(case)


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN_FILE)))


def inputs(case):
    """the case's x (n, C, H, W) and text (n, tokens, width): N(0, 1) drawn in float64, the LAST image scaled and shifted,
    rounded to fp16"""
    C, _, n, H, W, T, TW = case
    rs = np.random.RandomState(zlib.crc32(case_key(case).encode()) & 0x7FFFFFFF)
    x = rs.standard_normal((n, C, H, W)) * 1.5
    x[-1] = x[-1] * 0.5 + 1.0
    t = rs.standard_normal((n, T, TW))
    return torch.from_numpy(x).to(torch.float16), torch.from_numpy(t).to(torch.float16)


class Attention(nn.Module):
    """a stand-in for diffusers' Attention with its default processor: fp32 (or float64) arithmetic, one rounding"""

    def __init__(self, dim, heads, cross_dim=None):
        super().__init__()
        self.heads = heads
        self.to_q = nn.Linear(dim, dim, bias=False)
        self.to_k = nn.Linear(cross_dim or dim, dim, bias=False)
        self.to_v = nn.Linear(cross_dim or dim, dim, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **kwargs):
        assert attention_mask is None and not kwargs
        ct = torch.float64 if hidden_states.dtype == torch.float64 else torch.float32
        x = hidden_states.to(ct)
        e = x if encoder_hidden_states is None else encoder_hidden_states.to(ct)
        n, L, D = x.shape
        split = lambda t: t.view(n, -1, self.heads, D // self.heads).transpose(1, 2)  # noqa: E731
        q, k, v = split(x @ self.to_q.weight.to(ct).t()), split(e @ self.to_k.weight.to(ct).t()), split(e @ self.to_v.weight.to(ct).t())
        p = torch.softmax(q @ k.transpose(-1, -2) * (D // self.heads) ** -0.5, dim=-1)
        o = (p @ v).transpose(1, 2).reshape(n, L, D)
        o = o @ self.to_out[0].weight.to(ct).t() + self.to_out[0].bias.to(ct)
        return o.to(hidden_states.dtype)


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)

    def forward(self, x, q=_ident):
        value, gate = q(self.proj(x)).chunk(2, dim=-1)
        return q(value * q(F.gelu(gate)))


class FeedForward(nn.Module):
    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * mult), nn.Dropout(0.0), nn.Linear(dim * mult, dim)])

    def forward(self, x, q=_ident, taps=None):
        g = self.net[0](x, q)
        if taps is not None and "tap" not in taps:
            taps["tap"] = g
        return q(self.net[2](self.net[1](g)))


class Block(nn.Module):
    """BasicTransformerBlock, restated"""

    def __init__(self, dim, heads, cross_dim):
        super().__init__()
        self.only_cross_attention = False
        self.use_ada_layer_norm = self.use_ada_layer_norm_zero = False
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn1 = Attention(dim, heads)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn2 = Attention(dim, heads, cross_dim)
        self.norm3 = nn.LayerNorm(dim, eps=LN_EPS)
        self.ff = FeedForward(dim)
        self._chunk_size = None
        self._chunk_dim = 0

    def forward(self, h, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None, timestep=None,
                cross_attention_kwargs=None, class_labels=None, q=_ident, taps=None):
        kw = cross_attention_kwargs if cross_attention_kwargs is not None else {}
        a = q(self.attn1(q(self.norm1(h)), encoder_hidden_states=None, attention_mask=attention_mask, **kw))
        h = q(a + h)
        a = q(self.attn2(q(self.norm2(h)), encoder_hidden_states=encoder_hidden_states, attention_mask=encoder_attention_mask, **kw))
        h = q(a + h)
        return q(self.ff(q(self.norm3(h)), q, taps) + h)


class Output:
    def __init__(self, sample):
        self.sample = sample


class Transformer(nn.Module):
    """Transformer2DModel, restated (continuous input, 1 x 1 convolutions in and out)"""

    def __init__(self, channels, heads, cross_dim, layers=1, groups=32):
        super().__init__()
        self.use_linear_projection = False
        self.is_input_continuous = True
        self.norm = nn.GroupNorm(groups, channels, eps=GN_EPS)
        self.proj_in = nn.Conv2d(channels, channels, 1)
        self.transformer_blocks = nn.ModuleList([Block(channels, heads, cross_dim) for _ in range(layers)])
        self.proj_out = nn.Conv2d(channels, channels, 1)

    def forward(self, hidden_states, encoder_hidden_states=None, timestep=None, class_labels=None, cross_attention_kwargs=None,
                attention_mask=None, encoder_attention_mask=None, return_dict=True, q=_ident, taps=None):
        n, _, H, W = hidden_states.shape
        residual = hidden_states
        h = q(self.proj_in(q(self.norm(hidden_states))))
        D = h.shape[1]
        h = h.permute(0, 2, 3, 1).reshape(n, H * W, D)
        for blk in self.transformer_blocks:
            h = blk(h, attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states,
                    encoder_attention_mask=encoder_attention_mask, timestep=timestep,
                    cross_attention_kwargs=cross_attention_kwargs, class_labels=class_labels, q=q, taps=taps)
        if taps is not None:
            taps["tokens"] = h
        h = h.reshape(n, H, W, D).permute(0, 3, 1, 2).contiguous()
        out = q(q(self.proj_out(h)) + residual)
        return Output(out) if return_dict else (out,)


class Tree(nn.Module):
    """a resnet, a transformer behind it (as a CrossAttnDownBlock2D pairs them), and a consumer that reads the result as
    tokens"""

    def __init__(self, c=320, heads=8, cross_dim=64, temb_channels=R.TEMB_CHANNELS):
        super().__init__()
        self.resnets = nn.ModuleList([R.Resnet(c, c, temb_channels)])
        self.attentions = nn.ModuleList([Transformer(c, heads, cross_dim)])
        self.proj = nn.Linear(c, 64)

    def forward(self, x, temb, text, q=_ident):
        h = self.resnets[0](x, temb) if q is _ident else self.resnets[0](x, temb, q)
        if q is _ident:
            h = self.attentions[0](h, encoder_hidden_states=text, return_dict=False)[0]
        else:
            h = self.attentions[0](h, encoder_hidden_states=text, return_dict=False, q=q)[0]
        n, c, H, W = h.shape
        tokens = h.permute(0, 2, 3, 1).reshape(n, H * W, c)
        return q(self.proj(tokens))


# ---------------------------------------------------------------------------------------------------------------------
# stand-in weights
# ---------------------------------------------------------------------------------------------------------------------
def standin_value(seed_name, name, shape):
    """float64 stand-in of one parameter: norm scales U(0.75, 1.25), norm shifts and biases 0.1 N(0, 1), the weights behind a
    SiLU or the GEGLU product (the resnet's conv1 / conv2 / time_emb_proj, ff.net.2) sqrt(2 / fan_in) N(0, 1), any other
    weight sqrt(1 / fan_in) N(0, 1)"""
    rs = np.random.RandomState(zlib.crc32(seed_name.encode()) & 0x7FFFFFFF)
    leaf = name.rsplit(".", 2)[-2]
    if "norm" in leaf and name.endswith(".weight"):
        return rs.uniform(0.75, 1.25, shape)
    if name.endswith(".bias"):
        return 0.1 * rs.standard_normal(shape)
    fan_in = int(np.prod(shape[1:]))
    gain = 2.0 if leaf in ("conv1", "conv2", "time_emb_proj") or name.endswith("ff.net.2.weight") else 1.0
    return math.sqrt(gain / fan_in) * rs.standard_normal(shape)


def standin_state_dict(module, tag, dtype=torch.float64):
    """every value is rounded to fp16 once, here: the float64, fp32 and fp16 runs and the packed weights carry the same VALUES"""
    return OrderedDict((name, torch.from_numpy(np.asarray(standin_value("%s.%s" % (tag, name), name, tuple(v.shape)), np.float64)
                                               .astype(np.float16).astype(np.float64)).to(dtype))
                       for name, v in module.state_dict().items())


def build(channels, heads, cross_dim, dtype=torch.float32, layers=1):
    """the restated module with its stand-in weights, in eval mode"""
    net = Transformer(channels, heads, cross_dim, layers)
    net.load_state_dict(standin_state_dict(net, "tf%dh%dx%d" % (channels, heads, cross_dim)))
    return net.to(dtype).eval()


def build_tree(dtype=torch.float32, c=320, heads=8, cross_dim=64):
    net = Tree(c, heads, cross_dim)
    net.load_state_dict(standin_state_dict(net, "tftree%d" % c))
    return net.to(dtype).eval()


def record(case):
    """(float64 GEGLU tap (n, H, W, inner), float64 output (n, H, W, C), noise [tap, out], peak [tap, out], largest
    activation): the float64 run of the case, and the reference arithmetic's noise against it = max|difference| /
    max|float64| of the fp32 run with every layer's output rounded to fp16"""
    C, heads, n, H, W, _, TW = case
    x, text = inputs(case)
    net64, net32 = build(C, heads, TW, torch.float64), build(C, heads, TW, torch.float32)
    seen = [0.0]

    def see(m, i, o):
        if isinstance(o, torch.Tensor):
            seen[0] = max(seen[0], float(o.detach().abs().max()))
    hooks = [m.register_forward_hook(see) for net in (net64, net32) for m in net.modules() if not list(m.children())]
    t64, t16 = {}, {}
    with torch.no_grad():
        o64 = net64(x.double(), text.double(), taps=t64).sample.permute(0, 2, 3, 1)
        o16 = net32(x.float(), text.float(), q=round16, taps=t16).sample.permute(0, 2, 3, 1)
    for h in hooks:
        h.remove()
    tap64, tap16 = (t["tap"].reshape(n, H, W, -1) for t in (t64, t16))
    peaks = [float(tap64.abs().max()), float(o64.abs().max())]
    noise = [float((tap16.double() - tap64).abs().max() / peaks[0]), float((o16.double() - o64).abs().max() / peaks[1])]
    act = max(seen[0], peaks[0], peaks[1], float(t64["tokens"].abs().max()), float(t16["tokens"].abs().max()))
    return tap64.contiguous(), o64.contiguous(), noise, peaks, act
