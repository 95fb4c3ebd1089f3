"""Stand-ins and restatements shared by tests/golden/make_unet_shell_golden.py, tests/test_unet_shell_cpu.py and
tests/test_gpu_unet_shell.py.

Torch restatements of what diffusers 0.19.3 puts around the resnets and transformers of the SD-1.5 UNet and ControlNet, under
its attribute and parameter names:

  Downsample2D       channels, out_channels, use_conv, padding, name, conv           models/resnet.py
  Upsample2D         channels, out_channels, use_conv, use_conv_transpose, name, conv; forward(x, output_size=None)
  Timesteps          num_channels, flip_sin_to_cos, downscale_freq_shift             models/embeddings.py
  TimestepEmbedding  linear_1, act, linear_2, cond_proj, post_act; forward(sample, condition=None)
  ControlNetConditioningEmbedding  conv_in, blocks, conv_out                         models/controlnet.py
  conv_in, conv_norm_out, conv_act, conv_out, time_proj, time_embedding              models/unet_2d_condition.py
  controlnet_cond_embedding, controlnet_down_blocks, controlnet_mid_block            models/controlnet.py

and the two skeletons patch_unet_shell is tried on, built from unet_resnet_model.Resnet and these modules: `UNetSkeleton`
(conv_in, the time MLP, three resnet + downsampler levels, three upsampler + resnet levels with torch.cat skips, the output
end) and `ControlNetSkeleton` (conv_in + the condition embedding, the time MLP, four levels of two resnets with three
downsamplers, a mid resnet, twelve + one zero convolutions, the conditioning-scale multiply).  The skeletons hold no
transformer block.

diffusers is NOT installed where these tests run: the names, the attributes and the forwards come from its published source
and are UNVERIFIED against the real modules.

  * weights: unet_resnet_model.standin_value's closed forms, seeded by (tag, parameter name), rounded to fp16 once;
  * `forward(..., q)`: q is applied to every layer's output -- the identity for the float64 record, a round trip through fp16
    for the reference arithmetic's noise (the module run in fp32 with every layer's output rounded to fp16).
"""
import math
import os
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import unet_resnet_model as R
from unet_resnet_model import standin_state_dict, standin_value  # noqa: F401
from vae_model import round16, thin  # noqa: F401

GOLDEN_FILE = "unet_shell_golden.npz"
ACT_LIMIT = 65504.0 / 8
EMBED_CHANNELS = (16, 32, 96, 256)
# (kind, widths, n, H, W): H, W of the module's INPUT plane
CASES = [("down", 320, 2, 12, 20), ("down", 1280, 1, 4, 4),
         ("up", 1280, 2, 4, 6), ("up", 640, 1, 10, 14),
         ("conv_in", 320, 2, 8, 12),
         ("conv_out", 320, 2, 8, 12),
         ("time", 320, 2, 1, 1),
         ("cond", 320, 2, 32, 48),
         ("zero", 640, 2, 4, 6)]
TIMESTEPS = (999.0, 251.0, 1.0, 0.0)

_ident = lambda t: t  # noqa: E731


def case_key(case):
    return "shell_%s%d_%dx%dx%d" % tuple(case)


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN_FILE)))


# ---------------------------------------------------------------------------------------------------------------------
# the modules, restated
# ---------------------------------------------------------------------------------------------------------------------
class Downsample2D(nn.Module):
    def __init__(self, channels, use_conv=True, out_channels=None, padding=1, name="conv"):
        super().__init__()
        self.channels, self.out_channels = channels, out_channels or channels
        self.use_conv, self.padding, self.name = use_conv, padding, name
        self.conv = nn.Conv2d(channels, self.out_channels, 3, stride=2, padding=padding) if use_conv else nn.AvgPool2d(2, 2)

    def forward(self, hidden_states, q=_ident):
        if self.use_conv and self.padding == 0:
            hidden_states = F.pad(hidden_states, (0, 1, 0, 1), mode="constant", value=0)
        return q(self.conv(hidden_states))


class Upsample2D(nn.Module):
    def __init__(self, channels, use_conv=True, use_conv_transpose=False, out_channels=None, name="conv"):
        super().__init__()
        self.channels, self.out_channels = channels, out_channels or channels
        self.use_conv, self.use_conv_transpose, self.name = use_conv, use_conv_transpose, name
        self.conv = nn.Conv2d(channels, self.out_channels, 3, padding=1) if use_conv else None

    def forward(self, hidden_states, output_size=None, q=_ident):
        if output_size is None:
            hidden_states = F.interpolate(hidden_states, scale_factor=2.0, mode="nearest")
        else:
            hidden_states = F.interpolate(hidden_states, size=output_size, mode="nearest")
        return q(self.conv(hidden_states)) if self.use_conv else hidden_states


def timestep_embedding(timesteps, dim, flip_sin_to_cos=True, downscale_freq_shift=0.0, max_period=10000):
    """get_timestep_embedding, in the dtype of `timesteps` (diffusers: fp32)"""
    half = dim // 2
    exponent = -math.log(max_period) * torch.arange(half, dtype=timesteps.dtype, device=timesteps.device)
    exponent = exponent / (half - downscale_freq_shift)
    emb = timesteps[:, None] * torch.exp(exponent)[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
    if flip_sin_to_cos:
        emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)
    return emb


class Timesteps(nn.Module):
    def __init__(self, num_channels, flip_sin_to_cos=True, downscale_freq_shift=0):
        super().__init__()
        self.num_channels, self.flip_sin_to_cos, self.downscale_freq_shift = num_channels, flip_sin_to_cos, downscale_freq_shift

    def forward(self, timesteps):
        return timestep_embedding(timesteps, self.num_channels, self.flip_sin_to_cos, self.downscale_freq_shift)


class TimestepEmbedding(nn.Module):
    def __init__(self, in_channels, time_embed_dim):
        super().__init__()
        self.linear_1 = nn.Linear(in_channels, time_embed_dim)
        self.cond_proj = None
        self.act = nn.SiLU()
        self.linear_2 = nn.Linear(time_embed_dim, time_embed_dim)
        self.post_act = None

    def forward(self, sample, condition=None, q=_ident):
        if condition is not None:
            sample = sample + self.cond_proj(condition)
        sample = q(self.linear_1(sample))
        sample = q(self.act(sample))
        return q(self.linear_2(sample))


class CondEmbedding(nn.Module):
    """ControlNetConditioningEmbedding"""

    def __init__(self, conditioning_embedding_channels, conditioning_channels=3, block_out_channels=EMBED_CHANNELS):
        super().__init__()
        b = block_out_channels
        self.conv_in = nn.Conv2d(conditioning_channels, b[0], 3, padding=1)
        self.blocks = nn.ModuleList([])
        for i in range(len(b) - 1):
            self.blocks.append(nn.Conv2d(b[i], b[i], 3, padding=1))
            self.blocks.append(nn.Conv2d(b[i], b[i + 1], 3, padding=1, stride=2))
        self.conv_out = nn.Conv2d(b[-1], conditioning_embedding_channels, 3, padding=1)

    def forward(self, conditioning, q=_ident):
        e = q(F.silu(q(self.conv_in(conditioning))))
        for block in self.blocks:
            e = q(F.silu(q(block(e))))
        return q(self.conv_out(e))


class _Ends(nn.Module):
    """conv_in and the time MLP, as both models have them"""

    def _ends(self, c):
        self.conv_in = nn.Conv2d(4, c, 3, padding=1)
        self.time_proj = Timesteps(c, True, 0)
        self.time_embedding = TimestepEmbedding(c, 4 * c)

    def _emb(self, sample, timesteps, q):
        t_emb = self.time_proj(timesteps)
        t_emb = q(t_emb.to(dtype=sample.dtype))   # "timesteps does not contain any weights and will always return f32 tensors"
        return self.time_embedding(t_emb) if q is _ident else self.time_embedding(t_emb, None, q)


def _call(m, q, *args):
    return m(*args) if q is _ident else m(*args, q=q)


class UNetSkeleton(_Ends):
    def __init__(self, c=320):
        super().__init__()
        self._ends(c)
        self.down_resnets = nn.ModuleList([R.Resnet(c, c, 4 * c) for _ in range(3)])
        self.downsamplers = nn.ModuleList([Downsample2D(c) for _ in range(3)])
        self.upsamplers = nn.ModuleList([Upsample2D(c) for _ in range(3)])
        self.up_resnets = nn.ModuleList([R.Resnet(2 * c, c, 4 * c) for _ in range(3)])
        self.conv_norm_out = nn.GroupNorm(32, c, eps=1e-5)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(c, 4, 3, padding=1)

    def forward(self, sample, timesteps, q=_ident):
        emb = self._emb(sample, timesteps, q)
        h = q(self.conv_in(sample))
        skips = []
        for r, d in zip(self.down_resnets, self.downsamplers):
            h = _call(r, q, h, emb)
            skips.append(h)
            h = _call(d, q, h)
        for u, r in zip(self.upsamplers, self.up_resnets):
            h = _call(u, q, h)
            h = _call(r, q, torch.cat([h, skips.pop()], dim=1), emb)
        h = q(self.conv_act(q(self.conv_norm_out(h))))
        return q(self.conv_out(h))


class ControlNetSkeleton(_Ends):
    def __init__(self, c=320):
        super().__init__()
        self._ends(c)
        self.controlnet_cond_embedding = CondEmbedding(c)
        self.resnets = nn.ModuleList([R.Resnet(c, c, 4 * c) for _ in range(8)])
        self.downsamplers = nn.ModuleList([Downsample2D(c) for _ in range(3)])
        self.mid_resnet = R.Resnet(c, c, 4 * c)
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(c, c, 1) for _ in range(12)])
        self.controlnet_mid_block = nn.Conv2d(c, c, 1)

    def forward(self, sample, timesteps, controlnet_cond, conditioning_scale=1.0, q=_ident):
        emb = self._emb(sample, timesteps, q)
        h = q(self.conv_in(sample))
        cond = _call(self.controlnet_cond_embedding, q, controlnet_cond)
        h = q(h + cond)
        samples = [h]
        for level in range(4):
            for r in self.resnets[2 * level:2 * level + 2]:
                h = _call(r, q, h, emb)
                samples.append(h)
            if level < 3:
                h = _call(self.downsamplers[level], q, h)
                samples.append(h)
        h = _call(self.mid_resnet, q, h, emb)
        down = [q(q(z(s)) * conditioning_scale) for z, s in zip(self.controlnet_down_blocks, samples)]
        mid = q(q(self.controlnet_mid_block(h)) * conditioning_scale)
        return down, mid


def build_skeleton(kind, dtype=torch.float32, c=320):
    net = {"unet": UNetSkeleton, "controlnet": ControlNetSkeleton}[kind](c)
    net.load_state_dict(standin_state_dict(net, "%s_skeleton%d" % (kind, c)))
    return net.to(dtype).eval()


def skeleton_inputs(n=2, H=8, W=8):
    """latents (n, 4, H, W), timesteps (n) fp32, condition (n, 3, 8 H, 8 W): fp16 values; the last image shifted"""
    rs = np.random.RandomState(20)
    x = rs.standard_normal((n, 4, H, W))
    x[-1] = x[-1] * 0.5 + 0.5
    cond = rs.uniform(0.0, 1.0, (n, 3, 8 * H, 8 * W))
    return (torch.from_numpy(x).to(torch.float16), torch.tensor(TIMESTEPS[:n], dtype=torch.float32),
            torch.from_numpy(cond).to(torch.float16))


# ---------------------------------------------------------------------------------------------------------------------
# one module per case
# ---------------------------------------------------------------------------------------------------------------------
class _OutputEnd(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv_norm_out = nn.GroupNorm(32, c, eps=1e-5)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(c, 4, 3, padding=1)

    def forward(self, x, q=_ident):
        return q(self.conv_out(q(self.conv_act(q(self.conv_norm_out(x))))))


class _TimeEnd(_Ends):
    def __init__(self, c):
        super().__init__()
        self._ends(c)
        del self.conv_in

    def forward(self, timesteps, q=_ident, dtype=None):
        """dtype: the `sample.dtype` the sinusoid is cast to (default: that of the timesteps)"""
        return self._emb(torch.empty(0, dtype=dtype or timesteps.dtype), timesteps, q)


class _Plain(nn.Module):
    """a bare Conv2d with the q of the other restatements"""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv

    def forward(self, x, q=_ident):
        return q(self.conv(x))


def build(case, dtype=torch.float32):
    """the case's module with its stand-in weights, in eval mode"""
    kind, c = case[:2]
    net = {"down": lambda: Downsample2D(c), "up": lambda: Upsample2D(c), "conv_in": lambda: _Plain(nn.Conv2d(4, c, 3, padding=1)),
           "conv_out": lambda: _OutputEnd(c), "time": lambda: _TimeEnd(c), "cond": lambda: CondEmbedding(c),
           "zero": lambda: _Plain(nn.Conv2d(c, c, 1))}[kind]()
    net.load_state_dict(standin_state_dict(net, "%s%d" % (kind, c)))
    return net.to(dtype).eval()


def inputs(case):
    """the case's input, fp16 values (the timesteps fp32): N(0, 1) x 1.5 with the LAST image scaled and shifted; the condition
    image U(0, 1); the latents N(0, 1)"""
    kind, c, n, H, W = case
    rs = np.random.RandomState(zlib.crc32(case_key(case).encode()) & 0x7FFFFFFF)
    if kind == "time":
        return torch.tensor(TIMESTEPS[:n], dtype=torch.float32)
    if kind == "cond":
        return torch.from_numpy(rs.uniform(0.0, 1.0, (n, 3, H, W))).to(torch.float16)
    cin = 4 if kind == "conv_in" else c
    x = rs.standard_normal((n, cin, H, W)) * (1.0 if kind == "conv_in" else 1.5)
    x[-1] = x[-1] * 0.5 + 1.0
    return torch.from_numpy(x).to(torch.float16)


def as_record(case, out):
    """the module's output (logical NCHW, or (n, C) of the time MLP) as the (n, H, W, C) tensor the golden file thins: NHWC;
    the four output channels of conv_out go beside the columns, (n, H, 4 W, 1), so that thinning keeps all four"""
    if case[0] == "time":
        return out[:, None, None, :]
    o = out.permute(0, 2, 3, 1)
    if case[0] == "conv_out":
        n, H, W, C = o.shape
        return o.reshape(n, H, W * C, 1)
    return o.contiguous()


def record(case):
    """(float64 output as_record, noise, peak, largest activation): the float64 run of the case, and the reference
    arithmetic's noise against it = max|difference| / max|float64| of the fp32 run with every layer's output rounded to fp16"""
    x = inputs(case)
    net64, net32 = build(case, torch.float64), build(case, torch.float32)
    seen = [0.0]

    def see(m, i, o):
        seen[0] = max(seen[0], float(o.detach().abs().max()))
    hooks = [m.register_forward_hook(see) for net in (net64, net32) for m in net.modules() if not list(m.children())]
    with torch.no_grad():
        if case[0] == "time":
            o64 = net64(x.double())
            o16 = net32(x.float(), round16)
        else:
            o64 = net64(x.double())
            o16 = net32(x.float(), q=round16)
    for h in hooks:
        h.remove()
    o64, o16 = as_record(case, o64), as_record(case, o16)
    peak = float(o64.abs().max())
    noise = float((o16.double() - o64).abs().max() / peak)
    return o64.contiguous(), noise, peak, max(seen[0], peak)
