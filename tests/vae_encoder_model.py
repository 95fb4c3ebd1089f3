"""Stand-ins and restatements shared by tests/golden/make_vae_encoder_golden.py, tests/test_vae_encoder_cpu.py,
tests/test_gpu_vae_encoder.py and tools/bench_vae_encoder.py: the encoder half beside tests/vae_model.py's decoder half.

A torch restatement of `AutoencoderKL.encode` as the SD-1.5 VAE configures it, under the parameter names of diffusers 0.19.3:

  encoder.conv_in (3 -> 128), encoder.down_blocks.{0..3}.resnets.{0,1} (conv_shortcut where cin != cout: blocks 1 and 2,
  resnet 0), encoder.down_blocks.{0..2}.downsamplers.0.conv, encoder.mid_block.{resnets.{0,1},attentions.0} as in the decoder,
  encoder.conv_norm_out, encoder.conv_out (512 -> 8), quant_conv (8 -> 8).

diffusers is NOT installed where these tests run: the names, the block layout (two resnets per down block, Downsample2D with
padding 0 = F.pad(x, (0, 1, 0, 1)) and then Conv2d(c, c, 3, stride 2, padding 0), no downsampler behind the last block, SiLU
after conv_norm_out, quant_conv on conv_out's eight channels, DiagonalGaussianDistribution with logvar clamped to [-30, 20])
come from its published source (models/autoencoder_kl.py, vae.py, unet_2d_blocks.py, resnet.py) and are UNVERIFIED against
the real module.

  * the resnets, the attention, the mid block, the stand-in rule, `thin` and `round16` are vae_model's, imported;
  * weights: `standin_value` by parameter name, every value rounded to fp16 once; encoder.conv_out.weight gets the gain of
    a layer behind SiLU (vae_model's rule knows only the decoder's conv_out by name), quant_conv the identity + 0.2 N(0, 1), so
    that logvar keeps conv_out's scale and stays inside (-30, 20) on every case (the golden maker asserts it);
  * inputs: deterministic images in about [-1, 1], see `images`;
  * `VAE.encode_forward(x, taps, q)`: q is applied to every layer's output, as in vae_model.
"""
import math
import os
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import vae_model as M
from vae_model import ACT_LIMIT, BLOCK_CHANNELS, Attention, MidBlock, Resnet, round16, standin_value, thin  # noqa: F401

CASES = [(2, 64, 96), (1, 128, 64), (1, 160, 224), (1, 68, 100)]  # images (n, H, W); the last one's third level is 17 x 25
GOLDEN_FILE = "vae_encoder_golden.npz"
FULLSIZE_CASES = [(2, 192, 192), (1, 512, 512)]  # tests/golden/make_vae_encoder_fullsize_golden.py: vae_model.FULLSIZE_CASES' images
FULLSIZE_GOLDEN_FILE = "vae_encoder_fullsize_golden.npz"
NAMES_FILE = "vae_encoder_names.txt"
TAPS = ("conv_in", "down0", "down1", "down2", "down3", "mid", "norm_out")
PREFIXES = ("encoder.", "quant_conv.")
_ident = lambda t: t  # noqa: E731


def case_key(case):
    return "vaeenc_%dx%dx%d" % case


def load_golden(golden_dir, name=GOLDEN_FILE):
    return dict(np.load(os.path.join(golden_dir, name)))


def images(case, dtype=torch.float16):
    """the case's images (n, 3, H, W) in about [-1, 1]: per channel a linear gradient and two sinusoids whose direction,
    frequency and phase come from the seed, plus N(0, 0.1); drawn in float64 from a seed of the case name and rounded to
    fp16 (every run starts from these values)"""
    n, H, W = case
    rs = np.random.RandomState(zlib.crc32(case_key(case).encode()) & 0x7FFFFFFF)
    y, x = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    out = np.empty((n, 3, H, W))
    for i in range(n):
        for c in range(3):
            a = rs.uniform(0, 2 * math.pi)
            img = 0.4 * (math.cos(a) * x + math.sin(a) * y)
            for amp in (0.3, 0.2):
                f, th, ph = rs.uniform(1, 6), rs.uniform(0, math.pi), rs.uniform(0, 2 * math.pi)
                img = img + amp * np.sin(f * math.pi * (math.cos(th) * x + math.sin(th) * y) + ph)
            out[i, c] = img + 0.1 * rs.standard_normal((H, W))
    return torch.from_numpy(out).to(torch.float16).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the encoder, restated
# ---------------------------------------------------------------------------------------------------------------------
class Downsample(nn.Module):
    """Downsample2D(use_conv=True, padding=0)"""

    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 2, 0)

    def forward(self, x, q=_ident):
        return q(self.conv(F.pad(x, (0, 1, 0, 1))))


class DownBlock(nn.Module):
    def __init__(self, cin, cout, downsample):
        super().__init__()
        self.resnets = nn.ModuleList([Resnet(cin if i == 0 else cout, cout) for i in range(2)])
        if downsample:
            self.downsamplers = nn.ModuleList([Downsample(cout)])

    def forward(self, x, q=_ident):
        for r in self.resnets:
            x = r(x, q)
        return self.downsamplers[0](x, q) if hasattr(self, "downsamplers") else x


class Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv_in = nn.Conv2d(3, BLOCK_CHANNELS[0], 3, 1, 1)
        self.down_blocks = nn.ModuleList()
        cin = BLOCK_CHANNELS[0]
        for b, cout in enumerate(BLOCK_CHANNELS):
            self.down_blocks.append(DownBlock(cin, cout, b < len(BLOCK_CHANNELS) - 1))
            cin = cout
        self.mid_block = MidBlock(BLOCK_CHANNELS[-1])
        self.conv_norm_out = nn.GroupNorm(32, BLOCK_CHANNELS[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(BLOCK_CHANNELS[-1], 8, 3, 1, 1)


class DiagonalGaussianDistribution:
    """diffusers/models/vae.py, without the deterministic switch, kl and nll"""

    def __init__(self, parameters):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, generator=None):
        dev = self.parameters.device
        if generator is not None and generator.device.type == "cpu" and dev.type != "cpu":  # (randn_tensor's rule)
            sample = torch.randn(self.mean.shape, generator=generator, device="cpu", dtype=self.parameters.dtype).to(dev)
        else:
            sample = torch.randn(self.mean.shape, generator=generator, device=dev, dtype=self.parameters.dtype)
        return self.mean + self.std * sample

    def mode(self):
        return self.mean


class VAE(M.VAE):
    """vae_model.VAE (post_quant_conv + decoder) with the other half: encoder + quant_conv.  encode(x) -> an object with
    .latent_dist like the real module, encode_forward(x, taps, q) -> the distribution's parameters (n, 8, H / 8, W / 8) with
    the TAPS tensors (NHWC) left in `taps`."""

    def __init__(self):
        super().__init__()
        self.encoder = Encoder()
        self.quant_conv = nn.Conv2d(8, 8, 1)

    def encode_forward(self, x, taps=None, q=_ident):
        taps = {} if taps is None else taps
        nhwc = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
        e = self.encoder
        x = q(e.conv_in(x))
        taps["conv_in"] = nhwc(x)
        for b, blk in enumerate(e.down_blocks):
            x = blk(x, q)
            taps["down%d" % b] = nhwc(x)
        x = e.mid_block(x, q)
        taps["mid"] = nhwc(x)
        x = q(F.silu(q(e.conv_norm_out(x))))
        taps["norm_out"] = nhwc(x)
        return q(self.quant_conv(q(e.conv_out(x))))

    def encode(self, x, return_dict=True):
        class Out:
            pass
        o = Out()
        o.latent_dist = DiagonalGaussianDistribution(self.encode_forward(x))
        return o if return_dict else (o.latent_dist,)


# ---------------------------------------------------------------------------------------------------------------------
# stand-in weights
# ---------------------------------------------------------------------------------------------------------------------
def encoder_standin_value(name, shape):
    """vae_model.standin_value with the encoder's two exceptions (see the module docstring)"""
    if name == "encoder.conv_out.weight":
        return math.sqrt(2.0 / int(np.prod(shape[1:]))) * M._rs(name).standard_normal(shape)
    if name == "quant_conv.weight":
        return np.eye(8).reshape(shape) + 0.2 * M._rs(name).standard_normal(shape)
    return standin_value(name, shape)


def standin_state_dict(names_shapes, dtype=torch.float32):
    """as vae_model.standin_state_dict: every value rounded to fp16 once"""
    from collections import OrderedDict
    return OrderedDict((name, torch.from_numpy(np.asarray(encoder_standin_value(name, tuple(shape)), np.float64)
                                               .astype(np.float16).astype(np.float64)).to(dtype))
                       for name, shape in names_shapes)


def encoder_names_shapes(module):
    """the encoder.* and quant_conv.* entries of the module's state dict"""
    return [(k, s) for k, s in M.module_names_shapes(module) if k.startswith(PREFIXES)]


def read_names_shapes(golden_dir):
    """the committed list: one `name d0xd1x..` line per parameter"""
    out = []
    for line in open(os.path.join(golden_dir, NAMES_FILE)):
        if line.strip():
            name, shape = line.split()
            out.append((name, tuple(int(d) for d in shape.split("x"))))
    return out


def build(dtype=torch.float32):
    """the restated module, both halves, with its stand-in weights, in eval mode"""
    net = VAE()
    net.load_state_dict(standin_state_dict(M.module_names_shapes(net), torch.float64))
    return net.to(dtype).eval()
