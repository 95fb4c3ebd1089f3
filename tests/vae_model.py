"""Stand-ins and restatements shared by tests/golden/make_vae_golden.py, tests/test_vae_cpu.py and tests/test_gpu_vae.py.

A torch restatement of the decoder half of diffusers' AutoencoderKL as the SD-1.5 VAE configures it (block_out_channels
(128, 256, 512, 512), layers_per_block 2, norm_num_groups 32, eps 1e-6, one single-head attention block with a residual in
the mid block), under the parameter names of diffusers 0.19.3:

  post_quant_conv, decoder.conv_in, decoder.mid_block.resnets.{0,1}.{norm1,conv1,norm2,conv2},
  decoder.mid_block.attentions.0.{group_norm,to_q,to_k,to_v,to_out.0},
  decoder.up_blocks.{0..3}.resnets.{0..2} (conv_shortcut where cin != cout), decoder.up_blocks.{0..2}.upsamplers.0.conv,
  decoder.conv_norm_out, decoder.conv_out.

diffusers is NOT installed where these tests run: the names, the block layout (channels walked in reverse, the up blocks'
third resnet, nearest 2x upsample then a padded 3 x 3 convolution, SiLU after every norm of a resnet and after
conv_norm_out, softmax(q k^T / sqrt(512)) v, to_out, + residual) come from its published source (models/autoencoder_kl.py,
vae.py, unet_2d_blocks.py, resnet.py, attention_processor.py) and are UNVERIFIED against the real module.

  * weights: closed-form stand-ins seeded by parameter name (`standin_state_dict`), drawn in float64, scaled so that every
    activation stays below 65504 / 8 (the golden maker asserts it);
  * `forward(z, taps, q)`: q is applied to every layer's output -- the identity for the float64 record, a round trip through
    fp16 for the reference arithmetic's noise (the module run in fp32 with every layer's output rounded to fp16).
"""
import math
import os
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

CASES = [(2, 8, 12), (1, 16, 8), (1, 20, 28)]  # latents (n, h, w): 96, 128 and 560 tokens in the mid block
GOLDEN_FILE = "vae_golden.npz"
# tests/golden/make_vae_fullsize_golden.py: 576 tokens in the mid block with two images, and GroupNorm past one grid pass of
# its apply kernel at every width; the real 512 x 512 frame (4096 tokens), recorded without its whole uint8 image
FULLSIZE_CASES = [(2, 24, 24), (1, 64, 64)]
FULLSIZE_GOLDEN_FILE = "vae_fullsize_golden.npz"
NAMES_FILE = "vae_decoder_names.txt"
TAPS = ("conv_in", "mid", "up0", "up1", "up2", "up3", "norm_out")
TAP_STRIDE = 16     # the golden file keeps every 16th channel of a tap ...
TAP_VALUES = 768    # ... at the rows and columns of a stride that leaves about this many values per frame
IMAGE_STRIDE = 4    # rows / columns of the float64 image the file keeps (the last ones always); the uint8 image is whole
BLOCK_CHANNELS = (128, 256, 512, 512)
ACT_LIMIT = 65504.0 / 8
OLD_ATTENTION = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}


def case_key(case):
    return "vae_%dx%dx%d" % case


def load_golden(golden_dir, name=GOLDEN_FILE):
    return dict(np.load(os.path.join(golden_dir, name)))


def _picks(size, stride):
    return np.unique(np.r_[0:size:stride, size - 1])


def thin(t):
    """a tap (n, H, W, C), torch or numpy -> numpy, as the golden file keeps it (midas_model.thin's rule for maps): every
    TAP_STRIDE-th channel at every s-th row and column plus the last ones, s the smallest stride that leaves at most
    TAP_VALUES values per frame"""
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    t = t[..., ::TAP_STRIDE]
    _, H, W, C = t.shape
    s = max(1, int(math.ceil(math.sqrt(H * W * C / float(TAP_VALUES)))))
    return np.ascontiguousarray(t[:, _picks(H, s)][:, :, _picks(W, s)])


def thin_image(img):
    """the image (n, 3, H, W) at every IMAGE_STRIDE-th row and column plus the last ones"""
    img = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    return np.ascontiguousarray(img[:, :, _picks(img.shape[2], IMAGE_STRIDE)][:, :, :, _picks(img.shape[3], IMAGE_STRIDE)])


def tensor2numpy(img):
    """src/utils.py:17-21 of the reference"""
    image = (img / 2 + 0.5).clamp(0, 1)
    image = image.detach().cpu().permute(0, 2, 3, 1).numpy()
    return (image * 255).round().astype("uint8")


def latents(case, dtype=torch.float16):
    """the case's latents (n, 4, h, w): N(0, 1) drawn in float64 and rounded to fp16 (every run starts from these values)"""
    n, h, w = case
    rs = np.random.RandomState(zlib.crc32(case_key(case).encode()) & 0x7FFFFFFF)
    return torch.from_numpy(rs.standard_normal((n, 4, h, w))).to(torch.float16).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the decoder, restated
# ---------------------------------------------------------------------------------------------------------------------
_ident = lambda t: t  # noqa: E731


def round16(t):
    return t.to(torch.float16).to(t.dtype)


class Resnet(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm1 = nn.GroupNorm(32, cin, eps=1e-6)
        self.conv1 = nn.Conv2d(cin, cout, 3, 1, 1)
        self.norm2 = nn.GroupNorm(32, cout, eps=1e-6)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x, q=_ident):
        h = q(F.silu(q(self.norm1(x))))
        h = q(self.conv1(h))
        h = q(F.silu(q(self.norm2(h))))
        h = q(self.conv2(h))
        if hasattr(self, "conv_shortcut"):
            x = q(self.conv_shortcut(x))
        return q(x + h)


class Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.group_norm = nn.GroupNorm(32, c, eps=1e-6)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c), nn.Identity()])

    def forward(self, x, q=_ident):
        n, c, H, W = x.shape
        h = q(self.group_norm(x.reshape(n, c, H * W))).transpose(1, 2)
        qq, k, v = q(self.to_q(h)), q(self.to_k(h)), q(self.to_v(h))
        p = q(torch.softmax(q(qq @ k.transpose(1, 2) * c ** -0.5), dim=-1))
        o = q(self.to_out[0](q(p @ v)))
        return q(o.transpose(1, 2).reshape(n, c, H, W) + x)


class Upsample(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 1, 1)

    def forward(self, x, q=_ident):
        return q(self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest")))


class MidBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attentions = nn.ModuleList([Attention(c)])
        self.resnets = nn.ModuleList([Resnet(c, c), Resnet(c, c)])

    def forward(self, x, q=_ident):
        return self.resnets[1](self.attentions[0](self.resnets[0](x, q), q), q)


class UpBlock(nn.Module):
    def __init__(self, cin, cout, upsample):
        super().__init__()
        self.resnets = nn.ModuleList([Resnet(cin if i == 0 else cout, cout) for i in range(3)])
        if upsample:
            self.upsamplers = nn.ModuleList([Upsample(cout)])

    def forward(self, x, q=_ident):
        for r in self.resnets:
            x = r(x, q)
        return self.upsamplers[0](x, q) if hasattr(self, "upsamplers") else x


class Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        rev = BLOCK_CHANNELS[::-1]
        self.conv_in = nn.Conv2d(4, rev[0], 3, 1, 1)
        self.up_blocks = nn.ModuleList()
        cin = rev[0]
        for b, cout in enumerate(rev):
            self.up_blocks.append(UpBlock(cin, cout, b < len(rev) - 1))
            cin = cout
        self.mid_block = MidBlock(rev[0])
        self.conv_norm_out = nn.GroupNorm(32, rev[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(rev[-1], 3, 3, 1, 1)


class VAE(nn.Module):
    """post_quant_conv + decoder of AutoencoderKL; decode(z) -> an object with .sample like the real module, forward(z, taps,
    q) -> the image with the TAPS tensors (NHWC) left in `taps`"""
    use_slicing = False
    use_tiling = False

    def __init__(self):
        super().__init__()
        self.post_quant_conv = nn.Conv2d(4, 4, 1)
        self.decoder = Decoder()

    def forward(self, z, taps=None, q=_ident):
        taps = {} if taps is None else taps
        nhwc = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
        d = self.decoder
        x = q(d.conv_in(q(self.post_quant_conv(z))))
        taps["conv_in"] = nhwc(x)
        x = d.mid_block(x, q)
        taps["mid"] = nhwc(x)
        for b, blk in enumerate(d.up_blocks):
            x = blk(x, q)
            taps["up%d" % b] = nhwc(x)
        x = q(F.silu(q(d.conv_norm_out(x))))
        taps["norm_out"] = nhwc(x)
        return q(d.conv_out(x))

    def decode(self, z, return_dict=True):
        class Out:
            pass
        o = Out()
        o.sample = self.forward(z)
        return o if return_dict else (o.sample,)


# ---------------------------------------------------------------------------------------------------------------------
# stand-in weights
# ---------------------------------------------------------------------------------------------------------------------
def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def standin_value(name, shape):
    """float64 stand-in of one parameter: norm scales U(0.75, 1.25), norm shifts and biases 0.1 N(0, 1), post_quant_conv the
    identity + 0.2 N(0, 1), every other weight sqrt(g / fan_in) N(0, 1) with g = 2 behind a SiLU (the 3 x 3 convolutions of the
    resnets, conv_out) and 1 elsewhere"""
    rs = _rs(name)
    is_norm = "norm" in name.rsplit(".", 2)[-2]
    if is_norm and name.endswith(".weight"):
        return rs.uniform(0.75, 1.25, shape)
    if name.endswith(".bias"):
        return 0.1 * rs.standard_normal(shape)
    if name == "post_quant_conv.weight":
        return np.eye(4).reshape(shape) + 0.2 * rs.standard_normal(shape)
    fan_in = int(np.prod(shape[1:]))
    behind_silu = len(shape) == 4 and shape[2] == 3 and ("resnets" in name or name == "decoder.conv_out.weight")
    return math.sqrt((2.0 if behind_silu else 1.0) / fan_in) * rs.standard_normal(shape)


def standin_state_dict(names_shapes, dtype=torch.float32):
    """names_shapes: iterable of (name, shape) -- a module's state dict, or the committed list.  Every value is rounded to
    fp16 once, here: the float64, fp32 and fp16 runs and the packed weights all carry the same weight VALUES."""
    return OrderedDict((name, torch.from_numpy(np.asarray(standin_value(name, tuple(shape)), np.float64)
                                               .astype(np.float16).astype(np.float64)).to(dtype))
                       for name, shape in names_shapes)


def module_names_shapes(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def read_names_shapes(golden_dir):
    """the committed list: one `name d0xd1x..` line per parameter"""
    out = []
    for line in open(os.path.join(golden_dir, NAMES_FILE)):
        if line.strip():
            name, shape = line.split()
            out.append((name, tuple(int(d) for d in shape.split("x"))))
    return out


def old_spelling(sd):
    """the same tensors under the attention block's older names (query, key, value, proj_attn)"""
    out = OrderedDict()
    for k, v in sd.items():
        for new, old in OLD_ATTENTION.items():
            if ".attentions." in k and "." + new + "." in k:
                k = k.replace("." + new + ".", "." + old + ".")
                break
        out[k] = v
    return out


def build(dtype=torch.float32):
    """the restated module with its stand-in weights, in eval mode"""
    net = VAE()
    net.load_state_dict(standin_state_dict(module_names_shapes(net), torch.float64))
    return net.to(dtype).eval()
