"""Stand-ins and restatements shared by tests/golden/make_unet_resnet_golden.py, tests/test_unet_resnet_cpu.py and
tests/test_gpu_unet_resnet.py.

A torch restatement of diffusers 0.19.3's `ResnetBlock2D` (models/resnet.py) as the SD-1.5 UNet and ControlNet configure it
-- groups 32, eps 1e-5, swish, time_embedding_norm "default", output_scale_factor 1.0, no up or down sampling, a 1 x 1
conv_shortcut iff cin != cout, a time embedding of 1280 channels -- under diffusers' parameter names:

  norm1, conv1, time_emb_proj, norm2, conv2, conv_shortcut

and its forward: conv2(SiLU(norm2(conv1(SiLU(norm1(x))) + time_emb_proj(SiLU(temb))[:, :, None, None]))) + shortcut(x).

diffusers is NOT installed where these tests run: the names, the attributes (`time_embedding_norm`, `up`, `down`,
`output_scale_factor`, `nonlinearity`, `dropout`, `upsample`, `downsample`) and the forward come from its published source
and are UNVERIFIED against the real module.

  * weights: closed-form stand-ins seeded by (cin, cout, parameter name), drawn in float64 and rounded to fp16 once, scaled so
    that every activation stays below 65504 / 8 (the golden maker asserts it);
  * `forward(x, temb, q)`: q is applied to every layer's output -- the identity for the float64 record, a round trip through
    fp16 for the reference arithmetic's noise (the module run in fp32 with every layer's output rounded to fp16);
  * `Tree`: two resnets with a torch.cat skip between them and a consumer that does permute(0, 2, 3, 1).reshape: what
    patch_unet_resnets is tried on.
"""
import math
import os
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from vae_model import round16, thin  # noqa: F401  (the VAE golden's thinning rule and fp16 round trip)

# (cin, cout, n, H, W)
CASES = [(320, 320, 2, 8, 12),      # identity shortcut, two images
         (960, 320, 1, 16, 8),
         (1920, 640, 1, 10, 14),    # ragged in both tile directions
         (2560, 1280, 2, 8, 8),     # K = 23040, the 8 x 8 plane
         (640, 1280, 1, 4, 4)]
GOLDEN_FILE = "unet_resnet_golden.npz"
TEMB_CHANNELS = 1280
EPS = 1e-5
ACT_LIMIT = 65504.0 / 8
TENSORS = ("tap", "out")  # the order of a case's *_noise and *_peak entries: conv1 + temb, the block's output

_ident = lambda t: t  # noqa: E731


def case_key(case):
    return "resnet_%dto%d_%dx%dx%d" % tuple(case)


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN_FILE)))


def inputs(case):
    """the case's x (n, cin, H, W) and temb (n, 1280): N(0, 1) drawn in float64, the LAST image scaled and shifted (statistics
    that bleed across images would show), rounded to fp16"""
    cin, _, n, H, W = case
    rs = np.random.RandomState(zlib.crc32(case_key(case).encode()) & 0x7FFFFFFF)
    x = rs.standard_normal((n, cin, H, W)) * 1.5
    x[-1] = x[-1] * 0.5 + 1.0
    t = rs.standard_normal((n, TEMB_CHANNELS))
    t[-1] = t[-1] * 0.5 - 0.25
    return torch.from_numpy(x).to(torch.float16), torch.from_numpy(t).to(torch.float16)


class Resnet(nn.Module):
    """ResnetBlock2D, restated"""

    def __init__(self, cin, cout, temb_channels=TEMB_CHANNELS, groups=32, eps=EPS):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=eps)
        self.conv1 = nn.Conv2d(cin, cout, 3, 1, 1)
        self.time_emb_proj = nn.Linear(temb_channels, cout)
        self.norm2 = nn.GroupNorm(groups, cout, eps=eps)
        self.dropout = nn.Dropout(0.0)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1)
        self.nonlinearity = nn.SiLU()
        self.time_embedding_norm = "default"
        self.output_scale_factor = 1.0
        self.up = self.down = False
        self.upsample = self.downsample = None
        self.conv_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else None

    def forward(self, x, temb, q=_ident, taps=None):
        h = q(self.nonlinearity(q(self.norm1(x))))
        h = q(self.conv1(h))
        t = q(self.time_emb_proj(q(self.nonlinearity(temb))))[:, :, None, None]
        h = q(h + t)
        if taps is not None:
            taps["tap"] = h.permute(0, 2, 3, 1)
        h = q(self.nonlinearity(q(self.norm2(h))))
        h = q(self.conv2(self.dropout(h)))
        if self.conv_shortcut is not None:
            x = q(self.conv_shortcut(x))
        return q((x + h) / self.output_scale_factor)


class Tree(nn.Module):
    """two resnets (c -> c, 2 c -> c) with a torch.cat skip between them, and a consumer that reads the result as tokens"""

    def __init__(self, c=320, temb_channels=TEMB_CHANNELS):
        super().__init__()
        self.down = nn.ModuleList([Resnet(c, c, temb_channels)])
        self.up = nn.ModuleDict({"resnets": nn.ModuleList([Resnet(2 * c, c, temb_channels)])})
        self.proj = nn.Linear(c, 64)

    def forward(self, x, temb, q=_ident):
        h = self.down[0](x, temb) if q is _ident else self.down[0](x, temb, q)
        h = torch.cat([h, x], dim=1)
        r = self.up["resnets"][0]
        h = r(h, temb) if q is _ident else r(h, temb, q)
        n, c, H, W = h.shape
        tokens = h.permute(0, 2, 3, 1).reshape(n, H * W, c)
        return q(self.proj(tokens))


# ---------------------------------------------------------------------------------------------------------------------
# stand-in weights
# ---------------------------------------------------------------------------------------------------------------------
def standin_value(seed_name, name, shape):
    """float64 stand-in of one parameter: norm scales U(0.75, 1.25), norm shifts and biases 0.1 N(0, 1), the 3 x 3 convolutions
    (behind a SiLU) sqrt(2 / fan_in) N(0, 1), time_emb_proj (behind a SiLU too) sqrt(2 / fan_in) N(0, 1), the shortcut and any
    other weight sqrt(1 / fan_in) N(0, 1)"""
    rs = np.random.RandomState(zlib.crc32(seed_name.encode()) & 0x7FFFFFFF)
    leaf = name.rsplit(".", 2)[-2]
    if "norm" in leaf and name.endswith(".weight"):
        return rs.uniform(0.75, 1.25, shape)
    if name.endswith(".bias"):
        return 0.1 * rs.standard_normal(shape)
    fan_in = int(np.prod(shape[1:]))
    behind_silu = leaf in ("conv1", "conv2", "time_emb_proj")
    return math.sqrt((2.0 if behind_silu else 1.0) / fan_in) * rs.standard_normal(shape)


def standin_state_dict(module, tag, dtype=torch.float64):
    """every value is rounded to fp16 once, here: the float64, fp32 and fp16 runs and the packed weights carry the same VALUES"""
    return OrderedDict((name, torch.from_numpy(np.asarray(standin_value("%s.%s" % (tag, name), name, tuple(v.shape)), np.float64)
                                               .astype(np.float16).astype(np.float64)).to(dtype))
                       for name, v in module.state_dict().items())


def build(cin, cout, dtype=torch.float32):
    """the restated block with its stand-in weights, in eval mode"""
    net = Resnet(cin, cout)
    net.load_state_dict(standin_state_dict(net, "%dto%d" % (cin, cout)))
    return net.to(dtype).eval()


def build_tree(dtype=torch.float32, c=320):
    net = Tree(c)
    net.load_state_dict(standin_state_dict(net, "tree%d" % c))
    return net.to(dtype).eval()


def record(case):
    """(float64 tap (n, H, W, cout), float64 output (n, H, W, cout), noise [tap, out], peak [tap, out], largest activation):
    the float64 run of the case, and the reference arithmetic's noise against it = max|difference| / max|float64| of the
    fp32 run with every layer's output rounded to fp16"""
    cin, cout = case[:2]
    x, temb = inputs(case)
    net64, net32 = build(cin, cout, torch.float64), build(cin, cout, torch.float32)
    seen = [0.0]

    def see(m, i, o):
        seen[0] = max(seen[0], float(o.detach().abs().max()))
    hooks = [m.register_forward_hook(see) for net in (net64, net32) for m in net.modules() if not list(m.children())]
    t64, t16 = {}, {}
    with torch.no_grad():
        o64 = net64(x.double(), temb.double(), taps=t64).permute(0, 2, 3, 1)
        o16 = net32(x.float(), temb.float(), round16, t16).permute(0, 2, 3, 1)
    for h in hooks:
        h.remove()
    peaks = [float(t64["tap"].abs().max()), float(o64.abs().max())]
    noise = [float((t16["tap"].double() - t64["tap"]).abs().max() / peaks[0]), float((o16.double() - o64).abs().max() / peaks[1])]
    return t64["tap"].contiguous(), o64.contiguous(), noise, peaks, max(seen[0], peaks[0], peaks[1])
