"""Stand-ins and restatements shared by tests/golden/make_midas_golden.py, tests/test_midas_cpu.py and tests/test_gpu_midas.py.

A torch restatement of the MiDaS depth annotator (src/ControlNet/annotator/midas: MidasDetector around
DPTDepthModel(backbone="vitb_rn50_384", non_negative=True)), written from its description:

  * the backbone is `timm`'s vit_base_resnet50_384 -- a ResNetV2 (layers 3, 4, 9; weight-standardised "same" convolutions,
    GroupNorm(32)) in front of a ViT-B.  `timm` is NOT installed where these tests run, so `VisionTransformer` below (and
    everything under it) is a restatement that could not be compared with the real module: parameter names, the padding
    origins, eps values and the block layout are taken from timm's published source and are UNVERIFIED here.  The golden
    file is the reference's own reassemble / decoder / head code (vit.py, blocks.py, dpt_depth.py) around this restated
    backbone; `DPT` below restates those files as well, and tests/test_midas_cpu.py holds it against that record.
  * `cv2` is not installed either: `sobel` restates cv2.Sobel(src, CV_32F, dx, dy, ksize=3) (separable [-1 0 1] x [1 2 1],
    BORDER_REFLECT_101, fp32) and `tail` the lines after the network of annotator/midas/__init__.py; where cv2 can be
    imported tests/test_midas_cpu.py compares the two.
  * weights: closed-form stand-ins seeded by parameter name (`standin_state_dict`), drawn in float64 and cast, scaled so that
    every activation stays below half of what the operand planes hold at scale 64 (the golden maker asserts it).
  * frames: hed_model.frames(case).
"""
import math
import os
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import hed_model

CASES = [(2, 64, 96), (1, 128, 64), (1, 192, 256), (1, 256, 320)]
GOLDEN_FILE = "midas_golden.npz"
# the recorded taps, in graph order (NHWC for maps, (n, L, C) for tokens)
TAPS = ("stem", "stage0", "stage1", "stage2", "tokens0", "tokens8", "tokens11", "layer3", "layer4", "path_4", "path_3",
        "path_2", "path_1")
TAP_STRIDE = 16    # the golden file keeps every 16th channel of a tap ...
TAP_VALUES = 768   # ... and, of a map, the rows and columns of a stride that leaves about this many values per frame
FULL_DEPTH_CASES = CASES[:2]  # the file keeps the whole fp32 depth of these: `tail` is held to the detector's own maps on it
DEPTH_STRIDE = 4   # rows / columns of the fp32 depth the file keeps (the last ones always)
A, BG_TH = np.pi * 2.0, 0.1
SEED_SALT = ""

frames = hed_model.frames
digest = hed_model.digest


def case_key(case):
    return "midas_%dx%dx%d" % case


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN_FILE)))


def _picks(size, stride):
    return np.unique(np.r_[0:size:stride, size - 1])


def thin(t):
    """a tap as the golden file keeps it.  t: a (n, H, W, C) map or (n, L, C) tokens, torch or numpy -> numpy: every
    TAP_STRIDE-th channel; maps additionally at every s-th row and column plus the last ones, tokens at every s-th token
    (the cls token first) plus the last one, s the smallest stride that leaves at most TAP_VALUES values per frame"""
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    t = t[..., ::TAP_STRIDE]
    if t.ndim == 4:
        _, H, W, C = t.shape
        s = max(1, int(math.ceil(math.sqrt(H * W * C / float(TAP_VALUES)))))
        t = t[:, _picks(H, s)][:, :, _picks(W, s)]
    else:
        _, L, C = t.shape
        t = t[:, _picks(L, max(1, int(math.ceil(L * C / float(TAP_VALUES)))))]
    return np.ascontiguousarray(t)


def thin_depth(d):
    d = d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d)
    return np.ascontiguousarray(d[:, _picks(d.shape[1], DEPTH_STRIDE)][:, :, _picks(d.shape[2], DEPTH_STRIDE)])


# ---------------------------------------------------------------------------------------------------------------------
# the backbone (timm: resnetv2.py, vision_transformer.py, vision_transformer_hybrid.py), restated
# ---------------------------------------------------------------------------------------------------------------------
def same_pad(size, k, stride):
    """(before, after) of TensorFlow's "same" padding of one axis"""
    total = max((-(-size // stride) - 1) * stride + k - size, 0)
    return total // 2, total - total // 2


def standardise(w, eps=1e-8):
    """StdConv2dSame's weight: per output channel, (w - mean) / sqrt(biased variance + eps) over (cin, kh, kw)"""
    m = w.mean(dim=(1, 2, 3), keepdim=True)
    v = w.var(dim=(1, 2, 3), keepdim=True, unbiased=False)
    return (w - m) / torch.sqrt(v + eps)


class StdConv2dSame(nn.Conv2d):
    def __init__(self, cin, cout, k, stride=1, eps=1e-8):
        super().__init__(cin, cout, k, stride=stride, padding=0, bias=False)
        self.eps = eps

    def forward(self, x):
        k, s = self.kernel_size[0], self.stride[0]
        (t, b), (l, r) = same_pad(x.shape[2], k, s), same_pad(x.shape[3], k, s)
        return F.conv2d(F.pad(x, (l, r, t, b)), standardise(self.weight, self.eps), None, s)


class GroupNormAct(nn.GroupNorm):
    def __init__(self, c, apply_act=True):
        super().__init__(32, c, eps=1e-5)
        self.apply_act = apply_act

    def forward(self, x):
        x = F.group_norm(x, self.num_groups, self.weight, self.bias, self.eps)
        return F.relu(x) if self.apply_act else x


class MaxPool2dSame(nn.Module):
    def forward(self, x):
        (t, b), (l, r) = same_pad(x.shape[2], 3, 2), same_pad(x.shape[3], 3, 2)
        return F.max_pool2d(F.pad(x, (l, r, t, b), value=float("-inf")), 3, 2)


class DownsampleConv(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv = StdConv2dSame(cin, cout, 1, stride)
        self.norm = GroupNormAct(cout, apply_act=False)

    def forward(self, x):
        return self.norm(self.conv(x))


class Bottleneck(nn.Module):
    def __init__(self, cin, cout, stride, project):
        super().__init__()
        mid = cout // 4
        self.downsample = DownsampleConv(cin, cout, stride) if project else None
        self.conv1 = StdConv2dSame(cin, mid, 1)
        self.norm1 = GroupNormAct(mid)
        self.conv2 = StdConv2dSame(mid, mid, 3, stride)
        self.norm2 = GroupNormAct(mid)
        self.conv3 = StdConv2dSame(mid, cout, 1)
        self.norm3 = GroupNormAct(cout, apply_act=False)

    def forward(self, x):
        shortcut = x if self.downsample is None else self.downsample(x)
        x = self.norm1(self.conv1(x))
        x = self.norm2(self.conv2(x))
        x = self.norm3(self.conv3(x))
        return F.relu(x + shortcut)


class ResNetStage(nn.Module):
    def __init__(self, cin, cout, stride, depth):
        super().__init__()
        self.blocks = nn.Sequential(*[Bottleneck(cin if b == 0 else cout, cout, stride if b == 0 else 1, b == 0)
                                      for b in range(depth)])

    def forward(self, x):
        return self.blocks(x)


class ResNetV2(nn.Module):
    def __init__(self, layers=(3, 4, 9)):
        super().__init__()
        self.stem = nn.Sequential(OrderedDict([("conv", StdConv2dSame(3, 64, 7, 2)), ("norm", GroupNormAct(64)),
                                               ("pool", MaxPool2dSame())]))
        stages, cin = [], 64
        for cout, stride, depth in zip((256, 512, 1024), (1, 2, 2), layers):
            stages.append(ResNetStage(cin, cout, stride, depth))
            cin = cout
        self.stages = nn.Sequential(*stages)
        self.norm = nn.Identity()

    def forward(self, x):
        return self.norm(self.stages(self.stem(x)))


class HybridEmbed(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = ResNetV2()
        self.proj = nn.Conv2d(1024, 768, 1)


class Attention(nn.Module):
    def __init__(self, dim=768, heads=12):
        super().__init__()
        self.num_heads, self.scale = heads, (dim // heads) ** -0.5
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, L, C = x.shape
        q, k, v = self.qkv(x).reshape(B, L, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        attn = ((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(B, L, C))


class Mlp(nn.Module):
    def __init__(self, dim=768):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim=768):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class VisionTransformer(nn.Module):
    """vit_base_resnet50_384: what the reference's forward_flex reads of it (cls_token, pos_embed, patch_embed.backbone / proj,
    pos_drop, blocks, norm) plus the classifier `head`, which the published checkpoint carries and nothing runs"""

    def __init__(self):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, 768))
        self.pos_embed = nn.Parameter(torch.zeros(1, 577, 768))
        self.patch_embed = HybridEmbed()
        self.pos_drop = nn.Identity()
        self.blocks = nn.Sequential(*[Block() for _ in range(12)])
        self.norm = nn.LayerNorm(768, eps=1e-6)
        self.head = nn.Linear(768, 1000)


def resize_pos_embed(pos, gh, gw):
    grid = pos[0, 1:].reshape(1, 24, 24, -1).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bilinear")
    return torch.cat([pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, gh * gw, -1)], dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# reassemble, decoder and head (vit.py, blocks.py, dpt_depth.py), restated
# ---------------------------------------------------------------------------------------------------------------------
class ProjectReadout(nn.Module):
    def __init__(self):
        super().__init__()
        self.project = nn.Sequential(nn.Linear(1536, 768), nn.GELU())

    def forward(self, x):
        return self.project(torch.cat((x[:, 1:], x[:, :1].expand_as(x[:, 1:])), -1))


class RCU(nn.Module):
    def __init__(self, c=256):
        super().__init__()
        self.conv1 = nn.Conv2d(c, c, 3, 1, 1)
        self.conv2 = nn.Conv2d(c, c, 3, 1, 1)

    def forward(self, x):
        return self.conv2(F.relu(self.conv1(F.relu(x)))) + x


class Fusion(nn.Module):
    def __init__(self, c=256):
        super().__init__()
        self.out_conv = nn.Conv2d(c, c, 1)
        self.resConfUnit1 = RCU(c)
        self.resConfUnit2 = RCU(c)

    def forward(self, x, skip=None):
        if skip is not None:
            x = x + self.resConfUnit1(skip)
        x = self.resConfUnit2(x)
        return self.out_conv(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True))


class Upsample2(nn.Module):
    def forward(self, x):
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


class DPT(nn.Module):
    """DPTDepthModel(backbone="vitb_rn50_384", non_negative=True) with the reference's state-dict names; forward(x, taps)
    fills `taps` with the TAPS tensors (maps as NHWC) and returns the depth (n, H, W)"""

    def __init__(self):
        super().__init__()
        self.pretrained = nn.Module()
        self.pretrained.model = VisionTransformer()
        ident = lambda: nn.Sequential(nn.Identity(), nn.Identity(), nn.Identity())  # noqa: E731
        self.pretrained.act_postprocess1, self.pretrained.act_postprocess2 = ident(), ident()
        self.pretrained.act_postprocess3 = nn.Sequential(ProjectReadout(), nn.Identity(), nn.Identity(), nn.Conv2d(768, 768, 1))
        self.pretrained.act_postprocess4 = nn.Sequential(ProjectReadout(), nn.Identity(), nn.Identity(), nn.Conv2d(768, 768, 1),
                                                         nn.Conv2d(768, 768, 3, 2, 1))
        self.scratch = nn.Module()
        for k, c in enumerate((256, 512, 768, 768), 1):
            setattr(self.scratch, "layer%d_rn" % k, nn.Conv2d(c, 256, 3, 1, 1, bias=False))
        for k in (1, 2, 3, 4):
            setattr(self.scratch, "refinenet%d" % k, Fusion())
        self.scratch.output_conv = nn.Sequential(nn.Conv2d(256, 128, 3, 1, 1), Upsample2(), nn.Conv2d(128, 32, 3, 1, 1),
                                                 nn.ReLU(), nn.Conv2d(32, 1, 1), nn.ReLU(), nn.Identity())

    def forward(self, x, taps=None):
        taps = {} if taps is None else taps
        nhwc = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
        vit, sc = self.pretrained.model, self.scratch
        n, _, H, W = x.shape
        gh, gw = H // 16, W // 16
        bb = vit.patch_embed.backbone
        stem = bb.stem.norm(bb.stem.conv(x))
        taps["stem"] = nhwc(stem)
        s0 = bb.stages[0](bb.stem.pool(stem))
        s1 = bb.stages[1](s0)
        s2 = bb.stages[2](s1)
        taps.update(stage0=nhwc(s0), stage1=nhwc(s1), stage2=nhwc(s2))
        tok = vit.patch_embed.proj(s2).flatten(2).transpose(1, 2)
        tok = torch.cat((vit.cls_token.expand(n, -1, -1), tok), dim=1) + resize_pos_embed(vit.pos_embed, gh, gw)
        keep = {}
        for i, blk in enumerate(vit.blocks):
            tok = blk(tok)
            if i in (0, 8, 11):
                keep[i] = taps["tokens%d" % i] = tok
        layers = []
        for post, t in ((self.pretrained.act_postprocess3, keep[8]), (self.pretrained.act_postprocess4, keep[11])):
            y = post[0](t).transpose(1, 2).reshape(n, 768, gh, gw)
            for m in list(post)[3:]:
                y = m(y)
            layers.append(y)
        taps.update(layer3=nhwc(layers[0]), layer4=nhwc(layers[1]))
        p4 = sc.refinenet4(sc.layer4_rn(layers[1]))
        p3 = sc.refinenet3(p4, sc.layer3_rn(layers[0]))
        p2 = sc.refinenet2(p3, sc.layer2_rn(s1))
        p1 = sc.refinenet1(p2, sc.layer1_rn(s0))
        taps.update(path_4=nhwc(p4), path_3=nhwc(p3), path_2=nhwc(p2), path_1=nhwc(p1))
        return sc.output_conv(p1).squeeze(1)


# ---------------------------------------------------------------------------------------------------------------------
# stand-in weights
# ---------------------------------------------------------------------------------------------------------------------
def _rs(name):
    return np.random.RandomState(zlib.crc32((SEED_SALT + name).encode()) & 0x7FFFFFFF)


def standin_value(name, shape):
    """float64 stand-in of one parameter.  Norm scales U(0.75, 1.25) (x 0.5 on every norm3: nine residual blocks must not
    double the stream each), norm shifts and biases 0.1 N(0, 1); standardised convolutions N(0, 1) (their scale is
    normalised away); tokens 0.3 N(0, 1); every other weight sqrt(g / fan_in) N(0, 1), g = 2 in front of a ReLU (the decoder's
    3 x 3 convolutions, the head) and 1 elsewhere; the last convolution's weights are |.|: on mixed signs the final ReLU cuts
    nearly the whole depth map to zero."""
    rs = _rs(name)
    leaf = name.rsplit(".", 2)
    is_norm = ".norm" in name and "backbone" in name or ".norm1." in name or ".norm2." in name or name.startswith("pretrained.model.norm.")
    if name.endswith(("cls_token", "pos_embed")):
        return 0.3 * rs.standard_normal(shape)
    if is_norm and name.endswith(".weight"):
        return rs.uniform(0.75, 1.25, shape) * (0.5 if ".norm3." in name else 1.0)
    if name == "scratch.output_conv.4.weight":
        return np.abs(math.sqrt(1.0 / shape[1]) * rs.standard_normal(shape))
    if name.endswith(".bias"):
        return 0.1 * rs.standard_normal(shape)
    if "backbone" in name:
        return rs.standard_normal(shape)
    fan_in = int(np.prod(shape[1:]))
    gain = 2.0 if (name.startswith("scratch.") and "out_conv" not in name and len(shape) == 4 and shape[2] == 3) or \
        leaf[-2:] == ["fc1", "weight"] else 1.0
    return math.sqrt(gain / fan_in) * rs.standard_normal(shape)


def standin_state_dict(names_shapes, dtype=torch.float32):
    """names_shapes: iterable of (name, shape) -- a module's state dict, or the golden file's list"""
    return OrderedDict((name, torch.from_numpy(np.asarray(standin_value(name, tuple(shape)), np.float64)).to(dtype))
                       for name, shape in names_shapes)


def module_names_shapes(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def build(dtype=torch.float32):
    """the restated network with its stand-in weights, in eval mode"""
    net = DPT()
    net.load_state_dict(standin_state_dict(module_names_shapes(net)))
    return net.to(dtype).eval()


# ---------------------------------------------------------------------------------------------------------------------
# input and tail (annotator/midas/__init__.py)
# ---------------------------------------------------------------------------------------------------------------------
def network_input(frames_u8, dtype=torch.float32):
    """x / 127.5 - 1 as NCHW: in fp32 the reference's own two roundings; in float64 the same expression"""
    x = torch.from_numpy(np.asarray(frames_u8)).to(dtype)
    return (x / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()


def _reflect101(a, axis):
    first, second = np.take(a, [1], axis), np.take(a, [a.shape[axis] - 2], axis)
    return np.concatenate([first, a, second], axis)


def sobel(d, dx, dy):
    """cv2.Sobel(d, cv2.CV_32F, dx, dy, ksize=3) for (dx, dy) = (1, 0) or (0, 1) on a 2-D array, in d's precision: [-1 0 1]
    along the derivative's axis, then [1 2 1] across it as (a + c) + 2 b; BORDER_REFLECT_101; no scale, no delta"""
    assert (dx, dy) in ((1, 0), (0, 1)) and d.ndim == 2
    two = d.dtype.type(2)
    if dx == 1:
        p = _reflect101(d, 1)
        r = _reflect101(p[:, 2:] - p[:, :-2], 0)
        return (r[:-2] + r[2:]) + two * r[1:-1]
    p = _reflect101(d, 1)
    s = _reflect101((p[:, :-2] + p[:, 2:]) + two * p[:, 1:-1], 0)
    return s[2:] - s[:-2]


def tail(depth, a=A, bg_th=BG_TH, sobel_fn=None):
    """one frame's depth (H, W) float32 -> (depth_image uint8 (H, W), normal_image uint8 (H, W, 3)): the reference's lines,
    numpy float32 throughout.  A constant frame gives zeros and the flat normal (the reference divides by zero)."""
    sobel_fn = sobel_fn or (lambda d, dx, dy: sobel(d, dx, dy))
    depth = np.asarray(depth)
    f = depth.dtype.type
    pt = depth - depth.min()
    top = pt.max()
    pt = pt / top if top > 0 else np.zeros_like(pt)
    depth_image = (pt * f(255.0)).clip(0, 255).astype(np.uint8)
    x, y = sobel_fn(depth, 1, 0), sobel_fn(depth, 0, 1)
    z = np.ones_like(x) * f(a)
    x[pt < f(bg_th)] = 0
    y[pt < f(bg_th)] = 0
    normal = np.stack([x, y, z], axis=2)
    normal = normal / np.sqrt((normal[..., 0] ** 2 + normal[..., 1] ** 2) + normal[..., 2] ** 2)[..., None]
    return depth_image, (normal * f(127.5) + f(127.5)).clip(0, 255).astype(np.uint8)
