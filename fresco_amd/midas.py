"""The MiDaS depth detector behind FRESCO's ControlNet condition (`controlnet_type: depth`), batched over frames and
resident on the GPU.

Reference: src/ControlNet/annotator/midas/__init__.py -- one frame per call: host -> device copy, an fp32 forward of
MiDaSInference("dpt_hybrid") = DPTDepthModel(backbone="vitb_rn50_384", non_negative=True), two .cpu() copies, two cv2.Sobel
calls; run_fresco.py:199-202 then uploads the depth map again and builds the condition.  Here a batch of uint8 frames on the
device goes through

    ops.midas_input -> ops.midas_stem_conv -> ops.midas_groupnorm -> ops.midas_pool -> 16 bottlenecks [ops.fn_gemm x 3
    (+ 1 shortcut) on weight-standardised planes, ops.midas_groupnorm between them and for the residual add] ->
    patch_embed.proj -> ops.midas_tokens -> 12 transformer blocks [ops.midas_layernorm, q | k | v as one ops.fn_gemm,
    ops.attention_f32, ops.midas_head_merge, proj / MLP on ops.fn_gemm, ops.fn_prep for the residual adds] -> reassemble
    [readout as two products + ops.midas_rowbias_gelu] -> decoder [ops.fn_gemm 3 x 3 convolutions, ops.egnet_resize_add] ->
    head -> ops.midas_tail (normalise, uint8, Sobel normals, the condition)

with no host round trip.  The module tree carries the reference checkpoint's parameter names (`pretrained.model.*`,
`pretrained.act_postprocessK.*`, `scratch.*`), so `load_state_dict(torch.load("dpt_hybrid-midas-501f0c75.pt"))` works
unchanged, and `forward` is the reference's forward on library ops.  The backbone follows timm's vit_base_resnet50_384;
DESIGN.md section 16 has the data flow, the padding origins and what is unverified; INTEGRATION.md recipe K the two ways to
use it.
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _detector, ops
from ._detector import Act as _Act
from .fnweights import WeightPlanes

CHECKPOINT_NAME = "dpt_hybrid-midas-501f0c75.pt"
SIDE_MULTIPLE = 32  # layer 4 is the 1/16 token grid halved once more
STAGES = ("backbone", "transformer", "reassemble", "decoder")
# the tensors depth(taps=...) records, in graph order (maps NHWC fp32, tokens (n, L, 768))
TAPS = ("stem", "stage0", "stage1", "stage2", "tokens0", "tokens8", "tokens11", "layer3", "layer4", "path_4", "path_3",
        "path_2", "path_1")
HOOKS = (0, 8, 11)  # transformer blocks whose output is kept: the tap after block 0, and layers 3 and 4 of the reassemble
STD_EPS, GN_EPS, LN_EPS = 1e-8, 1e-5, 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the module tree (names and shapes of timm's vit_base_resnet50_384 and of midas/vit.py, blocks.py, dpt_depth.py)
# ---------------------------------------------------------------------------------------------------------------------
def same_padding(size, k, stride):
    """(before, after) of the "same" padding of one axis: the surplus goes after"""
    total = max((-(-size // stride) - 1) * stride + k - size, 0)
    return total // 2, total - total // 2


def standardise(w, eps=STD_EPS):
    """StdConv2dSame's weight in w's precision: (w - mean) / sqrt(biased variance + eps) per output channel"""
    m = w.mean(dim=(1, 2, 3), keepdim=True)
    return (w - m) / torch.sqrt(w.var(dim=(1, 2, 3), keepdim=True, unbiased=False) + eps)


class StdConv2dSame(nn.Conv2d):
    def __init__(self, cin, cout, k, stride=1):
        super().__init__(cin, cout, k, stride=stride, padding=0, bias=False)

    def forward(self, x):
        k, s = self.kernel_size[0], self.stride[0]
        (t, b), (l, r) = same_padding(x.shape[2], k, s), same_padding(x.shape[3], k, s)
        return F.conv2d(F.pad(x, (l, r, t, b)), standardise(self.weight), None, s)


class GroupNormAct(nn.GroupNorm):
    def __init__(self, channels, apply_act=True):
        super().__init__(32, channels, eps=GN_EPS)
        self.apply_act = apply_act

    def forward(self, x):
        x = super().forward(x)
        return F.relu(x) if self.apply_act else x


class MaxPool2dSame(nn.Module):
    def forward(self, x):
        (t, b), (l, r) = same_padding(x.shape[2], 3, 2), same_padding(x.shape[3], 3, 2)
        return F.max_pool2d(F.pad(x, (l, r, t, b), value=float("-inf")), 3, 2)


class DownsampleConv(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv = StdConv2dSame(cin, cout, 1, stride)
        self.norm = GroupNormAct(cout, apply_act=False)

    def forward(self, x):
        return self.norm(self.conv(x))


class Bottleneck(nn.Module):
    """ResNetV2's post-activation bottleneck: the stride sits on the 3 x 3 convolution"""

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
        x = self.norm3(self.conv3(self.norm2(self.conv2(self.norm1(self.conv1(x))))))
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

    def forward(self, x):
        return self.stages(self.stem(x))


class HybridEmbed(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = ResNetV2()
        self.proj = nn.Conv2d(1024, 768, 1)


class Attention(nn.Module):
    def __init__(self, dim=768, heads=12):
        super().__init__()
        self.num_heads = heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, L, C = x.shape
        q, k, v = self.qkv(x).reshape(B, L, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        attn = ((q @ k.transpose(-2, -1)) * (C // self.num_heads) ** -0.5).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(B, L, C))


class Mlp(nn.Module):
    def __init__(self, dim=768):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim=768):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = Attention(dim)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = Mlp(dim)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class VisionTransformer(nn.Module):
    """vit_base_resnet50_384 as the depth model reads it.  `norm` and `head` are in the published checkpoint and feed nothing."""

    def __init__(self):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, 768))
        self.pos_embed = nn.Parameter(torch.zeros(1, 577, 768))
        self.patch_embed = HybridEmbed()
        self.blocks = nn.Sequential(*[Block() for _ in range(12)])
        self.norm = nn.LayerNorm(768, eps=LN_EPS)
        self.head = nn.Linear(768, 1000)


class ProjectReadout(nn.Module):
    def __init__(self):
        super().__init__()
        self.project = nn.Sequential(nn.Linear(1536, 768), nn.GELU())

    def forward(self, x):
        return self.project(torch.cat((x[:, 1:], x[:, :1].expand_as(x[:, 1:])), -1))


class ResidualConvUnit(nn.Module):
    def __init__(self, features=256):
        super().__init__()
        self.conv1 = nn.Conv2d(features, features, 3, 1, 1)
        self.conv2 = nn.Conv2d(features, features, 3, 1, 1)

    def forward(self, x):
        return self.conv2(F.relu(self.conv1(F.relu(x)))) + x


def _up2(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


class FeatureFusionBlock(nn.Module):
    def __init__(self, features=256):
        super().__init__()
        self.out_conv = nn.Conv2d(features, features, 1)
        self.resConfUnit1 = ResidualConvUnit(features)
        self.resConfUnit2 = ResidualConvUnit(features)

    def forward(self, x, skip=None):
        if skip is not None:
            x = x + self.resConfUnit1(skip)
        return self.out_conv(_up2(self.resConfUnit2(x)))


class _Up2(nn.Module):
    def forward(self, x):
        return _up2(x)


class DPTDepthModel(nn.Module):
    """DPTDepthModel(backbone="vitb_rn50_384", non_negative=True).
    split_scales: the power of two each stage's activation planes are written with, one per STAGES entry.  A plane holds
    |x| * scale up to 65000: 2^6 carries activations up to 1015.  A network whose activations exceed that trips the range flag
    on every call and runs on library ops (with a warning); HALVE the scale of the stage that overflows (DESIGN.md
    section 16).
    library_ops=True (or FRESCO_MIDAS_LIBRARY_OPS=1): the same module on PyTorch's own kernels between the input and tail
    kernels -- the A/B and benchmark baseline.
    max_frames: frames per pass through the network."""

    def __init__(self, split_scales=(64.0,) * len(STAGES), library_ops=False, max_frames=8):
        super().__init__()
        if len(split_scales) != len(STAGES):
            raise ValueError("DPTDepthModel: one split scale per stage %s, got %r" % (STAGES, split_scales))
        if int(max_frames) < 1:
            raise ValueError("DPTDepthModel: max_frames %r" % (max_frames,))
        self.split_scales = tuple(ops._split_scale(s) for s in split_scales)
        self.library_ops = bool(library_ops)
        self.max_frames = int(max_frames)
        self.pretrained = nn.Module()
        self.pretrained.model = VisionTransformer()
        self.pretrained.act_postprocess3 = nn.Sequential(ProjectReadout(), nn.Identity(), nn.Identity(), nn.Conv2d(768, 768, 1))
        self.pretrained.act_postprocess4 = nn.Sequential(ProjectReadout(), nn.Identity(), nn.Identity(), nn.Conv2d(768, 768, 1),
                                                         nn.Conv2d(768, 768, 3, 2, 1))
        self.scratch = nn.Module()
        for k, c in enumerate((256, 512, 768, 768), 1):
            setattr(self.scratch, "layer%d_rn" % k, nn.Conv2d(c, 256, 3, 1, 1, bias=False))
        for k in (1, 2, 3, 4):
            setattr(self.scratch, "refinenet%d" % k, FeatureFusionBlock(256))
        self.scratch.output_conv = nn.Sequential(nn.Conv2d(256, 128, 3, 1, 1), _Up2(), nn.Conv2d(128, 32, 3, 1, 1),
                                                 nn.ReLU(True), nn.Conv2d(32, 1, 1), nn.ReLU(True), nn.Identity())
        self._wts = WeightPlanes()
        self._pos = {}
        self._rows = {}
        self._warned = False

    # ---- the reference's forward on library ops: x (n, 3, H, W) = frame / 127.5 - 1 -> depth (n, H, W) ----
    def pos_embed_for(self, gh, gw):
        """pos_embed with its 24 x 24 grid part resized to (gh, gw) (bilinear, align_corners=False): (1 + gh gw, 768).
        Weight preparation: made once per geometry and parameter version."""
        p = self.pretrained.model.pos_embed
        key = (gh, gw, p._version, p.data_ptr(), p.dtype)
        hit = self._pos.get((gh, gw))
        if hit is None or hit[0] != key:
            grid = p.detach()[0, 1:].reshape(1, 24, 24, -1).permute(0, 3, 1, 2)
            grid = F.interpolate(grid, size=(gh, gw), mode="bilinear")
            pos = torch.cat([p.detach()[0, :1], grid.permute(0, 2, 3, 1).reshape(gh * gw, -1)], dim=0).contiguous()
            hit = self._pos[(gh, gw)] = (key, pos)
        return hit[1]

    def forward(self, x, taps=None):
        taps = {} if taps is None else taps
        nhwc = lambda t: t.permute(0, 2, 3, 1).float().contiguous()  # noqa: E731
        vit, sc, pre = self.pretrained.model, self.scratch, self.pretrained
        n, _, H, W = x.shape
        gh, gw = H // 16, W // 16
        bb = vit.patch_embed.backbone
        stem = bb.stem.norm(bb.stem.conv(x))
        s0 = bb.stages[0](bb.stem.pool(stem))
        s1 = bb.stages[1](s0)
        s2 = bb.stages[2](s1)
        tok = vit.patch_embed.proj(s2).flatten(2).transpose(1, 2)
        tok = torch.cat((vit.cls_token.expand(n, -1, -1), tok), dim=1) + self.pos_embed_for(gh, gw)
        keep = {}
        for i, blk in enumerate(vit.blocks):
            tok = blk(tok)
            if i in HOOKS:
                keep[i] = tok
        layers = []
        for post, t in ((pre.act_postprocess3, keep[8]), (pre.act_postprocess4, keep[11])):
            y = post[0](t).transpose(1, 2).reshape(n, 768, gh, gw)
            for m in list(post)[3:]:
                y = m(y)
            layers.append(y)
        p4 = sc.refinenet4(sc.layer4_rn(layers[1]))
        p3 = sc.refinenet3(p4, sc.layer3_rn(layers[0]))
        p2 = sc.refinenet2(p3, sc.layer2_rn(s1))
        p1 = sc.refinenet1(p2, sc.layer1_rn(s0))
        taps.update(zip(TAPS, [nhwc(stem), nhwc(s0), nhwc(s1), nhwc(s2)] + [keep[i].float() for i in HOOKS]
                        + [nhwc(t) for t in (layers[0], layers[1], p4, p3, p2, p1)]))
        return sc.output_conv(p1).squeeze(1)

    # ---- the same graph on the HIP kernels ----
    def _scale(self, stage):
        return self.split_scales[STAGES.index(stage)]

    def _std(self, conv, kind="conv"):
        """planes of a StdConv2dSame's standardised weight, folded once per parameter version in float64"""
        return self._wts.get_prepared(conv.weight, kind, "std", lambda w: standardise(w.double()))

    def _gemm(self, a, w, cout, bias=None, act=0, k=1, stride=1, pad=0, size=None, want_f32=False, want_split=True,
              stage=None, a_rows=None):
        """one linear layer / convolution of activation `a` (its planes) -> _Act.  size: the (H, W) of the map behind the
        planes when it differs from a's (the far-side border of a "same" stride-2 convolution)"""
        scale = self._scale(stage)
        H, W = size or (a.H, a.W)
        plain = k == 1 and stride == 1
        conv = None if plain else (a.n, H, W, k, k, stride, pad)
        OH, OW = (a.H, a.W) if plain else ops.conv_out_size(H, W, k, k, stride, pad)
        out, planes = ops.fn_gemm(a.planes, w, cout, w[0].shape[1], bias=bias, act=act, conv=conv, want_f32=want_f32,
                                  want_split=want_split, a_scale=a.scale, out_scale=scale, a_rows=a_rows)
        return _Act(out, planes, scale, a.n, OH, OW, cout)

    def _norm(self, h, norm, relu, residual=None, want_f32=False, want_split=True, far_border=False):
        y, planes = ops.midas_groupnorm(h.nhwc(), norm.weight, norm.bias, relu=relu,
                                        residual=None if residual is None else residual.view(h.n, h.H, h.W, h.C),
                                        eps=norm.eps, want_f32=want_f32, want_split=want_split, far_border=far_border,
                                        scale=h.scale)
        return _Act(None if y is None else y.view(-1, h.C), planes, h.scale, h.n, h.H, h.W, h.C)

    def _bottleneck(self, blk, a):
        st, stride = "backbone", blk.conv2.stride[0]
        mid, cout = blk.conv1.out_channels, blk.conv3.out_channels
        raw = dict(want_f32=True, want_split=False, stage=st)  # a convolution's fp32 rows: GroupNorm reads them
        h = self._norm(self._gemm(a, self._std(blk.conv1), mid, **raw), blk.norm1, True, far_border=stride == 2)
        if stride == 2:  # "same": 0 before, 1 after = pad 0 on the map with norm1's far-side zero border
            h = self._gemm(h, self._std(blk.conv2), mid, k=3, stride=2, pad=0, size=(h.H + 1, h.W + 1), **raw)
        else:
            h = self._gemm(h, self._std(blk.conv2), mid, k=3, pad=1, **raw)
        h = self._norm(h, blk.norm2, True)
        h = self._gemm(h, self._std(blk.conv3), cout, **raw)
        if blk.downsample is not None:
            ds = blk.downsample
            res = self._norm(self._gemm(a, self._std(ds.conv), cout, stride=stride, **raw), ds.norm, False, want_f32=True,
                             want_split=False).f32
        else:
            res = a.f32
        return self._norm(h, blk.norm3, False, residual=res, want_f32=True)

    def _grid_rows(self, n, L, device):
        """int32 row tables of a (n L, 768) token matrix: the cls rows, and the grid rows in image order"""
        key = (n, L, device)
        if key not in self._rows:
            r = torch.arange(n * L, dtype=torch.int32, device=device).view(n, L)
            self._rows[key] = (r[:, 0].contiguous(), r[:, 1:].reshape(-1).contiguous())
        return self._rows[key]

    def _block(self, blk, x, n, L):
        wts, st = self._wts, "transformer"
        sc = self._scale(st)
        _, p = ops.midas_layernorm(x, blk.norm1.weight, blk.norm1.bias, eps=blk.norm1.eps, scale=sc)
        # q | k | v as one product: 36 head matrices (which, head) of (n L, 64) rows = the (head n, L, 64) batches of the attention
        qkv, _ = ops.fn_gemm(p, wts.get(blk.attn.qkv.weight, "lin"), 2304, 768, bias=blk.attn.qkv.bias, out_blocks=36,
                             a_scale=sc)
        heads = blk.attn.num_heads
        q, k, v = (qkv[i * heads:(i + 1) * heads].view(heads * n, L, 64) for i in range(3))
        o = ops.attention_f32(q, k, v, 0.125)
        _, p = ops.midas_head_merge(o, n, scale=sc)
        h, _ = ops.fn_gemm(p, wts.get(blk.attn.proj.weight, "lin"), 768, 768, bias=blk.attn.proj.bias, a_scale=sc)
        x, _ = ops.fn_prep(h, residual=x, want_f32=True, want_split=False)
        _, p = ops.midas_layernorm(x, blk.norm2.weight, blk.norm2.bias, eps=blk.norm2.eps, scale=sc)
        _, p = ops.fn_gemm(p, wts.get(blk.mlp.fc1.weight, "lin"), 3072, 768, bias=blk.mlp.fc1.bias, act=2, want_f32=False,
                           want_split=True, a_scale=sc, out_scale=sc)
        h, _ = ops.fn_gemm(p, wts.get(blk.mlp.fc2.weight, "lin"), 768, 3072, bias=blk.mlp.fc2.bias, a_scale=sc)
        return ops.fn_prep(h, residual=x, want_f32=True, want_split=False)[0]

    def _reassemble(self, post, tok, n, L, gh, gw):
        """ProjectReadout + the 1 x 1 convolution (+ layer 4's 3 x 3 stride-2 one) on a kept token matrix (n L, 768)"""
        wts, st = self._wts, "reassemble"
        sc = self._scale(st)
        lin = post[0].project[0]
        cls_rows, grid_rows = self._grid_rows(n, L, tok.device)
        _, tp = ops.fn_prep(tok, scale=sc)
        # cat(tokens, cls) W^T + b = tokens W[:, :768]^T + (cls W[:, 768:]^T + b): the second term is one row per image
        w_tok = wts.get_prepared(lin.weight, "lin", "readout_tokens", lambda w: w[:, :768])
        w_cls = wts.get_prepared(lin.weight, "lin", "readout_cls", lambda w: w[:, 768:])
        row, _ = ops.fn_gemm(tp, w_cls, 768, 768, bias=lin.bias, a_rows=cls_rows, a_scale=sc)
        g, _ = ops.fn_gemm(tp, w_tok, 768, 768, a_rows=grid_rows, a_scale=sc)
        _, gp = ops.midas_rowbias_gelu(g, row, L - 1, scale=sc)
        a = _Act(None, gp, sc, n, gh, gw, 768)
        last = len(post) == 4
        a = self._gemm(a, wts.get(post[3].weight, "conv"), 768, bias=post[3].bias, want_f32=last, stage=st)
        if not last:
            a = self._gemm(a, wts.get(post[4].weight, "conv"), 768, bias=post[4].bias, k=3, stride=2, pad=1, want_f32=True,
                           stage=st)
        return a

    def _rcu(self, rcu, x):
        """conv2(relu(conv1(relu(x)))) of a ResidualConvUnit WITHOUT its skip: fp32 rows"""
        st = "decoder"
        _, p = ops.fn_prep(x.f32, relu_a=True, scale=self._scale(st))
        a = _Act(None, p, self._scale(st), x.n, x.H, x.W, x.C)
        a = self._gemm(a, self._wts.get(rcu.conv1.weight, "conv"), x.C, bias=rcu.conv1.bias, act=1, k=3, pad=1, stage=st)
        return self._gemm(a, self._wts.get(rcu.conv2.weight, "conv"), x.C, bias=rcu.conv2.bias, k=3, pad=1, want_f32=True,
                          want_split=False, stage=st).f32

    def _fusion(self, blk, x, skip=None, want_split=False):
        st = "decoder"
        add = lambda a, b: ops.fn_prep(a, residual=b, want_f32=True, want_split=False)[0]  # noqa: E731
        f = x.f32
        if skip is not None:
            f = add(add(self._rcu(blk.resConfUnit1, skip), skip.f32), f)  # x + (conv2(...) + skip), the reference's order
        x = _Act(f, None, x.scale, x.n, x.H, x.W, x.C)
        x = _Act(add(self._rcu(blk.resConfUnit2, x), f), None, x.scale, x.n, x.H, x.W, x.C)
        _, up = ops.egnet_resize_add(x.nhwc(), (2 * x.H, 2 * x.W), want_f32=False, want_split=True, scale=self._scale(st))
        a = _Act(None, up, self._scale(st), x.n, 2 * x.H, 2 * x.W, x.C)
        return self._gemm(a, self._wts.get(blk.out_conv.weight, "conv"), x.C, bias=blk.out_conv.bias, want_f32=True,
                          want_split=want_split, stage=st)

    def _depth_native(self, frames, taps=None, mark=None):
        """frames (n, H, W, 3) uint8 on the GPU -> depth (n, H, W) fp32.  mark: called with "backbone", "transformer",
        "decoder" as each part has been enqueued (tools/bench_midas.py's split)"""
        mark = mark or (lambda stage: None)
        vit, sc, pre, wts = self.pretrained.model, self.scratch, self.pretrained, self._wts
        bb = vit.patch_embed.backbone
        n, H, W, _ = frames.shape
        gh, gw = H // 16, W // 16
        L = gh * gw + 1
        sb = self._scale("backbone")
        x = ops.midas_input(frames)
        y = ops.midas_stem_conv(x, self._std(bb.stem.conv, "stem"))
        stem, _ = ops.midas_groupnorm(y, bb.stem.norm.weight, bb.stem.norm.bias, relu=True, eps=bb.stem.norm.eps)
        _, pp = ops.midas_pool(stem, scale=sb)
        a = _Act(None, pp, sb, n, H // 4, W // 4, 64)
        feats = []
        for stage in bb.stages:
            for blk in stage.blocks:
                a = self._bottleneck(blk, a)
            feats.append(a)
        proj = vit.patch_embed.proj
        grid = self._gemm(a, wts.get(proj.weight, "conv"), 768, bias=proj.bias, want_f32=True, want_split=False,
                          stage="transformer").f32
        mark("backbone")
        tok = ops.midas_tokens(grid.view(n, L - 1, 768), vit.cls_token.detach().reshape(768), self.pos_embed_for(gh, gw))
        tok = tok.view(n * L, 768)
        keep = {}
        for i, blk in enumerate(vit.blocks):
            tok = self._block(blk, tok, n, L)
            if i in HOOKS:
                keep[i] = tok
            if i == HOOKS[-1]:
                break  # (the blocks after the last hook, and the final norm, feed nothing)
        mark("transformer")
        l3 = self._reassemble(pre.act_postprocess3, keep[8], n, L, gh, gw)
        l4 = self._reassemble(pre.act_postprocess4, keep[11], n, L, gh, gw)
        rn = [self._gemm(f, wts.get(getattr(sc, "layer%d_rn" % k).weight, "conv"), 256, k=3, pad=1, want_f32=True,
                         want_split=False, stage="decoder") for k, f in enumerate((feats[0], feats[1], l3, l4), 1)]
        p4 = self._fusion(sc.refinenet4, rn[3])
        p3 = self._fusion(sc.refinenet3, p4, rn[2])
        p2 = self._fusion(sc.refinenet2, p3, rn[1])
        p1 = self._fusion(sc.refinenet1, p2, rn[0], want_split=True)
        if taps is not None:
            taps.update(zip(TAPS, [stem, feats[0].nhwc(), feats[1].nhwc(), feats[2].nhwc()]
                            + [keep[i].view(n, L, 768) for i in HOOKS] + [t.nhwc() for t in (l3, l4, p4, p3, p2, p1)]))
        head = sc.output_conv
        h = self._gemm(p1, wts.get(head[0].weight, "conv"), 128, bias=head[0].bias, k=3, pad=1, want_f32=True, want_split=False,
                       stage="decoder")
        _, up = ops.egnet_resize_add(h.nhwc(), (H, W), want_f32=False, want_split=True, scale=self._scale("decoder"))
        h = _Act(None, up, self._scale("decoder"), n, H, W, 128)
        h = self._gemm(h, wts.get(head[2].weight, "conv"), 32, bias=head[2].bias, act=1, k=3, pad=1, stage="decoder")
        # 32 -> 1: one weight row; the kernel's column blocks past N read the zero page and store nothing
        d = self._gemm(h, wts.get(head[4].weight, "conv"), 1, bias=head[4].bias, act=1, want_f32=True, want_split=False,
                       stage="decoder")
        mark("decoder")
        return d.f32.view(n, H, W)

    def _depth_library(self, frames, taps=None):
        x = ops.midas_input(frames).permute(0, 3, 1, 2).to(self.pretrained.model.cls_token.dtype)
        return self.forward(x, taps).float().contiguous()

    def _use_library(self):
        return self.library_ops or os.environ.get("FRESCO_MIDAS_LIBRARY_OPS", "0") == "1"

    @torch.no_grad()
    def depth(self, frames, taps=None):
        """frames (n, H, W, 3) uint8 on the GPU -> the depth maps (n, H, W) fp32.  Frames go through the network max_frames
        at a time.  taps: a dict that receives the TAPS tensors -- of the last chunk when there are several."""
        frames = check_frames(frames)
        if not frames.is_cuda:
            raise ops.FrescoHipError("fresco_amd MiDaS runs on the GPU only (got %s frames)" % frames.device)
        chunks = [c.contiguous() for c in frames.split(self.max_frames)]
        maps = _detector.guarded_run(
            self, frames.device, lambda: [self._depth_native(c, taps) for c in chunks],
            lambda: [self._depth_library(c, taps) for c in chunks],
            "fresco_amd.midas: an activation or a weight left the range of the split-fp16 products "
            "(|activation| * split_scale < 65000, |weight| < 63); calls of this module are recomputed with library ops "
            "-- lower the stage's split scale", use_library=self._use_library())
        return maps[0] if len(maps) == 1 else torch.cat(maps, 0)

    def detect(self, frames, a=np.pi * 2.0, bg_th=0.1, cond_dtype=None):
        """-> (depth image (n, H, W) uint8, normal image (n, H, W, 3) uint8, condition (n, 3, H, W) or None)"""
        return ops.midas_tail(self.depth(frames), a, bg_th, cond_dtype=cond_dtype)


def check_frames(frames):
    """a uint8 (n, H, W, 3) tensor, or a list of (H, W, 3) uint8 ndarrays of one size -> the uint8 (n, H, W, 3) tensor
    (on the host for ndarrays: the caller moves it).  The sides must be multiples of 32: the token grid is the frame / 16
    and layer 4 halves it once more (FRESCO resizes its frames to multiples of 64)."""
    return _detector.check_frames(frames, "MiDaS", multiple=SIDE_MULTIPLE)


def condition_dtype(dtype):
    return _detector.condition_dtype(dtype, "MiDaS")


def load_checkpoint(network, path):
    """the reference's BaseModel.load: a plain state dict, or a training checkpoint with the weights under "model" """
    parameters = torch.load(path, map_location="cpu")
    if "optimizer" in parameters:
        parameters = parameters["model"]
    network.load_state_dict(parameters, strict=True)
    return network


class MidasDetector:
    """Drop-in for annotator.midas.MidasDetector: `detector(img, a, bg_th)` takes an (H, W, 3) uint8 RGB array and returns
    (depth_image (H, W) uint8, normal_image (H, W, 3) uint8), so the reference's apply_control works unchanged.  Nothing is
    downloaded: the checkpoint is read from `model_path`, or from the reference's `annotator_ckpts_path` when that package is
    importable; pass `network=` to use a module that already holds its weights.  max_frames: frames per pass through the
    network; None keeps the module's own value."""

    def __init__(self, model_path=None, *, network=None, max_frames=None):
        if network is None:
            path = model_path or _detector.default_checkpoint(CHECKPOINT_NAME)
            if path is None or not os.path.exists(path):
                raise FileNotFoundError(
                    "fresco_amd.MidasDetector: no checkpoint%s. Put %s (lllyasviel/ControlNet, annotator/ckpts) into the "
                    "reference's src/ControlNet/annotator/ckpts/ or pass model_path=; this package downloads nothing."
                    % ("" if path is None else " at %s" % path, CHECKPOINT_NAME))
            network = load_checkpoint(DPTDepthModel(), path).float().cuda()
        if max_frames is not None:
            if int(max_frames) < 1:
                raise ValueError("MidasDetector: max_frames %r" % (max_frames,))
            network.max_frames = int(max_frames)
        self.model = network.eval()

    def _device(self):
        return self.model.pretrained.model.cls_token.device

    def detect_batch(self, frames, a=np.pi * 2.0, bg_th=0.1):
        """frames: uint8 (n, H, W, 3) tensor or a list of (H, W, 3) uint8 arrays -> (depth images (n, H, W) uint8, normal
        images (n, H, W, 3) uint8), on the GPU"""
        return self.model.detect(check_frames(frames).to(self._device()), a, bg_th)[:2]

    def control_image(self, frames, dtype, guidance=True):
        """The ControlNet condition run_fresco.py:199-202 builds from the frames' depth maps:
        cat([numpy2tensor(d[:, :, None]) ...]).repeat(1, 3, 1, 1) * 0.5 + 0.5 -> .to(dtype) [-> cat x 2 under
        classifier-free guidance]: (2n | n, 3, H, W)."""
        dtype = condition_dtype(dtype)
        cond = self.model.detect(check_frames(frames).to(self._device()), cond_dtype=dtype)[2]
        return torch.cat([cond] * 2) if guidance else cond

    def __call__(self, input_image, a=np.pi * 2.0, bg_th=0.1):
        assert input_image.ndim == 3
        depth, normal = self.detect_batch([np.ascontiguousarray(input_image)], a, bg_th)
        return depth[0].cpu().numpy(), normal[0].cpu().numpy()


def patch_midas(module=None):
    """Rebind MidasDetector on the reference's annotator.midas (default) or on a module that imported the name from it
    (run_fresco, webUI): `detector = MidasDetector()` then builds this package's."""
    if module is None:
        import annotator.midas as module
    module.MidasDetector = MidasDetector
    return module
