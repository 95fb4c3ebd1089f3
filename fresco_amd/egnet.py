"""The EGNet saliency detector behind FRESCO's background smoothing (`use_salinecy: True` in every shipped config), batched
over frames and resident on the GPU.

Reference: src/utils.py:96-102 `get_saliency` around src/EGNet/model.py (ResNet-50 backbone, src/EGNet/resnet.py) -- frame by
frame: host `cv2sod`, upload, 103 fp32 convolutions with every side head, sigmoid, `Dilate`.  `get_saliency` reads
`up_sal_final[-1]` alone, so here a batch of uint8 frames on the device goes through the LIVE part of the graph only,

    ops.egnet_input -> ops.fn_conv7_rgb (stem) -> ops.egnet_pool -> 16 bottlenecks [ops.fn_gemm x 3 (+ 1 shortcut),
    BatchNorm folded into weights and bias, ops.fn_prep for the residual add] -> convert -> merge1 / merge2
    [ops.fn_gemm 3 x 3, 5 x 5, 7 x 7 convolutions, ops.egnet_resize_add between the scales] -> ops.egnet_saliency

93 of the 103 convolutions, with no host round trip.  The module tree carries the reference's parameter and buffer names, so
`build_model('resnet').load_state_dict(torch.load(sod_path))` works unchanged, and `forward` is the reference's forward on
library ops (all three outputs).  DESIGN.md section 13 has the data flow and the range policy; INTEGRATION.md recipe H the
two ways to use it.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _detector, ops
from ._detector import Act as _Act
from .fnweights import WeightPlanes

MIN_SIDE = 32  # layer3 / layer4 of a 32-pixel side are 2 pixels
STAGES = ("stem", "layer1", "layer2", "layer3", "layer4", "convert", "merge1", "merge2")
# the tensors saliency_logit(taps=...) records, in graph order (NHWC fp32)
TAPS = ("stem", "layer1", "layer2", "layer3", "layer4", "convert0", "convert1", "convert2", "convert3", "convert4",
        "edge_feature", "sal_feature0", "sal_feature1", "sal_feature2", "sal_feature3", "tmp_fea")

CONVERT = ((64, 256, 512, 1024, 2048), (128, 256, 512, 512, 512))
# (channels, channels of the deeper feature that is projected down or 0, channels out, kernel, padding) per scale
MERGE1 = ((128, 256, 128, 3, 1), (256, 512, 256, 3, 1), (512, 0, 512, 5, 2), (512, 0, 512, 5, 2), (512, 0, 512, 7, 3))
MERGE2 = ((128,), (256, 512, 512, 512))
MERGE2_KERNELS = ((3, 1), (5, 2), (5, 2), (7, 3))


# ---------------------------------------------------------------------------------------------------------------------
# the module tree (names and shapes of src/EGNet/resnet.py and model.py)
# ---------------------------------------------------------------------------------------------------------------------
class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation_=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=stride, bias=False)  # (the stride sits on conv1)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=dilation_, bias=False, dilation=dilation_)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride
        for bn in (self.bn1, self.bn2, self.bn3):
            for p in bn.parameters():
                p.requires_grad = False

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        residual = x if self.downsample is None else self.downsample(x)
        return self.relu(out + residual)


class ResNet(nn.Module):
    """ResNet-50 as EGNet uses it: ceil-mode pooling, the stride on each block's first 1 x 1 convolution, layer4 at stride 1
    with dilation 2; forward returns the stem and the four layers' outputs"""

    def __init__(self, layers=(3, 4, 6, 3)):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        for p in self.bn1.parameters():
            p.requires_grad = False
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1, ceil_mode=True)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=1, dilation=2)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, 0.01)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make_layer(self, planes, blocks, stride=1, dilation=1):
        downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                                   nn.BatchNorm2d(planes * 4))
        for p in downsample[1].parameters():
            p.requires_grad = False
        layers = [Bottleneck(self.inplanes, planes, stride, dilation_=dilation, downsample=downsample)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.inplanes, planes, dilation_=dilation))
        return nn.Sequential(*layers)

    def forward(self, x):
        out = []
        x = self.relu(self.bn1(self.conv1(x)))
        out.append(x)
        x = self.maxpool(x)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            x = layer(x)
            out.append(x)
        return out


def resnet50():
    return ResNet((3, 4, 6, 3))


def _conv_relu(cin, cout):
    return nn.Sequential(nn.Conv2d(cin, cout, 1, 1, bias=False), nn.ReLU(inplace=True))


def _three_convs(cin, cout, k, pad):
    return nn.Sequential(nn.Conv2d(cin, cout, k, 1, pad), nn.ReLU(inplace=True), nn.Conv2d(cout, cout, k, 1, pad),
                         nn.ReLU(inplace=True), nn.Conv2d(cout, cout, k, 1, pad), nn.ReLU(inplace=True))


def _resize(x, size):
    return F.interpolate(x, size, mode="bilinear", align_corners=True)


class ConvertLayer(nn.Module):
    def __init__(self, list_k=CONVERT):
        super().__init__()
        self.convert0 = nn.ModuleList([_conv_relu(a, b) for a, b in zip(*list_k)])

    def forward(self, list_x):
        return [conv(x) for conv, x in zip(self.convert0, list_x)]


class MergeLayer1(nn.Module):
    """top-down saliency features (deepest first) and, from the deepest of them, the edge feature at the stem's scale"""

    def __init__(self, list_k=MERGE1):
        super().__init__()
        self.list_k = list_k
        trans = [_conv_relu(ik[1], ik[0]) for ik in list_k if ik[1] > 0]
        trans.append(_conv_relu(512, 128))
        up = [_three_convs(ik[0], ik[2], ik[3], ik[4]) for ik in list_k]
        score = [nn.Conv2d(ik[2], 1, 3, 1, 1) for ik in list_k]
        self.trans, self.up, self.score = nn.ModuleList(trans), nn.ModuleList(up), nn.ModuleList(score)
        self.relu = nn.ReLU()

    def forward(self, list_x, x_size):
        up_edge, up_sal, edge_feature, sal_feature = [], [], [], []
        num_f = len(list_x)
        u = self.up[num_f - 1](list_x[num_f - 1])
        sal_feature.append(u)
        up_sal.append(_resize(self.score[num_f - 1](u), x_size))
        for i in range(num_f - 2, 0, -1):
            if list_x[i].size(1) < u.size(1):
                u = self.trans[i](u)
            u = self.up[i](list_x[i] + _resize(u, list_x[i].shape[2:]))
            sal_feature.append(u)
            up_sal.append(_resize(self.score[i](u), x_size))
        e = self.up[0](list_x[0] + _resize(self.trans[-1](sal_feature[0]), list_x[0].shape[2:]))
        edge_feature.append(e)
        up_edge.append(_resize(self.score[0](e), x_size))
        return up_edge, edge_feature, up_sal, sal_feature


class MergeLayer2(nn.Module):
    """every saliency feature brought to the edge feature's scale and refined there; their running sum gives the final map"""

    def __init__(self, list_k=MERGE2):
        super().__init__()
        self.list_k = list_k
        trans, up, score = [], [], []
        for i in list_k[0]:
            trans.append(nn.ModuleList([_conv_relu(j, i) for j in list_k[1]]))
            up.append(nn.ModuleList([_three_convs(i, i, k, p) for (k, p), _ in zip(MERGE2_KERNELS, list_k[1])]))
            score.append(nn.ModuleList([nn.Conv2d(i, 1, 3, 1, 1) for _ in list_k[1]]))
        self.trans, self.up, self.score = nn.ModuleList(trans), nn.ModuleList(up), nn.ModuleList(score)
        c = list_k[0][0]
        self.final_score = nn.Sequential(nn.Conv2d(c, c, 5, 1, 2), nn.ReLU(inplace=True), nn.Conv2d(c, 1, 3, 1, 1))
        self.relu = nn.ReLU()

    def forward(self, list_x, list_y, x_size):
        up_score, feats = [], []
        list_y = list_y[::-1]
        for i, i_x in enumerate(list_x):
            for j, j_x in enumerate(list_y):
                f = self.up[i][j](_resize(self.trans[i][j](j_x), i_x.shape[2:]) + i_x)
                up_score.append(_resize(self.score[i][j](f), x_size))
                feats.append(f)
        fea = feats[0]
        for f in feats[1:]:
            fea = self.relu(torch.add(fea, _resize(f, feats[0].shape[2:])))
        up_score.append(_resize(self.final_score(fea), x_size))
        return up_score


class TUN_bone(nn.Module):
    """split_scales: the power of two each stage's activation planes are written with, one per STAGES entry (stem, layer1-4,
    convert, merge1, merge2).  A plane holds |x| * scale up to 65000: 2^6 carries activations up to 1015.  A network whose
    activations exceed that trips the range flag on every call and runs on library ops (with a warning); HALVE the scale
    of the stage that overflows -- each halving doubles the range and raises the smallest exactly-carried magnitude likewise
    (DESIGN.md section 13).
    library_ops=True (or FRESCO_EGNET_LIBRARY_OPS=1): the live graph on PyTorch's convolutions, pooling and interpolation,
    between the same input and tail kernels -- the A/B and benchmark baseline.
    max_frames: frames per pass through the network."""

    def __init__(self, base_model_cfg="resnet", split_scales=(64.0,) * len(STAGES), library_ops=False, max_frames=8):
        super().__init__()
        if base_model_cfg != "resnet":
            raise NotImplementedError("fresco_amd.egnet: the %r backbone (FRESCO runs EGNet on 'resnet')" % (base_model_cfg,))
        if len(split_scales) != len(STAGES):
            raise ValueError("TUN_bone: one split scale per stage %s, got %r" % (STAGES, split_scales))
        if int(max_frames) < 1:
            raise ValueError("TUN_bone: max_frames %r" % (max_frames,))
        self.base_model_cfg = base_model_cfg
        self.split_scales = tuple(ops._split_scale(s) for s in split_scales)
        self.library_ops = bool(library_ops)
        self.max_frames = int(max_frames)
        self.convert = ConvertLayer()
        self.base = resnet50()
        self.merge1 = MergeLayer1()
        self.merge2 = MergeLayer2()
        self._wts = WeightPlanes()
        self._warned = False

    def forward(self, x):
        """the reference's forward: x (n, 3, h, w) = cv2sod's tensor -> (up_edge, up_sal, up_sal_final); library ops"""
        x_size = x.shape[2:]
        feats = self.convert(self.base(x))
        up_edge, edge_feature, up_sal, sal_feature = self.merge1(feats, x_size)
        return up_edge, up_sal, self.merge2(edge_feature, sal_feature, x_size)

    # ---- the live graph: what up_sal_final[-1] depends on (no side scores, no merge1.trans[0]) ----
    def live_logit(self, x, taps=None, resize=True):
        """x (n, 3, h, w) -> up_sal_final[-1] (n, 1, h, w) on library ops, through the live graph alone (resize=False: the
        final score at the stem's scale, before its resize).  taps: a dict that receives the TAPS tensors as NCHW"""
        m1, m2 = self.merge1, self.merge2
        base = self.base(x)
        cv = self.convert(base)
        sal = [m1.up[4](cv[4])]
        u = sal[0]
        for i in (3, 2, 1):
            if cv[i].size(1) < u.size(1):
                u = m1.trans[i](u)
            u = m1.up[i](cv[i] + _resize(u, cv[i].shape[2:]))
            sal.append(u)
        edge = m1.up[0](cv[0] + _resize(m1.trans[-1](sal[0]), cv[0].shape[2:]))
        fea = None
        for j, y in enumerate(sal[::-1]):
            f = m2.up[0][j](_resize(m2.trans[0][j](y), edge.shape[2:]) + edge)
            fea = f if fea is None else F.relu(fea + f)
        if taps is not None:
            taps.update(zip(TAPS, base + cv + [edge] + sal + [fea]))
        score = m2.final_score(fea)
        return _resize(score, x.shape[2:]) if resize else score

    # ---- the same graph on the HIP kernels ----
    def _scale(self, stage):
        return self.split_scales[STAGES.index(stage)]

    def _conv(self, a, planes_bias, cout, k=1, stride=1, pad=0, dilation=1, relu=True, want_f32=False, want_split=True,
              stage=None):
        """one convolution of activation `a` (its planes) -> _Act; 1 x 1 / stride 1 as a plain product"""
        (w, bias), scale = planes_bias, self._scale(stage)
        plain = k == 1 and stride == 1
        OH, OW = ops.conv_out_size(a.H, a.W, k, k, stride, pad, dilation)
        out, planes = ops.fn_gemm(a.planes, w, cout, w[0].shape[1], bias=bias, act=1 if relu else 0,
                                  conv=None if plain else (a.n, a.H, a.W, k, k, stride, pad, dilation), want_f32=want_f32,
                                  want_split=want_split, a_scale=a.scale, out_scale=scale)
        return _Act(out, planes, scale, a.n, OH, OW, cout)

    def _own(self, conv):
        """planes and bias of a convolution that carries its own (or no) bias"""
        return self._wts.get(conv.weight, "conv"), conv.bias

    def _bottleneck(self, blk, a, stage):
        wts = self._wts
        dil = blk.conv2.dilation[0]
        h = self._conv(a, wts.get_folded(blk.conv1.weight, blk.bn1, "conv"), blk.conv1.out_channels, stride=blk.stride,
                       stage=stage)
        h = self._conv(h, wts.get_folded(blk.conv2.weight, blk.bn2, "conv"), blk.conv2.out_channels, k=3, pad=dil,
                       dilation=dil, stage=stage)
        h = self._conv(h, wts.get_folded(blk.conv3.weight, blk.bn3, "conv"), blk.conv3.out_channels, relu=False,
                       want_f32=True, want_split=False, stage=stage)
        if blk.downsample is not None:
            ds = blk.downsample
            res = self._conv(a, wts.get_folded(ds[0].weight, ds[1], "conv"), ds[0].out_channels, stride=ds[0].stride[0],
                             relu=False, want_f32=True, want_split=False, stage=stage).f32
        else:
            res = a.f32
        # the tail: conv3's fp32 rows + the shortcut, ReLU -> fp32 rows (the next block's shortcut) and planes
        y, planes = ops.fn_prep(h.f32, residual=res, relu_b=True, want_f32=True, want_split=True, scale=h.scale)
        return _Act(y, planes, h.scale, h.n, h.H, h.W, h.C)

    def _three(self, seq, a, stage, want_split=True):
        """Conv + ReLU three times (merge1.up[i], merge2.up[0][j]): planes between them, fp32 rows (and planes) at the end"""
        k, pad = seq[0].kernel_size[0], seq[0].padding[0]
        for idx in (0, 2):
            a = self._conv(a, self._own(seq[idx]), seq[idx].out_channels, k=k, pad=pad, stage=stage)
        return self._conv(a, self._own(seq[4]), seq[4].out_channels, k=k, pad=pad, want_f32=True, want_split=want_split,
                          stage=stage)

    def _resize_add(self, x, like, stage, addend=None, relu=False, want_f32=False, want_split=True):
        scale = self._scale(stage)
        y, planes = ops.egnet_resize_add(x.nhwc(), (like.H, like.W), addend=None if addend is None else addend.nhwc(),
                                         relu=relu, want_f32=want_f32, want_split=want_split, scale=scale)
        return _Act(None if y is None else y.view(-1, x.C), planes, scale, x.n, like.H, like.W, x.C)

    def _score_native(self, frames, taps=None, mark=None):
        """frames (n, H, W, 3) uint8 on the GPU -> the final score at the stem's scale, (n, h1, w1) fp32.
        mark: called with "backbone", "merge1", "merge2" as each stage has been enqueued (tools/bench_egnet.py's split)"""
        mark = mark or (lambda stage: None)
        base, m1, m2, wts = self.base, self.merge1, self.merge2, self._wts
        x = ops.egnet_input(frames)
        n = x.shape[0]
        # stem: the BatchNorm scale sits in the weights; fresco_fn_conv7_rgb has no bias, so shift + ReLU are a prep pass
        w, shift = wts.get_folded(base.conv1.weight, base.bn1, "stem")
        y = ops.fn_conv7_rgb(x, w)
        _, H1, W1, _ = y.shape
        rows = n * H1 * W1
        s32, sp = ops.fn_prep(y.view(rows, 64), mean=(-shift).view(1, 64), rstd=torch.ones_like(shift).view(1, 64),
                              rows_per_img=rows, relu_a=True, want_f32=True, want_split=True, scale=self._scale("stem"))
        feats = [_Act(s32, sp, self._scale("stem"), n, H1, W1, 64)]
        _, pp = ops.egnet_pool(feats[0].nhwc(), scale=self._scale("layer1"))
        a = _Act(None, pp, self._scale("layer1"), n, ops.egnet_pool_size(H1), ops.egnet_pool_size(W1), 64)
        for stage in STAGES[1:5]:
            for blk in getattr(base, stage):
                a = self._bottleneck(blk, a, stage)
            feats.append(a)
        # convert: fp32 rows are the addends of merge1; the deepest one feeds merge1.up[4] directly
        cv = [self._conv(f, (wts.get(c[0].weight, "conv"), None), c[0].out_channels, want_f32=True, want_split=i == 4,
                         stage="convert") for i, (c, f) in enumerate(zip(self.convert.convert0, feats))]
        mark("backbone")
        sal = [self._three(m1.up[4], cv[4], "merge1")]
        u = sal[0]
        for i in (3, 2, 1):
            if cv[i].C < u.C:
                u = self._conv(u, self._own(m1.trans[i][0]), cv[i].C, want_f32=True, want_split=False, stage="merge1")
            u = self._three(m1.up[i], self._resize_add(u, cv[i], "merge1", addend=cv[i]), "merge1")
            sal.append(u)
        t = self._conv(sal[0], self._own(m1.trans[-1][0]), 128, want_f32=True, want_split=False, stage="merge1")
        edge = self._three(m1.up[0], self._resize_add(t, cv[0], "merge1", addend=cv[0]), "merge1", want_split=False)
        mark("merge1")
        fea = None
        for j, yj in enumerate(sal[::-1]):
            t = self._conv(yj, self._own(m2.trans[0][j][0]), 128, want_f32=True, want_split=False, stage="merge2")
            f = self._three(m2.up[0][j], self._resize_add(t, edge, "merge2", addend=edge), "merge2", want_split=False)
            # the running sum relu(fea + f): same-size "resize" = an exact copy; the last sum also leaves final_score's planes
            fea = f if fea is None else self._resize_add(f, fea, "merge2", addend=fea, relu=True, want_f32=True,
                                                         want_split=j == len(sal) - 1)
        if taps is not None:
            taps.update((name, t_.nhwc()) for name, t_ in zip(TAPS, feats + cv + [edge] + sal + [fea]))
        h = self._conv(fea, self._own(m2.final_score[0]), 128, k=5, pad=2, stage="merge2")
        # 128 -> 1: one weight row; the kernel's column blocks past N read the zero page and store nothing
        score = self._conv(h, self._own(m2.final_score[2]), 1, k=3, pad=1, relu=False, want_f32=True, want_split=False,
                           stage="merge2")
        mark("merge2")
        return score.f32.view(n, H1, W1)

    def _score_library(self, frames, taps=None):
        x = ops.egnet_input(frames).permute(0, 3, 1, 2).to(self.base.conv1.weight.dtype)
        nchw = {} if taps is not None else None
        score = self.live_logit(x, nchw, resize=False)
        if taps is not None:
            taps.update((k, v.permute(0, 2, 3, 1).float().contiguous()) for k, v in nchw.items())
        return score[:, 0].float().contiguous()

    def _use_library(self):
        return self.library_ops or os.environ.get("FRESCO_EGNET_LIBRARY_OPS", "0") == "1"

    @torch.no_grad()
    def detect(self, frames, k=7, want_logit=False, taps=None):
        """frames (n, H, W, 3) uint8 on the GPU -> (saliency (n, 1, H // 2, W // 2) fp32 = 1 - dilate_k(sigmoid(logit)),
        the logit up_sal_final[-1] as (n, H // 2, W // 2) or None).  Frames go through the network max_frames at a time.
        taps: a dict that receives the TAPS tensors (NHWC fp32) -- of the last chunk when there are several."""
        frames = check_frames(frames)
        if not frames.is_cuda:
            raise ops.FrescoHipError("fresco_amd EGNet runs on the GPU only (got %s frames)" % frames.device)
        if self.training:
            raise RuntimeError("fresco_amd.egnet: the detector folds BatchNorm's running statistics -- call .eval() first")
        size = (frames.shape[1] // 2, frames.shape[2] // 2)
        chunks = [c.contiguous() for c in frames.split(self.max_frames)]
        scores = _detector.guarded_run(
            self, frames.device, lambda: [self._score_native(c, taps) for c in chunks],
            lambda: [self._score_library(c, taps) for c in chunks],
            "fresco_amd.egnet: an activation or a folded weight left the range of the split-fp16 convolutions "
            "(|activation| * split_scale < 65000, |weight| < 63); calls of this module are recomputed with library ops "
            "-- lower the stage's split scale", use_library=self._use_library())
        outs = [ops.egnet_saliency(s, size, k=k, want_logit=want_logit) for s in scores]
        sal = outs[0][0] if len(outs) == 1 else torch.cat([o[0] for o in outs], 0)
        logit = None
        if want_logit:
            logit = outs[0][1] if len(outs) == 1 else torch.cat([o[1] for o in outs], 0)
        return sal, logit

    def saliency_logit(self, frames_u8, taps=None):
        """frames (n, H, W, 3) uint8 on the GPU -> up_sal_final[-1] at cv2sod's size, (n, H // 2, W // 2) fp32"""
        return self.detect(frames_u8, want_logit=True, taps=taps)[1]


def build_model(base_model_cfg="resnet"):
    """the reference's build_model: TUN_bone on the ResNet-50 backbone (its 'vgg' variant is not built here)"""
    return TUN_bone(base_model_cfg)


def check_frames(frames):
    """a uint8 (n, H, W, 3) tensor, or a list of (H, W, 3) uint8 ndarrays of one size -> the uint8 (n, H, W, 3) tensor
    (on the host for ndarrays: the caller moves it)"""
    return _detector.check_frames(frames, "EGNet", min_side=MIN_SIDE)


def get_saliency(imgs, sod_model, dilate):
    """Drop-in for src/utils.py::get_saliency: imgs a list of (H, W, 3) uint8 arrays of one size (or a uint8 (n, H, W, 3)
    tensor), sod_model this package's TUN_bone, dilate a Dilate (its kernel_size is the box) -> (n, 1, H // 2, W // 2) fp32 on
    the GPU: 1 - dilate(sigmoid(up_sal_final[-1]))."""
    if not isinstance(sod_model, TUN_bone):
        raise TypeError("fresco_amd.get_saliency: sod_model is %s, not fresco_amd.egnet.TUN_bone -- build it with "
                        "fresco_amd.egnet.build_model (patch_saliency rebinds the reference's); there is no fallback to a "
                        "foreign module" % type(sod_model).__name__)
    frames = check_frames(imgs)
    return sod_model.detect(frames.to(sod_model.base.conv1.weight.device), k=int(dilate.kernel_size))[0]


def patch_saliency(module=None):
    """Rebind get_saliency on the reference's src.utils (default) or on a module that star-imported it (run_fresco, webUI),
    and build_model on the reference's EGNet `model` module where that is importable: `sod_model = build_model('resnet')`
    then builds this package's."""
    if module is None:
        import src.utils as module
    module.get_saliency = get_saliency
    if getattr(module, "build_model", None) is not None:
        module.build_model = build_model
    try:
        import model as ref_model
    except ImportError:
        ref_model = None
    if ref_model is not None and hasattr(ref_model, "TUN_bone"):
        ref_model.build_model = build_model
    return module
