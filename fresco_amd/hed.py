"""The HED edge detector behind FRESCO's ControlNet condition (`controlnet_type: hed`, the default of every shipped
config), batched over frames and resident on the GPU.

Reference: src/ControlNet/annotator/hed/__init__.py -- one frame per call: host -> device copy, 13 fp32 convolutions, five
side maps back to the host, cv2.resize x 5, float64 sigmoid, uint8; run_fresco.py:199-202 then uploads the result again
and builds the condition.  Here a batch of uint8 frames on the device goes through

    ops.hed_input -> per block [ops.fn_gemm 3 x 3 convolutions, bias + ReLU in the epilogue] -> ops.hed_side_pool
    (side projection + the next block's pooled operand planes in one pass) -> ops.hed_fuse (resize, mean, sigmoid, uint8,
    and the condition tensor)

with no host round trip.  The module tree carries the reference's parameter names (`norm`, `blockK.convs.J.weight|bias`,
`blockK.projection.weight|bias`), so `load_state_dict(torch.load("ControlNetHED.pth"))` works unchanged.  DESIGN.md
section 12 has the data flow, the bytes and the range policy; INTEGRATION.md recipe G the two ways to use it.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _detector, ops
from .fnweights import WeightPlanes

CHECKPOINT_NAME = "ControlNetHED.pth"
MIN_SIDE = 16  # level 5 is the frame halved four times


class DoubleConvBlock(nn.Module):
    def __init__(self, input_channel, output_channel, layer_number):
        super().__init__()
        self.convs = nn.Sequential()
        self.convs.append(nn.Conv2d(input_channel, output_channel, 3, stride=1, padding=1))
        for _ in range(1, layer_number):
            self.convs.append(nn.Conv2d(output_channel, output_channel, 3, stride=1, padding=1))
        self.projection = nn.Conv2d(output_channel, 1, 1)

    def forward(self, x, down_sampling=False):
        h = x
        if down_sampling:
            h = F.max_pool2d(h, kernel_size=(2, 2), stride=(2, 2))
        for conv in self.convs:
            h = F.relu(conv(h))
        return h, self.projection(h)


class ControlNetHED_Apache2(nn.Module):
    """split_scales: the power of two each block's activation planes are written with (block 1's also scales the input
    planes).  A plane holds |x| * scale up to 65000: 2^6 carries activations up to 1015.  A network whose activations
    exceed that trips the range flag on every forward and runs on library ops (with a warning); HALVE the scale of the
    block that overflows (`ControlNetHED_Apache2(split_scales=(64, 64, 32, 32, 32))`) -- each halving doubles the range and
    raises the smallest exactly-carried magnitude likewise.
    library_ops=True (or FRESCO_HED_LIBRARY_OPS=1): the same module on PyTorch's convolutions and pooling, the fuse kernel
    on their projections -- the A/B and benchmark baseline."""

    def __init__(self, split_scales=(64.0,) * 5, library_ops=False, max_frames=8):
        super().__init__()
        if len(split_scales) != 5:
            raise ValueError("ControlNetHED_Apache2: one split scale per block (5), got %r" % (split_scales,))
        self.split_scales = tuple(ops._split_scale(s) for s in split_scales)
        if int(max_frames) < 1:
            raise ValueError("ControlNetHED_Apache2: max_frames %r" % (max_frames,))
        self.library_ops = bool(library_ops)
        self.max_frames = int(max_frames)
        self.norm = nn.Parameter(torch.zeros(size=(1, 3, 1, 1)))
        self.block1 = DoubleConvBlock(3, 64, 2)
        self.block2 = DoubleConvBlock(64, 128, 2)
        self.block3 = DoubleConvBlock(128, 256, 3)
        self.block4 = DoubleConvBlock(256, 512, 3)
        self.block5 = DoubleConvBlock(512, 512, 3)
        self._wts = WeightPlanes()
        self._warned = False

    @property
    def blocks(self):
        return (self.block1, self.block2, self.block3, self.block4, self.block5)

    def forward(self, x, n_blocks=5):
        """the reference's forward: x (n, 3, H, W) float RGB in 0..255 -> the five projections (n, 1, h, w); library ops"""
        h = x - self.norm
        out = []
        for k, blk in enumerate(self.blocks[:n_blocks]):
            h, p = blk(h, down_sampling=k > 0)
            out.append(p)
        return tuple(out)

    # ---- side maps of one chunk of frames (n, H, W, 3) uint8 on the GPU -> five (n, h, w) fp32 tensors
    # (n_blocks < 5: the first blocks only -- tools/bench_hed.py times the network block by block)
    def _sides_library(self, frames, n_blocks=5):
        x = frames.permute(0, 3, 1, 2).to(self.norm.dtype)
        return [p[:, 0].float().contiguous() for p in self.forward(x, n_blocks)]

    def _sides_native(self, frames, n_blocks=5):
        n, H, W, _ = frames.shape
        wts, sc = self._wts, self.split_scales
        xs = ops.hed_input(frames, self.norm.detach().reshape(3).float().contiguous(), scale=sc[0])
        sides = []
        for k, blk in enumerate(self.blocks[:n_blocks]):
            h = None
            for j, conv in enumerate(blk.convs):
                last = j == len(blk.convs) - 1
                w = wts.get(conv.weight, "conv", 32 if (k == 0 and j == 0) else None)
                # intermediate convolutions leave operand planes only; the block's last one the fp32 rows side_pool reads
                h, xs = ops.fn_gemm(xs, w, conv.out_channels, w[0].shape[1], bias=conv.bias, act=1,
                                    conv=(n, H, W, 3, 3, 1, 1), want_f32=last, want_split=not last, a_scale=sc[k],
                                    out_scale=sc[k])
            pool = k + 1 < n_blocks
            proj, xs = ops.hed_side_pool(h, n, H, W, blk.projection.weight.detach().reshape(-1).float().contiguous(),
                                         blk.projection.bias.detach().reshape(-1).float().contiguous(), want_pool=pool,
                                         scale=sc[k + 1] if pool else sc[k])
            sides.append(proj)
            H, W = H // 2, W // 2
        return sides

    def _use_library(self):
        return self.library_ops or os.environ.get("FRESCO_HED_LIBRARY_OPS", "0") == "1"

    @torch.no_grad()
    def side_maps(self, frames):
        """frames (n, H, W, 3) uint8 on the GPU -> the five side maps, level k (n, H >> k, W >> k) fp32.  Frames go
        through the network max_frames at a time (block 1's activations are 64 fp32 channels per pixel)."""
        frames = check_frames(frames)
        if not frames.is_cuda:
            raise ops.FrescoHipError("fresco_amd HED runs on the GPU only (got %s frames)" % frames.device)
        chunks = frames.split(self.max_frames)
        per_chunk = _detector.guarded_run(
            self, frames.device, lambda: [self._sides_native(c.contiguous()) for c in chunks],
            lambda: [self._sides_library(c) for c in chunks],
            "fresco_amd.ControlNetHED_Apache2: an activation or weight left the range of the split-fp16 convolutions "
            "(|activation| * split_scale < 65000, |weight| < 63); forwards of this module are recomputed with library ops "
            "-- lower the block's split scale", use_library=self._use_library())
        if len(per_chunk) == 1:
            return per_chunk[0]
        return [torch.cat([s[k] for s in per_chunk], 0) for k in range(5)]

    @torch.no_grad()
    def detect(self, frames, want_logit=False, cond_dtype=None):
        """-> (edge map (n, H, W) uint8, fused logit (n, H, W) fp32 or None, condition (n, 3, H, W) or None)"""
        return ops.hed_fuse(self.side_maps(frames), want_logit=want_logit, cond_dtype=cond_dtype)


def check_frames(frames):
    """a uint8 (n, H, W, 3) tensor, or a list of (H, W, 3) uint8 ndarrays of one size -> the uint8 (n, H, W, 3) tensor
    (on the host for ndarrays: the caller moves it)"""
    return _detector.check_frames(frames, "HED", min_side=MIN_SIDE)


def condition_dtype(dtype):
    return _detector.condition_dtype(dtype, "HED")


class HEDdetector:
    """Drop-in for annotator.hed.HEDdetector: `detector(img)` takes an (H, W, 3) uint8 RGB array and returns the (H, W)
    uint8 edge map, so the reference's apply_control works unchanged.  Nothing is downloaded: the checkpoint is read from
    `model_path`, or from the reference's `annotator_ckpts_path/ControlNetHED.pth` when that package is importable; pass
    `network=` to use a module that already holds its weights.  max_frames: frames per pass through the network; None keeps
    the module's own value (8 unless it was built with another)."""

    def __init__(self, model_path=None, *, network=None, max_frames=None):
        if network is None:
            path = model_path or _detector.default_checkpoint(CHECKPOINT_NAME)
            if path is None or not os.path.exists(path):
                raise FileNotFoundError(
                    "fresco_amd.HEDdetector: no checkpoint%s. Put %s (lllyasviel/Annotators) into the reference's "
                    "src/ControlNet/annotator/ckpts/ or pass model_path=; this package downloads nothing."
                    % ("" if path is None else " at %s" % path, CHECKPOINT_NAME))
            network = ControlNetHED_Apache2()
            network.load_state_dict(torch.load(path, map_location="cpu"))
            network = network.float().cuda()
        if max_frames is not None:
            if int(max_frames) < 1:
                raise ValueError("HEDdetector: max_frames %r" % (max_frames,))
            network.max_frames = int(max_frames)
        self.netNetwork = network.eval()

    def _device(self):
        return self.netNetwork.norm.device

    def detect_batch(self, frames):
        """frames: uint8 (n, H, W, 3) tensor or a list of (H, W, 3) uint8 arrays -> the edge maps, uint8 (n, H, W) on the GPU"""
        return self.netNetwork.detect(check_frames(frames).to(self._device()))[0]

    def control_image(self, frames, dtype, guidance=True):
        """The ControlNet condition run_fresco.py:199-202 builds from the frames' edge maps:
        cat([numpy2tensor(e[:, :, None]) ...]).repeat(1, 3, 1, 1) * 0.5 + 0.5 -> .to(dtype) [-> cat x 2 under
        classifier-free guidance]: (2n | n, 3, H, W)."""
        dtype = condition_dtype(dtype)
        cond = self.netNetwork.detect(check_frames(frames).to(self._device()), cond_dtype=dtype)[2]
        return torch.cat([cond] * 2) if guidance else cond

    def __call__(self, input_image):
        assert input_image.ndim == 3
        return self.detect_batch([np.ascontiguousarray(input_image)])[0].cpu().numpy()


def patch_hed(module=None):
    """Rebind HEDdetector on the reference's annotator.hed (default) or on a module that imported the name from it
    (run_fresco, webUI): `detector = HEDdetector()` then builds this package's."""
    if module is None:
        import annotator.hed as module
    module.HEDdetector = HEDdetector
    return module
