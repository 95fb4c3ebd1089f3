"""What the detectors (hed.py, egnet.py, midas.py, canny.py) and gmflow.py share on the host: the frame and dtype checks, the
reference's checkpoint directory, the activation record of the native paths, and the run of a native path under the range
guard with its recomputation on library ops."""
import os
import warnings

import numpy as np
import torch

from . import ops


def check_frames(frames, who, min_side=None, multiple=None):
    """a uint8 (n, H, W, 3) tensor, or a list of (H, W, 3) uint8 ndarrays of one size -> the uint8 (n, H, W, 3) tensor
    (on the host for ndarrays: the caller moves it; a tensor is returned as it came).  who: the messages' prefix.
    min_side: the smallest side; multiple: what both sides must be multiples of."""
    if isinstance(frames, np.ndarray):
        frames = [frames] if frames.ndim == 3 else list(frames)
    if isinstance(frames, (list, tuple)):
        if not frames:
            raise ValueError("%s: no frames" % who)
        for f in frames:
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise TypeError("%s: frames are (H, W, 3) uint8 arrays" % who)
            if f.shape != frames[0].shape:
                raise ValueError("%s: frames of one batch share a size, got %s and %s" % (who, frames[0].shape, f.shape))
        frames = torch.from_numpy(np.stack(frames, 0))
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise TypeError("%s: frames must be a uint8 tensor (n, H, W, 3) or a list of uint8 arrays (H, W, 3)" % who)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] == 0:
        raise ValueError("%s: frames must be (n, H, W, 3), got %s" % (who, tuple(frames.shape)))
    H, W = frames.shape[1:3]
    if min_side is not None and (H < min_side or W < min_side):
        raise ValueError("%s: frames of at least %d x %d, got %d x %d" % (who, min_side, min_side, H, W))
    if multiple is not None and (H % multiple or W % multiple or 0 in (H, W)):
        raise ValueError("%s: frame sides must be multiples of %d, got %d x %d" % (who, multiple, H, W))
    return frames


def condition_dtype(dtype, who):
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise TypeError("%s: the ControlNet condition is fp16, bf16 or fp32, got %s" % (who, dtype))
    return dtype


def default_checkpoint(name):
    """`name` in the reference's annotator checkpoint directory, None when that package is not importable"""
    try:
        from annotator.util import annotator_ckpts_path
    except ImportError:
        return None
    return os.path.join(annotator_ckpts_path, name)


class Act:
    """an activation of a native path: NHWC rows as fp32 (M, C) and / or operand planes written with `scale`"""
    __slots__ = ("f32", "planes", "scale", "n", "H", "W", "C")

    def __init__(self, f32, planes, scale, n, H, W, C):
        self.f32, self.planes, self.scale, self.n, self.H, self.W, self.C = f32, planes, scale, n, H, W, C

    def nhwc(self):
        return self.f32.view(self.n, self.H, self.W, self.C)


def guarded_run(module, device, native, library, message, use_library=False, once=True):
    """native() under the range guard, or library() when use_library, or when a producer tripped the guard.
    The operand planes saturate beyond 65000 / scale (weights: beyond 63): every producer flags that on the device, ONE word
    is read back per call, and the call is recomputed with library ops when it is set -- with `message` as a RuntimeWarning
    blamed on the caller of the (torch.no_grad-wrapped) method that calls this, the first time for this module (once) or
    every time.  module: carries the weight planes `_wts` and, for once, the `_warned` mark."""
    if use_library:
        return library()
    module._wts.out_of_range = False
    with ops.fn_range_guard(device) as guard:
        out = native()
    if not (guard.tripped() or module._wts.out_of_range):
        return out
    if not (once and module._warned):
        if once:
            module._warned = True
        warnings.warn(message, RuntimeWarning, stacklevel=4)
    return library()
