"""The Canny edge detector behind FRESCO's ControlNet condition `controlnet_type: canny`, batched over frames and
resident on the GPU.

Reference: src/ControlNet/annotator/canny/__init__.py -- one `cv2.Canny(img, low, high)` per frame on the host;
run_fresco.py:199-202 then uploads each map and builds the condition.  Here a batch of uint8 frames on the device goes
through

    ops.canny_classify (Sobel, channel choice, non-maximum suppression: one launch) -> ops.canny_hysteresis (union-find
    labelling of the weak / strong pixels, the edge map and the condition tensor: four launches)

with no host round trip and a launch count that does not depend on the picture.  The arithmetic is OpenCV's generic path
for an 8-bit 3-channel image (aperture 3, L1 magnitude), all integer.  DESIGN.md section 14 has the rules, the passes and
what is verified; INTEGRATION.md recipe I the two ways to use it.
"""
import math

import numpy as np
import torch

from . import _detector, ops


def check_frames(frames):
    """a uint8 (n, H, W, 3) tensor, or a list of (H, W, 3) uint8 ndarrays of one size -> the uint8 (n, H, W, 3) tensor
    (on the host for ndarrays: the caller moves it)"""
    if isinstance(frames, np.ndarray):
        frames = [frames] if frames.ndim <= 3 else list(frames)
    if isinstance(frames, (list, tuple)):
        if not frames:
            raise ValueError("Canny: no frames")
        for f in frames:
            if not isinstance(f, np.ndarray):
                raise TypeError("Canny: frames are (H, W, 3) uint8 arrays, got %s" % type(f).__name__)
            if f.dtype != np.uint8:
                raise TypeError("Canny: frames are uint8, got %s" % f.dtype)
            if f.ndim != 3 or f.shape[2] != 3:
                raise ValueError("Canny: frames are 3-channel (H, W, 3) images, got %s (one-channel input is not built)"
                                 % (f.shape,))
            if f.shape != frames[0].shape:
                raise ValueError("Canny: frames of one batch share a size, got %s and %s" % (frames[0].shape, f.shape))
        frames = torch.from_numpy(np.stack(frames, 0))
    if not isinstance(frames, torch.Tensor):
        raise TypeError("Canny: frames must be a uint8 tensor (n, H, W, 3) or a list of uint8 arrays (H, W, 3)")
    if frames.dtype != torch.uint8:
        raise TypeError("Canny: frames are uint8, got %s" % frames.dtype)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("Canny: frames must be (n, H, W, 3) with three channels, got %s" % (tuple(frames.shape),))
    return frames


def check_thresholds(low_threshold, high_threshold):
    """ints or floats -> their floors as ints (what cv2.Canny does with them); the kernel swaps low > high"""
    out = []
    for name, v in (("low_threshold", low_threshold), ("high_threshold", high_threshold)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("Canny: %s must be a number, got %s" % (name, type(v).__name__))
        if not math.isfinite(v):
            raise ValueError("Canny: %s is %r" % (name, v))
        v = math.floor(v)
        if abs(v) >= 2 ** 31:
            raise ValueError("Canny: %s %d is no 32-bit integer" % (name, v))
        out.append(int(v))
    return tuple(out)


def condition_dtype(dtype):
    return _detector.condition_dtype(dtype, "Canny")


class CannyDetector:
    """Drop-in for annotator.canny.CannyDetector: `detector(img, low, high)` takes an (H, W, 3) uint8 array and returns the
    (H, W) uint8 edge map, so the reference's apply_control works unchanged; detect_batch / control_image keep a batch of
    frames on the device."""

    def _detect(self, frames, low_threshold, high_threshold, cond_dtype=None):
        low, high = check_thresholds(low_threshold, high_threshold)
        is_tensor = isinstance(frames, torch.Tensor)
        frames = check_frames(frames)
        if not is_tensor:  # host arrays: uploaded in one piece; a tensor batch stays where it is (the ops refuse the CPU)
            frames = frames.cuda()
        return ops.canny_hysteresis(ops.canny_classify(frames.contiguous(), low, high), cond_dtype=cond_dtype)

    def detect_batch(self, frames, low_threshold=50, high_threshold=100):
        """frames: uint8 (n, H, W, 3) tensor on the GPU or a list of (H, W, 3) uint8 arrays -> the edge maps, uint8
        (n, H, W) on the GPU"""
        return self._detect(frames, low_threshold, high_threshold)[0]

    def control_image(self, frames, dtype, guidance=True, low_threshold=50, high_threshold=100):
        """The ControlNet condition run_fresco.py:199-202 builds from the frames' edge maps:
        cat([numpy2tensor(e[:, :, None]) ...]).repeat(1, 3, 1, 1) * 0.5 + 0.5 -> .to(dtype) [-> cat x 2 under
        classifier-free guidance]: (2n | n, 3, H, W)."""
        cond = self._detect(frames, low_threshold, high_threshold, cond_dtype=condition_dtype(dtype))[1]
        return torch.cat([cond] * 2) if guidance else cond

    def __call__(self, img, low_threshold, high_threshold):
        if not isinstance(img, np.ndarray):
            raise TypeError("Canny: the image is an (H, W, 3) uint8 array, got %s" % type(img).__name__)
        return self.detect_batch([np.ascontiguousarray(img)], low_threshold, high_threshold)[0].cpu().numpy()


def patch_canny(module=None):
    """Rebind CannyDetector on the reference's annotator.canny (default) or on a module that imported the name from it
    (run_fresco, webUI): `detector = CannyDetector()` then builds this package's."""
    if module is None:
        import annotator.canny as module
    module.CannyDetector = CannyDetector
    return module
