"""Blending of the forward and backward Ebsynth propagations on the GPU: the per-frame step of video_blend.py's
process_seq (error mask with flow propagation, min-error image, histogram blend, Poisson gradient fusion).

``blend_frame`` is one call into libfresco_hip.so (``fresco_blend_frame``) on the current stream; ``blend_interval``
is process_seq's loop on tensors, with the mask kept on the device between frames; ``patch_video_blend`` rebinds a
loaded ``video_blend`` module's ``process_seq`` to it (recipe D).  The reference's stage functions
(``histogram_blend``, ``poisson_fusion``, ``error_mask``) and the Lab conversions are here under their names too.
Images are uint8 (H, W, 3) BGR GPU tensors; DESIGN.md section 10 has the semantics and the departures.
"""
import time

import numpy as np
import torch

from . import _lib, ops
from ._lib import FrescoHipError

GRADIENT = 1  # FRESCO_BLEND_GRADIENT
GRAD_WEIGHT = (2.5, 0.5, 0.5)
MAX_SIDE = 4096


def _check_image(name, t, hw=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("%s must be a uint8 (H, W, 3) BGR tensor" % name)
    if hw is not None and tuple(t.shape[:2]) != tuple(hw):
        raise ValueError("%s is %dx%d, expected %dx%d" % ((name,) + tuple(t.shape[:2]) + tuple(hw)))


def _check_plane(name, t, dtype, hw):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(hw):
        raise ValueError("%s must be a %s tensor of shape %s" % (name, dtype, tuple(hw)))


def _check_flow(flow, hw):
    if not isinstance(flow, torch.Tensor) or flow.dtype != torch.float32 or \
            tuple(flow.shape[-3:]) != (2,) + tuple(hw) or flow.dim() not in (3, 4) or flow.numel() != 2 * hw[0] * hw[1]:
        raise ValueError("flow must be a float32 (1, 2, H, W) or (2, H, W) tensor for a %dx%d frame" % tuple(hw))


def _grad_weight(grad_weight):
    gw = [float(v) for v in grad_weight]
    if len(gw) != 3 or not all(np.isfinite(gw)):
        raise ValueError("grad_weight needs three finite values (L, a, b), got %r" % (grad_weight,))
    return (_lib._c.c_float * 3)(*gw)


def workspace_bytes(h, w):
    """bytes of device workspace one frame of (h, w) needs (0 for sides outside 2..4096)"""
    return int(_lib.load().fresco_blend_workspace_bytes(int(w), int(h)))


def _workspace(h, w, dev):
    n = workspace_bytes(h, w)
    if n == 0:
        raise FrescoHipError("fresco_amd.blend: a %dx%d frame is unsupported (sides 2..%d)" % (h, w, MAX_SIDE))
    return torch.empty(n, dtype=torch.uint8, device=dev)


def bgr_to_lab(img):
    """cv2.cvtColor(img, COLOR_BGR2Lab) for uint8 (..., 3) GPU tensors (OpenCV's documented 8-bit formula)"""
    return _convert(img, "fresco_bgr_to_lab_u8")


def lab_to_bgr(img):
    """cv2.cvtColor(img, COLOR_Lab2BGR) for uint8 (..., 3) GPU tensors"""
    return _convert(img, "fresco_lab_to_bgr_u8")


def _convert(img, fn):
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() < 1 or img.shape[-1] != 3:
        raise ValueError("expected a uint8 (..., 3) tensor")
    ops._need_gpu(img)
    img = img.contiguous()
    out = torch.empty_like(img)
    _lib.check(getattr(_lib.load(), fn)(img.data_ptr(), out.data_ptr(), img.numel() // 3, ops._stream()), fn)
    return out


def error_mask(d1, d2, weight1=1, weight2=1):
    """video_blend.py g_error_mask on fp32 (H, W) GPU tensors: uint8 0 where weight1 d1 < weight2 d2, else 1.  Runs the
    mask of fresco_blend_frame, so weight2 must be 1 - weight1."""
    if abs(float(weight1) + float(weight2) - 1.0) > 1e-12:
        raise ValueError("error_mask: the kernel takes weight2 = 1 - weight1, got %r, %r" % (weight1, weight2))
    if not isinstance(d1, torch.Tensor) or d1.dim() != 2:
        raise ValueError("d1 must be a float32 (H, W) tensor")
    hw = tuple(d1.shape)
    z = torch.zeros(hw + (3,), dtype=torch.uint8, device=d1.device)
    _, mask = blend_frame(z, z, d1, d2, weight1, gradient=False)
    return mask


def histogram_blend(a, b, min_error, weight1=0.5, weight2=0.5, return_lab=False):
    """blender/histogram_blend.py blend: Lab mean / std transfer of a * weight1 + b * weight2 onto min_error's Lab
    statistics -> uint8 BGR (and, with return_lab, the rounded Lab bytes it was converted from)."""
    _check_image("a", a)
    _check_image("b", b, a.shape[:2])
    _check_image("min_error", min_error, a.shape[:2])
    ops._need_gpu(a, b, min_error)
    h, w = a.shape[:2]
    a, b, min_error = (t.contiguous() for t in (a, b, min_error))
    out = torch.empty_like(a)
    lab = torch.empty_like(a) if return_lab else None
    ws = _workspace(h, w, a.device)
    rc = _lib.load().fresco_histogram_blend(a.data_ptr(), b.data_ptr(), min_error.data_ptr(), w, h, float(weight1),
                                            float(weight2), out.data_ptr(), ops._ptr(lab), ws.data_ptr(), ws.numel(),
                                            ops._stream())
    _lib.check(rc, "fresco_histogram_blend(%dx%d)" % (h, w))
    return (out, lab) if return_lab else out


def poisson_fusion(blendI, I1, I2, mask, grad_weight=GRAD_WEIGHT, return_lab=False):
    """blender/poisson_fusion.py poisson_fusion: keep blendI's Lab values, take the gradients of I1 (I2 where
    mask > 0), solved exactly per channel with weights grad_weight (L, a, b) -> uint8 BGR (and, with return_lab, the
    truncated Lab bytes it was converted from).  mask: uint8 (H, W)."""
    _check_image("blendI", blendI)
    hw = tuple(blendI.shape[:2])
    _check_image("I1", I1, hw)
    _check_image("I2", I2, hw)
    _check_plane("mask", mask, torch.uint8, hw)
    gw = _grad_weight(grad_weight)
    ops._need_gpu(blendI, I1, I2, mask)
    h, w = hw
    blendI, I1, I2, mask = (t.contiguous() for t in (blendI, I1, I2, mask))
    out = torch.empty_like(blendI)
    lab = torch.empty_like(blendI) if return_lab else None
    ws = _workspace(h, w, blendI.device)
    rc = _lib.load().fresco_poisson_fusion(blendI.data_ptr(), I1.data_ptr(), I2.data_ptr(), mask.data_ptr(), w, h, gw,
                                           out.data_ptr(), ops._ptr(lab), ws.data_ptr(), ws.numel(), ops._stream())
    _lib.check(rc, "fresco_poisson_fusion(%dx%d)" % (h, w))
    return (out, lab) if return_lab else out


def blend_frame(oa, ob, d1, d2, weight1, prev_mask=None, flow=None, gradient=True, grad_weight=GRAD_WEIGHT,
                workspace=None):
    """One in-between frame of process_seq: oa / ob the forward / backward Ebsynth outputs (uint8 BGR), d1 / d2 their
    fp32 (H, W) error maps, weight1 = k / (interval - 1).  With prev_mask (uint8 (H, W), the previous frame's mask)
    the mask ORs in prev_mask warped by flow (fp32 (1, 2, H, W), x first; the backward flow of flow_f_*.npy).
    Returns (image uint8 BGR, mask uint8 (H, W)).  ``workspace``: an optional uint8 GPU tensor of at least
    ``workspace_bytes(H, W)`` reused across calls."""
    _check_image("oa", oa)
    hw = tuple(oa.shape[:2])
    _check_image("ob", ob, hw)
    _check_plane("d1", d1, torch.float32, hw)
    _check_plane("d2", d2, torch.float32, hw)
    if (prev_mask is None) != (flow is None):
        raise ValueError("prev_mask and flow go together")
    if prev_mask is not None:
        _check_plane("prev_mask", prev_mask, torch.uint8, hw)
        _check_flow(flow, hw)
    weight1 = float(weight1)
    if not 0.0 <= weight1 <= 1.0:
        raise ValueError("weight1 must lie in [0, 1], got %r" % weight1)
    gw = _grad_weight(grad_weight)
    ops._need_gpu(oa, ob, d1, d2, prev_mask, flow, workspace)
    h, w = hw
    dev = oa.device
    oa, ob, d1, d2 = (t.contiguous() for t in (oa, ob, d1, d2))
    if prev_mask is not None:
        prev_mask, flow = prev_mask.contiguous(), flow.contiguous()
    ws = _workspace(h, w, dev) if workspace is None else workspace
    out = torch.empty_like(oa)
    mask = torch.empty(hw, dtype=torch.uint8, device=dev)
    rc = _lib.load().fresco_blend_frame(oa.data_ptr(), ob.data_ptr(), d1.data_ptr(), d2.data_ptr(), w, h, weight1,
                                        ops._ptr(prev_mask), ops._ptr(flow), GRADIENT if gradient else 0, gw,
                                        mask.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    _lib.check(rc, "fresco_blend_frame(%dx%d)" % (h, w))
    return out, mask


def blend_interval(oas, obs, d1s, d2s, flows, gradient=True, grad_weight=GRAD_WEIGHT):
    """process_seq's loop over the n in-between frames of one key interval on tensors: frame k (0 .. n-1) blends
    oas[k] / obs[k] with error maps d1s[k] / d2s[k] at weight1 = k / n, and for k >= 1 ORs in frame k-1's mask warped
    by flows[k - 1] (so len(flows) == n - 1).  Returns the n blended uint8 BGR images; nothing leaves the device."""
    n = len(oas)
    if n == 0 or not (len(obs) == len(d1s) == len(d2s) == n):
        raise ValueError("blend_interval: oas, obs, d1s and d2s need the same length >= 1")
    if len(flows) != n - 1:
        raise ValueError("blend_interval: %d frames need %d flows, got %d" % (n, n - 1, len(flows)))
    _check_image("oas[0]", oas[0])
    ops._need_gpu(oas[0])
    ws = _workspace(oas[0].shape[0], oas[0].shape[1], oas[0].device)
    images, prev = [], None
    for k in range(n):
        img, prev = blend_frame(oas[k], obs[k], d1s[k], d2s[k], k / n, prev, flows[k - 1] if k else None, gradient,
                                grad_weight, ws)
        images.append(img)
    return images


def patch_video_blend(vb):
    """Rebind ``vb.process_seq`` (vb: the reference's loaded video_blend module) to the GPU blend.  Reads and writes
    go through the module's own cv2.imread / imwrite, load_error and flow_calc.get_flow; the error maps are paired as
    the reference pairs them (the backward map of frame end-1-k for frame beg+1+k)."""

    def process_seq(video_sequence, i, blend_histogram=True, blend_gradient=True):
        if not blend_histogram:
            raise ValueError("fresco_amd.blend: process_seq(blend_histogram=False) is not supported (the reference "
                             "feeds float32 into cvtColor there, and video_blend.main never takes that branch)")
        cv2 = vb.cv2
        key1_img = cv2.imread(video_sequence.get_key_img(i))
        img_shape = key1_img.shape
        interval = video_sequence.interval(i)
        beg_id = video_sequence.get_sequence_beg_id(i)

        oas = video_sequence.get_output_sequence(i)
        obs = video_sequence.get_output_sequence(i, False)
        binas = [x.replace('jpg', 'bin') for x in oas]
        binbs = [x.replace('jpg', 'bin') for x in obs]
        obs = [obs[0]] + list(reversed(obs[1:]))  # the images are reversed, binbs is not (kept)
        inputs = video_sequence.get_input_sequence(i)
        oas = [cv2.imread(x) for x in oas]
        obs = [cv2.imread(x) for x in obs]
        inputs = [cv2.imread(x) for x in inputs]
        flow_seq = video_sequence.get_flow_sequence(i)
        dist1s = [vb.load_error(binas[k + 1], img_shape) for k in range(interval - 1)]
        dist2s = [vb.load_error(binbs[k + 1], img_shape) for k in range(interval - 1)]

        beg = time.time()
        cv2.imwrite(video_sequence.get_blending_img(beg_id), key1_img)
        dev = torch.device("cuda", torch.cuda.current_device())

        def gpu(x, dtype=None):
            return torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x).to(dev, dtype)

        n = interval - 1
        flows = [gpu(vb.flow_calc.get_flow(inputs[k], inputs[k + 1], flow_seq[k]), torch.float32)
                 for k in range(1, n)]
        images = blend_interval([gpu(oas[k + 1]) for k in range(n)], [gpu(obs[k + 1]) for k in range(n)],
                                [gpu(d, torch.float32) for d in dist1s], [gpu(d, torch.float32) for d in dist2s],
                                flows, gradient=blend_gradient) if n else []
        for k, img in enumerate(images):
            cv2.imwrite(video_sequence.get_blending_img(beg_id + k + 1), img.cpu().numpy())
        end = time.time()
        print('others:', end - beg)

    vb.process_seq = process_seq
    return vb


__all__ = ["blend_frame", "blend_interval", "histogram_blend", "poisson_fusion", "error_mask", "bgr_to_lab",
           "lab_to_bgr", "patch_video_blend", "workspace_bytes", "FrescoHipError"]
