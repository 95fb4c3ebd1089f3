"""A drop-in for FRESCO's ``FlowCalc`` (src/ebsynth/flow/flow_utils.py) on this package's GMFlow, batched over pairs.

The reference makes one bidirectional GMFlow forward per ``get_flow`` call, at batch 1, in eager PyTorch, from host
float copies of the frames, then unpads and runs the forward / backward consistency check as a chain of small torch
ops.  Here:

* ``fresco_flowcalc_input`` (csrc/flowcalc.hip) builds the network's normalised, replicate-padded input for P pairs
  from the n distinct uint8 frames, uploaded once each;
* ``fresco_amd.gmflow.GMFlow.forward_normalised`` runs the network on its own HIP kernels, at most ``max_pairs`` pairs
  per forward;
* ``fresco_flowcalc_output`` unpads and checks consistency (the arithmetic of ``fresco_flow_occlusion``) and writes the
  backward flow and its 0 / 255 mask, plus the forward half for a requested swapped pair: ``get_flow(b, a)`` is the
  forward half of the bidirectional forward of ``(a, b)``, so a pair whose swap is also requested costs no forward
  of its own (``share=True``);
* flows and masks of a forward come back in one copy and are written as the reference writes them: ``np.save`` of the
  (1, 2, H, W) fp32 flow, ``cv2.imwrite`` of the (H, W, 1) int64 0 / 255 mask, through ``self.cv2`` (the caller
  module's cv2: ``patch_flow_calc`` binds it).

Existing save paths are read back and nothing is computed, as in the reference.  ``warp`` implements the one mode
video_blend.py uses, ``'nearest'``; there is no eager fallback.  DESIGN.md section 9.2, INTEGRATION.md recipe E.
"""
import os

import numpy as np
import torch

from . import _lib, ops

ALPHA, BETA = 0.01, 0.5  # forward_backward_consistency_check's defaults, as get_flow calls it
SPLITS = 2  # attn_splits_list=[2]
PADDING_FACTOR = 8
MAX_PAIRS = 8
# GMFlow as FlowCalc.__init__ builds it
CONFIG = dict(feature_channels=128, num_scales=1, upsample_factor=8, num_head=1, attention_type="swin",
              ffn_dim_expansion=4, num_transformer_layers=6)


# ---------------------------------------------------------------------------------------------------------------------
# sizes
def padding(h, w):
    """InputPadder((h, w), mode='sintel', padding_factor=8)._pad as (top, bottom, left, right)"""
    f = PADDING_FACTOR
    ph = (((h // f) + 1) * f - h) % f
    pw = (((w // f) + 1) * f - w) % f
    return ph // 2, ph - ph // 2, pw // 2, pw - pw // 2


def padded_size(h, w):
    t, b, l, r = padding(h, w)
    return h + t + b, w + l + r


def check_size(h, w):
    """Refuse what the network cannot take, before any launch: sides below 2 (the consistency warps divide by
    side - 1) and padded sizes whose 1/8 feature map does not split into 2 x 2 attention windows (the reference fails
    on those inside its transformer)."""
    if h < 2 or w < 2:
        raise ValueError("frames of %dx%d: both sides must be at least 2" % (h, w))
    hp, wp = padded_size(h, w)
    fh, fw = hp // PADDING_FACTOR, wp // PADDING_FACTOR
    if fh % SPLITS or fw % SPLITS:
        raise ValueError("frames of %dx%d pad to %dx%d, whose %dx%d feature map is not divisible into %d x %d windows"
                         % (h, w, hp, wp, fh, fw, SPLITS, SPLITS))


def check_frames(frames):
    """frames: uint8 (h, w, 3) arrays of one size; returns (h, w)"""
    if not frames:
        raise ValueError("no frames")
    shapes = {tuple(np.shape(f)) for f in frames}
    if len(shapes) != 1:
        raise ValueError("frames of different sizes: %s" % sorted(shapes))
    shape = shapes.pop()
    if len(shape) != 3 or shape[2] != 3 or any(np.asarray(f).dtype != np.uint8 for f in frames):
        raise ValueError("frames must be uint8 (h, w, 3) images as cv2.imread gives them, got %s" % (shape,))
    check_size(shape[0], shape[1])
    return shape[0], shape[1]


# ---------------------------------------------------------------------------------------------------------------------
# kernels
def flowcalc_input(frames, first, second):
    """The network's input for P pairs: frames uint8 (n, h, w, 3) on the GPU, first / second (P,) frame indices.
    Returns (2P, 3, H', W') fp32, first images then second images, padded and normalised."""
    ops._need_gpu(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("frames must be uint8 (n, h, w, 3), got %s %s" % (frames.dtype, tuple(frames.shape)))
    n, h, w, _ = (int(v) for v in frames.shape)
    check_size(h, w)
    idx = [np.asarray(v, np.int64).reshape(-1) for v in (first, second)]
    if idx[0].shape != idx[1].shape or idx[0].size == 0:
        raise ValueError("first and second must name the same number (>= 1) of frames")
    if min(int(v.min()) for v in idx) < 0 or max(int(v.max()) for v in idx) >= n:
        raise ValueError("frame index outside [0, %d)" % n)
    P = int(idx[0].size)
    tab = torch.from_numpy(np.concatenate(idx).astype(np.int32)).to(frames.device)
    hp, wp = padded_size(h, w)
    x = frames.contiguous()
    out = torch.empty(2 * P, 3, hp, wp, dtype=torch.float32, device=frames.device)
    rc = _lib.load().fresco_flowcalc_input(x.data_ptr(), tab.data_ptr(), tab[P:].data_ptr(), out.data_ptr(), n, P, h,
                                           w, ops._stream())
    _lib.check(rc, "fresco_flowcalc_input(%d pairs of %dx%d)" % (P, h, w))
    return out


def flowcalc_output(flows, h, w, swapped=False, alpha=ALPHA, beta=BETA, out=None):
    """Unpad + consistency check of the network's (2P, 2, H', W') flows.  Returns (bwd_flow (P, 2, h, w) fp32,
    bwd_occ (P, h, w) uint8 0 / 255) and, with swapped=True, also (fwd_flow, fwd_occ).  ``out``: a uint8 device buffer
    of output_bytes(P, h, w, swapped) bytes to carve the results from (one copy brings them all back)."""
    ops._need_gpu(flows)
    hp, wp = padded_size(h, w)
    if flows.dtype != torch.float32 or flows.dim() != 4 or flows.shape[0] % 2 or tuple(flows.shape[1:]) != (2, hp, wp):
        raise ValueError("flows must be float32 (2P, 2, %d, %d) for %dx%d frames, got %s"
                         % (hp, wp, h, w, tuple(flows.shape)))
    check_size(h, w)
    P = int(flows.shape[0]) // 2
    if out is None:
        out = torch.empty(output_bytes(P, h, w, swapped), dtype=torch.uint8, device=flows.device)
    views = carve_outputs(out, P, h, w, swapped)
    f = flows.contiguous()
    bf, bo = views[0], views[1]
    ff, fo = (views[2], views[3]) if swapped else (None, None)
    rc = _lib.load().fresco_flowcalc_output(f.data_ptr(), bf.data_ptr(), bo.data_ptr(),
                                            ff.data_ptr() if swapped else None, fo.data_ptr() if swapped else None,
                                            P, h, w, float(alpha), float(beta), ops._stream())
    _lib.check(rc, "fresco_flowcalc_output(%d pairs of %dx%d)" % (P, h, w))
    return views


def output_bytes(P, h, w, swapped):
    k = 2 if swapped else 1
    return k * P * h * w * (2 * 4 + 1)


def carve_outputs(buf, P, h, w, swapped):
    """(bwd_flow, bwd_occ[, fwd_flow, fwd_occ]) views of one uint8 buffer: the flows first (4-byte aligned), then the
    masks"""
    k = 2 if swapped else 1
    nf, no = P * 2 * h * w * 4, P * h * w
    if buf.dtype != torch.uint8 or buf.numel() < output_bytes(P, h, w, swapped):
        raise ValueError("output buffer too small")
    flows = [buf[i * nf:(i + 1) * nf].view(torch.float32).view(P, 2, h, w) for i in range(k)]
    occs = [buf[k * nf + i * no:k * nf + (i + 1) * no].view(P, h, w) for i in range(k)]
    return (flows[0], occs[0]) + ((flows[1], occs[1]) if swapped else ())


# ---------------------------------------------------------------------------------------------------------------------
# scheduling and files
def schedule(pairs, share=True):
    """Forwards for the requested (first, second) frame index pairs.  Returns (forwards, plan): forwards is the list of
    distinct (a, b) pairs to run, in first-seen order; plan[r] = (forward index, swapped) for request r.  A repeated
    pair reuses its forward; with ``share`` a pair (b, a) whose swap (a, b) runs takes that forward's forward half."""
    forwards, at, plan = [], {}, []
    for a, b in pairs:
        key = (int(a), int(b))
        if key in at:
            plan.append((at[key], False))
        elif share and key[::-1] in at:
            plan.append((at[key[::-1]], True))
        else:
            at[key] = len(forwards)
            forwards.append(key)
            plan.append((at[key], False))
    return forwards, plan


def mask_path_of(save_path):
    return os.path.splitext(save_path)[0] + ".png"


def write_outputs(cv2, save_path, flow, occ):
    """get_flow's files: np.save(save_path, flow (1, 2, h, w) fp32) and cv2.imwrite of the mask as the reference builds
    it, bwd_occ.permute(1, 2, 0).to(torch.long).numpy() * 255: (h, w, 1) int64 of 0 / 255.  occ: (h, w) 0 / 255."""
    np.save(save_path, np.ascontiguousarray(flow, np.float32).reshape((1,) + tuple(np.shape(flow)[-3:])))
    arr = (np.asarray(occ).reshape(np.shape(occ)[-2:] + (1,)) != 0).astype(np.int64) * 255
    cv2.imwrite(mask_path_of(save_path), arr)


def read_flow(save_path):
    """flow_utils.read_flow"""
    return torch.from_numpy(np.load(save_path))


def read_mask(save_path, cv2=None):
    """flow_utils.read_mask (through `cv2`, default the real one)"""
    if cv2 is None:
        import cv2
    mask = cv2.imread(mask_path_of(save_path))
    return cv2.cvtColor(mask, cv2.COLOR_BGR2GRAY)


# ---------------------------------------------------------------------------------------------------------------------
class FlowCalc:
    """flow_utils.FlowCalc on fresco_amd.gmflow.GMFlow (module docstring).  ``flow_model``: a ready GMFlow-like model
    with ``forward_normalised`` (then model_path is not read); ``max_pairs``: pairs per forward; ``share``: take a
    requested swapped pair from its partner's forward; ``cv2``: the module files go through (default: import cv2 on
    first use; patch_flow_calc binds video_blend's)."""

    def __init__(self, model_path='./model/gmflow_sintel-0c07dcb3.pth', *, flow_model=None, max_pairs=MAX_PAIRS,
                 share=True, cv2=None):
        if flow_model is None:
            from .gmflow import GMFlow
            flow_model = GMFlow(**CONFIG).to('cuda')
            checkpoint = torch.load(model_path, map_location=lambda storage, loc: storage)
            weights = checkpoint['model'] if 'model' in checkpoint else checkpoint
            flow_model.load_state_dict(weights, strict=False)
            flow_model.eval()
        self.model = flow_model
        self.max_pairs = max(1, int(max_pairs))
        self.share = bool(share)
        self._cv2 = cv2
        self.stats = {"forwards": 0, "pairs": 0}

    @property
    def cv2(self):
        if self._cv2 is None:
            import cv2
            self._cv2 = cv2
        return self._cv2

    @cv2.setter
    def cv2(self, mod):
        self._cv2 = mod

    def _device(self):
        p = next(iter(self.model.parameters()), None)
        return p.device if p is not None else torch.device("cuda", torch.cuda.current_device())

    def _forwards(self, frames, pairs):
        """Run the pairs, forward by forward (sizes checked before the first launch).  After each forward, yields
        [(request index, bwd_flow (1, 2, h, w) device, bwd_occ (h, w) uint8 device, bwd_flow host, bwd_occ host)] for
        every request it serves; nothing of a forward is kept once the caller asks for the next, so memory is bounded
        by max_pairs (and one uint8 copy of each distinct frame on the device)."""
        forwards, plan = schedule(pairs, self.share)
        used = sorted({i for ab in forwards for i in ab})
        h, w = check_frames([frames[i] for i in used])
        slot = {f: k for k, f in enumerate(used)}
        served = {}
        for r, (f, sw) in enumerate(plan):
            served.setdefault(f, []).append((r, sw))
        dev = self._device()
        frames_dev = torch.from_numpy(np.stack([np.ascontiguousarray(frames[i]) for i in used])).to(dev)
        for s in range(0, len(forwards), self.max_pairs):
            idx = list(range(s, min(s + self.max_pairs, len(forwards))))
            P = len(idx)
            swapped = any(sw for k in idx for _, sw in served[k])
            x = flowcalc_input(frames_dev, [slot[forwards[k][0]] for k in idx], [slot[forwards[k][1]] for k in idx])
            flow = self.model.forward_normalised(x, SPLITS, True)["flow_preds"][-1]
            del x
            buf = torch.empty(output_bytes(P, h, w, swapped), dtype=torch.uint8, device=dev)
            dv = flowcalc_output(flow, h, w, swapped, out=buf)
            del flow
            hv = carve_outputs(buf.cpu(), P, h, w, swapped)  # one copy per forward
            self.stats["forwards"] += 1
            self.stats["pairs"] += P
            out = []
            for j, k in enumerate(idx):
                for r, sw in served[k]:
                    o = 2 if sw else 0
                    out.append((r, dv[o][j:j + 1], dv[o + 1][j], hv[o][j:j + 1].numpy(), hv[o + 1][j].numpy()))
            yield out
            del out, dv, hv, buf

    @torch.no_grad()
    def get_flows(self, frames, pairs, save_paths=None, return_flows=True):
        """get_flow for many pairs at once: frames, uint8 (h, w, 3) images of one size; pairs, (i, j) indices into
        frames (get_flow(frames[i], frames[j], ...)); save_paths, one per pair (or None).  Pairs whose save path exists
        are read back, the rest run in forwards of at most max_pairs pairs, and each forward's files are written as
        soon as it is back.  Returns, per pair, the backward flow (1, 2, h, w) on the host (read_flow's tensor: what a
        later get_flow of that save path returns), or None with return_flows=False (the driver: nothing is kept)."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        save_paths = list(save_paths) if save_paths is not None else [None] * len(pairs)
        if len(save_paths) != len(pairs):
            raise ValueError("one save path per pair")
        for a, b in pairs:
            if not (0 <= a < len(frames) and 0 <= b < len(frames)):
                raise ValueError("pair (%d, %d) names a frame outside [0, %d)" % (a, b, len(frames)))
        res = [None] * len(pairs)
        todo = []
        for r, p in enumerate(save_paths):
            if p is None or not os.path.exists(p):
                todo.append(r)
            elif return_flows:
                res[r] = read_flow(p)
        for batch in self._forwards(frames, [pairs[r] for r in todo]) if todo else ():
            for q, _, _, fh, oh in batch:
                r = todo[q]
                if save_paths[r] is not None:
                    write_outputs(self.cv2, save_paths[r], fh, oh)
                if return_flows:
                    res[r] = torch.from_numpy(fh.copy())
        return res if return_flows else None

    def _one(self, image1, image2):
        """(bwd_flow device, bwd_occ device, bwd_flow host, bwd_occ host) of one pair"""
        (batch,) = list(self._forwards([image1, image2], [(0, 1)]))
        return batch[0][1:]

    @torch.no_grad()
    def get_flow(self, image1, image2, save_path=None):
        """flow_utils.FlowCalc.get_flow: the backward flow (1, 2, h, w) (a device tensor when computed, read_flow's
        when save_path exists)"""
        if save_path is not None and os.path.exists(save_path):
            return read_flow(save_path)
        fd, _, fh, oh = self._one(image1, image2)
        if save_path is not None:
            write_outputs(self.cv2, save_path, fh, oh)
        return fd

    @torch.no_grad()
    def get_mask(self, image1, image2, save_path=None):
        """flow_utils.FlowCalc.get_mask: read_mask of an existing <save_path>.png; else computed, saved like get_flow,
        and returned as the reference returns it ((h, w, 1) int64 0 / 255 when saved, else (1, h, w) float on the
        device)"""
        if save_path is not None and os.path.exists(mask_path_of(save_path)):
            return self.read_mask(save_path)
        fd, od, fh, oh = self._one(image1, image2)
        if save_path is None:
            return (od != 0).float().unsqueeze(0)
        write_outputs(self.cv2, save_path, fh, oh)
        return (oh != 0).astype(np.int64)[..., None] * 255

    def read_flow(self, save_path):
        return read_flow(save_path)

    def read_mask(self, save_path):
        return read_mask(save_path, self.cv2)

    def warp(self, img, flow, mode='bilinear'):
        """flow_utils.FlowCalc.warp for mode 'nearest' (the one video_blend.py uses) of an (h, w) / (h, w, c) numpy
        image of any real dtype, bit-exact.  As the reference: the image goes to fp32 (torch's conversion), every pixel
        takes the fp32 value of its nearest source pixel or 0 outside, and the result goes back to the input dtype
        (torch's conversion).  A nearest warp only moves whole pixels, so the fp32 values travel through
        fresco_warp_nearest as 4 bytes per channel, whatever they are; 1-byte images (uint8, int8, bool), which that
        round trip leaves unchanged, are warped as they are.  PositionalGuide's first image is float64.  Other modes
        are not implemented."""
        if mode != 'nearest':
            raise NotImplementedError("fresco_amd.FlowCalc.warp implements mode 'nearest' only (what video_blend.py "
                                      "uses), got %r; there is no eager fallback" % (mode,))
        a = np.asarray(img)
        if a.dtype.kind not in "biuf" or a.ndim not in (2, 3):
            raise NotImplementedError("fresco_amd.FlowCalc.warp: (h, w) or (h, w, c) images of a real dtype, got %s %s"
                                      % (a.dtype, a.shape))
        expand = a.ndim == 2
        a = np.ascontiguousarray(a[..., None] if expand else a)
        if a.dtype.itemsize == 1:
            res = self._warp_bytes(a.view(np.uint8), flow).view(a.dtype)
        else:
            x = torch.from_numpy(a).to(torch.float32).numpy()
            res = self._warp_bytes(x.view(np.uint8), flow).view(np.float32)
            res = torch.from_numpy(res).to(torch.from_numpy(a[:0]).dtype).numpy()
        return res[:, :, 0] if expand else res

    def _warp_bytes(self, u, flow):
        """fresco_warp_nearest of a uint8 (h, w, k) array, any k: in runs of at most 16 channels"""
        from . import ebsynth as E
        h, w, k = u.shape
        dev = self._device()
        fl = torch.as_tensor(flow).to(dev, torch.float32).reshape(1, 2, h, w)
        x = torch.from_numpy(u).to(dev)
        out = torch.cat([E.warp_nearest(x[..., c:c + 16].contiguous(), fl) for c in range(0, k, 16)], -1)
        return np.ascontiguousarray(out.cpu().numpy())


def patch_flow_calc(vb, flow_calc):
    """Rebind ``vb.flow_calc`` (vb: the reference's loaded video_blend module) and the guide module's ``flow_calc``
    (blender.guide, whose guides warp through it) to ``flow_calc``, whose files then go through ``vb.cv2``.  Returns
    vb."""
    from .propagate import _guide_module
    gm = _guide_module(vb)
    if hasattr(vb, "cv2"):
        flow_calc.cv2 = vb.cv2
    vb.flow_calc = flow_calc
    gm.flow_calc = flow_calc
    return vb


__all__ = ["FlowCalc", "patch_flow_calc", "read_flow", "read_mask", "schedule", "padding", "padded_size",
           "check_size", "check_frames", "flowcalc_input", "flowcalc_output", "write_outputs"]
