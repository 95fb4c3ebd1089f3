"""Weight operands of the split-fp16 dense layers (csrc/flownet.hip), cached per parameter version: what the flow network
(gmflow.py), the HED annotator (hed.py), the EGNet saliency detector (egnet.py) and the MiDaS depth annotator (midas.py)
hand to ops.fn_gemm."""
import torch
import torch.nn.functional as F

from . import ops


class WeightPlanes:
    """(hi, lo) fp16 planes of a layer's weight as the (N, K) matrix fresco_fn_gemm reads, made once per parameter version.
    Range: the planes hold w * 2^10, so |w| >= 63.5 saturates; the split pass flags that on the device (ops.fn_range_guard)
    and the verdict is kept WITH the cached planes -- `out_of_range` turns True whenever such planes are handed out, and the
    forward that used them is recomputed with library ops (GMFlow.forward, ControlNetHED_Apache2).  Staleness: the key is the parameter's version
    counter and address; an update that bypasses the counter (`p.data.copy_()`) needs `invalidate()`."""

    def __init__(self):
        self.cache = {}
        self.out_of_range = False

    def invalidate(self):
        self.cache.clear()
        self.out_of_range = False

    @staticmethod
    def _stamp(p):
        try:
            return (p._version, p.data_ptr())
        except RuntimeError:  # inference tensors track no version: never served from the cache
            return None

    def get(self, p, kind, pad_cin=None):
        key = (id(p), kind)
        hit = self.cache.get(key)
        stamp = self._stamp(p)
        if hit is not None and stamp is not None and hit[0] == stamp:
            self.out_of_range |= hit[2]
            return hit[1]
        w = p.detach().float()
        if kind == "conv":  # (cout, cin, kh, kw) -> (cout, kh, kw, cin [padded]) -> (cout, K)
            w = w.permute(0, 2, 3, 1)
            if pad_cin is not None and pad_cin > w.shape[-1]:
                w = F.pad(w, (0, pad_cin - w.shape[-1]))
            w = w.reshape(w.shape[0], -1)
        with ops.fn_range_guard(w.device) as g:
            if kind == "stem":  # (64, 3, 7, 7) -> the (64, 224) layout of fresco_fn_conv7_rgb
                val = ops.fn_conv7_weight(w)
            else:
                _, val = ops.fn_prep(w.contiguous(), scale=ops.FN_W_SCALE)
        bad = g.tripped()  # (one host sync per parameter version)
        self.out_of_range |= bad
        self.cache[key] = (stamp, val, bad)
        return val

    def get_prepared(self, p, kind, tag, prepare):
        """planes of prepare(p) -- a tensor in p's layout made from p alone (a weight-standardised convolution, a column
        slice of a linear layer: MiDaS) -- cached per version of p under (kind, tag).  kind as in get()."""
        key = (id(p), kind, tag)
        hit = self.cache.get(key)
        stamp = self._stamp(p)
        if hit is not None and stamp is not None and hit[0] == stamp:
            self.out_of_range |= hit[2]
            return hit[1]
        w = prepare(p.detach()).float()
        if kind == "conv":
            w = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
        with ops.fn_range_guard(w.device) as g:
            if kind == "stem":
                val = ops.fn_conv7_weight(w)
            else:
                _, val = ops.fn_prep(w.contiguous(), scale=ops.FN_W_SCALE)
        bad = g.tripped()  # (one host sync per parameter version)
        self.out_of_range |= bad
        self.cache[key] = (stamp, val, bad)
        return val

    def get_folded(self, p, bn, kind):
        """planes of a bias-free convolution's weight with the eval-mode BatchNorm `bn` that follows it folded in, and the
        bias that leaves: rows x gamma / sqrt(running_var + eps), bias = beta - running_mean gamma / sqrt(running_var + eps),
        both formed in float64 -> ((hi, lo), bias fp32).  kind: "conv" or "stem" as in get().  The cache entry is stamped with
        the weight AND the four BatchNorm tensors: an update of any of them makes new planes."""
        members = (p, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        key = (id(p), id(bn), kind, "folded")
        stamps = tuple(self._stamp(t) for t in members) + (float(bn.eps),)
        hit = self.cache.get(key)
        if hit is not None and None not in stamps and hit[0] == stamps:
            self.out_of_range |= hit[2]
            return hit[1]
        g = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + float(bn.eps))
        bias = (bn.bias.detach().double() - bn.running_mean.detach().double() * g).float().contiguous()
        w = (p.detach().double() * g.view(-1, 1, 1, 1)).float()
        with ops.fn_range_guard(w.device) as guard:
            if kind == "stem":
                planes = ops.fn_conv7_weight(w)
            else:
                _, planes = ops.fn_prep(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous(), scale=ops.FN_W_SCALE)
        bad = guard.tripped()  # (one host sync per parameter version)
        self.out_of_range |= bad
        val = (planes, bias)
        self.cache[key] = (stamps, val, bad)
        return val

    def get_stacked(self, params):
        """planes of the row-stacked weights of several nn.Linear layers of one input (q | k | v as ONE product): the
        single layers' planes concatenated, cached per version of every member"""
        key = tuple(id(p) for p in params) + ("stack",)
        stamps = tuple(self._stamp(p) for p in params)
        hit = self.cache.get(key)
        if hit is not None and None not in stamps and hit[0] == stamps:
            self.out_of_range |= hit[2]
            return hit[1]
        parts = [self.get(p, "lin") for p in params]
        bad = any(self.cache[(id(p), "lin")][2] for p in params)
        val = (torch.cat([h for h, _ in parts], 0).contiguous(), torch.cat([l for _, l in parts], 0).contiguous())
        self.out_of_range |= bad
        self.cache[key] = (stamps, val, bad)
        return val
