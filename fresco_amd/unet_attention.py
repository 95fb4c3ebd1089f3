"""UNetAttnProcessor: a plain attention processor on this package's kernels for the attention modules of the SD-1.5 UNet and
ControlNet that carry no FRESCO processor -- `attn2` everywhere, and `attn1` of the encoder, the mid block, `up_blocks.1` and
the ControlNet.  fp16 pipelines on the GPU; there is no fallback to PyTorch.

It has the call signature of diffusers' `AttnProcessor2_0`, `(attn, hidden_states, encoder_hidden_states=None,
attention_mask=None, temb=None)`, and computes what that processor computes for a 3-D input without a mask:

  self-attention    to_q | to_k | to_v in ONE launch that reads the hidden states once: fresco_linear with the three weights
                    where it takes the width (320, 640: `ops.linear_supported(K, N, fp16, 3)`), otherwise vae_conv 1 x 1 over
                    the three weights stacked as one (3 C, C) matrix, all rows of all images as one run of rows; q, k and v
                    are then column slices of the (rows, 3 C) result, no copies
  cross-attention   to_q the same way with one weight; to_k | to_v of the text as one vae_conv 1 x 1 over the stacked
                    (2 C, text width) matrix into a (B Lt, 2 C) buffer whose halves are K and V
  attention         head dims 40 and 80: fresco_attn_fwd (ops.attention), the kernels and the workspace handling of the
                    FRESCO processor; head dim 160: unet_attention (ops.unet_attention); any other head dim raises
  to_out[0]         with its bias: fresco_linear where it takes the width, otherwise vae_conv 1 x 1 with the bias in fp32;
                    to_out[1] is called as it is
`residual_connection` and `rescale_output_factor` are honoured as the FRESCO processor honours them.

TEXT K | V CACHE (`cache_text_kv=True`, the default).  The projected text is kept per attention module and reused while a
call passes the same text tensor OBJECT at the same `_version`: the pipeline hands every denoising step the same
`prompt_embeds`, so all steps but the first skip the projection.  The processor holds the tensor, so the key is identity and
not `data_ptr()`: an address can be reused by another tensor, an object that is held cannot.  An in-place change of the text
bumps its version and projects again.  `clear()` drops the buffers; `cache_text_kv=False` projects on every call.

PACKED COPIES.  The stacked weights and the fp32 bias are COPIES, kept per module and keyed by the source parameters'
identity and `_version`: an in-place weight update (load_state_dict, an optimiser step) is seen on the next call and the copy
is made again; so is a replaced Parameter.  Where fresco_linear runs, nothing is copied: it reads the weights where they live.

REFUSALS, each a NotImplementedError that names its cause: an attention_mask; a 4-D input; spatial_norm, group_norm,
norm_cross or added_kv_proj_dim; to_q / to_k / to_v with a bias or not a plain nn.Linear; to_out[0] without a bias; tensors
or weights that are not fp16 or not on the GPU; widths that are no multiple of 32; a head dim other than 40, 80 or 160.

`patch_unet_attention(model)` sets one shared processor on every attention module of `model` that carries no FRESCO
processor; `unpatch_unet_attention(model)` puts the previous processors back.  diffusers is not imported, and not installed
where this package is built and tested: the attributes read from the `Attention` module (`heads`, `to_q`, `to_k`, `to_v`,
`to_out`, `spatial_norm`, `group_norm`, `norm_cross`, `added_kv_proj_dim`, `residual_connection`, `rescale_output_factor`,
`processor`, `set_processor`) come from its published source (0.19.3, models/attention_processor.py) and are UNVERIFIED
against the real module.
"""
import math
import weakref

import torch

from . import _dropin, _lib, ops
from ._dropin import rows16 as _rows16
from .processor import FRESCOAttnProcessor2_0, _plain_linear

HEAD_DIMS_FLASH = (40, 80)                 # ops.attention
HEAD_DIM_UNET = ops.UNET_ATTN_HEAD_DIM     # ops.unet_attention
WIDTH_STEP = 32                            # K and N of vae_conv 1 x 1
PARTS = ("to_q", "to_k", "to_v", "to_out", "heads", "processor")   # what makes a module an attention module for the patch
_ATTR = "_fresco_unet_attention_previous"
_WHO = "fresco_amd.unet_attention"


def _is_linear(m):
    return type(m) is torch.nn.Linear


class UNetAttnProcessor:
    """plain self- and cross-attention of a diffusers `Attention` module on HIP kernels (see the module docstring); one
    instance may serve every module of a UNet and a ControlNet: what it keeps is kept per module"""

    def __init__(self, cache_text_kv=True):
        _lib.load()  # fail here, loudly, when the HIP library is absent
        self.cache_text_kv = bool(cache_text_kv)
        self._ws = ops.Workspace()
        self._packed = weakref.WeakKeyDictionary()   # attn -> {slot: ([(parameter, version)], value)}
        self._text = weakref.WeakKeyDictionary()     # attn -> (text tensor, version, packed K | V weight, (B Lt, 2 C) buffer)

    def clear(self):
        """drop the cached text projections (the packed weight copies stay: they follow their parameters' versions)"""
        self._text.clear()

    # ---- what the module must be ------------------------------------------------------------------------------------
    @staticmethod
    def refusal(attn):
        """why `attn` (a module with PARTS) is outside what this processor computes, or None; reads shapes and dtypes only"""
        for name in ("spatial_norm", "group_norm"):
            if getattr(attn, name, None) is not None:
                return "has a %s" % name
        if getattr(attn, "norm_cross", None):
            return "has norm_cross"
        if getattr(attn, "added_kv_proj_dim", None) is not None:
            return "has an added_kv_proj_dim"
        for name in ("to_q", "to_k", "to_v"):
            m = getattr(attn, name, None)
            if not _is_linear(m):
                return "%s is %s, not a plain nn.Linear" % (name, type(m).__name__)
            if m.bias is not None:
                return "%s has a bias" % name
        try:
            out0, out1 = attn.to_out[0], attn.to_out[1]
        except (TypeError, IndexError, KeyError):
            return "to_out is not a (Linear, Dropout) pair"
        if not _is_linear(out0) or not callable(out1):
            return "to_out[0] is %s, not a plain nn.Linear" % type(out0).__name__
        if out0.bias is None:
            return "to_out[0] has no bias"
        C = attn.to_q.out_features
        if attn.to_k.out_features != C or attn.to_v.out_features != C or out0.in_features != C \
                or attn.to_k.in_features != attn.to_v.in_features:
            return "projects to %d / %d / %d channels and back from %d" % (C, attn.to_k.out_features, attn.to_v.out_features,
                                                                          out0.in_features)
        for m in (attn.to_q, attn.to_k, attn.to_v, out0):
            for p in (m.weight, m.bias):
                if p is not None and p.dtype != torch.float16:
                    return "has %s weights, fp16 modules only" % p.dtype
        for w in (attn.to_q.in_features, attn.to_k.in_features, C, out0.out_features):
            if w % WIDTH_STEP:
                return "is %d wide, the projection kernels take multiples of %d" % (w, WIDTH_STEP)
        heads = int(attn.heads)
        if heads <= 0 or C % heads or C // heads not in HEAD_DIMS_FLASH + (HEAD_DIM_UNET,):
            return "has head dim %s (%d channels on %d heads), only %s" % (C // heads if heads > 0 and C % heads == 0 else "?", C,
                                                                          heads, "/".join(map(str, HEAD_DIMS_FLASH + (HEAD_DIM_UNET,))))
        return None

    # ---- packed copies ----------------------------------------------------------------------------------------------
    def _pack(self, attn, slot, params, build):
        store = self._packed.get(attn)
        if store is None:
            store = self._packed[attn] = {}
        hit = store.get(slot)
        if hit is not None and len(hit[0]) == len(params) and all(p is s and p._version == ver
                                                                  for p, (s, ver) in zip(params, hit[0])):
            return hit[1]
        with torch.no_grad():
            value = build()
        store[slot] = ([(p, p._version) for p in params], value)
        return value

    def _stacked(self, attn, names):
        mods = [getattr(attn, n) for n in names]
        params = [m.weight for m in mods]
        return self._pack(attn, "|".join(names), params, lambda: torch.cat([p.detach() for p in params], dim=0).contiguous())

    def _project(self, attn, x, names):
        """[attn.<name>(x) for name in names], bias-free, in one launch that reads x once -> tensors (B, L, C), column slices
        of one buffer on the vae_conv path"""
        mods = [getattr(attn, n) for n in names]
        N = mods[0].out_features
        if all(_plain_linear(m, False, len(mods)) and m.weight.is_contiguous() and m.weight.data_ptr() % 16 == 0 for m in mods):
            return ops.linear(x, [m.weight.detach() for m in mods], None, None)
        w = self._stacked(attn, names)
        out = ops.conv_rows(_rows16(x), w)
        return [out[..., i * N:(i + 1) * N] for i in range(len(mods))]

    def _text_kv(self, attn, text):
        """to_k | to_v of the text as one (B, Lt, 2 C) buffer, cached per module by the text tensor's identity and version"""
        w = self._stacked(attn, ("to_k", "to_v"))
        if self.cache_text_kv:
            hit = self._text.get(attn)
            if hit is not None and hit[0] is text and hit[1] == text._version and hit[2] is w:
                return hit[3]
        kv = ops.conv_rows(_rows16(text), w)
        if self.cache_text_kv:
            self._text[attn] = (text, text._version, w, kv)
        return kv

    def _project_out(self, attn, hs):
        lin = attn.to_out[0]
        if _plain_linear(lin, True, 1) and lin.weight.is_contiguous() and lin.weight.data_ptr() % 16 == 0 \
                and lin.bias.is_contiguous():
            return ops.linear(hs, [lin.weight.detach()], [lin.bias.detach()])[0]
        w = self._pack(attn, "to_out.w", [lin.weight], lambda: _rows16(lin.weight.detach()))
        b = self._pack(attn, "to_out.b", [lin.bias], lambda: lin.bias.detach().to(torch.float32).contiguous())
        return ops.conv_rows(_rows16(hs), w, b)

    # ---- the call ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        def refuse(why):
            raise _dropin.refusal(_WHO, "", why)
        if attention_mask is not None:
            refuse("an attention_mask is not supported (the pipeline passes None)")
        if not isinstance(hidden_states, torch.Tensor) or hidden_states.dim() != 3:
            refuse("hidden_states must be (batch, tokens, channels), got a %s input"
                   % ("%d-D" % hidden_states.dim() if isinstance(hidden_states, torch.Tensor) else type(hidden_states).__name__))
        why = self.refusal(attn)
        if why:
            raise _dropin.refusal(_WHO, "the attention module", why)
        text = encoder_hidden_states
        if text is not None and (not isinstance(text, torch.Tensor) or text.dim() != 3 or text.shape[0] != hidden_states.shape[0]):
            refuse("encoder_hidden_states must be (batch, tokens, width) with the batch of hidden_states")
        if hidden_states.shape[-1] != attn.to_q.in_features or (text if text is not None else hidden_states).shape[-1] \
                != attn.to_k.in_features:
            refuse("inputs %d / %d wide, the module projects from %d / %d"
                   % (hidden_states.shape[-1], (text if text is not None else hidden_states).shape[-1], attn.to_q.in_features,
                      attn.to_k.in_features))
        if hidden_states.numel() == 0 or (text is not None and text.numel() == 0):
            refuse("empty inputs")
        for t, nm in ((hidden_states, "hidden_states"), (text, "encoder_hidden_states"), (attn.to_q.weight, "the weights")):
            if t is not None and t.dtype != torch.float16:
                refuse("%s are %s, fp16 only" % (nm, t.dtype))
        for t, nm in ((hidden_states, "hidden_states"), (text, "encoder_hidden_states"), (attn.to_q.weight, "the weights"),
                      (attn.to_out[0].weight, "the weights")):
            if t is not None and not t.is_cuda:
                refuse("%s are on %s, GPU tensors only" % (nm, t.device))

        residual = hidden_states
        heads = int(attn.heads)
        if text is None:
            q, k, v = self._project(attn, hidden_states, ("to_q", "to_k", "to_v"))
        else:
            (q,) = self._project(attn, hidden_states, ("to_q",))
            kv = self._text_kv(attn, text)
            C = kv.shape[-1] // 2
            k, v = kv[..., :C], kv[..., C:]
        head_dim = q.shape[-1] // heads
        scale = 1.0 / math.sqrt(head_dim)
        if head_dim == HEAD_DIM_UNET:
            hs = ops.unet_attention(q, k, v, heads, scale)
        else:
            hs = ops.attention(q, k, v, heads, scale, workspace=self._ws)
        hs = self._project_out(attn, hs)
        hs = attn.to_out[1](hs)
        if getattr(attn, "residual_connection", False):
            hs = hs + residual
        if getattr(attn, "rescale_output_factor", 1.0) != 1.0:  # x / 1.0 == x exactly: skip the elementwise pass
            hs = hs / attn.rescale_output_factor
        return hs


def _set(m, proc):
    if hasattr(m, "set_processor"):
        m.set_processor(proc)
    else:
        m.processor = proc


def patch_unet_attention(model, include_fresco_cross=False, processor=None):
    """set ONE shared UNetAttnProcessor (`processor`, or a new one) on every attention module of `model` (pipe.unet, or the
    ControlNet) whose current processor is not a FRESCOAttnProcessor2_0; with include_fresco_cross also on the modules whose
    name ends in `.attn2` and that carry a FRESCO processor (on cross-attention that processor does nothing FRESCO-specific).
    An attention module is a module that has to_q, to_k, to_v, to_out, heads and a processor.  Every module is checked first:
    one outside what the processor computes raises NotImplementedError with its name before anything is patched.  Returns the
    number of modules patched; call it after apply_FRESCO_attn.  unpatch_unet_attention puts the previous processors back."""
    unpatch_unet_attention(model)
    chosen = [(name, m) for name, m in _dropin.find(model, PARTS)
              if not isinstance(m.processor, FRESCOAttnProcessor2_0) or (include_fresco_cross and name.endswith(".attn2"))]
    _dropin.check_all(_WHO, chosen, UNetAttnProcessor)
    proc = processor if processor is not None else UNetAttnProcessor()
    for _, m in chosen:
        m.__dict__[_ATTR] = m.processor
        _set(m, proc)
    return len(chosen)


def unpatch_unet_attention(model):
    """the processors from before patch_unet_attention again; returns the number of modules restored"""
    count = 0
    for _, m in model.named_modules():
        if _ATTR in vars(m):
            _set(m, m.__dict__.pop(_ATTR))
            count += 1
    return count
