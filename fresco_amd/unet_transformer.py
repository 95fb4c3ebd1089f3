"""Transformer2DModel of the SD-1.5 UNet and ControlNet on this package's kernels, for fp16 pipelines:
everything of the module except its attention layers, which stay the caller's modules with whatever processor is set on them
(FRESCO's on `attn1` of the decoder).

`UNetTransformer.from_module(transformer)` reads one module's weights; `UNetTransformer(state_dict, prefix, attentions)`
packs them from a state dict and takes the attention modules as a list of (attn1, attn2) pairs;
`patch_unet_transformers(model)` replaces `forward` on every transformer of `pipe.unet` or of the ControlNet.  A call with
B blocks is 3 + 6 B launches into libfresco_hip.so (include/fresco_unet.h, fresco_unet_tf.h, fresco_vae.h) around 2 B calls
of the attention modules:

  1. unet_groupnorm(x, eps of norm, no SiLU)        norm
  2. vae_conv 1 x 1 + bias                          proj_in -> tokens (n, HW, D); all rows of all images as ONE run of rows
  per block:
  3. unet_layernorm(h)                              norm1
     block.attn1(y, encoder_hidden_states=None, attention_mask=None, **cross_attention_kwargs)
  4. unet_layernorm(a, residual=h) -> y, h          h = a + h rounded once, norm2 of the fp32 sum
     block.attn2(y, encoder_hidden_states=encoder_hidden_states, attention_mask=None, **cross_attention_kwargs)
  5. unet_layernorm(a, residual=h) -> y, h          norm3
  6. unet_geglu(y)                                  ff.net.0: value * gelu(gate); the (rows, 8 D) projection is never written
  7. vae_conv 1 x 1 + bias + residual h             ff.net.2
  last:
  8. vae_conv 1 x 1 + bias + residual x (NHWC)      proj_out

This is diffusers 0.19.3's `Transformer2DModel.forward` / `BasicTransformerBlock.forward` for a continuous input with 1 x 1
convolutions as `proj_in` / `proj_out` (`use_linear_projection=False`), plain affine LayerNorms, `attn2` present, a GEGLU
feed-forward, no dropout and no feed-forward chunking.  Against PyTorch's fp16 module each residual sum is rounded to fp16
once and the norm behind it reads the fp32 sum; the GEGLU's value and gate are never rounded.

Layout: tensors are logical NCHW, as diffusers passes them, and NHWC in memory.  An input that is `channels_last`-contiguous
(what a patched resnet hands over) is read in place, any other is converted once; the output is `(n, C, H, W)` in
`torch.channels_last` unless `memory_format=torch.contiguous_format` asks for the plain layout (one more copy).

There is no fallback: a module outside this configuration, not fp16 or not on the GPU raises.  diffusers is not installed
where this package is built and tested: the parameter names, the attributes and the forward come from its published source
(models/transformer_2d.py, models/attention.py) and are UNVERIFIED against the real modules.
"""
import torch

from . import _dropin, _lib, ops
from ._dropin import f32 as _f32
from .vae import pack_conv_weight

GROUPS = 32
PARTS = ("norm", "proj_in", "transformer_blocks", "proj_out")    # what makes a module a transformer for patch_unet_transformers
BLOCK_PARTS = ("norm1", "attn1", "norm2", "attn2", "norm3", "ff")
_ATTR = "_fresco_unet_transformer"
_WHO = "fresco_amd.unet_transformer"


def pack_geglu_weight(weight, bias):
    """diffusers' `ff.net.0.proj` (weight (2 inner, K): rows 0 .. inner - 1 the value, inner .. 2 inner - 1 the gate; bias
    (2 inner)) in unet_geglu's order: blocks of 64 rows, the 32 value rows of channels 32 b .. 32 b + 31 and then their 32
    gate rows.  -> (weight fp16 (2 inner, K), bias fp32 (2 inner)); value row c is at packed row 64 (c // 32) + c % 32, its
    gate 32 rows on."""
    if weight.dim() != 2 or weight.shape[0] % 2 or tuple(bias.shape) != (weight.shape[0],):
        raise ValueError("%s: pack_geglu_weight takes a (2 inner, K) weight and a (2 inner) bias, got %s and %s"
                         % (_WHO, tuple(weight.shape), tuple(bias.shape)))
    inner, K = weight.shape[0] // 2, weight.shape[1]
    if inner % ops.UNET_GEGLU_STEP or K % ops.UNET_GEGLU_STEP:
        raise ValueError("%s: a GEGLU of %d -> %d channels; inner and K must be multiples of %d"
                         % (_WHO, K, inner, ops.UNET_GEGLU_STEP))

    def order(t):
        tail = tuple(t.shape[1:])
        v, g = t[:inner].reshape((inner // 32, 1, 32) + tail), t[inner:].reshape((inner // 32, 1, 32) + tail)
        return torch.cat([v, g], dim=1).reshape((2 * inner,) + tail)
    return order(weight.detach()).to(torch.float16).contiguous(), order(bias.detach()).to(torch.float32).contiguous()


class UNetTransformerOutput:
    """what `return_dict=True` gives: `.sample`, as diffusers' Transformer2DModelOutput"""

    def __init__(self, sample):
        self.sample = sample


class _Block:
    pass


class UNetTransformer:
    """One Transformer2DModel (C channels, blocks of width D) on HIP kernels around its own attention modules."""

    def __init__(self, state_dict, prefix, attentions, norm_eps=1e-6, ln_eps=1e-5, device=None,
                 memory_format=torch.channels_last):
        attentions = list(attentions)
        names = ["norm", "proj_in", "proj_out"]
        for i in range(len(attentions)):
            b = "transformer_blocks.%d." % i
            names += [b + "norm1", b + "norm2", b + "norm3", b + "ff.net.0.proj", b + "ff.net.2"]
        sd, what = _dropin.intake(state_dict, prefix, [p + s for p in names for s in (".weight", ".bias")], _WHO,
                                  "the transformer")
        if not attentions or any(len(p) != 2 or not callable(p[0]) or not callable(p[1]) for p in attentions):
            raise ValueError("%s: attentions must be a list of (attn1, attn2) modules, one pair per block" % what)
        if sd["proj_in.weight"].dim() != 4 or tuple(sd["proj_in.weight"].shape[2:]) != (1, 1):
            raise NotImplementedError("%s: proj_in is not a 1 x 1 convolution (use_linear_projection?)" % what)
        D, C = (int(v) for v in sd["proj_in.weight"].shape[:2])
        why = _width_refusal(C, D, int(sd["transformer_blocks.0.ff.net.0.proj.weight"].shape[0]) // 2)
        if why:
            raise NotImplementedError("%s: %s" % (what, why))
        inner = int(sd["transformer_blocks.0.ff.net.0.proj.weight"].shape[0]) // 2
        shapes = {"norm.weight": (C,), "norm.bias": (C,), "proj_in.weight": (D, C, 1, 1), "proj_in.bias": (D,),
                  "proj_out.weight": (C, D, 1, 1), "proj_out.bias": (C,)}
        for i in range(len(attentions)):
            b = "transformer_blocks.%d." % i
            for nm in ("norm1", "norm2", "norm3"):
                shapes.update({b + nm + ".weight": (D,), b + nm + ".bias": (D,)})
            shapes.update({b + "ff.net.0.proj.weight": (2 * inner, D), b + "ff.net.0.proj.bias": (2 * inner,),
                           b + "ff.net.2.weight": (D, inner), b + "ff.net.2.bias": (D,)})
        _dropin.check_shapes(sd, shapes, what, only=False)
        dev = torch.device(device) if device is not None else sd["proj_in.weight"].device
        self.channels, self.width, self.inner = C, D, inner
        self.norm_eps, self.ln_eps = float(norm_eps), float(ln_eps)
        self.device, self.memory_format = dev, memory_format
        self.gn_g, self.gn_b = _f32(sd["norm.weight"], dev), _f32(sd["norm.bias"], dev)
        self.w_in, self.b_in = pack_conv_weight(sd["proj_in.weight"]).to(dev), _f32(sd["proj_in.bias"], dev)
        self.w_out, self.b_out = pack_conv_weight(sd["proj_out.weight"]).to(dev), _f32(sd["proj_out.bias"], dev)
        self.blocks = []
        for i, (attn1, attn2) in enumerate(attentions):
            b = "transformer_blocks.%d." % i
            blk = _Block()
            blk.attn1, blk.attn2 = attn1, attn2
            blk.ln = [(_f32(sd[b + nm + ".weight"], dev), _f32(sd[b + nm + ".bias"], dev)) for nm in ("norm1", "norm2", "norm3")]
            w, bias = pack_geglu_weight(sd[b + "ff.net.0.proj.weight"], sd[b + "ff.net.0.proj.bias"])
            blk.w_ff1, blk.b_ff1 = w.to(dev), bias.to(dev)
            blk.w_ff2 = sd[b + "ff.net.2.weight"].detach().to(dev, torch.float16).contiguous()
            blk.b_ff2 = _f32(sd[b + "ff.net.2.bias"], dev)
            self.blocks.append(blk)

    @staticmethod
    def refusal(tf):
        """why `tf` (a module with PARTS) is outside the supported configuration, or None"""
        for part in PARTS:
            if getattr(tf, part, None) is None:
                return "has no %s" % part
        dtypes = {p.dtype for part in ("norm", "proj_in", "proj_out") for p in getattr(tf, part).parameters()}
        for blk in tf.transformer_blocks:
            for part in ("norm1", "norm2", "norm3", "ff"):
                sub = getattr(blk, part, None)
                if isinstance(sub, torch.nn.Module):
                    dtypes |= {p.dtype for p in sub.parameters()}
        if dtypes != {torch.float16}:
            return "is %s, fp16 modules only" % "/".join(sorted(str(d) for d in dtypes))
        w_in = getattr(tf.proj_in, "weight", None)
        if getattr(tf, "use_linear_projection", False) or not isinstance(tf.proj_in, torch.nn.Conv2d) or w_in.dim() != 4 \
                or tuple(w_in.shape[2:]) != (1, 1) or not isinstance(tf.proj_out, torch.nn.Conv2d) \
                or tuple(tf.proj_out.weight.shape[2:]) != (1, 1):
            return "projects with a Linear (use_linear_projection), only 1 x 1 convolutions"
        if getattr(tf.proj_in, "bias", None) is None or getattr(tf.proj_out, "bias", None) is None:
            return "has a projection without a bias"
        if getattr(tf.norm, "num_groups", None) != GROUPS:
            return "GroupNorm of %s groups, only %d" % (getattr(tf.norm, "num_groups", None), GROUPS)
        if getattr(tf.norm, "weight", None) is None:
            return "GroupNorm without affine parameters"
        if len(tf.transformer_blocks) == 0:
            return "has no transformer block"
        D, C = int(w_in.shape[0]), int(w_in.shape[1])
        inner0 = None
        eps = set()
        for i, blk in enumerate(tf.transformer_blocks):
            at = "transformer_blocks.%d" % i
            for part in BLOCK_PARTS:
                if part != "attn2" and getattr(blk, part, None) is None:
                    return "%s has no %s" % (at, part)
            if getattr(blk, "attn2", None) is None:
                return "%s.attn2 is None" % at
            if getattr(blk, "only_cross_attention", False):
                return "%s is only_cross_attention" % at
            for nm in ("norm1", "norm2", "norm3"):
                norm = getattr(blk, nm)
                if type(norm) is not torch.nn.LayerNorm or norm.weight is None or norm.bias is None \
                        or getattr(blk, "use_ada_layer_norm", False) or getattr(blk, "use_ada_layer_norm_zero", False):
                    return "%s.%s is %s, only a plain nn.LayerNorm with affine parameters" % (at, nm, type(norm).__name__)
                if tuple(norm.normalized_shape) != (D,):
                    return "%s.%s normalises %s, the block is %d wide" % (at, nm, tuple(norm.normalized_shape), D)
                eps.add(float(norm.eps))
            if getattr(blk, "_chunk_size", None) is not None:
                return "%s chunks its feed-forward (_chunk_size = %s)" % (at, blk._chunk_size)
            net = getattr(blk.ff, "net", None)
            if net is None or len(net) != 3 or not isinstance(getattr(net[0], "proj", None), torch.nn.Linear):
                return "%s.ff is not a GEGLU feed-forward (its first layer has no proj)" % at
            if type(net[0]).__name__ not in ("GEGLU",):
                return "%s.ff.net.0 is %s, only GEGLU" % (at, type(net[0]).__name__)
            for sub in blk.ff.modules():
                if isinstance(sub, torch.nn.Dropout) and sub.p != 0.0:
                    return "%s.ff has dropout %s" % (at, sub.p)
            if not isinstance(net[2], torch.nn.Linear) or net[0].proj.bias is None or net[2].bias is None:
                return "%s.ff.net.2 is not a Linear with a bias" % at
            w1, w2 = net[0].proj.weight, net[2].weight
            inner = int(w1.shape[0]) // 2
            if int(w1.shape[1]) != D or w1.shape[0] % 2 or tuple(w2.shape) != (D, inner):
                return "%s.ff is %s then %s, the block is %d wide" % (at, tuple(w1.shape), tuple(w2.shape), D)
            if inner0 is not None and inner != inner0:
                return "%s.ff is %d wide inside, the first block's %d" % (at, inner, inner0)
            inner0 = inner
        if len(eps) != 1:
            return "LayerNorms of several values of eps"
        if tuple(tf.proj_out.weight.shape[:2]) != (C, D):
            return "proj_out is %s, expected %d -> %d" % (tuple(tf.proj_out.weight.shape), D, C)
        return _width_refusal(C, D, inner0)

    @classmethod
    def from_module(cls, tf, device=None, memory_format=torch.channels_last, name="the transformer"):
        why = cls.refusal(tf)
        if why:
            raise _dropin.refusal(_WHO, name, why)
        sd = {k: v for k, v in tf.state_dict().items() if ".attn1." not in k and ".attn2." not in k}
        return cls(sd, "", [(b.attn1, b.attn2) for b in tf.transformer_blocks], float(tf.norm.eps),
                   float(tf.transformer_blocks[0].norm1.eps), device=device, memory_format=memory_format)

    def _attend(self, attn, y, enc, kw, shape):
        a = attn(y, encoder_hidden_states=enc, attention_mask=None, **kw)
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float16 or tuple(a.shape) != shape:
            raise TypeError("%s: an attention module returned %s, expected a fp16 tensor of %s"
                            % (_WHO, (a.dtype, tuple(a.shape)) if isinstance(a, torch.Tensor) else type(a).__name__, shape))
        return _dropin.rows16(a)

    @torch.no_grad()
    def __call__(self, hidden_states, encoder_hidden_states=None, timestep=None, class_labels=None, cross_attention_kwargs=None,
                 attention_mask=None, encoder_attention_mask=None, return_dict=True, *, memory_format=None, taps=None):
        """hidden_states (n, C, H, W) fp16 on the GPU -> Transformer2DModel.forward's result: an object with `.sample`
        (n, C, H, W) fp16, or with return_dict=False the 1-tuple of it.  taps: a dict that receives "geglu", the first block's
        GEGLU output (n, HW, inner), and "tokens", the tokens (n, HW, D) after the last block."""
        for v, nm in ((timestep, "timestep"), (class_labels, "class_labels"), (attention_mask, "attention_mask"),
                      (encoder_attention_mask, "encoder_attention_mask")):
            if v is not None:
                raise _dropin.refusal(_WHO, nm, "is not supported (the pipeline passes None)")
        x = hidden_states
        if not isinstance(x, torch.Tensor):
            raise TypeError("%s: hidden_states must be a tensor" % _WHO)
        if x.dtype != torch.float16:
            raise TypeError("%s: fp16 hidden_states only (got %s)" % (_WHO, x.dtype))
        if x.dim() != 4 or x.shape[1] != self.channels or x.numel() == 0:
            raise ValueError("%s: hidden_states must be (n, %d, H, W), got %s" % (_WHO, self.channels, tuple(x.shape)))
        fmt = self.memory_format if memory_format is None else memory_format
        _dropin.check_format(_WHO, fmt)
        ops._need_gpu(x)
        kw = dict(cross_attention_kwargs) if cross_attention_kwargs is not None else {}
        n, C, H, W = x.shape
        xn = _dropin.nhwc(x)
        h = ops.unet_groupnorm(xn, self.gn_g, self.gn_b, self.norm_eps, silu=False)
        shape = (n, H * W, self.width)
        h = ops.conv_rows(h.view(n, H * W, C), self.w_in, self.b_in)      # tokens: all rows of all images as one run of rows
        for i, blk in enumerate(self.blocks):
            y = ops.unet_layernorm(h, blk.ln[0][0], blk.ln[0][1], self.ln_eps)
            a = self._attend(blk.attn1, y, None, kw, shape)
            y, h = ops.unet_layernorm(a, blk.ln[1][0], blk.ln[1][1], self.ln_eps, residual=h, want_sum=True)
            a = self._attend(blk.attn2, y, encoder_hidden_states, kw, shape)
            y, h = ops.unet_layernorm(a, blk.ln[2][0], blk.ln[2][1], self.ln_eps, residual=h, want_sum=True)
            g = ops.unet_geglu(y, blk.w_ff1, blk.b_ff1)
            if taps is not None and i == 0:
                taps["geglu"] = g
            h = ops.conv_rows(g, blk.w_ff2, blk.b_ff2, residual=h)
        if taps is not None:
            taps["tokens"] = h
        out = _dropin.nchw(ops.conv_rows(h.view(n, H, W, self.width), self.w_out, self.b_out, residual=xn), fmt)
        return UNetTransformerOutput(out) if return_dict else (out,)


def _width_refusal(C, D, inner):
    if not ops.unet_gn_channels(C):
        return "%d channels, the GroupNorm kernel takes multiples of %d in %d .. %d" % (C, ops.UNET_GN_STEP, ops.UNET_GN_MIN,
                                                                                        ops.UNET_GN_MAX)
    if not ops.unet_ln_channels(D) or D % ops.UNET_GEGLU_STEP:
        return "blocks %d wide, the kernels take multiples of %d in %d .. %d" % (D, ops.UNET_GEGLU_STEP, ops.UNET_LN_MIN,
                                                                                ops.UNET_LN_MAX)
    if inner <= 0 or inner % ops.UNET_GEGLU_STEP:
        return "a feed-forward %d wide inside, the GEGLU kernel takes multiples of %d" % (inner, ops.UNET_GEGLU_STEP)
    return None


def patch_unet_transformers(model, memory_format=torch.channels_last):
    """replace `forward` on every module of `model` (pipe.unet, a ControlNet) that has norm, proj_in, transformer_blocks and
    proj_out by a UNetTransformer built from it; returns the number of modules patched.  The blocks' attention modules stay
    as they are and are called with whatever processor is set on them at call time.  A matching module outside the supported
    configuration raises NotImplementedError with its name, before anything is patched.  The modules' own methods stay on
    their class: unpatch_unet_transformers removes the bindings.  The weights are copied: patch again after loading others."""
    return _dropin.patch(model, UNetTransformer, PARTS, _WHO, _ATTR, memory_format)


def unpatch_unet_transformers(model):
    """the modules' own forwards again; returns the number of modules restored"""
    return _dropin.unpatch(model, _ATTR)
