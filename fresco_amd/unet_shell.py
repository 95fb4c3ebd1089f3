"""What is left of the SD-1.5 UNet and ControlNet around their resnets, transformer blocks and attention, on this package's
kernels, for fp16 pipelines (include/fresco_unet_shell.h, include/fresco_vae.h, include/fresco_unet.h):

  UNetDownsample           Downsample2D: Conv2d(c, c, 3, stride 2, padding 1)       unet_conv3, stride 2
  UNetUpsample             Upsample2D: nearest 2x + Conv2d(c, c, 3, padding 1)      vae_conv with up2: the 2x plane is never written
  UNetConvIn               conv_in, 4 -> 320                                        unet_input (4 -> 32 channels) + vae_conv
  UNetConvOut              conv_norm_out + conv_act + conv_out                      unet_groupnorm(SiLU) + vae_conv -> NCHW
  UNetTimeEmbedding        time_proj + time_embedding (linear_1, SiLU, linear_2)    two unet_time_linear launches
  ControlNetCondEmbedding  ControlNetConditioningEmbedding: eight 3 x 3 + SiLU      unet_input (3 -> 32) + eight unet_conv3
  UNetZeroConv             controlnet_down_blocks[i], controlnet_mid_block (1 x 1)  vae_conv, ksize 1

`patch_unet_shell(model)` binds whichever of these `model` has and returns the counts per kind; `unpatch_unet_shell(model)`
removes the bindings.  With patch_unet_resnets, patch_unet_transformers and patch_unet_attention a patched model runs no
PyTorch convolution, GEMM, normalisation, interpolation or activation kernel.  What stays in PyTorch: `sample *
conditioning_scale` and the residual additions of `ControlNetModel.forward` and of the pipeline's own forward -- they are no
module's forward -- and the small copies at a drop-in's boundary.  bf16 is not supported.

Layout: tensors are logical NCHW, as diffusers passes them, and NHWC in memory (`torch.channels_last`) in and out, as the
resnet drop-in; conv_in takes the latents in any layout and conv_out returns plain NCHW (four channels).  Weights are COPIED
at patch time: patch again after loading others.

THE TIME EMBEDDING.  diffusers computes `time_proj(timesteps)` (fp32 sinusoid), `.to(sample.dtype)` and then
`time_embedding(...)`.  Under the patch `time_proj` returns the fp32 timesteps themselves as a marker -- one value per image
-- and keeps them; `time_embedding` recognises the marker (1-D, whatever dtype the model cast it to) and runs
unet_time_linear twice: sinusoid + linear_1, then SiLU + linear_2.  A 2-D input (a sinusoid computed elsewhere) is refused.

THE CONDITION CACHE.  The embedding's result is kept and reused while a call passes the same condition tensor OBJECT at the
same `_version` (the rule UNetAttnProcessor uses for the text): the pipeline passes the same tensor on every step.  An
in-place edit bumps the version and computes again; `clear()` drops it; `cache=False` computes on every call.

There is no fallback: a module outside these configurations, not fp16 or not on the GPU raises, by name, before anything is
patched.  diffusers is not installed where this package is built and tested: the attribute and parameter names come from its
published source (models/resnet.py, models/embeddings.py, models/controlnet.py, models/unet_2d_condition.py of 0.19.3) and
are UNVERIFIED against the real modules.
"""
import torch
import torch.nn as nn

from . import _dropin, _lib, ops
from ._dropin import f32 as _f32
from .vae import pack_conv_weight

_ATTR = "_fresco_unet_shell"
_WHO = "fresco_amd.unet_shell"
CPAD = ops.VAE_CIN_PAD  # 32: the convolution's K chunk
KINDS = ("down", "up", "conv_in", "conv_out", "time", "cond_embedding", "zero_conv")
DOWN_PARTS = ("conv", "use_conv", "padding")
UP_PARTS = ("conv", "use_conv", "use_conv_transpose")
EMBED_PARTS = ("conv_in", "blocks", "conv_out")


def _pad32(c):
    return (c + CPAD - 1) // CPAD * CPAD


def _fp16_only(m):
    dtypes = {p.dtype for p in m.parameters()}
    if dtypes and dtypes != {torch.float16}:
        return "is %s, fp16 modules only" % "/".join(sorted(str(d) for d in dtypes))
    return None


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _conv_is(conv, k, stride, pad):
    """why `conv` is not Conv2d(k x k, stride, padding pad, dilation 1, groups 1, zero padding, with a bias), or None"""
    if not isinstance(conv, nn.Conv2d):
        return "is %s, not a Conv2d" % type(conv).__name__
    if _pair(conv.kernel_size) != (k, k) or _pair(conv.stride) != (stride, stride) or _pair(conv.padding) != (pad, pad):
        return "is %s stride %s padding %s, only %d x %d stride %d padding %d" % (
            "%d x %d" % _pair(conv.kernel_size), _pair(conv.stride)[0], _pair(conv.padding), k, k, stride, pad)
    if _pair(conv.dilation) != (1, 1) or conv.groups != 1 or getattr(conv, "padding_mode", "zeros") != "zeros":
        return "is dilated, grouped or not zero-padded"
    if conv.bias is None:
        return "has no bias"
    return None


def _pack(conv, cin_pad=None, cout_pad=None):
    """(packed fp16 weight (cout', k k cin'), fp32 bias (cout')) of a Conv2d on its own device: input channels zero-padded to
    cin_pad, output channels to cout_pad by zero rows and zero biases"""
    w = pack_conv_weight(conv.weight, cin_pad)
    b = _f32(conv.bias, conv.weight.device)
    cout = w.shape[0]
    if cout_pad is not None and cout_pad > cout:
        w = torch.cat([w, w.new_zeros(cout_pad - cout, w.shape[1])])
        b = torch.cat([b, b.new_zeros(cout_pad - cout)])
    return w.to(conv.weight.device).contiguous(), b.contiguous()


def _take(x, what, c):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: %s expects a tensor" % (_WHO, what))
    if x.dtype != torch.float16:
        raise TypeError("%s: %s takes fp16 only (got %s)" % (_WHO, what, x.dtype))
    if x.dim() != 4 or x.shape[1] != c or x.numel() == 0:
        raise ValueError("%s: %s takes (n, %d, H, W), got %s" % (_WHO, what, c, tuple(x.shape)))
    ops._need_gpu(x)


class _DropIn:
    """what the seven share: the name for messages and the output layout"""
    kind = None

    def _init(self, name, memory_format):
        _dropin.check_format(_WHO, memory_format)
        self.name, self.memory_format = name, memory_format

    @classmethod
    def from_module(cls, m, memory_format=torch.channels_last, name=None):
        why = cls.refusal(m)
        if why:
            raise _dropin.refusal(_WHO, name or cls.__name__, why)
        return cls(m, memory_format=memory_format, name=name or cls.__name__)


class UNetDownsample(_DropIn):
    """Downsample2D(use_conv=True, padding=1): (n, c, H, W) -> (n, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1)"""
    kind = "down"

    def __init__(self, m, memory_format=torch.channels_last, name="downsampler"):
        self._init(name, memory_format)
        self.cin, self.cout = m.conv.in_channels, m.conv.out_channels
        self.w, self.b = _pack(m.conv)

    @staticmethod
    def refusal(m):
        if not m.use_conv:
            return "has use_conv=False (average pooling)"
        if m.padding != 1:
            return "has padding %s, only 1" % (m.padding,)
        why = _conv_is(m.conv, 3, 2, 1)
        if why:
            return "conv " + why
        if m.conv.in_channels % CPAD:
            return "conv reads %d channels, not a multiple of %d" % (m.conv.in_channels, CPAD)
        return _fp16_only(m)

    @torch.no_grad()
    def __call__(self, x, *args, **kwargs):
        _take(x, self.name, self.cin)
        return _dropin.nchw(ops.unet_conv3(_dropin.nhwc(x), self.w, self.b, stride=2), self.memory_format)


class UNetUpsample(_DropIn):
    """Upsample2D(use_conv=True): conv(nearest 2x(x)): (n, c, H, W) -> (n, cout, 2 H, 2 W); the 2x plane stays unwritten"""
    kind = "up"

    def __init__(self, m, memory_format=torch.channels_last, name="upsampler"):
        self._init(name, memory_format)
        self.cin, self.cout = m.conv.in_channels, m.conv.out_channels
        self.w, self.b = _pack(m.conv)

    @staticmethod
    def refusal(m):
        if m.use_conv_transpose:
            return "has use_conv_transpose=True"
        if not m.use_conv:
            return "has use_conv=False"
        why = _conv_is(m.conv, 3, 1, 1)
        if why:
            return "conv " + why
        if m.conv.in_channels % CPAD:
            return "conv reads %d channels, not a multiple of %d" % (m.conv.in_channels, CPAD)
        return _fp16_only(m)

    @torch.no_grad()
    def __call__(self, x, output_size=None, *args, **kwargs):
        _take(x, self.name, self.cin)
        n, _, H, W = x.shape
        if output_size is not None and tuple(int(s) for s in output_size) != (2 * H, 2 * W):
            raise _dropin.refusal(_WHO, self.name, "was asked for output_size %s from a %d x %d plane, only None or (%d, %d)"
                                  % (tuple(output_size), H, W, 2 * H, 2 * W))
        out = ops.vae_conv(_dropin.nhwc(x), self.w, self.b, n, 2 * H, 2 * W, self.cin, self.cout, 3, up2=True)
        return _dropin.nchw(out, self.memory_format)


class UNetConvIn(_DropIn):
    """conv_in: Conv2d(c <= 32, cout, 3, padding 1) on latents in any layout"""
    kind = "conv_in"

    def __init__(self, m, memory_format=torch.channels_last, name="conv_in"):
        self._init(name, memory_format)
        self.cin, self.cout = m.in_channels, m.out_channels
        self.w, self.b = _pack(m, cin_pad=CPAD)

    @staticmethod
    def refusal(m):
        why = _conv_is(m, 3, 1, 1)
        if why:
            return why
        if m.in_channels > CPAD:
            return "reads %d channels, at most %d" % (m.in_channels, CPAD)
        return _fp16_only(m)

    @torch.no_grad()
    def __call__(self, x, *args, **kwargs):
        _take(x, self.name, self.cin)
        n, _, H, W = x.shape
        h = ops.unet_input(x.contiguous(), CPAD)
        return _dropin.nchw(ops.vae_conv(h, self.w, self.b, n, H, W, CPAD, self.cout, 3), self.memory_format)


class UNetConvOut(_DropIn):
    """conv_norm_out + conv_act + conv_out: `norm` is bound on conv_norm_out (GroupNorm and SiLU in one launch), `act` on
    conv_act (returns its argument), `conv` on conv_out (-> plain NCHW)"""
    kind = "conv_out"

    def __init__(self, m, memory_format=torch.channels_last, name="conv_out"):
        self._init(name, memory_format)
        norm, conv = m.conv_norm_out, m.conv_out
        self.cin, self.cout, self.eps = conv.in_channels, conv.out_channels, float(norm.eps)
        self.g, self.beta = _f32(norm.weight, norm.weight.device), _f32(norm.bias, norm.weight.device)
        self.w, self.b = _pack(conv)

    @staticmethod
    def refusal(m):
        """m: the model, with conv_norm_out, conv_act and conv_out"""
        norm, act, conv = m.conv_norm_out, m.conv_act, m.conv_out
        if not isinstance(act, nn.SiLU):
            return "conv_act is %s, only SiLU" % type(act).__name__
        if not isinstance(norm, nn.GroupNorm) or norm.num_groups != 32 or not norm.affine:
            return "conv_norm_out is not an affine GroupNorm of 32 groups"
        if not ops.unet_gn_channels(norm.num_channels):
            return "conv_norm_out has %d channels, the kernel takes multiples of %d in %d .. %d" % (
                norm.num_channels, ops.UNET_GN_STEP, ops.UNET_GN_MIN, ops.UNET_GN_MAX)
        why = _conv_is(conv, 3, 1, 1)
        if why:
            return "conv_out " + why
        if conv.in_channels != norm.num_channels:
            return "conv_out reads %d channels behind a norm of %d" % (conv.in_channels, norm.num_channels)
        return _fp16_only(norm) or _fp16_only(conv)

    @torch.no_grad()
    def norm(self, x, *args, **kwargs):
        _take(x, self.name + "'s norm", self.cin)
        return _dropin.nchw(ops.unet_groupnorm(_dropin.nhwc(x), self.g, self.beta, self.eps, silu=True), torch.channels_last)

    @staticmethod
    def act(x, *args, **kwargs):
        return x

    @torch.no_grad()
    def conv(self, x, *args, **kwargs):
        _take(x, self.name, self.cin)
        n, _, H, W = x.shape
        return ops.vae_conv(_dropin.nhwc(x), self.w, self.b, n, H, W, self.cin, self.cout, 3, out_kind=_lib.VAE_OUT_F16_NCHW)

    def __call__(self, x):
        return self.conv(self.act(self.norm(x)))


class UNetTimeEmbedding(_DropIn):
    """time_proj + time_embedding: `proj` is bound on time_proj (returns the fp32 timesteps as a marker and keeps them), the
    object itself on time_embedding"""
    kind = "time"

    def __init__(self, m, memory_format=torch.channels_last, name="time_embedding"):
        self._init(name, memory_format)
        l1, l2 = m.time_embedding.linear_1, m.time_embedding.linear_2
        dev = l1.weight.device
        self.K, self.inner, self.cout = l1.in_features, l1.out_features, l2.out_features
        self.w1, self.b1 = l1.weight.detach().to(dev, torch.float16).contiguous(), _f32(l1.bias, dev)
        self.w2, self.b2 = l2.weight.detach().to(dev, torch.float16).contiguous(), _f32(l2.bias, dev)
        self._kept = None

    @staticmethod
    def refusal(m):
        """m: the model, with time_proj and time_embedding"""
        tp, te = m.time_proj, m.time_embedding
        for part in ("linear_1", "linear_2"):
            lin = getattr(te, part, None)
            if not isinstance(lin, nn.Linear) or lin.bias is None:
                return "time_embedding.%s is not a Linear with a bias" % part
        if getattr(te, "cond_proj", None) is not None:
            return "time_embedding has a cond_proj"
        if getattr(te, "post_act", None) is not None:
            return "time_embedding has a post_act"
        if not isinstance(getattr(te, "act", None), nn.SiLU):
            return "time_embedding's act is %s, only SiLU" % type(getattr(te, "act", None)).__name__
        if not getattr(tp, "flip_sin_to_cos", False):
            return "time_proj has flip_sin_to_cos=False"
        if float(getattr(tp, "downscale_freq_shift", 0)) != 0.0:
            return "time_proj has downscale_freq_shift %s, only 0" % (tp.downscale_freq_shift,)
        K = te.linear_1.in_features
        if getattr(tp, "num_channels", K) != K or K % 8 or te.linear_1.out_features % 8 \
                or te.linear_2.in_features != te.linear_1.out_features:
            return "time_proj of %s channels into %d -> %d -> %d (multiples of 8 that chain)" % (
                getattr(tp, "num_channels", None), K, te.linear_1.out_features, te.linear_2.out_features)
        return _fp16_only(te)

    @torch.no_grad()
    def proj(self, timesteps, *args, **kwargs):
        if not isinstance(timesteps, torch.Tensor) or timesteps.dim() != 1 or timesteps.numel() == 0:
            raise ValueError("%s: %s's time_proj takes a 1-D tensor of timesteps" % (_WHO, self.name))
        ops._need_gpu(timesteps)
        self._kept = timesteps.to(torch.float32).contiguous()
        return self._kept

    @torch.no_grad()
    def __call__(self, marker, condition=None, *args, **kwargs):
        if condition is not None:
            raise _dropin.refusal(_WHO, self.name, "was given a condition (timestep_cond)")
        if not isinstance(marker, torch.Tensor) or marker.dim() != 1:
            raise _dropin.refusal(_WHO, self.name, "takes what its patched time_proj returned (the timesteps, 1-D), not a "
                                  "sinusoid computed elsewhere")
        kept = self._kept
        ts = kept if kept is not None and kept.shape == marker.shape and kept.device == marker.device \
            else marker.to(torch.float32).contiguous()
        if ts.shape[0] > ops.UNET_TIME_MAX_N:
            raise _dropin.refusal(_WHO, self.name, "was given %d timesteps, at most %d" % (ts.shape[0], ops.UNET_TIME_MAX_N))
        h = ops.unet_time_linear(ts, self.w1, self.b1)
        return ops.unet_time_linear(h, self.w2, self.b2)


class ControlNetCondEmbedding(_DropIn):
    """ControlNetConditioningEmbedding: conv_in, blocks[0 .. 5], conv_out, SiLU after all but conv_out; (n, 3, H, W) ->
    (n, 320, H / 8, W / 8)"""
    kind = "cond_embedding"

    def __init__(self, m, memory_format=torch.channels_last, name="controlnet_cond_embedding", cache=True):
        self._init(name, memory_format)
        convs = [m.conv_in] + list(m.blocks) + [m.conv_out]
        self.cin, self.cout = m.conv_in.in_channels, m.conv_out.out_channels
        self.layers = []   # (packed weight, bias, stride, SiLU)
        for i, c in enumerate(convs):
            last = i == len(convs) - 1
            w, b = _pack(c, cin_pad=_pad32(c.in_channels), cout_pad=None if last else _pad32(c.out_channels))
            self.layers.append((w, b, _pair(c.stride)[0], not last))
        self.cache = bool(cache)
        self._hit = None   # (condition tensor, version, output)

    def clear(self):
        """drop the cached embedding"""
        self._hit = None

    @staticmethod
    def refusal(m):
        convs = [("conv_in", m.conv_in)] + [("blocks.%d" % i, c) for i, c in enumerate(m.blocks)] + [("conv_out", m.conv_out)]
        prev = None
        for label, c in convs:
            if not isinstance(c, nn.Conv2d):
                return "%s is %s, not a Conv2d" % (label, type(c).__name__)
            why = _conv_is(c, 3, _pair(c.stride)[0], 1)
            if why is None and _pair(c.stride)[0] not in (1, 2):
                why = "has stride %d, only 1 or 2" % _pair(c.stride)[0]
            if why:
                return "%s %s" % (label, why)
            if prev is not None and c.in_channels != prev:
                return "%s reads %d channels behind %d" % (label, c.in_channels, prev)
            prev = c.out_channels
        if m.conv_in.in_channels > CPAD:
            return "conv_in reads %d channels, at most %d" % (m.conv_in.in_channels, CPAD)
        return _fp16_only(m)

    @torch.no_grad()
    def __call__(self, cond, *args, **kwargs):
        _take(cond, self.name, self.cin)
        if self.cache and self._hit is not None and self._hit[0] is cond and self._hit[1] == cond._version:
            return self._hit[2]
        h = ops.unet_input(cond.contiguous(), CPAD)
        for w, b, stride, silu in self.layers:
            h = ops.unet_conv3(h, w, b, stride=stride, silu=silu)
        out = _dropin.nchw(h, self.memory_format)
        if self.cache:
            self._hit = (cond, cond._version, out)
        return out


class UNetZeroConv(_DropIn):
    """a ControlNet zero convolution: Conv2d(c, cout, 1)"""
    kind = "zero_conv"

    def __init__(self, m, memory_format=torch.channels_last, name="zero convolution"):
        self._init(name, memory_format)
        self.cin, self.cout = m.in_channels, m.out_channels
        self.w, self.b = _pack(m)

    @staticmethod
    def refusal(m):
        why = _conv_is(m, 1, 1, 0)
        if why:
            return why
        if m.in_channels % CPAD:
            return "reads %d channels, not a multiple of %d" % (m.in_channels, CPAD)
        return _fp16_only(m)

    @torch.no_grad()
    def __call__(self, x, *args, **kwargs):
        _take(x, self.name, self.cin)
        n, _, H, W = x.shape
        out = ops.vae_conv(_dropin.nhwc(x), self.w, self.b, n, H * W, 1, self.cin, self.cout, 1)
        return _dropin.nchw(out.view(n, H, W, self.cout), self.memory_format)


def _plan(model):
    """[(kind, name, module the class reads, class)] for whatever of the seven kinds `model` has"""
    plan = []
    for name, m in _dropin.find(model, DOWN_PARTS):
        if not hasattr(m, "use_conv_transpose"):
            plan.append((name, m, UNetDownsample))
    plan += [(name, m, UNetUpsample) for name, m in _dropin.find(model, UP_PARTS)]
    if hasattr(model, "time_embedding") and isinstance(getattr(model, "conv_in", None), nn.Module):
        plan.append(("conv_in", model.conv_in, UNetConvIn))
    if all(getattr(model, p, None) is not None for p in ("conv_norm_out", "conv_act", "conv_out")):
        plan.append(("conv_out", model, UNetConvOut))
    if all(getattr(model, p, None) is not None for p in ("time_proj", "time_embedding")):
        plan.append(("time_embedding", model, UNetTimeEmbedding))
    plan += [(name, m, ControlNetCondEmbedding) for name, m in _dropin.find(model, EMBED_PARTS)
             if isinstance(getattr(m, "blocks", None), (nn.ModuleList, list, tuple))]
    zero = getattr(model, "controlnet_down_blocks", None)
    if zero is not None:
        plan += [("controlnet_down_blocks.%d" % i, m, UNetZeroConv) for i, m in enumerate(zero)]
    if getattr(model, "controlnet_mid_block", None) is not None:
        plan.append(("controlnet_mid_block", model.controlnet_mid_block, UNetZeroConv))
    return plan


def _bind(m, native, forward):
    m.__dict__[_ATTR] = native
    m.__dict__["forward"] = forward


def patch_unet_shell(model, memory_format=torch.channels_last, cache=True):
    """bind the drop-ins of this module on whichever parts `model` (pipe.unet, a ControlNet) has; -> {kind: count} over KINDS.
    Every part is checked first: one outside its supported configuration raises NotImplementedError with its name before
    anything is patched.  The modules' own methods stay on their class: unpatch_unet_shell removes the bindings.  cache: the
    condition embedding's (see the module docstring)."""
    _dropin.check_format(_WHO, memory_format)
    unpatch_unet_shell(model)
    plan = _plan(model)
    for name, m, cls in plan:
        why = cls.refusal(m)
        if why:
            raise _dropin.refusal(_WHO, name, why)
    counts = dict.fromkeys(KINDS, 0)
    for name, m, cls in plan:
        if cls is ControlNetCondEmbedding:
            native = cls(m, memory_format=memory_format, name=name, cache=cache)
        else:
            native = cls(m, memory_format=memory_format, name=name)
        if cls is UNetConvOut:
            _bind(m.conv_norm_out, native, native.norm)
            _bind(m.conv_act, native, native.act)
            _bind(m.conv_out, native, native.conv)
        elif cls is UNetTimeEmbedding:
            _bind(m.time_proj, native, native.proj)
            _bind(m.time_embedding, native, native)
        else:
            _bind(m, native, native)
        counts[cls.kind] += 1
    return counts


def unpatch_unet_shell(model):
    """the modules' own forwards again; returns the number of modules whose forward was restored"""
    return _dropin.unpatch(model, _ATTR)
