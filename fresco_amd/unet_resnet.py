"""ResnetBlock2D of the SD-1.5 UNet and ControlNet on this package's kernels, for fp16 and bf16 pipelines (DESIGN.md
section 19).

`UNetResnet(state_dict, prefix, cin, cout)` packs one block's weights; `UNetResnet.from_module(block)` reads them from a
module; `patch_unet_resnets(model)` replaces `forward` on every resnet block of `pipe.unet` or of the ControlNet.  All three
take `dtype=` (default torch.float16): the pipeline's dtype, as `torch_dtype=` is in `from_pretrained`; with
`dtype=torch.bfloat16` the parameters, x, temb and the result are bf16 and the same launches run the kernels' bf16 forms
(csrc/net_bf16.hip; the norms' scales and every bias are fp32 either way).  A call is
six launches into libfresco_hip.so, seven with a shortcut (include/fresco_unet.h, include/fresco_vae.h):

  1. unet_groupnorm(x, SiLU)                    norm1 + swish
  2. vae_conv 3 x 3, no bias                    conv1 (its bias goes into 3)
  3. unet_temb                                  time_emb_proj(SiLU(temb)) + its bias + conv1's bias -> fp32 (n, cout)
  4. unet_groupnorm(h, addend = 3, SiLU)        norm2(conv1 + temb) + swish
  5. vae_conv 1 x 1                             conv_shortcut, where cin != cout
  6. vae_conv 3 x 3 + bias + residual           conv2 + (x or 5)

This is diffusers 0.19.3's `ResnetBlock2D.forward` with 32 groups, swish, `time_embedding_norm="default"`,
`output_scale_factor=1.0`, no up or down sampling inside the block and a 1 x 1 `conv_shortcut` iff cin != cout.  Against
PyTorch's fp16 (bf16) module the intermediate `conv1 + temb` is rounded to fp16 (bf16) once (conv1's output without its bias)
instead of twice: bias and time embedding are added in fp32 inside the second norm.

Layout: tensors are logical NCHW, as diffusers passes them, and NHWC in memory.  An input that is `channels_last`-contiguous
is read in place, any other is converted once; the output is `(n, cout, H, W)` in `torch.channels_last` unless
`memory_format=torch.contiguous_format` asks for the plain layout (one more copy).

There is no fallback: a block outside this configuration, not of `dtype` or not on the GPU raises.  diffusers is not installed where
this package is built and tested: the parameter names and the forward come from its published source (models/resnet.py) and
are UNVERIFIED against the real module.
"""
import torch

from . import _dropin, _lib, ops
from ._dropin import f32 as _f32
from .vae import pack_conv_weight

GROUPS = 32
PARTS = ("norm1", "conv1", "time_emb_proj", "norm2", "conv2")  # what makes a module a resnet block for patch_unet_resnets
_ATTR = "_fresco_unet_resnet"
_WHO = "fresco_amd.unet_resnet"


class UNetResnet:
    """One ResnetBlock2D (cin -> cout channels, a time embedding of temb_channels) on HIP kernels."""

    def __init__(self, state_dict, prefix, cin, cout, temb_channels=1280, eps=1e-5, device=None,
                 memory_format=torch.channels_last, dtype=torch.float16):
        self.dtype, self.dtype_name = dtype, _dropin.dtype_name(_WHO, dtype)
        sd, what = _dropin.intake(state_dict, prefix, [p + s for p in PARTS for s in (".weight", ".bias")], _WHO, "the block",
                                  dtype=dtype)
        if not (ops.unet_gn_channels(cin) and ops.unet_gn_channels(cout)):
            raise NotImplementedError("%s: %d -> %d channels; the GroupNorm kernel takes multiples of %d in %d .. %d"
                                      % (what, cin, cout, ops.UNET_GN_STEP, ops.UNET_GN_MIN, ops.UNET_GN_MAX))
        if temb_channels <= 0 or temb_channels % 8:
            raise NotImplementedError("%s: a time embedding of %d channels (must be a multiple of 8)" % (what, temb_channels))
        shapes = {"norm1.weight": (cin,), "norm1.bias": (cin,), "conv1.weight": (cout, cin, 3, 3), "conv1.bias": (cout,),
                  "time_emb_proj.weight": (cout, temb_channels), "time_emb_proj.bias": (cout,), "norm2.weight": (cout,),
                  "norm2.bias": (cout,), "conv2.weight": (cout, cout, 3, 3), "conv2.bias": (cout,)}
        has = "conv_shortcut.weight" in sd
        if has != (cin != cout):
            raise ValueError("%s: conv_shortcut %s at %d -> %d" % (what, "present" if has else "missing", cin, cout))
        if has:
            shapes.update({"conv_shortcut.weight": (cout, cin, 1, 1), "conv_shortcut.bias": (cout,)})
        _dropin.check_shapes(sd, shapes, what, only=True)
        dev = torch.device(device) if device is not None else sd["conv1.weight"].device
        self.cin, self.cout, self.temb_channels, self.eps = int(cin), int(cout), int(temb_channels), float(eps)
        self.device, self.memory_format = dev, memory_format
        self.g1, self.b1 = _f32(sd["norm1.weight"], dev), _f32(sd["norm1.bias"], dev)
        self.g2, self.b2 = _f32(sd["norm2.weight"], dev), _f32(sd["norm2.bias"], dev)
        self.w1 = pack_conv_weight(sd["conv1.weight"], dtype=dtype).to(dev)
        self.cb1 = _f32(sd["conv1.bias"], dev)
        self.wt = sd["time_emb_proj.weight"].detach().to(dev, dtype).contiguous()
        self.bt = _f32(sd["time_emb_proj.bias"], dev)
        self.w2 = pack_conv_weight(sd["conv2.weight"], dtype=dtype).to(dev)
        self.cb2 = _f32(sd["conv2.bias"], dev)
        self.ws = pack_conv_weight(sd["conv_shortcut.weight"], dtype=dtype).to(dev) if has else None
        self.cbs = _f32(sd["conv_shortcut.bias"], dev) if has else None

    @staticmethod
    def refusal(block, dtype=torch.float16):
        """why `block` (a module with PARTS) is outside the supported configuration of a `dtype` pipeline, or None"""
        want = _dropin.dtype_name(_WHO, dtype)
        for part in PARTS:
            if getattr(block, part, None) is None:
                return "has no %s" % part
        dtypes = {p.dtype for p in block.parameters()}
        if dtypes != {dtype}:
            return "is %s, %s blocks only" % ("/".join(sorted(str(d) for d in dtypes)), want)
        ten = getattr(block, "time_embedding_norm", "default")
        if ten != "default":
            return "time_embedding_norm is %r, only \"default\"" % (ten,)
        if getattr(block, "up", False) or getattr(block, "down", False) or getattr(block, "upsample", None) is not None \
                or getattr(block, "downsample", None) is not None:
            return "samples up or down inside the block"
        if float(getattr(block, "output_scale_factor", 1.0)) != 1.0:
            return "output_scale_factor is %s, only 1" % (block.output_scale_factor,)
        act = getattr(block, "nonlinearity", None)
        if act is not None and not isinstance(act, torch.nn.SiLU):
            return "its activation is %s, only swish" % type(act).__name__
        drop = getattr(block, "dropout", None)
        if isinstance(drop, torch.nn.Dropout) and drop.p != 0.0:
            return "dropout %s" % drop.p
        for norm in (block.norm1, block.norm2):
            if getattr(norm, "num_groups", None) != GROUPS:
                return "GroupNorm of %s groups, only %d" % (getattr(norm, "num_groups", None), GROUPS)
        if block.norm1.eps != block.norm2.eps:
            return "two values of eps"
        w1 = block.conv1.weight
        if w1.dim() != 4 or not (ops.unet_gn_channels(w1.shape[1]) and ops.unet_gn_channels(w1.shape[0])):
            return "%d -> %d channels, the kernels take multiples of %d in %d .. %d" % (
                w1.shape[1], w1.shape[0], ops.UNET_GN_STEP, ops.UNET_GN_MIN, ops.UNET_GN_MAX)
        return None

    @classmethod
    def from_module(cls, block, device=None, memory_format=torch.channels_last, name="the block", dtype=torch.float16):
        why = cls.refusal(block, dtype)
        if why:
            raise _dropin.refusal(_WHO, name, why)
        w1 = block.conv1.weight
        return cls(block.state_dict(), "", int(w1.shape[1]), int(w1.shape[0]), int(block.time_emb_proj.weight.shape[1]),
                   float(block.norm1.eps), device=device, memory_format=memory_format, dtype=dtype)

    @torch.no_grad()
    def __call__(self, x, temb, *args, memory_format=None, taps=None, **kwargs):
        """x (n, cin, H, W) on the GPU and temb (n, temb_channels), both of the block's dtype (fp16 or bf16) -> (n, cout, H, W)
        of that dtype.  taps: a dict that receives "conv1_temb" (n, H, W, cout) fp32 = conv1's 16-bit output + the addend,
        what the second norm normalises."""
        for t, name in ((x, "x"), (temb, "temb")):
            if not isinstance(t, torch.Tensor):
                raise TypeError("fresco_amd.unet_resnet: %s must be a tensor" % name)
            if t.dtype != self.dtype:
                raise TypeError("fresco_amd.unet_resnet: %s %s only (got %s)" % (self.dtype_name, name, t.dtype))
        if x.dim() != 4 or x.shape[1] != self.cin or x.numel() == 0:
            raise ValueError("fresco_amd.unet_resnet: x must be (n, %d, H, W), got %s" % (self.cin, tuple(x.shape)))
        n, _, H, W = x.shape
        if tuple(temb.shape) != (n, self.temb_channels):
            raise ValueError("fresco_amd.unet_resnet: temb must be (%d, %d), got %s" % (n, self.temb_channels, tuple(temb.shape)))
        fmt = self.memory_format if memory_format is None else memory_format
        _dropin.check_format(_WHO, fmt)
        ops._need_gpu(x, temb)
        xn = _dropin.nhwc(x)
        h = ops.unet_groupnorm(xn, self.g1, self.b1, self.eps, silu=True)
        h = ops.vae_conv(h, self.w1, None, n, H, W, self.cin, self.cout, 3)
        add = ops.unet_temb(temb.contiguous(), self.wt, self.bt, self.cb1)
        if taps is not None:
            taps["conv1_temb"] = h.float() + add[:, None, None, :]
        h = ops.unet_groupnorm(h, self.g2, self.b2, self.eps, silu=True, addend=add)
        skip = xn if self.ws is None else ops.vae_conv(xn, self.ws, self.cbs, n, H * W, 1, self.cin, self.cout, 1)
        return _dropin.nchw(ops.vae_conv(h, self.w2, self.cb2, n, H, W, self.cout, self.cout, 3, residual=skip), fmt)


def patch_unet_resnets(model, memory_format=torch.channels_last, dtype=torch.float16):
    """replace `forward` on every module of `model` (pipe.unet, a ControlNet) that has norm1, conv1, time_emb_proj, norm2 and
    conv2 by a UNetResnet built from it; returns the number of blocks patched.  dtype: the pipeline's dtype, torch.float16 or
    torch.bfloat16.  A matching block outside the supported configuration, or whose parameters are not of `dtype`, raises
    NotImplementedError with its name, before anything is patched.  The modules' own methods stay on
    their class: unpatch_unet_resnets removes the bindings.  The weights are copied: patch again after loading others."""
    _dropin.dtype_name(_WHO, dtype)
    return _dropin.patch(model, UNetResnet, PARTS, _WHO, _ATTR, memory_format, dtype=dtype)


def unpatch_unet_resnets(model):
    """the modules' own forwards again; returns the number of blocks restored"""
    return _dropin.unpatch(model, _ATTR)
