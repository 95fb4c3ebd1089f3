"""AutoencoderKL.decode and .encode of the SD-1.5 VAE on this package's kernels, for fp16 pipelines (DESIGN.md sections 17
and 18).

`VAEDecoder.from_vae(vae)` packs the weights of `vae.post_quant_conv` and `vae.decoder` from the module's state dict;
`decode(z)` returns what the reference's call sites consume (`pipe.vae.decode(z).sample`, pipe_FRESCO.py:44 and
run_fresco.py:251).  `patch_vae_decode(pipe)` rebinds `pipe.vae.decode`.  Every layer is a call into libfresco_hip.so
(include/fresco_vae.h): activations are fp16 NHWC between layers, the three Upsample2D layers are read through the next
convolution's `up2` addressing and never written, the mid block's attention runs Q K^T and P V on the same convolution
kernel with per-image weight matrices.  There is no fallback: what is not this architecture, not fp16 or not on the GPU
raises.

`VAEEncoder.from_vae(vae)` is the other half (`vae.encoder`, `vae.quant_conv`): `encode(x).latent_dist.sample()` is what
pipe_FRESCO.py:47 and :160 and diffusion_hacked.py:874 consume; `patch_vae_encode(pipe)` rebinds `pipe.vae.encode`,
`patch_vae(pipe)` both methods.  Its resnets, mid block and stride-1 convolutions are the decoder's code and kernels; the
three Downsample2D layers, the image input, quant_conv and the Gaussian's sample are include/fresco_vae_enc.h.

Parameter names and the module layout are those of diffusers 0.19.3 (models/autoencoder_kl.py, vae.py,
unet_2d_blocks.py, attention_processor.py), with the older spelling of the attention block (query / key / value /
proj_attn) that published checkpoints carry accepted as well.  diffusers is not installed where this package is built and
tested: the names come from its published source and are UNVERIFIED against the real module.
"""
from collections import OrderedDict

import torch

from . import _lib, ops

BLOCK_CHANNELS = (128, 256, 512, 512)   # block_out_channels of the SD-1.5 VAE; the decoder walks them in reverse
LAYERS_PER_BLOCK = 2                     # the decoder's up blocks have one resnet more
GROUPS, EPS = 32, 1e-6
LATENT_CHANNELS = 4
TAPS = ("conv_in", "mid", "up0", "up1", "up2", "up3", "norm_out")  # what decode(taps=...) fills, NHWC
_OLD_ATTENTION = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


class DecoderOutput:
    """what AutoencoderKL.decode returns with return_dict=True, as far as the call sites read it"""

    def __init__(self, sample):
        self.sample = sample


class EncoderOutput:
    """what AutoencoderKL.encode returns with return_dict=True, as far as the call sites read it"""

    def __init__(self, latent_dist):
        self.latent_dist = latent_dist


def canonical_state_dict(sd, prefixes=("decoder.", "post_quant_conv.")):
    """the post_quant_conv.* and decoder.* entries (or those under `prefixes`) of a VAE state dict under the 0.19.3 names
    (old attention spelling renamed)"""
    out = OrderedDict()
    for k, v in sd.items():
        if not k.startswith(tuple(prefixes)):
            continue
        parts = k.split(".")
        if "attentions" in parts:
            leaf = parts[-2]
            if leaf in _OLD_ATTENTION:
                k = ".".join(parts[:-2] + [_OLD_ATTENTION[leaf], parts[-1]])
        out[k] = v
    return out


def pack_conv_weight(w, cin_pad=None, dtype=torch.float16):
    """(cout, cin, kh, kw) or (cout, cin) -> `dtype` (fp16, or bf16 for vae_conv's bf16 form) (cout, kh kw cin') row-major with
    k = (ky, kx, ci), the input channels zero-padded to cin' = cin_pad: the weight matrix vae_conv reads"""
    if dtype not in (torch.float16, torch.bfloat16):
        raise TypeError("pack_conv_weight: dtype %s, expected torch.float16 or torch.bfloat16" % (dtype,))
    w = w.detach()
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    w = w.permute(0, 2, 3, 1)
    if cin_pad is not None and cin_pad > cin:
        w = torch.nn.functional.pad(w, (0, cin_pad - cin))
    return w.reshape(cout, -1).to(dtype).contiguous()


def up2_source_index(y, x, H, W):
    """the `up2` index rule of vae_conv: tap position (y, x) of the (H, W) upsampled plane -> source pixel, or None where the
    zero border is read (decided in upsampled coordinates)"""
    if y < 0 or y >= H or x < 0 or x >= W:
        return None
    return y >> 1, x >> 1


def down_source_index(yo, xo, ky, kx, H, W):
    """the index rule of vaeenc_conv_down: tap (ky, kx) of output pixel (yo, xo), yo < H // 2 and xo < W // 2, of an (H, W)
    plane -> source pixel, or None where the zero row below or the zero column to the right of the plane is read; nothing
    is padded on the top or left"""
    y, x = 2 * yo + ky, 2 * xo + kx
    if y >= H or x >= W:
        return None
    return y, x


class _Layer:
    def __init__(self, sd, prefix, device, ksize, cin_pad=None):
        w = sd[prefix + ".weight"]
        if w.dim() == 4 and tuple(w.shape[2:]) != (ksize, ksize):
            raise ValueError("fresco_amd.vae: %s.weight is %s, expected a %d x %d kernel" % (prefix, tuple(w.shape), ksize, ksize))
        if w.dim() not in (2, 4) or (w.dim() == 2 and ksize != 1):
            raise ValueError("fresco_amd.vae: %s.weight is %s" % (prefix, tuple(w.shape)))
        self.cout, self.cin_real = int(w.shape[0]), int(w.shape[1])
        self.cin = cin_pad or self.cin_real
        self.k = ksize
        self.w = pack_conv_weight(w, cin_pad).to(device)
        self.b = sd[prefix + ".bias"].detach().to(device, torch.float32).contiguous()
        if self.b.numel() != self.cout:
            raise ValueError("fresco_amd.vae: %s.bias of %d values for %d channels" % (prefix, self.b.numel(), self.cout))


class _Norm:
    def __init__(self, sd, prefix, device, C):
        self.g = sd[prefix + ".weight"].detach().to(device, torch.float32).contiguous()
        self.b = sd[prefix + ".bias"].detach().to(device, torch.float32).contiguous()
        if self.g.numel() != C or self.b.numel() != C:
            raise ValueError("fresco_amd.vae: %s has %d channels, expected %d" % (prefix, self.g.numel(), C))


class _Resnet:
    def __init__(self, sd, prefix, device, cin, cout):
        self.norm1 = _Norm(sd, prefix + ".norm1", device, cin)
        self.conv1 = _Layer(sd, prefix + ".conv1", device, 3)
        self.norm2 = _Norm(sd, prefix + ".norm2", device, cout)
        self.conv2 = _Layer(sd, prefix + ".conv2", device, 3)
        if (self.conv1.cin, self.conv1.cout, self.conv2.cin, self.conv2.cout) != (cin, cout, cout, cout):
            raise ValueError("fresco_amd.vae: %s is not a %d -> %d resnet" % (prefix, cin, cout))
        has = prefix + ".conv_shortcut.weight" in sd
        if has != (cin != cout):
            raise ValueError("fresco_amd.vae: %s: conv_shortcut %s at %d -> %d" % (prefix, "present" if has else "missing", cin, cout))
        self.shortcut = _Layer(sd, prefix + ".conv_shortcut", device, 1) if has else None
        if has and (self.shortcut.cin, self.shortcut.cout) != (cin, cout):
            raise ValueError("fresco_amd.vae: %s.conv_shortcut is not %d -> %d" % (prefix, cin, cout))


class _Half:
    """What the two halves of the VAE share: taking named layers out of a state dict and accounting for every entry, the
    mid block (resnet, single-head attention at the top width, resnet), and the layer calls."""

    def _open(self, state_dict, prefixes, device, module):
        sd = canonical_state_dict(state_dict, prefixes)
        if not sd:
            raise ValueError("fresco_amd.vae: the state dict has no %s entries" % " / ".join(p + "*" for p in prefixes))
        self.module = module
        self.device = torch.device(device) if device is not None else next(iter(sd.values())).device
        self._sd, self._used = sd, set()
        return sd

    def _take(self, cls, prefix, *a):
        obj = cls(self._sd, prefix, self.device, *a)
        self._used.update(k for k in self._sd if k.startswith(prefix + "."))
        return obj

    def _take_small_conv(self, name, c):
        """a 1 x 1 convolution of c -> c channels that runs in fp32: (weight (c, c), bias (c)) fp32"""
        w, b = self._sd.get(name + ".weight"), self._sd.get(name + ".bias")
        if w is None or b is None or tuple(w.shape) != (c, c, 1, 1) or b.numel() != c:
            raise ValueError("fresco_amd.vae: %s must be a 1 x 1 convolution of %d -> %d channels" % (name, c, c))
        self._used.update((name + ".weight", name + ".bias"))
        return (w.detach().reshape(c, c).to(self.device, torch.float32).contiguous(),
                b.detach().to(self.device, torch.float32).contiguous())

    def _take_mid(self, prefix, top):
        self.mid = [self._take(_Resnet, "%s.resnets.%d" % (prefix, i), top, top) for i in (0, 1)]
        ap = prefix + ".attentions.0"
        self.attn_norm = self._take(_Norm, ap + ".group_norm", top)
        self.attn = {k: self._take(_Layer, ap + "." + k, 1) for k in ("to_q", "to_k", "to_v", "to_out.0")}
        for k, lay in self.attn.items():
            if (lay.cin, lay.cout) != (top, top):
                raise ValueError("fresco_amd.vae: %s.%s is not %d -> %d" % (ap, k, top, top))

    def _close(self, what):
        extra = sorted(k for k in self._sd if k not in self._used)
        del self._sd, self._used
        if extra:
            raise ValueError("fresco_amd.vae: not the SD-1.5 %s: unexpected parameters %s" % (what, extra[:4]))

    def _refuse(self, x, name, channels, dims):
        """what decode and encode do not take, refused before anything touches the GPU"""
        m = self.module
        if m is not None and (getattr(m, "use_slicing", False) or getattr(m, "use_tiling", False)):
            raise NotImplementedError("fresco_amd.vae: slicing / tiling of the VAE is not supported; disable it on the module")
        if not isinstance(x, torch.Tensor):
            raise TypeError("fresco_amd.vae: %s must be a tensor" % name)
        if x.dtype != torch.float16:
            raise TypeError("fresco_amd.vae: fp16 %s only (got %s); bf16 and fp32 VAEs are not supported"
                            % ("latents" if name == "z" else "images", x.dtype))
        if x.dim() != 4 or x.shape[1] != channels or x.numel() == 0:
            raise ValueError("fresco_amd.vae: %s must be (n, %d, %s), got %s" % (name, channels, dims, tuple(x.shape)))

    # ---- layers ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _conv(x, lay, n, H, W, up2=False, residual=None, out_kind=_lib.VAE_OUT_F16):
        return ops.vae_conv(x, lay.w, lay.b, n, H, W, lay.cin, lay.cout, lay.k, up2=up2, residual=residual, out_kind=out_kind)

    def _resnet(self, x, r, n, H, W):
        h = ops.vae_groupnorm(x, r.norm1.g, r.norm1.b, EPS, silu=True)
        h = self._conv(h, r.conv1, n, H, W)
        h = ops.vae_groupnorm(h, r.norm2.g, r.norm2.b, EPS, silu=True)
        skip = x if r.shortcut is None else self._conv(x, r.shortcut, n, H, W)
        return self._conv(h, r.conv2, n, H, W, residual=skip)

    def _attention(self, x, n, H, W):
        C, L = x.shape[-1], H * W
        Lp = (L + 31) // 32 * 32  # the key axis is P V's K: padded to the kernel's chunk with zero probabilities
        a = self.attn
        h = ops.vae_groupnorm(x, self.attn_norm.g, self.attn_norm.b, EPS, silu=False)
        q = ops.conv_rows(h, a["to_q"].w, a["to_q"].b)
        k = ops.conv_rows(h, a["to_k"].w, a["to_k"].b)
        # V^T = W_v x^T: to_v's weight is the kernel's pixel operand there, its bias a per-row one
        vt = torch.zeros(n, C, Lp, dtype=torch.float16, device=x.device)
        ops.vae_conv(a["to_v"].w, h, a["to_v"].b, n, C, 1, C, L, 1, x_img_stride=0, w_img_stride=L * C, bias_rows=True,
                     ldo=Lp, out=vt)
        scores = torch.empty(n * L, Lp, dtype=torch.float32, device=x.device)
        ops.vae_conv(q, k, None, n, L, 1, C, L, 1, out_kind=_lib.VAE_OUT_F32, w_img_stride=L * C, ldo=Lp, out=scores)
        p = ops.vae_softmax(scores, L, float(C) ** -0.5, ld_out=Lp)
        o = ops.vae_conv(p, vt, None, n, L, 1, Lp, C, 1, w_img_stride=C * Lp)
        return ops.conv_rows(o, a["to_out.0"].w, a["to_out.0"].b, residual=x).view(n, H, W, C)

    def _mid(self, x, n, H, W):
        x = self._resnet(x, self.mid[0], n, H, W)
        x = self._attention(x, n, H, W)
        return self._resnet(x, self.mid[1], n, H, W)


class VAEDecoder(_Half):
    """The decoder half of an fp16 AutoencoderKL (block channels (128, 256, 512, 512), two layers per block, GroupNorm(32,
    eps 1e-6), single-head attention at 512 channels in the mid block) on HIP kernels."""

    def __init__(self, state_dict, device=None, module=None):
        sd = self._open(state_dict, ("decoder.", "post_quant_conv."), device, module)
        take = self._take
        rev = BLOCK_CHANNELS[::-1]
        top = rev[0]
        self.pq_w, self.pq_b = self._take_small_conv("post_quant_conv", LATENT_CHANNELS)
        self.conv_in = take(_Layer, "decoder.conv_in", 3, ops.VAE_CIN_PAD)
        if (self.conv_in.cin_real, self.conv_in.cout) != (LATENT_CHANNELS, top):
            raise ValueError("fresco_amd.vae: decoder.conv_in is not %d -> %d" % (LATENT_CHANNELS, top))
        self._take_mid("decoder.mid_block", top)
        self.up, cin = [], top
        for b, cout in enumerate(rev):
            res = [take(_Resnet, "decoder.up_blocks.%d.resnets.%d" % (b, i), cin if i == 0 else cout, cout)
                   for i in range(LAYERS_PER_BLOCK + 1)]
            ups = None
            if b < len(rev) - 1:
                ups = take(_Layer, "decoder.up_blocks.%d.upsamplers.0.conv" % b, 3)
                if (ups.cin, ups.cout) != (cout, cout):
                    raise ValueError("fresco_amd.vae: up block %d's upsampler is not %d -> %d" % (b, cout, cout))
            elif any(k.startswith("decoder.up_blocks.%d.upsamplers" % b) for k in sd):
                raise ValueError("fresco_amd.vae: the last up block has an upsampler")
            self.up.append((res, ups))
            cin = cout
        self.norm_out = take(_Norm, "decoder.conv_norm_out", rev[-1])
        self.conv_out = take(_Layer, "decoder.conv_out", 3)
        if (self.conv_out.cin, self.conv_out.cout) != (rev[-1], 3):
            raise ValueError("fresco_amd.vae: decoder.conv_out is not %d -> 3" % rev[-1])
        self._close("decoder")

    @classmethod
    def from_vae(cls, vae, device=None):
        """device: where the packed weights go; default: where the module's parameters are (decode needs the GPU)"""
        return cls(vae.state_dict(), device=device, module=vae)

    # ---- the decoder -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode(self, z, return_dict=True, generator=None, taps=None):
        """z (n, 4, h, w) fp16 on the GPU -> DecoderOutput(sample (n, 3, 8 h, 8 w) fp16), or (sample,) with
        return_dict=False.  taps: a dict that receives the TAPS tensors (NHWC copies)."""
        self._refuse(z, "z", LATENT_CHANNELS, "h, w")
        ops._need_gpu(z)
        keep = (lambda name, t: taps.__setitem__(name, t.clone())) if taps is not None else (lambda name, t: None)
        n, _, H, W = z.shape
        x = ops.vae_input(z.contiguous(), self.pq_w, self.pq_b)
        x = self._conv(x, self.conv_in, n, H, W)
        keep("conv_in", x)
        x = self._mid(x, n, H, W)
        keep("mid", x)
        for b, (res, ups) in enumerate(self.up):
            for r in res:
                x = self._resnet(x, r, n, H, W)
            if ups is not None:
                H, W = 2 * H, 2 * W
                x = self._conv(x, ups, n, H, W, up2=True)
            keep("up%d" % b, x)
        x = ops.vae_groupnorm(x, self.norm_out.g, self.norm_out.b, EPS, silu=True)
        keep("norm_out", x)
        img = self._conv(x, self.conv_out, n, H, W, out_kind=_lib.VAE_OUT_F16_NCHW)
        return DecoderOutput(img) if return_dict else (img,)

    __call__ = decode


class DiagonalGaussian:
    """diffusers' DiagonalGaussianDistribution over `parameters` (n, 8, h, w) fp16 (mean | logvar), as far as the call sites
    and the class's attributes go.  `sample` is one kernel (vaeenc_sample); the other attributes are views or small torch
    expressions for inspection."""

    def __init__(self, parameters):
        self.parameters = parameters
        self.mean = parameters[:, :LATENT_CHANNELS]

    @property
    def logvar(self):
        return torch.clamp(self.parameters[:, LATENT_CHANNELS:], -30.0, 20.0)

    @property
    def std(self):
        return torch.exp(0.5 * self.logvar)

    @property
    def var(self):
        return torch.exp(self.logvar)

    def mode(self):
        return self.mean

    def sample(self, generator=None, scale=1.0):
        """scale (mean + std noise), rounded once.  The noise is drawn as diffusers' randn_tensor draws it here -- one
        torch.randn of the mean's shape in fp16, on the parameters' device, or on the CPU and then moved where the generator
        is a CPU one -- so a seeded run consumes the random stream as the module would."""
        p = self.parameters
        shape = tuple(self.mean.shape)
        if generator is not None and generator.device.type == "cpu" and p.device.type != "cpu":
            noise = torch.randn(shape, generator=generator, device="cpu", dtype=p.dtype).to(p.device)
        else:
            noise = torch.randn(shape, generator=generator, device=p.device, dtype=p.dtype)
        return ops.vaeenc_sample(p, noise, scale)


class VAEEncoder(_Half):
    """The encoder half of the same AutoencoderKL on HIP kernels: conv_in, four down blocks of two resnets with a
    Downsample2D behind the first three, the mid block, conv_norm_out + SiLU, conv_out (512 -> 8) and quant_conv (8 -> 8)."""

    TAPS = ("conv_in", "down0", "down1", "down2", "down3", "mid", "norm_out")  # what encode(taps=...) fills, NHWC

    def __init__(self, state_dict, device=None, module=None):
        sd = self._open(state_dict, ("encoder.", "quant_conv."), device, module)
        take = self._take
        top = BLOCK_CHANNELS[-1]
        self.q_w, self.q_b = self._take_small_conv("quant_conv", 2 * LATENT_CHANNELS)
        self.conv_in = take(_Layer, "encoder.conv_in", 3, ops.VAE_CIN_PAD)
        if (self.conv_in.cin_real, self.conv_in.cout) != (3, BLOCK_CHANNELS[0]):
            raise ValueError("fresco_amd.vae: encoder.conv_in is not 3 -> %d" % BLOCK_CHANNELS[0])
        self.down, cin = [], BLOCK_CHANNELS[0]
        for b, cout in enumerate(BLOCK_CHANNELS):
            res = [take(_Resnet, "encoder.down_blocks.%d.resnets.%d" % (b, i), cin if i == 0 else cout, cout)
                   for i in range(LAYERS_PER_BLOCK)]
            down = None
            if b < len(BLOCK_CHANNELS) - 1:
                down = take(_Layer, "encoder.down_blocks.%d.downsamplers.0.conv" % b, 3)
                if (down.cin, down.cout) != (cout, cout):
                    raise ValueError("fresco_amd.vae: down block %d's downsampler is not %d -> %d" % (b, cout, cout))
            elif any(k.startswith("encoder.down_blocks.%d.downsamplers" % b) for k in sd):
                raise ValueError("fresco_amd.vae: the last down block has a downsampler")
            self.down.append((res, down))
            cin = cout
        self._take_mid("encoder.mid_block", top)
        self.norm_out = take(_Norm, "encoder.conv_norm_out", top)
        self.conv_out = take(_Layer, "encoder.conv_out", 3)
        if (self.conv_out.cin, self.conv_out.cout) != (top, 2 * LATENT_CHANNELS):
            raise ValueError("fresco_amd.vae: encoder.conv_out is not %d -> %d" % (top, 2 * LATENT_CHANNELS))
        self._close("encoder")

    @classmethod
    def from_vae(cls, vae, device=None):
        """device: where the packed weights go; default: where the module's parameters are (encode needs the GPU)"""
        return cls(vae.state_dict(), device=device, module=vae)

    @torch.no_grad()
    def encode(self, x, return_dict=True, taps=None):
        """x (n, 3, H, W) fp16 on the GPU, H and W >= 8 -> EncoderOutput(latent_dist), or (latent_dist,) with
        return_dict=False; latent_dist.parameters is (n, 8, H // 8, W // 8) fp16.  taps: a dict that receives the TAPS tensors
        (NHWC copies)."""
        self._refuse(x, "x", 3, "H, W")
        if x.shape[2] < 8 or x.shape[3] < 8:
            raise ValueError("fresco_amd.vae: x must be at least 8 x 8, got %s" % (tuple(x.shape),))
        ops._need_gpu(x)
        keep = (lambda name, t: taps.__setitem__(name, t.clone())) if taps is not None else (lambda name, t: None)
        n, _, H, W = x.shape
        x = ops.vaeenc_input(x.contiguous())
        x = self._conv(x, self.conv_in, n, H, W)
        keep("conv_in", x)
        for b, (res, down) in enumerate(self.down):
            for r in res:
                x = self._resnet(x, r, n, H, W)
            if down is not None:
                x = ops.vaeenc_conv_down(x, down.w, down.b)
                H, W = H // 2, W // 2
            keep("down%d" % b, x)
        x = self._mid(x, n, H, W)
        keep("mid", x)
        x = ops.vae_groupnorm(x, self.norm_out.g, self.norm_out.b, EPS, silu=True)
        keep("norm_out", x)
        h = self._conv(x, self.conv_out, n, H, W, out_kind=_lib.VAE_OUT_F32)  # fp32: nothing is rounded before quant_conv
        dist = DiagonalGaussian(ops.vaeenc_moments(h, self.q_w, self.q_b))
        return EncoderOutput(dist) if return_dict else (dist,)

    __call__ = encode


def patch_vae_decode(pipe):
    """rebind pipe.vae.decode to a VAEDecoder built from pipe.vae; returns the decoder.  The module's own method stays on
    its class: unpatch_vae_decode removes the binding."""
    vae = pipe.vae
    unpatch_vae_decode(pipe)
    dec = VAEDecoder.from_vae(vae)
    vae.decode = dec.decode
    return dec


def unpatch_vae_decode(pipe):
    vae = pipe.vae
    if "decode" in vars(vae):
        del vae.decode


def patch_vae_encode(pipe):
    """rebind pipe.vae.encode to a VAEEncoder built from pipe.vae; returns the encoder.  unpatch_vae_encode removes the
    binding."""
    vae = pipe.vae
    unpatch_vae_encode(pipe)
    enc = VAEEncoder.from_vae(vae)
    vae.encode = enc.encode
    return enc


def unpatch_vae_encode(pipe):
    vae = pipe.vae
    if "encode" in vars(vae):
        del vae.encode


def patch_vae(pipe):
    """both halves: returns (decoder, encoder)"""
    return patch_vae_decode(pipe), patch_vae_encode(pipe)


def unpatch_vae(pipe):
    unpatch_vae_decode(pipe)
    unpatch_vae_encode(pipe)
