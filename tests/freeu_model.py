"""FreeU (src/free_lunch_utils.py) restated in numpy float64, plus the seeded inputs and stand-in blocks that
tests/golden/make_freeu_golden.py, tests/test_freeu_cpu.py and tests/test_gpu_freeu.py share.

fourier_model is the closed form the kernels implement; backbone_model is the reference's
backbone scaling.  test_freeu_cpu.py pins both to records of the unmodified reference (freeu_golden.npz).

Inputs are not stored in the golden file: they come from numpy's legacy RandomState (the same stream on every machine and
numpy version), rounded so that every value is exact in fp16, bf16 and fp32 alike -- the GPU sees the very numbers the
reference saw, whatever dtype a test runs in.  The golden file keeps their sha256.
"""
import hashlib

import numpy as np

# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
FOURIER_SHAPES = [(2, 3, 2, 2), (1, 5, 3, 5), (2, 4, 8, 8), (1, 2, 7, 12), (1, 3, 32, 32), (1, 2, 64, 64), (1, 2, 33, 32),
                  (1, 1, 72, 128)]
FOURIER_SCALES = [0.0, 0.2, 0.9]
# fp32 records of the reference are kept for planes up to 32 x 32 (the float64 ones for every shape)
FOURIER_F32_MAX_HW = 1024

# Shapes past the golden file, held to fourier_model alone (test_freeu_cpu.py pins it to a float64 torch.fft restatement of
# the reference there).  The filter kernels switch at 1024 and 4096 elements per plane and between 16-byte packs and single
# elements: one workgroup per plane with single elements (1155 elements, odd); single elements for fp16 / bf16 but packs
# for fp32 (1156 = 4 * 289); packs with a partly filled last row of packs (4000); the two-pass kernel with single elements
# (4355, odd); the first plane size past 4096 (4160)
FOURIER_TILED_SHAPES = [(1, 2, 33, 35), (2, 3, 34, 34), (1, 2, 40, 100), (1, 1, 65, 67), (1, 1, 64, 65)]

BACKBONE_CASES = [(2, 8, 4, 4, 4), (1, 6, 3, 5, 7), (3, 1280, 640, 8, 8), (2, 640, 320, 32, 32)]  # B, C, n_scaled, H, W
BACKBONE_BS = [1.0, 1.2, 1.5]
# Planes of more than one pixel tile (a tile is 2048 elements for fp16 / bf16, 1024 for fp32, 256 on the single-element
# path): the last site of a 512 x 512 run (64 x 64: 2 / 4 tiles); 2304 elements, a nearly empty tail tile; channel splits of
# 3 channels with a 1-channel last split; odd planes of 323 (2 tiles) and 1023 (4 tiles) single elements
BACKBONE_TILED_CASES = [(2, 24, 12, 64, 64), (1, 12, 6, 48, 48), (1, 100, 50, 48, 48), (1, 6, 3, 17, 19), (3, 40, 20, 33, 31)]

SKIP_CH = 5
# name -> (hidden channels, output channels of each resnet, upsampler)
BLOCK_CONFIGS = {
    "c1280": (1280, (1280, 640, 640), True),
    "c640": (640, (320, 320), False),
    "c320": (320, (320, 320), False),
}
BLOCK_KINDS = ("UpBlock2D", "CrossAttnUpBlock2D")
BLOCK_SIZES = [(2, 4, 4), (1, 6, 10)]  # B, H, W
BLOCK_FACTORS = dict(b1=1.2, b2=1.5, s1=0.9, s2=0.2)


def fourier_key(shape, scale):
    return "fourier_%s_s%g" % ("x".join(map(str, shape)), scale)


def block_key(kind, name, size):
    return "block_%s_%s_%s" % (kind, name, "x".join(map(str, size)))


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def round_common(x):
    """float64 -> the nearest bfloat16 value (ties to even), with what fp16 cannot hold exactly flushed to zero: exact
    in bf16, fp16 and fp32"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    r = u.astype(np.uint32).view(np.float32).reshape(np.shape(x))
    r = np.where(r.astype(np.float16).astype(np.float32) == r, r, np.float32(0))
    return r.astype(np.float64)


def fourier_input(shape):
    """N(0.7, 1) with a different offset per plane (a kernel that mixes planes fails)"""
    B, C, H, W = shape
    rs = np.random.RandomState(1000 + 131 * H + W)
    x = 0.7 + rs.standard_normal(shape)
    off = (np.arange(B * C).reshape(B, C, 1, 1) * 0.37) % 2.0 - 0.8
    return round_common(x + off)


def pattern(B, H, W):
    """(B, 1, H, W): a smooth map per sample with its own offset and amplitude"""
    y, x = np.meshgrid(np.arange(H) / max(H - 1, 1), np.arange(W) / max(W - 1, 1), indexing="ij")
    g = np.sin(2.3 * x + 0.4) * np.cos(1.7 * y - 0.3)
    g = (g - g.min()) / (g.max() - g.min())
    amp = 1.0 + np.arange(B).reshape(B, 1, 1, 1)
    off = 0.3 * (1 + np.arange(B)).reshape(B, 1, 1, 1) * (-1.0) ** np.arange(B).reshape(B, 1, 1, 1)
    return off + amp * g[None, None]


def backbone_input(case):
    """every sample with its own mean and range; the pattern shared by all channels dominates the channel mean"""
    B, C, n, H, W = case
    rs = np.random.RandomState(2000 + 7 * C + H)
    return round_common(rs.standard_normal((B, C, H, W)) + pattern(B, H, W))


def block_inputs(name, size):
    """-> (hidden (B, C, H, W), tuple of skips in the order the UNet hands them over: the last one is used first)"""
    C, outs, _ = BLOCK_CONFIGS[name]
    B, H, W = size
    rs = np.random.RandomState(3000 + C + 17 * H)
    hidden = round_common(rs.standard_normal((B, C, H, W)) + pattern(B, H, W))
    skips = tuple(round_common(0.7 + rs.standard_normal((B, SKIP_CH, H, W)) + 0.25 * k) for k in range(len(outs)))
    return hidden, skips


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------
# the math
# ---------------------------------------------------------------------------------------------------------------
def fourier_model(x, scale):
    """Fourier_filter(x, 1, scale) in closed form, float64.  The reference holds `scale` in an fp32 mask: so does this."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    s = float(np.float32(scale))
    th = 2 * np.pi * np.arange(H)[:, None] / H
    ph = 2 * np.pi * np.arange(W)[None, :] / W
    basis = [np.ones((H, W)), np.cos(th) + 0 * ph, np.sin(th) + 0 * ph, np.cos(ph) + 0 * th, np.sin(ph) + 0 * th,
             np.cos(th + ph), np.sin(th + ph)]
    corr = np.zeros_like(x)
    for f in basis:
        corr += (x * f).sum(axis=(2, 3), keepdims=True) * f
    return x + (s - 1.0) / (H * W) * corr


def backbone_factor(hidden, b):
    """(B, 1, H, W): (b - 1) * normalised channel mean + 1  (free_lunch_utils.py:130-135)"""
    m = np.asarray(hidden, np.float64).mean(axis=1, keepdims=True)
    lo = m.min(axis=(2, 3), keepdims=True)
    hi = m.max(axis=(2, 3), keepdims=True)
    return (b - 1.0) * ((m - lo) / (hi - lo)) + 1.0


def backbone_model(hidden, n_scaled, b):
    out = np.array(hidden, np.float64)
    out[:, :n_scaled] *= backbone_factor(hidden, b)
    return out


def mean_map_condition(hidden):
    """the test inputs' guarantee: per sample, the channel-mean map's range is at least half its largest magnitude (this
    bounds the cancellation in (m - min) / (max - min))"""
    m = np.asarray(hidden, np.float64).mean(axis=1)
    rng = m.max(axis=(1, 2)) - m.min(axis=(1, 2))
    return bool(np.all(rng >= 0.5 * np.abs(m).max(axis=(1, 2))))


# ---------------------------------------------------------------------------------------------------------------
# stand-in blocks (torch): what the registered forwards are run on, by the reference on the CPU and by this package
# on the GPU
# ---------------------------------------------------------------------------------------------------------------
def kept_channels(C, n_scaled, total):
    """the channels of a (.., total, ..) tensor that the golden file records: both ends of the scaled range, the end of
    the hidden part and every skip channel"""
    idx = {0, 1, C - 1} | set(range(C, total))
    if n_scaled:
        idx |= {n_scaled - 1, n_scaled}
    return sorted(i for i in idx if 0 <= i < total)


def site_of(C):
    return {1280: 640, 640: 320}.get(C, 0)


class StandInResnet:
    """Records its input and applies a fixed seeded 1 x 1 projection with one non-zero weight per output channel: a
    power-of-two gain on an input channel that FreeU leaves untouched (hidden channels past the scaled half; any hidden
    channel where FreeU does not act).  Such a projection is exact in every dtype, so the hidden state that reaches the
    next resnet is the same bits in the float64 reference run and in an fp16 run on the GPU, and every resnet input --
    not only the first -- can be held to the kernels' own bounds."""

    def __init__(self, hidden_ch, out_ch, seed):
        import torch
        rs = np.random.RandomState(seed)
        lo = site_of(hidden_ch)
        self.index = torch.from_numpy(rs.randint(lo, hidden_ch, size=out_ch).astype(np.int64))
        self.gain = torch.from_numpy(np.array([0.5, 1.0, 2.0])[rs.randint(0, 3, size=out_ch)])
        self.inputs = []

    def __call__(self, x, temb=None):
        self.inputs.append(x.detach().clone())
        idx = self.index.to(x.device)
        return x.index_select(1, idx) * self.gain.to(device=x.device, dtype=x.dtype).view(1, -1, 1, 1)


class StandInAttention:
    def __init__(self):
        self.inputs = []

    def __call__(self, x, encoder_hidden_states=None, cross_attention_kwargs=None, attention_mask=None,
                 encoder_attention_mask=None, return_dict=True):
        assert return_dict is False
        self.inputs.append(x.detach().clone())
        return (x,)


class StandInUpsampler:
    def __call__(self, x, upsample_size=None):
        return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def _make_block(cls, name):
    C, outs, up = BLOCK_CONFIGS[name]
    blk = cls()
    blk.training = False
    blk.gradient_checkpointing = False
    blk.resnets, c = [], C
    for k, o in enumerate(outs):
        blk.resnets.append(StandInResnet(c, o, seed=4000 + 10 * C + k))
        c = o
    blk.upsamplers = [StandInUpsampler()] if up else None
    return blk


class UpBlock2D:  # recognised by name
    pass


class CrossAttnUpBlock2D:
    pass


def make_block(kind, name):
    if kind == "UpBlock2D":
        return _make_block(UpBlock2D, name)
    blk = _make_block(CrossAttnUpBlock2D, name)
    blk.attentions = [StandInAttention() for _ in blk.resnets]
    return blk


class _Unet:
    pass


class StandInPipe:
    def __init__(self, blocks):
        self.unet = _Unet()
        self.unet.up_blocks = list(blocks)


def run_block(register, kind, name, size, dtype, device="cpu", channels_last=False):
    """register(pipe, **BLOCK_FACTORS) on a fresh stand-in block, one forward.  -> dict(resnet_in=[...], out=...,
    hidden_after=..., block=...) of torch tensors"""
    import torch
    hidden, skips = block_inputs(name, size)
    blk = make_block(kind, name)
    register(StandInPipe([blk]), **BLOCK_FACTORS)
    h = torch.from_numpy(hidden).to(device=device, dtype=dtype)
    if channels_last:
        h = h.contiguous(memory_format=torch.channels_last)
    sk = tuple(torch.from_numpy(s).to(device=device, dtype=dtype) for s in skips)
    with torch.no_grad():
        out = blk.forward(h, sk)
    return dict(resnet_in=[r.inputs[0] for r in blk.resnets], out=out, hidden_after=h, block=blk)


def model_block(name, size):
    """the same forward from fourier_model / backbone_model in float64 -> dict of numpy arrays like run_block's"""
    import torch
    hidden, skips = block_inputs(name, size)
    blk = make_block("UpBlock2D", name)
    hidden_after = None
    h, res_in = hidden, []
    for resnet in blk.resnets:
        skip, skips = skips[-1], skips[:-1]
        n = site_of(h.shape[1])
        if n:
            assert mean_map_condition(h), (name, size)
            h = backbone_model(h, n, BLOCK_FACTORS["b1" if n == 640 else "b2"])
            skip = fourier_model(skip, BLOCK_FACTORS["s1" if n == 640 else "s2"])
        if hidden_after is None:
            hidden_after = h
        cat = np.concatenate([h, skip], axis=1)
        res_in.append(cat)
        h = resnet(torch.from_numpy(cat)).numpy()
    if blk.upsamplers is not None:
        h = blk.upsamplers[0](torch.from_numpy(h)).numpy()
    return dict(resnet_in=res_in, out=h, hidden_after=hidden_after)


def kept_of(name, stage_channels, total):
    """kept_channels for a resnet input whose hidden part has stage_channels channels"""
    return kept_channels(stage_channels, site_of(stage_channels), total)


def half_ulp(ref, dtype_name):
    """half a unit in the last place of the storage type at |ref| (0 for fp32: the kernels' fp32 result is what is
    stored); subnormal spacing below the smallest normal"""
    ref = np.abs(np.asarray(ref, np.float64))
    if dtype_name == "float32":
        return np.zeros_like(ref)
    bits, emin = (11, -14) if dtype_name == "float16" else (8, -126)
    e = np.floor(np.log2(np.maximum(ref, 2.0 ** emin)))
    return np.maximum(ref * 2.0 ** -bits, 2.0 ** (e - bits))
