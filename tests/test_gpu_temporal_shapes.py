"""The temporal-attention kernels (fresco_temporal_attn, _attn_packed, _pack, _unpack) at the shapes, strides, masks and
logit ranges the other tests leave out, against oracle.temporal_attention in fp64 on the fp16 / bf16 inputs.

Kernel forms (temporal.hip, launch_temporal; _form() restates the rule and every case asserts the form it names):
  mfma1  N <= 16: one 16-row MFMA tile of PB = 16 // N trajectories; heads split over hsplit = 1, 2 or 4 blocks; a staged
         row of more than 64 16-byte pieces takes two DMA parts
  mfma2  17 <= N <= 32: one trajectory, two key tiles
  valu   N > 32: running-maximum softmax on the vector ALUs, PB trajectories per block

Bars: fp16 |err| <= 1e-3 + 1e-3 |ref| (test_gpu_attention.py), bf16 |err| <= 2^-7 (rms(v) + |ref|)
(test_gpu_bf16_attention.py), every element.  Peaked logits: twice the larger of that bar and the distance of a CPU model
(P rounded to the storage type before P V, output rounded) from the fp64 reference; both are printed.

Maps and masks are real ones: pair_loop / chain_loop of tests/mapping_model.py on small grids (prefix / suffix block masks,
links broken at several pairs).  The checks that need no GPU (the swapped-slice and uniform-weight discrimination, the
model distances) carry no gpu mark."""
import functools
import math

import numpy as np
import pytest
import torch

import mapping_model as M
from oracle import fresco_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda"
F16, BF = torch.float16, torch.bfloat16
DT = {"f16": F16, "bf16": BF}


# ---------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------
def _form(N, H, D):
    """(form, PB, hsplit, DMA parts per staged row) as launch_temporal chooses them"""
    C = H * D
    if N > 32:
        per = N * C * 6 + N * 4 + N * N
        return "valu", max(1, min(76 * 1024 // per, (256 + N * H - 1) // (N * H))), 1, 1
    if N > 16:
        return "mfma2", 1, 1, (C // 8 + 63) // 64
    PB, hs = 16 // N, 1
    while hs < 4 and H % (hs * 2) == 0 and PB * N * 3 * (16 * ((C // hs // 8) | 1)) > 40 * 1024:
        hs *= 2
    return "mfma1", PB, hs, (C // hs // 8 + 63) // 64


@functools.lru_cache(maxsize=None)
def _traj(N, HW, seed=0):
    """fwd (N,HW) int64 and mask (HW,N,N) bool of a real chain: shifts of up to a pixel with a tenth of the pixels
    jittered (collisions, border losses) and 5 % occluded sources per pair"""
    H, W = (10, HW // 10) if HW % 10 == 0 else (1, HW)
    rng = np.random.RandomState(7 * N + HW + seed)
    gy, gx = M._grid(H, W)
    flow = np.zeros((N - 1, 2, H, W), np.float32)
    occ = (rng.rand(N - 1, H, W) < 0.05).astype(np.float32)
    for i in range(N - 1):
        dy, dx = rng.randint(-1, 2, size=2)
        jit = rng.rand(H, W) < 0.1
        ly = np.clip(gy + dy + jit * rng.randint(-1, 2, size=(H, W)), 0, H - 1)
        lx = np.clip(gx + dx + jit * rng.randint(-1, 2, size=(H, W)), 0, W - 1)
        flow[i] = M._to_flow(ly.astype(np.float32), lx.astype(np.float32), H, W)
    frames = rng.rand(N, 3, H, W).astype(np.float32)
    fwd, _, mask = M.model(flow, occ, frames, 1.0)
    return fwd, mask


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 12345)


def _qkv(g, B, HW, C, dtype, gain=1.0, vscale=1.0):
    q = (torch.randn(B, HW, C, generator=g) * gain).to(dtype)
    k = (torch.randn(B, HW, C, generator=g) * gain).to(dtype)
    v = (torch.randn(B, HW, C, generator=g) * vscale).to(dtype)
    return q, k, v


def _ref(q, k, v, fwd, tm, H, scale, chunk):
    return O.temporal_attention(q.double(), k.double(), v.double(), fwd, tm, H, scale, chunk)


def _rms(x):
    return float(x.double().pow(2).mean().sqrt())


def _frac(out, ref, v):
    """worst |err| / project bar over every element"""
    dtype = v.dtype
    assert out.dtype == dtype
    out = out.double().cpu()
    assert bool(torch.isfinite(out).all())
    bound = 1e-3 + 1e-3 * ref.abs() if dtype == F16 else 2.0 ** -7 * (_rms(v) + ref.abs())
    return float(((out - ref).abs() / bound).max())


def _run(q, k, v, fwd, tm, H, scale, chunk):
    import fresco_amd.ops as ops
    return ops.temporal_attention(q.to(DEV), k.to(DEV), v.to(DEV), fwd.to(DEV), tm.to(DEV), H, scale, chunk)


def _to_storage(xa, fwd):
    """(chunk, N, HW, C) in trajectory order -> (chunk*N, HW, C) in frame order: row fwd[f][p] of frame f = xa[:, f, p]"""
    ch, N, HW, C = xa.shape
    out = torch.empty_like(xa)
    out.scatter_(2, fwd.reshape(1, N, HW, 1).expand(ch, N, HW, C), xa)
    return out.reshape(ch * N, HW, C)


def _p_rounded_model(q, k, v, fwd, tm, H, scale, chunk):
    """the kernel's design on the CPU in fp64: P = exp(s - max) rounded to the storage type before the P V sum and before
    the row sum, the quotient rounded to the storage type"""
    dtype = q.dtype
    Bt, HW, C = q.shape
    n, D = Bt // chunk, C // H
    idx = fwd.reshape(1, n, HW, 1).expand(chunk, n, HW, C)

    def pp(x):
        return torch.gather(x.double().reshape(chunk, n, HW, C), 2, idx).reshape(chunk, n, HW, H, D).permute(0, 2, 3, 1, 4)

    qa, ka, va = pp(q), pp(k), pp(v)
    s = (qa @ ka.transpose(-1, -2)) * scale
    s = s.masked_fill(~tm.reshape(1, HW, 1, n, n), float("-inf"))
    p = torch.exp(s - s.max(-1, keepdim=True).values).to(dtype).double()
    oa = ((p @ va) / p.sum(-1, keepdim=True)).to(dtype).double()
    oa = oa.permute(0, 3, 1, 2, 4).reshape(chunk, n, HW, C)
    out = torch.empty_like(oa)
    out.scatter_(2, idx, oa)
    return out.reshape(Bt, HW, C)


# ---------------------------------------------------------------------------------------------------------------
# shapes: every N, head geometry, token count, chunk and dtype in each form it can reach, real maps and chain masks
# ---------------------------------------------------------------------------------------------------------------
SHAPES = [  # dtype, H, D, N, HW, chunk, form, PB, hsplit, DMA parts
    ("f16", 8, 40, 2, 150, 2, "mfma1", 8, 1, 1),     # 8 trajectories per tile, ragged last tile (150 % 8)
    ("bf16", 8, 80, 6, 149, 1, "mfma1", 2, 2, 1),    # 12 of 16 slots, ragged last tile
    ("f16", 8, 8, 9, 150, 3, "mfma1", 1, 1, 1),      # one trajectory, 7 idle slots
    ("f16", 12, 80, 15, 37, 1, "mfma1", 1, 4, 1),    # hsplit = 4
    ("bf16", 12, 80, 16, 20, 2, "mfma1", 1, 4, 1),   # hsplit = 4, full tile
    ("f16", 12, 80, 2, 3, 3, "mfma1", 8, 4, 1),      # hsplit = 4, HW < PB
    ("f16", 6, 80, 16, 33, 1, "mfma1", 1, 2, 1),     # hsplit stops at 2 (6 % 4)
    ("bf16", 6, 80, 15, 1, 2, "mfma1", 1, 2, 1),
    ("f16", 7, 80, 13, 41, 2, "mfma1", 1, 1, 2),     # unsplit, CC = 70: two DMA parts per row
    ("bf16", 7, 80, 6, 3, 3, "mfma1", 2, 1, 2),      # two DMA parts, ragged last tile
    ("f16", 5, 16, 15, 1, 2, "mfma1", 1, 1, 1),      # HW = 1
    ("bf16", 5, 16, 9, 150, 1, "mfma1", 1, 1, 1),
    ("f16", 8, 40, 16, 1, 1, "mfma1", 1, 1, 1),
    ("f16", 8, 80, 13, 3, 2, "mfma1", 1, 2, 1),
    ("bf16", 8, 8, 2, 1, 3, "mfma1", 8, 1, 1),       # HW = 1 < PB = 8
    ("f16", 8, 40, 17, 150, 1, "mfma2", 1, 1, 1),    # second key tile holds one key
    ("bf16", 8, 80, 31, 40, 3, "mfma2", 1, 1, 2),
    ("f16", 8, 8, 32, 150, 2, "mfma2", 1, 1, 1),
    ("f16", 12, 80, 17, 3, 2, "mfma2", 1, 1, 2),     # 99 KB of LDS: the opt-in limit
    ("bf16", 6, 80, 31, 1, 1, "mfma2", 1, 1, 1),
    ("f16", 7, 80, 32, 19, 3, "mfma2", 1, 1, 2),
    ("f16", 5, 16, 31, 150, 2, "mfma2", 1, 1, 1),
    ("bf16", 5, 16, 17, 3, 1, "mfma2", 1, 1, 1),
    ("f16", 8, 40, 33, 60, 1, "valu", 1, 1, 1),      # the first vector-ALU size
    ("bf16", 8, 80, 33, 20, 2, "valu", 1, 1, 1),
    ("f16", 8, 8, 48, 150, 3, "valu", 1, 1, 1),
    ("f16", 5, 16, 33, 3, 2, "valu", 2, 1, 1),       # PB = 2, ragged last block
    ("bf16", 6, 80, 33, 1, 3, "valu", 1, 1, 1),
    ("f16", 7, 80, 33, 10, 1, "valu", 1, 1, 1),
    ("bf16", 5, 16, 48, 150, 1, "valu", 2, 1, 1),
    ("f16", 5, 16, 48, 3, 2, "valu", 2, 1, 1),       # PB = 2, ragged last block
]


def _sid(c):
    return "%s-H%dD%d-N%d-HW%d-c%d-%s" % c[:7]


def test_shape_table_reaches_the_forms_it_names():
    for c in SHAPES:
        assert _form(c[3], c[1], c[2]) == c[6:], _sid(c)
    seen = {(c[6], c[8], c[9]) for c in SHAPES}
    assert {("mfma1", 4, 1), ("mfma1", 2, 1), ("mfma1", 1, 2), ("mfma2", 1, 2), ("valu", 1, 1)} <= seen
    for form, Ns in (("mfma1", {2, 6, 9, 13, 15, 16}), ("mfma2", {17, 31, 32}), ("valu", {33, 48})):
        rows = [c for c in SHAPES if c[6] == form]
        assert {c[3] for c in rows} == Ns
        assert {c[4] for c in rows} >= {1, 3, 150} and {c[5] for c in rows} == {1, 2, 3}
        assert {c[0] for c in rows} == {"f16", "bf16"}
        geo = {(c[1], c[2]) for c in rows}
        assert geo >= {(8, 8), (8, 40), (8, 80), (6, 80), (7, 80), (5, 16)}
        assert form == "valu" or (12, 80) in geo  # (12, 80) at N > 32 is past the LDS
    assert any(c[4] % c[7] for c in SHAPES if c[7] > 1 and c[6] == "mfma1") and any(c[4] % c[7] for c in SHAPES if c[6] == "valu")


@gpu
@pytest.mark.parametrize("case", SHAPES, ids=_sid)
def test_temporal_shapes_vs_fp64(case):
    dt, H, D, N, HW, chunk = case[:6]
    g = _gen(H, D, N, HW, chunk)
    fwd, tm = _traj(N, HW)
    q, k, v = _qkv(g, chunk * N, HW, H * D, DT[dt])
    scale = 0.2 / math.sqrt(D)
    out = _run(q, k, v, fwd, tm, H, scale, chunk)
    f = _frac(out, _ref(q, k, v, fwd, tm, H, scale, chunk), v)
    print("%s: worst |err| / bar = %.3f, %.0f %% of the frame pairs masked" % (_sid(case), f, 100 * (1 - tm.float().mean())))
    assert f <= 1.0


# one representative of every form (and of the split / two-part stagings) for the structural checks
REPS = [(8, 40, 6, 21, 2), (12, 80, 16, 5, 1), (7, 80, 9, 7, 3), (8, 40, 20, 12, 3), (7, 80, 17, 5, 1), (8, 40, 33, 6, 1),
        (5, 16, 33, 7, 2)]
REP_IDS = ["mfma1", "mfma1-hsplit4", "mfma1-2parts", "mfma2", "mfma2-2parts", "valu", "valu-PB2"]


# ---------------------------------------------------------------------------------------------------------------
# strided operands
# ---------------------------------------------------------------------------------------------------------------
def _strided(g, B, HW, C, dtype, layout):
    """q, k, v as views: 'fused3' q, k column slices of one (B,HW,3C) buffer, 'fused2' of a (B,HW,2C) one, v dense;
    'mixed' three different leading dimensions (3C, 2C, C + 8)"""
    b3 = torch.randn(B, HW, 3 * C, generator=g).mul(3.0).to(dtype)
    b2 = torch.randn(B, HW, 2 * C, generator=g).mul(3.0).to(dtype)
    vp = torch.randn(B, HW, C + 8, generator=g).to(dtype)
    if layout == "fused3":
        return (b3, b2, vp), lambda t: (t[0][..., :C], t[0][..., C:2 * C], t[2][..., :C].contiguous())
    if layout == "fused2":
        return (b3, b2, vp), lambda t: (t[1][..., :C], t[1][..., C:], t[2][..., :C].contiguous())
    return (b3, b2, vp), lambda t: (t[0][..., 2 * C:], t[1][..., C:], t[2][..., :C])


@pytest.mark.parametrize("layout", ["fused3", "fused2", "mixed"])
def test_swapped_slices_are_far_from_the_truth(layout):
    """a kernel that took q's leading dimension for k's (or the slices the other way round) would be caught: the oracle fed
    with q and k swapped misses the true one by more than 100 bars"""
    H, D, N, HW, chunk = REPS[0]
    fwd, tm = _traj(N, HW)
    bufs, views = _strided(_gen(1, N, HW), chunk * N, HW, H * D, F16, layout)
    q, k, v = views(bufs)
    scale = 0.2 / math.sqrt(D)
    ref = _ref(q, k, v, fwd, tm, H, scale, chunk)
    f = _frac(_ref(k, q, v, fwd, tm, H, scale, chunk).to(F16), ref, v)
    print("swapped q / k (%s): %.0f bars" % (layout, f))
    assert f > 100.0


@gpu
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("layout", ["fused3", "fused2", "mixed"])
@pytest.mark.parametrize("rep", REPS, ids=REP_IDS)
def test_strided_operands(rep, layout, dt):
    H, D, N, HW, chunk = rep
    fwd, tm = _traj(N, HW)
    bufs, views = _strided(_gen(1, N, HW), chunk * N, HW, H * D, DT[dt], layout)
    q, k, v = views(bufs)
    scale = 0.2 / math.sqrt(D)
    qd, kd, vd = views(tuple(b.to(DEV) for b in bufs))
    import fresco_amd.ops as ops
    assert not qd.is_contiguous() and not kd.is_contiguous() and vd.is_contiguous() == (layout != "mixed")
    out = ops.temporal_attention(qd, kd, vd, fwd.to(DEV), tm.to(DEV), H, scale, chunk)
    dense = ops.temporal_attention(qd.contiguous(), kd.contiguous(), vd.contiguous(), fwd.to(DEV), tm.to(DEV), H, scale, chunk)
    assert torch.equal(out.view(torch.int16), dense.view(torch.int16))
    f = _frac(out, _ref(q, k, v, fwd, tm, H, scale, chunk), v)
    print("strided %s %s %s: worst |err| / bar = %.3f" % (layout, dt, rep, f))
    assert f <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# masks with a known answer
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("rep", REPS, ids=REP_IDS)
def test_identity_mask_returns_v(rep, dt):
    """every query sees its own frame only: P = 1, denominator 1, the output is v bit for bit"""
    H, D, N, HW, chunk = rep
    fwd, _ = _traj(N, HW)
    q, k, v = _qkv(_gen(2, N, HW), chunk * N, HW, H * D, DT[dt], gain=3.0)
    tm = torch.eye(N, dtype=torch.bool).expand(HW, N, N).contiguous()
    out = _run(q, k, v, fwd, tm, H, 0.2 / math.sqrt(D), chunk)
    assert torch.equal(out.cpu(), v)


@gpu
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("rep", REPS, ids=REP_IDS)
def test_full_mask_identical_keys_gives_the_mean(rep, dt):
    """one key row repeated along each trajectory: every logit of a row is the same, the output is the mean of v along
    the trajectory"""
    H, D, N, HW, chunk = rep
    C = H * D
    fwd, _ = _traj(N, HW)
    g = _gen(3, N, HW)
    q, _, v = _qkv(g, chunk * N, HW, C, DT[dt], gain=3.0)
    ka = torch.randn(chunk, 1, HW, C, generator=g).mul(3.0).to(DT[dt]).expand(chunk, N, HW, C).contiguous()
    k = _to_storage(ka, fwd)
    tm = torch.ones(HW, N, N, dtype=torch.bool)
    out = _run(q, k, v, fwd, tm, H, 0.2 / math.sqrt(D), chunk)
    idx = fwd.reshape(1, N, HW, 1).expand(chunk, N, HW, C)
    va = torch.gather(v.double().reshape(chunk, N, HW, C), 2, idx)
    want = _to_storage(va.mean(1, keepdim=True).expand(chunk, N, HW, C).contiguous(), fwd)
    f = _frac(out, want, v)
    print("mean along the trajectory %s %s: worst |err| / bar = %.3f" % (dt, rep, f))
    assert f <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# peaked logits
# ---------------------------------------------------------------------------------------------------------------
PEAKED = [(8, 40, 8, 40, 2), (8, 80, 16, 20, 1), (12, 80, 15, 9, 1), (8, 40, 24, 20, 3), (8, 80, 32, 10, 1),
          (8, 40, 33, 12, 2), (8, 8, 48, 30, 1)]


def _peaked(rep, dtype):
    """q and k along one direction per trajectory and head, amplitudes such that the logits of a row span about +-12;
    v of scale 0.4"""
    H, D, N, HW, chunk = rep
    C = H * D
    g = _gen(4, N, HW, D)
    fwd, tm = _traj(N, HW)
    scale = 0.2 / math.sqrt(D)
    u = torch.randn(chunk, 1, HW, H, D, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    amp = math.sqrt(12.0 / scale)
    a = torch.where(torch.rand(chunk, N, HW, H, 1, generator=g) < 0.5, -1.0, 1.0) * amp
    b = (torch.rand(chunk, N, HW, H, 1, generator=g) * 2 - 1) * amp
    noise = 0.05 * torch.randn(chunk, N, HW, H, D, generator=g)
    q = _to_storage(((a * u + noise).reshape(chunk, N, HW, C)).to(dtype), fwd)
    k = _to_storage(((b * u + noise.flip(1)).reshape(chunk, N, HW, C)).to(dtype), fwd)
    v = (0.4 * torch.randn(chunk * N, HW, C, generator=g)).to(dtype)
    return q, k, v, fwd, tm, scale


@functools.lru_cache(maxsize=None)
def _peaked_ref(rep, dt):
    H, D, N, HW, chunk = rep
    q, k, v, fwd, tm, scale = _peaked(rep, DT[dt])
    ref = _ref(q, k, v, fwd, tm, H, scale, chunk)
    model = _frac(_p_rounded_model(q, k, v, fwd, tm, H, scale, chunk).to(DT[dt]), ref, v)
    return ref, model


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("rep", PEAKED, ids=lambda r: "H%dD%d-N%d-HW%d-c%d" % r)
def test_peaked_logits_are_peaked(rep, dt):
    """the logits of a row span +-12 or so, and an answer with uniform weights over the allowed keys misses the reference by
    more than 100 bars; prints the P-rounded model's own distance from the reference (DESIGN.md records it)"""
    H, D, N, HW, chunk = rep
    q, k, v, fwd, tm, scale = _peaked(rep, DT[dt])
    ref, model = _peaked_ref(rep, dt)
    C = H * D
    idx = fwd.reshape(1, N, HW, 1).expand(chunk, N, HW, C)
    qa = torch.gather(q.double().reshape(chunk, N, HW, C), 2, idx).reshape(chunk, N, HW, H, D).permute(0, 2, 3, 1, 4)
    ka = torch.gather(k.double().reshape(chunk, N, HW, C), 2, idx).reshape(chunk, N, HW, H, D).permute(0, 2, 3, 1, 4)
    s = (qa @ ka.transpose(-1, -2)) * scale
    span = float((s.max(-1).values - s.min(-1).values).median())
    assert 12.0 <= span <= 30.0, span
    uniform = _ref(torch.zeros_like(q), k, v, fwd, tm, H, scale, chunk)
    miss = _frac(uniform.to(DT[dt]), ref, v)
    print("peaked %s %s: median logit span %.1f, uniform weights miss by %.0f bars, P-rounded model at %.3f bars"
          % (dt, rep, span, miss, model))
    assert miss > 100.0


@gpu
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("rep", PEAKED, ids=lambda r: "H%dD%d-N%d-HW%d-c%d" % r)
def test_peaked_logits(rep, dt):
    H, D, N, HW, chunk = rep
    q, k, v, fwd, tm, scale = _peaked(rep, DT[dt])
    ref, model = _peaked_ref(rep, dt)
    out = _run(q, k, v, fwd, tm, H, scale, chunk)
    f = _frac(out, ref, v)
    allowed = 2.0 * max(1.0, model)
    print("peaked %s %s (%s): kernel at %.3f bars, P-rounded model at %.3f bars, allowed %.3f"
          % (dt, rep, _form(N, H, D)[0], f, model, allowed))
    assert f <= allowed


# ---------------------------------------------------------------------------------------------------------------
# tile isolation
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("N", [2, 3, 4, 5, 7, 8])
def test_trajectories_sharing_a_tile_are_independent(N, dt):
    """16 // N trajectories share one MFMA tile: the q, k, v rows of one trajectory per tile times 50 must leave every
    other trajectory's output bit-identical"""
    H, D, chunk = 8, 40, 2
    PB = 16 // N
    assert _form(N, H, D)[:2] == ("mfma1", PB)
    HW = 3 * PB + 1
    C = H * D
    fwd, tm = _traj(N, HW)
    tm = torch.ones_like(tm) if N % 2 else tm
    q, k, v = _qkv(_gen(5, N), chunk * N, HW, C, DT[dt])
    hot = torch.tensor([t * PB + t % PB for t in range((HW + PB - 1) // PB) if t * PB + t % PB < HW])
    gain = torch.ones(1, N, HW, 1)
    gain[0, :, hot] = 50.0
    gain = _to_storage(gain.expand(chunk, N, HW, 1).contiguous(), fwd)  # per stored row
    scale = 0.2 / math.sqrt(D)
    base = _run(q, k, v, fwd, tm, H, scale, chunk).cpu()
    pert = _run((q.float() * gain).to(DT[dt]), (k.float() * gain).to(DT[dt]), (v.float() * gain).to(DT[dt]), fwd, tm, H, scale,
                chunk).cpu()
    assert bool(torch.isfinite(pert.float()).all())
    cold = (gain == 1.0).expand(chunk * N, HW, C)
    assert int(cold.sum()) == chunk * N * (HW - len(hot)) * C
    assert torch.equal(pert[cold].view(torch.int16), base[cold].view(torch.int16))
    assert not torch.equal(pert[~cold], base[~cold])


# ---------------------------------------------------------------------------------------------------------------
# packed form
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("H,D,N", [(8, 40, 8), (12, 80, 16), (8, 40, 20), (8, 40, 33)], ids=["mfma1", "mfma1-hsplit4", "mfma2", "valu"])
@pytest.mark.parametrize("P,chunk", [(1, 3), (37, 1), (75, 3), (75, 1)])
def test_packed_form(P, chunk, H, D, N, dt):
    """fresco_temporal_attn_packed on rows gathered in torch: against the oracle (identity map on the gathered rows), and
    bit-equal to the gather form.  The range starts at trajectory 16, a multiple of every PB here, so that both forms put
    the same trajectories into a tile (slot order inside an MFMA may change the rounding of a sum)."""
    import fresco_amd.ops as ops
    HW, p0, C = 100, 16, H * D
    assert p0 % _form(N, H, D)[1] == 0
    fwd, tm = _traj(N, HW)
    q, k, v = _qkv(_gen(6, N, P), chunk * N, HW, C, DT[dt])
    scale = 0.2 / math.sqrt(D)
    rows = fwd[:, p0:p0 + P]                                    # (N, P)
    idx = rows.reshape(1, N, P, 1).expand(chunk, N, P, C)
    qkv = torch.cat([torch.gather(t.reshape(chunk, N, HW, C), 2, idx) for t in (q, k, v)], -1)   # (chunk, N, P, 3C)
    qkv = qkv.permute(1, 0, 2, 3).contiguous()                 # (N, chunk, P, 3C)
    out = ops.temporal_attention_packed(qkv.to(DEV), tm[p0:p0 + P].to(DEV), H, scale, chunk)
    assert tuple(out.shape) == (N, chunk, P, C)
    got = out.cpu().permute(1, 0, 2, 3).reshape(chunk * N, P, C)
    qg, kg, vg = (qkv[..., i * C:(i + 1) * C].permute(1, 0, 2, 3).reshape(chunk * N, P, C) for i in range(3))
    ident = torch.arange(P).expand(N, P).contiguous()
    f = _frac(got, _ref(qg, kg, vg, ident, tm[p0:p0 + P], H, scale, chunk), vg)
    print("packed P=%d chunk=%d N=%d %s: worst |err| / bar = %.3f" % (P, chunk, N, dt, f))
    assert f <= 1.0
    full = _run(q, k, v, fwd, tm, H, scale, chunk).cpu()
    same = torch.gather(full.reshape(chunk, N, HW, C), 2, idx).reshape(chunk * N, P, C)
    assert torch.equal(got.view(torch.int16), same.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------
# pack / unpack: copies
# ---------------------------------------------------------------------------------------------------------------
def _pack_expected(q, k, v, fwd, chunk, n_loc, f0, world):
    Bl, HW, C = q.shape
    Pw = HW // world
    rows = fwd[f0:f0 + n_loc].reshape(n_loc, world, Pw)                                   # [fl][d][pl]
    idx = rows.reshape(1, n_loc, HW, 1).expand(chunk, n_loc, HW, 3 * C)
    qkv = torch.cat([q, k, v], -1).reshape(chunk, n_loc, HW, 3 * C)
    g = torch.gather(qkv, 2, idx).reshape(chunk, n_loc, world, Pw, 3 * C)
    return g.permute(2, 1, 0, 3, 4).contiguous()                                          # (world, n_loc, chunk, Pw, 3C)


def _pack_sources(g, Bl, HW, C, dtype, strided):
    """(buffers, views): dense q, k, v, or q and k as column slices of one (Bl,HW,3C) buffer and v of a (Bl,HW,C+16) one"""
    if not strided:
        return _qkv(g, Bl, HW, C, dtype), lambda t: t
    b3 = torch.randn(Bl, HW, 3 * C, generator=g).to(dtype)
    vp = torch.randn(Bl, HW, C + 16, generator=g).to(dtype)
    return (b3, vp), lambda t: (t[0][..., C:2 * C], t[0][..., :C], t[1][..., :C])


@gpu
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("world,N,n_loc,f0,HW,C,chunk", [
    (1, 3, 3, 0, 50, 64, 2), (2, 4, 2, 2, 150, 320, 1), (4, 8, 2, 6, 100, 40, 3), (4, 5, 1, 3, 8, 8, 2),
    (2, 3, 1, 1, 4400, 640, 1)],                      # the last: HW * 3C / 8 > 4096 * 256, the grid-stride second pass
    ids=["w1", "w2-f0", "w4-f0", "w4-tiny", "w2-gridstride"])
def test_pack_unpack_are_the_index_arithmetic(world, N, n_loc, f0, HW, C, chunk, strided, dt):
    import fresco_amd.ops as ops
    g = _gen(7, world, HW, C)
    fwd = torch.stack([torch.randperm(HW, generator=g) for _ in range(N)]) if HW > 160 else _traj(N, HW)[0]
    bufs, views = _pack_sources(g, chunk * n_loc, HW, C, DT[dt], strided)
    q, k, v = views(bufs)
    assert (HW * 3 * C // 8 > 4096 * 256) == (HW == 4400)
    src = views(tuple(b.to(DEV) for b in bufs))  # views of the device buffers, not copies of the views
    assert src[0].is_contiguous() != strided
    buf = ops.temporal_pack(src[0], src[1], src[2], fwd.to(DEV), chunk, n_loc, f0, world)
    want = _pack_expected(q, k, v, fwd, chunk, n_loc, f0, world)
    assert buf.dtype == DT[dt] and tuple(buf.shape) == tuple(want.shape)
    assert torch.equal(buf.cpu().view(torch.int16), want.view(torch.int16))
    out = ops.temporal_unpack(buf[..., :C].contiguous(), fwd.to(DEV), chunk, n_loc, f0, world)
    assert torch.equal(out.cpu().view(torch.int16), q.contiguous().view(torch.int16))
    # unpack alone, from rows that are not a pack's output
    rnd = torch.randn(world, n_loc, chunk, HW // world, C, generator=g).to(DT[dt])
    out = ops.temporal_unpack(rnd.to(DEV), fwd.to(DEV), chunk, n_loc, f0, world).cpu()
    back = _pack_expected(out, out, out, fwd, chunk, n_loc, f0, world)[..., :C]
    assert torch.equal(back.view(torch.int16), rnd.view(torch.int16))


def _map_forms(fwd):
    """the same (N, HW) table as the wrappers may meet it, built on fwd's device (a copy across would be dense again)"""
    N, HW = fwd.shape
    big = torch.zeros(N, 2 * HW + 3, dtype=torch.int64, device=fwd.device)
    big[:, 3:HW + 3] = fwd
    every = torch.zeros(2 * N, HW, dtype=torch.int64, device=fwd.device)
    every[::2] = fwd
    return {"int32": fwd.to(torch.int32), "N1HW": fwd.reshape(N, 1, HW), "columns": big[:, 3:HW + 3], "rows": every[::2],
            "int32-columns": big.to(torch.int32)[:, 3:HW + 3]}


@gpu
@pytest.mark.parametrize("form", ["int32", "N1HW", "columns", "rows", "int32-columns"])
def test_pack_unpack_normalise_the_map(form):
    """ops.temporal_pack / temporal_unpack read the table as contiguous int64, whatever they are given"""
    import fresco_amd.ops as ops
    N, n_loc, f0, HW, C, chunk, world = 4, 2, 1, 50, 64, 2, 2
    fwd = _traj(N, HW)[0]
    g = _gen(8, HW)
    q, k, v = (t.to(DEV) for t in _qkv(g, chunk * n_loc, HW, C, F16))
    m = _map_forms(fwd.to(DEV))[form]
    assert form == "N1HW" or m.dtype == torch.int32 or not m.is_contiguous()
    want = ops.temporal_pack(q, k, v, fwd.to(DEV), chunk, n_loc, f0, world)
    assert torch.equal(want.cpu(), _pack_expected(q.cpu(), k.cpu(), v.cpu(), fwd, chunk, n_loc, f0, world))
    assert torch.equal(ops.temporal_pack(q, k, v, m, chunk, n_loc, f0, world), want)
    buf = want[..., :C].contiguous()
    assert torch.equal(ops.temporal_unpack(buf, m, chunk, n_loc, f0, world), q)
    assert torch.equal(ops.temporal_unpack(buf, fwd.to(DEV), chunk, n_loc, f0, world), q)


@pytest.mark.parametrize("form", ["int32", "N1HW", "columns", "rows", "int32-columns"])
def test_map_normalisation_on_the_host(form):
    """what the wrappers hand to the kernels is a dense int64 (N, HW) table with the same entries"""
    import fresco_amd.ops as ops
    fwd = _traj(4, 50)[0]
    m = ops._prep_fwd_map(_map_forms(fwd)[form], -1, 50)
    assert m.dtype == torch.int64 and m.is_contiguous() and torch.equal(m, fwd)
