"""The warp family (csrc/warp.hip) off the square, past one pass of its loops, and the derived-tensor cache in front of it.

Every kernel against a plain reference of the same operation (oracle/fresco_oracle.py, in fp32 where bits are compared and
in float64 where a bar is): channel groups past CPT = 8 and ragged ones, ragged 256-pixel blocks, flows shared by B / Bf
frames, max-pool windows that are no multiple of 64 lanes on planes that are no multiple of the window, Dilate with a radius
beyond the plane, AdaIN rows of 2 ... 4097 elements, DDPM sizes that are no multiple of the block and noise periods that are no
power of two, the shortest frame chains, the colour test of flow_occlusion on one frame.

Bars (DESIGN.md section 2 lists what was measured):
  flow_warp, integer shifts at h - 1, w - 1 powers of two   exact (the normalise / denormalise round trip is exact there)
  flow_warp, random flows, randn features                  1e-5  (test_gpu_warp.py)
  max_pool                                                 exact
  dilate, 0/1 data                                         exact
  dilate, |x| <= 0.3                                       k k 2^-23: an fp32 sum of k k terms of size <= 0.3
  AdaIN, per row                                           8 2^-24 (max|c| / std_c std_s + max|out|): fp32 conditioning
  calc_mean_std                                            mean 8 2^-24 max|c|, std the same + 8 2^-24 std
  16-bit AdaIN / calc_mean_std                             half an ulp of the type at |ref| + the fp32 bar
  DDPM kernels, fp32                                       4 2^-24 (sum of the |terms|); 16-bit: the fp32 result rounded once
  warp_tensor                                              5e-5  (test_gpu_warp.py)
  flow_occlusion                                           <= 4 pixels, occluded share in (0.02, 0.98)  (test_gpu_paras.py)
"""
import sys

import pytest
import torch

import synth
from oracle import fresco_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24  # unit roundoff of fp32


def maxdiff(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def _report(what, ratio):
    print("warp shapes: %s: worst |err| / bar = %.3g" % (what, ratio))


# ---- flow_warp ----------------------------------------------------------------------------------------------------------
CHANNELS = (1, 8, 9, 17)          # one group, a full group, a ragged second group, a ragged third group (CPT = 8)
BATCHES = ((2, 2), (6, 2), (3, 1))  # (B, Bf): the flow of frame b is flow[b % Bf]


def _shifted(x, dx, dy):
    """out[..., y, x] = x[..., y + dy, x + dx], zeros outside"""
    h, w = x.shape[-2:]
    out = torch.zeros_like(x)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y1 > y0 and x1 > x0:
        out[..., y0:y1, x0:x1] = x[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


@pytest.mark.parametrize("B,Bf", BATCHES)
@pytest.mark.parametrize("h,w", [(17, 33), (33, 17), (65, 129)])
def test_flow_warp_integer_shifts_exact(h, w, B, Bf):
    import fresco_amd.ops as ops
    g = synth.gen(100 + h + B)
    per_frame = [(2, -3), (-5, 1)][:Bf]
    shift_sets = [[(0, 0)] * Bf, [(3, -2)] * Bf, [(-w, 0)] * Bf, [(w - 1, h - 1)] * Bf, per_frame]
    for C in CHANNELS:
        x = torch.randn(B, C, h, w, generator=g)
        xd = x.to(DEV)
        for shifts in shift_sets:
            flow = torch.empty(Bf, 2, h, w)
            for f, (dx, dy) in enumerate(shifts):
                flow[f, 0], flow[f, 1] = float(dx), float(dy)
            out = ops.flow_warp(xd, flow.to(DEV)).cpu()
            want = torch.stack([_shifted(x[b], *shifts[b % Bf]) for b in range(B)])
            assert torch.equal(out, want), (C, shifts, maxdiff(out, want))


def _ragged_flow(Bf, h, w, g):
    """6 randn flows (many samples outside), the first / last column sampled in (-1, 0) / (w - 1, w) and the first / last row in
    (-1, 0) / (h - 1, h): taps half inside the zero padding; two entries far outside the int range"""
    flow = 6 * torch.randn(Bf, 2, h, w, generator=g)
    flow[:, 0, :, 0] = -(0.1 + 0.8 * torch.rand(Bf, h, generator=g))
    flow[:, 0, :, w - 1] = 0.1 + 0.8 * torch.rand(Bf, h, generator=g)
    flow[:, 1, :, 0] = 0.3 * torch.randn(Bf, h, generator=g)
    flow[:, 1, :, w - 1] = 0.3 * torch.randn(Bf, h, generator=g)
    flow[:, 1, 0, 1:w - 1] = -(0.1 + 0.8 * torch.rand(Bf, w - 2, generator=g))
    flow[:, 1, h - 1, 1:w - 1] = 0.1 + 0.8 * torch.rand(Bf, w - 2, generator=g)
    flow[:, 0, 0, 1:w - 1] = 0.3 * torch.randn(Bf, w - 2, generator=g)
    flow[:, 0, h - 1, 1:w - 1] = 0.3 * torch.randn(Bf, w - 2, generator=g)
    flow[0, 0, 1, 2] = 1e9
    flow[Bf - 1, 1, 2, 3] = -1e9
    return flow


@pytest.mark.parametrize("B,Bf", BATCHES)
@pytest.mark.parametrize("h,w", [(13, 37), (37, 13), (24, 40)])
def test_flow_warp_random_flows_vs_oracle(h, w, B, Bf):
    import fresco_amd.ops as ops
    g = synth.gen(200 + h + B)
    flow = _ragged_flow(Bf, h, w, g)
    ix, iy = O.sample_coords(flow)
    assert bool(((ix[:, :, 0] > -1) & (ix[:, :, 0] < 0)).all()) and bool(((ix[:, :, -1] > w - 1) & (ix[:, :, -1] < w)).all())
    worst = 0.0
    for C in CHANNELS:
        x = torch.randn(B, C, h, w, generator=g)
        out = ops.flow_warp(x.to(DEV), flow.to(DEV))
        ref = O.flow_warp(x, flow.repeat(B // Bf, 1, 1, 1))
        assert float(ref.abs().max()) > 1 and float((ref == 0).float().mean()) > 0.05  # (inside and outside both occur)
        worst = max(worst, maxdiff(out, ref) / 1e-5)
        assert maxdiff(out, ref) < 1e-5, C
    _report("flow_warp random %dx%d B=%d Bf=%d" % (h, w, B, Bf), worst)


# ---- max_pool -----------------------------------------------------------------------------------------------------------
# (k, H, W): H % k != 0, W % k != 0, H != W; windows (H // k) (W // k) = 8, 3, 5, 8, 1, 6, 8, 6, 4, 2: blocks of four
# waves that are full, ragged and a single wave
POOL_WAVE = [(8, 35, 20), (9, 13, 29), (12, 62, 17), (13, 30, 55), (13, 17, 20), (16, 50, 37), (32, 70, 130), (64, 130, 200),
             (64, 70, 259), (64, 129, 70)]
POOL_SMALL = [(k, H, W) for k in (1, 3, 7) for H, W in ((50, 77), (77, 50))]


def _window_positions(k, g):
    """window positions i = dy k + dx to plant the maximum at: the ends of the first, second and last 64-lane pass, the row
    seams, and random ones until every lane i % 64 has owned the maximum once"""
    kk = k * k
    pos = []
    for p in (0, 63, 64, 65, k - 1, k, k * (k - 1), kk - 64, kk - 1):
        if 0 <= p < kk and p not in pos:
            pos.append(p)
    for r in range(min(64, kk)):
        if not any(p % 64 == r for p in pos):
            trips = (kk - r + 63) // 64
            pos.append(r + 64 * int(torch.randint(0, trips, (1,), generator=g)))
    assert all(0 <= p < kk for p in pos) and {p % 64 for p in pos} == set(range(min(64, kk)))
    return pos


def _planted(k, H, W, positions, g):
    """six planes per position: background in [-2, -1], in every window one value in [-0.5, -0.1] at that position"""
    ho, wo = H // k, W // k
    x = -(1 + torch.rand(len(positions), 6, H, W, generator=g))
    vals = -(0.1 + 0.4 * torch.rand(len(positions), 6, ho, wo, generator=g))
    for j, p in enumerate(positions):
        dy, dx = divmod(p, k)
        x[j, :, dy:ho * k:k, dx:wo * k:k] = vals[j]
    return x, vals


@pytest.mark.parametrize("k,H,W", POOL_SMALL + POOL_WAVE)
def test_max_pool_planted_maximum(k, H, W):
    import fresco_amd.ops as ops
    assert H != W and (k < 8 or (H % k and W % k))
    g = synth.gen(300 + k + H)
    positions = _window_positions(k, g)
    for i in range(0, len(positions), 10):  # (60 planes a call)
        x, vals = _planted(k, H, W, positions[i:i + 10], g)
        ref = O.max_pool(x, k)
        assert torch.equal(ref, vals) and float(x.max()) < 0
        out = ops.max_pool(x.to(DEV), k).cpu()
        assert out.shape == ref.shape
        assert torch.equal(out, ref), (positions[i:i + 10], maxdiff(out, ref))


@pytest.mark.parametrize("k,H,W", [c for c in POOL_SMALL + POOL_WAVE if c[0] in (3, 8, 13)])
def test_max_pool_all_distinct(k, H, W):
    import fresco_amd.ops as ops
    g = synth.gen(350 + k + H)
    x = (torch.randperm(6 * H * W, generator=g).float() - 3 * H * W).view(2, 3, H, W)
    out = ops.max_pool(x.to(DEV), k).cpu()
    assert torch.equal(out, O.max_pool(x, k))


# ---- dilate -------------------------------------------------------------------------------------------------------------
DILATE_SHAPES = [(20, 45), (45, 20), (5, 4), (1, 30)]  # (5 x 4 and 1 x 30: the radius of k = 13 covers the plane)


@pytest.mark.parametrize("H,W", DILATE_SHAPES)
@pytest.mark.parametrize("k", [1, 3, 7, 13])
def test_dilate_binary_exact(k, H, W):
    import fresco_amd
    g = synth.gen(400 + k + H)
    x = torch.stack([(torch.rand(1, H, W, generator=g) < p).float() for p in (0.004, 0.03, 0.3)])  # three unequal planes
    x[0, 0, H // 2, W // 2] = 1.0
    out = fresco_amd.Dilate(k)(x.to(DEV)).cpu()
    ref = O.dilate(x, k)
    assert torch.equal(out, ref)
    if k == 1:
        assert torch.equal(out, x)


@pytest.mark.parametrize("H,W", DILATE_SHAPES)
@pytest.mark.parametrize("k", [1, 3, 7, 13])
def test_dilate_signed_sums(k, H, W):
    """uniform data in [-0.3, 0.3]: box sums on both sides of both clamps"""
    import fresco_amd.ops as ops
    g = synth.gen(450 + k + H)
    x = (torch.rand(1, 3, H, W, generator=g) - 0.5) * 0.6
    ref = O.dilate(x.double(), k)
    if k > 1 and H * W == 900:  # (the data does what it is for: clamped below, unclamped, and from k = 7 up clamped above)
        assert float(ref.min()) == 0.0 and float(((ref > 0) & (ref < 1)).double().mean()) > 0.1
        assert k < 7 or float(ref.max()) == 1.0
    out = ops.dilate(x.to(DEV), k)
    ratio = maxdiff(out, ref) / (k * k * 2.0 ** -23)
    _report("dilate signed k=%d %dx%d" % (k, H, W), ratio)
    assert ratio <= 1.0


# ---- AdaIN / calc_mean_std ---------------------------------------------------------------------------------------------
ADAIN_L = [2, 3, 63, 255, 256, 257, 1792, 4096, 4097]
ADAIN_DISTS = [(0.3, 1.7), (8.0, 0.5), (100.0, 0.05), (0.0, 1e-4)]  # content (mean, std)


def _adain_inputs(L, rows, mean, std, g):
    """(1, rows, plane) content and style; with six rows, row 4 has constant content and row 5 constant style"""
    plane = (32, 56) if L == 1792 else (L, 1)
    c = mean + std * torch.randn(1, rows, *plane, generator=g)
    s = 0.6 * torch.randn(1, rows, *plane, generator=g) - 0.2
    if rows == 6:
        c[0, 4] = 0.7
        s[0, 5] = -0.2
    return c, s


def _adain_ref_and_bar(c, s):
    """O.adain in float64 and the per-row fp32 bar 8 u (max|c| / std_c std_s + max|out|), all from float64"""
    c, s = c.double(), s.double()
    rows = c.shape[0] * c.shape[1]
    ref = O.adain(c, s)
    xc, xs = c.reshape(rows, -1), s.reshape(rows, -1)
    std_c = (xc.var(1) + 1e-5).sqrt()
    std_s = (xs.var(1) + 1.0).sqrt()
    bar = 8 * U * (xc.abs().amax(1) / std_c * std_s + ref.reshape(rows, -1).abs().amax(1))
    return ref, bar.view(c.shape[0], c.shape[1], *([1] * (c.dim() - 2)))


def _mean_std_ref_and_bars(c, factor=8):
    c = c.double()
    rows = c.shape[0] * c.shape[1]
    xc = c.reshape(rows, -1)
    mean, std = xc.mean(1), (xc.var(1) + 1e-5).sqrt()
    bar_m = factor * U * xc.abs().amax(1)
    shape = (c.shape[0], c.shape[1], 1, 1)
    return mean.view(shape), std.view(shape), bar_m.view(shape), (bar_m + factor * U * std).view(shape)


def _half_ulp(ref, dtype):
    """half the spacing of `dtype` at |ref| (float64 in, float64 out)"""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    _, e = torch.frexp(ref.abs())  # |ref| = m 2^e, m in [0.5, 1)
    e = (e - 1).clamp(min=emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - mant - 1).double())


@pytest.mark.parametrize("rows", [1, 6])
@pytest.mark.parametrize("L", ADAIN_L)
def test_adain_row_lengths(L, rows):
    import fresco_amd
    g = synth.gen(500 + L + rows)
    worst = 0.0
    for mean, std in ADAIN_DISTS:
        c, s = _adain_inputs(L, rows, mean, std, g)
        ref, bar = _adain_ref_and_bar(c, s)
        out = fresco_amd.adaptive_instance_normalization(c.to(DEV), s.to(DEV))
        assert out.dtype == torch.float32 and out.shape == c.shape
        ratio = float(((out.double().cpu() - ref).abs() / bar).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (mean, std, ratio)
    _report("adain L=%d rows=%d" % (L, rows), worst)


@pytest.mark.parametrize("rows", [1, 6])
@pytest.mark.parametrize("L", ADAIN_L)
def test_calc_mean_std_row_lengths(L, rows):
    import fresco_amd
    g = synth.gen(500 + L + rows)
    worst = 0.0
    for mean, std in ADAIN_DISTS:
        c, _ = _adain_inputs(L, rows, mean, std, g)
        rm, rs, bar_m, bar_s = _mean_std_ref_and_bars(c)
        m, sd = fresco_amd.calc_mean_std(c.to(DEV))
        assert m.shape == sd.shape == (1, rows, 1, 1) and m.dtype == sd.dtype == torch.float32
        ratio = max(float(((m.double().cpu() - rm).abs() / bar_m).max()), float(((sd.double().cpu() - rs).abs() / bar_s).max()))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (mean, std, ratio)
    _report("calc_mean_std L=%d rows=%d" % (L, rows), worst)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("L", [257, 4096])
def test_adain_and_mean_std_16bit(L, dtype):
    import fresco_amd
    g = synth.gen(560 + L)
    worst = 0.0
    for mean, std in ADAIN_DISTS:
        c, s = _adain_inputs(L, 6, mean, std, g)
        c, s = c.to(dtype), s.to(dtype)  # the reference sees the rounded inputs
        ref, bar = _adain_ref_and_bar(c, s)
        out = fresco_amd.adaptive_instance_normalization(c.to(DEV), s.to(DEV))
        assert out.dtype == dtype
        ratio = float(((out.double().cpu() - ref).abs() / (_half_ulp(ref, dtype) + bar)).max())
        rm, rs, bar_m, bar_s = _mean_std_ref_and_bars(c)
        m, sd = fresco_amd.calc_mean_std(c.to(DEV))
        assert m.dtype == dtype and sd.dtype == dtype
        ratio = max(ratio, float(((m.double().cpu() - rm).abs() / (_half_ulp(rm, dtype) + bar_m)).max()),
                    float(((sd.double().cpu() - rs).abs() / (_half_ulp(rs, dtype) + bar_s)).max()))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (mean, std, ratio)
    _report("adain + calc_mean_std %s L=%d" % (str(dtype).split(".")[1], L), worst)


# ---- DDPM step kernels -------------------------------------------------------------------------------------------------
DDPM_SHAPES = [(1,), (255,), (257,), (3, 5, 7, 11)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def _ddpm_inputs(shape, dtype, g):
    xt, eu, ec = (torch.randn(*shape, generator=g) * s for s in (1.3, 1.0, 1.0))
    return [t.to(dtype) for t in (xt, eu, ec)]


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", DDPM_SHAPES)
def test_predict_x0_sizes(shape, dtype, cfg):
    """fp32: x0 = (x_t - sqrt(1 - a) eps) / sqrt(a), eps = e_u + s (e_c - e_u), against float64 within 4 u (sum of |terms|).
    16-bit: the fp32 kernel's result on the upcast inputs, rounded once."""
    import fresco_amd
    g = synth.gen(600 + len(shape))
    a, gs = 0.37, 7.5
    xt, eu, ec = _ddpm_inputs(shape, dtype, g)
    args = (xt.to(DEV), eu.to(DEV), ec.to(DEV) if cfg else None)
    x0, eps = fresco_amd.predict_x0(*args, guidance_scale=gs, alpha_prod_t=a)
    assert x0.dtype == dtype and eps.dtype == dtype and x0.shape == xt.shape and eps.shape == xt.shape
    if dtype != torch.float32:
        up = [None if t is None else t.float() for t in args]
        x0f, epsf = fresco_amd.predict_x0(*up, guidance_scale=gs, alpha_prod_t=a)
        assert torch.equal(x0, x0f.to(dtype)) and torch.equal(eps, epsf.to(dtype))
        return
    xt, eu, ec = xt.double(), eu.double(), ec.double()
    sb, sa = (1 - a) ** 0.5, a ** 0.5
    e_ref = eu + gs * (ec - eu) if cfg else eu
    e_terms = eu.abs() + gs * (ec.abs() + eu.abs()) if cfg else eu.abs()
    x0_ref = (xt - sb * e_ref) / sa
    r_e = float(((eps.double().cpu() - e_ref).abs() / (4 * U * e_terms)).max())
    r_x = float(((x0.double().cpu() - x0_ref).abs() / (4 * U * (xt.abs() + sb * e_terms) / sa)).max())
    _report("predict_x0 n=%d cfg=%d" % (xt.numel(), cfg), max(r_e, r_x))
    assert r_e <= 1.0 and r_x <= 1.0, (r_e, r_x)
    if not cfg:
        assert torch.equal(eps.cpu(), eu.float())


@pytest.mark.parametrize("t", [701, 1])
@pytest.mark.parametrize("rep", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_step_noise_period_not_a_power_of_two(dtype, rep, t, monkeypatch):
    """batch 3 of 5 x 7 x 11 latents: n = 1155, and with repeat_noise the noise period is 385.  fp32:
    x_{t-1} = c0 x0 + c1 x_t + sigma z against float64 within 4 u (sum of |terms|), on the x0 the step returned; 16-bit: the
    fp32 kernel's result on the same stored x0, rounded once."""
    import fresco_amd
    S = sys.modules["fresco_amd.step"]  # `fresco_amd.step` itself is the function
    import make_step_golden as msg
    g = synth.gen(650)
    shape = (3, 5, 7, 11)
    x, eps, _ = _ddpm_inputs(shape, dtype, g)
    noise = torch.randn(*shape, generator=g).to(dtype).to(DEV)
    monkeypatch.setattr(S.torch, "randn", lambda *a, **k: noise.to(k.get("dtype", torch.float32)))
    dx, de = x.to(DEV), eps.to(DEV)
    prev, x0 = fresco_amd.step(msg.P(), de, t, dx, None, repeat_noise=rep)
    assert prev.dtype == dtype and x0.dtype == dtype and prev.shape == x.shape
    if dtype != torch.float32:
        _, x0_f = fresco_amd.step(msg.P(), de.float(), t, dx.float(), None, repeat_noise=rep)
        assert torch.equal(x0, x0_f.to(dtype))
        with monkeypatch.context() as m:
            m.setattr(S, "predict_x0", lambda *a, **k: (x0.float(), None))
            prev_f, _ = fresco_amd.step(msg.P(), de.float(), t, dx.float(), None, repeat_noise=rep)
        assert prev_f.dtype == torch.float32 and torch.equal(prev, prev_f.to(dtype))
        return
    ac = msg.P.scheduler.alphas_cumprod
    a_t = float(ac[t])
    a_prev = float(ac[t - 50]) if t - 50 >= 0 else 1.0
    cur_a = a_t / a_prev
    c0 = a_prev ** 0.5 * (1 - cur_a) / (1 - a_t)
    c1 = cur_a ** 0.5 * (1 - a_prev) / (1 - a_t)
    sigma = max((1 - a_prev) / (1 - a_t) * (1 - cur_a), 1e-20) ** 0.5
    xd, ed = x.double(), eps.double()
    x0_ref = (xd - (1 - a_t) ** 0.5 * ed) / a_t ** 0.5
    r_x = float(((x0.double().cpu() - x0_ref).abs() / (4 * U * (xd.abs() + (1 - a_t) ** 0.5 * ed.abs()) / a_t ** 0.5)).max())
    z = noise.double().cpu()
    if rep:
        z = z[0:1].expand(3, -1, -1, -1)
    x0d = x0.double().cpu()
    prev_ref = c0 * x0d + c1 * xd + sigma * z
    r_p = float(((prev.double().cpu() - prev_ref).abs() / (4 * U * (c0 * x0d.abs() + c1 * xd.abs() + sigma * z.abs()))).max())
    _report("step t=%d repeat_noise=%d" % (t, rep), max(r_x, r_p))
    assert r_x <= 1.0 and r_p <= 1.0, (r_x, r_p)
    if t == 701:  # (at t = 1 sigma is 1e-10: the noise does not reach the result)
        assert maxdiff(prev, prev_ref) < 1e-5 < maxdiff(prev, prev_ref - sigma * z)


# ---- warp_tensor chain --------------------------------------------------------------------------------------------------
def _flows(N, H, W, g, occ_p=0.1):
    """the data of test_gpu_nonsquare.py: constant (3, -2) px + 0.3 px noise, fwd = -bwd, Bernoulli occlusions"""
    base = torch.tensor([3.0, -2.0]).view(1, 2, 1, 1)
    bwd = base + 0.3 * torch.randn(N, 2, H, W, generator=g)
    fo = (torch.rand(N, H, W, generator=g) < occ_p).float()
    bo = (torch.rand(N, H, W, generator=g) < occ_p).float()
    return [-bwd, bwd], [fo, bo]


def _gpu(ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize("C", [1, 9])
@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("N", [2, 3])
def test_warp_tensor_short_chains(N, chunk, C):
    import fresco_amd
    g = synth.gen(700 + 10 * N + chunk + C)
    flows, occs = _flows(N, 48, 80, g)
    sal = torch.rand(N, 1, 24, 40, generator=g)
    x = torch.randn(chunk * N, C, 12, 20, generator=g)
    xd = x.to(DEV)
    out = fresco_amd.warp_tensor(xd, _gpu(flows), _gpu(occs), sal.to(DEV), chunk)
    assert torch.equal(xd.cpu(), x)  # the chain ran on a private copy
    ref = O.warp_tensor(x, flows, occs, sal, chunk, compute_dtype=torch.float32)
    assert maxdiff(ref, x) > 0.1
    e = maxdiff(out, ref)
    _report("warp_tensor N=%d chunk=%d C=%d" % (N, chunk, C), e / 5e-5)
    assert e < 5e-5, e


# ---- flow_occlusion, colour path ---------------------------------------------------------------------------------------
def _occlusion_case(N, C, H, W, seed):
    g = synth.gen(seed)
    (fwd, bwd), _ = _flows(N, H, W, g)
    # the round trip closes almost everywhere, with patches where it does not (test_gpu_paras.py)
    bwd = bwd + 0.4 * (torch.rand(N, 1, H, W, generator=g) < 0.05).float() * torch.randn(N, 2, H, W, generator=g)
    images = torch.rand(N, C, H, W, generator=g) * 255.0
    images = torch.nn.functional.avg_pool2d(images, 9, 1, 4)  # smooth: the colour test near its threshold
    images = (images - images.mean()) * 6.0 + 128.0
    return images, fwd, bwd


@pytest.mark.parametrize("N,C,H,W", [(1, 1, 40, 56), (3, 3, 56, 40)])
def test_flow_occlusion_colour_small(N, C, H, W):
    """N = 1 pairs the frame with itself ((n + 1) % N = n); C = 1 makes the channel mean a single term"""
    import fresco_amd.ops as ops
    images, fwd, bwd = _occlusion_case(N, C, H, W, 800 + N)
    fo, bo = ops.flow_occlusion(fwd.to(DEV), bwd.to(DEV), images.to(DEV))
    ro, rb = O.flow_occlusions(images, fwd, bwd)
    r2, rb2 = O.fb_consistency_check(fwd, bwd)
    assert int((ro != r2).sum()) > 10 and int((rb != rb2).sum()) > 10  # (the colour test decides pixels of its own)
    for a, b in ((fo, ro), (bo, rb)):
        frac = float(b.mean())
        assert 0.02 < frac < 0.98, frac
        assert tuple(a.shape) == (N, H, W)
        assert int((a.cpu() != b).sum()) <= 4  # last-bit ties of a float threshold


# ---- the derived-tensor cache in front of the kernels -----------------------------------------------------------------
@pytest.fixture
def clean_cache():
    from fresco_amd import warp
    warp.invalidate_cache()
    yield warp
    warp.invalidate_cache()


def test_warp_tensor_cache_hit_and_in_place_miss(clean_cache, monkeypatch):
    import fresco_amd
    import fresco_amd.ops as ops
    warp = clean_cache
    g = synth.gen(900)
    N, chunk = 3, 2
    flows, occs = _flows(N, 48, 80, g)
    sal = torch.rand(N, 1, 24, 40, generator=g)
    x = torch.randn(chunk * N, 9, 12, 20, generator=g)
    fd, od, sd, xd = _gpu(flows), _gpu(occs), sal.to(DEV), x.to(DEV)
    calls = []
    real = ops.resize_bilinear
    monkeypatch.setattr(ops, "resize_bilinear", lambda *a, **k: calls.append(1) or real(*a, **k))
    out1 = fresco_amd.warp_tensor(xd, fd, od, sd, chunk)
    assert len(calls) == 3 and len(warp._derived) == 2  # two flows, the saliency; one flow_occ and one saliency entry
    out2 = fresco_amd.warp_tensor(xd, fd, od, sd, chunk)
    assert len(calls) == 3 and torch.equal(out1, out2)
    assert maxdiff(out1, O.warp_tensor(x, flows, occs, sal, chunk)) < 5e-5
    fd[1].mul_(1.5)
    out3 = fresco_amd.warp_tensor(xd, fd, od, sd, chunk)
    assert len(calls) == 6  # both flows again (one entry holds them); the saliency entry is keyed on the flows too: rebuilt
    new_flows = [f.cpu() for f in fd]
    assert maxdiff(out3, O.warp_tensor(x, new_flows, occs, sal, chunk)) < 5e-5
    assert maxdiff(out3, out1) > 1e-2
    # the documented hole and its remedy
    od[1].data.copy_(torch.zeros_like(od[1]))
    assert torch.equal(fresco_amd.warp_tensor(xd, fd, od, sd, chunk), out3)
    warp.invalidate_cache()
    out4 = fresco_amd.warp_tensor(xd, fd, od, sd, chunk)
    assert maxdiff(out4, O.warp_tensor(x, new_flows, [occs[0], torch.zeros_like(occs[1])], sal, chunk)) < 5e-5


def test_cache_keeps_dilated_and_plain_occlusions_apart(clean_cache):
    """optimize_feature (no Dilate) and warp_tensor (Dilate-13) at scale 1 on the same flows: two flow_occ entries"""
    import fresco_amd
    warp = clean_cache
    g = synth.gen(910)
    N, chunk, h, w = 3, 2, 24, 40
    flows, occs = _flows(N, h, w, g, occ_p=0.004)
    sal = torch.rand(N, 1, h, w, generator=g)
    x = torch.randn(chunk * N, 9, h, w, generator=g)
    fd, od, xd = _gpu(flows), _gpu(occs), x.to(DEV)
    for order in (0, 1):
        warp.invalidate_cache()
        for which in ((0, 1), (1, 0))[order]:
            if which == 0:
                opt = fresco_amd.optimize_feature(xd, fd, od, [], iters=0, unet_chunk_size=chunk)
            else:
                wt = fresco_amd.warp_tensor(xd, fd, od, sal.to(DEV), chunk)
        entries = {k[1]: v[1] for k, v in warp._derived.items() if k[0] == "flow_occ"}
        assert set(entries) == {(h, True), (h, False)}
        want = O.warp_prepare(h, flows, occs, None, torch.float32)[:4]
        plain = O.opt_prepare(h, flows, occs, 1, torch.float32)
        assert float(want[3].sum()) > 2 * float(plain[3].sum()) > 0  # (Dilate does something here)
        for got, ref_d in zip(entries[(h, True)], want):
            assert maxdiff(got.view(ref_d.shape), ref_d) < 1e-6
        for got, ref_p in zip(entries[(h, False)], plain):
            assert maxdiff(got.view(ref_p.shape), ref_p) < 1e-6
        assert torch.equal(entries[(h, False)][3].cpu().view(N, h, w), occs[1])
        assert maxdiff(wt, O.warp_tensor(x, flows, occs, sal, chunk)) < 5e-5
        ref, bar = _adain_ref_and_bar(x, x)  # optimize_feature with no iteration is AdaIN of the sample onto itself
        assert maxdiff(O.optimize_feature(x.double(), flows, occs, [], iters=0, unet_chunk_size=chunk,
                                          compute_dtype=torch.float64), ref) == 0
        assert float(((opt.double().cpu() - ref).abs() / bar).max()) <= 1.0
