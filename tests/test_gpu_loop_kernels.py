"""loop_update and loop_image_to_frames (csrc/loop.hip) on the GPU, called through the C ABI.

loop_update: frames 1, 2 and 3 of 4, 36, 256 and 1020 elements (below one block, ragged, one block, several blocks with a
ragged tail) and one launch of 3 x 49152; every tensor is a view one element behind a 16-byte boundary, with a sentinel in
front of and behind it.  Inputs are finite normal draws (latents, eps and noise of a pipeline are about unit variance) with
the coefficients of timestep 601 of the SD-1.5 schedule.

  * fp32: the bits of fresco_ddpm_prev(fresco_ddpm_x0(...)) on the same inputs (nothing is rounded in between).
  * every dtype against the float64 formula: |got - ref| <= u |ref| + 16 * 2^-24 * mass + tiny, u = 2^-11 (fp16), 2^-8 (bf16)
    or 2^-24 (fp32) for the one rounding of the result, mass = |c_x0| (|xt| + sqrt_beta (|e_u| + |g| (|e_c| + |e_u|))) /
    sqrt_alpha + |c_xt xt| + |sigma z| for the about ten fp32 operations on magnitudes of at most mass, tiny the dtype's
    smallest subnormal.
  * restored rows, record rows and both model-input halves: torch.equal with what they copy.

loop_image_to_frames: every fp16 bit pattern against the reference's recorded table; C = 1 and C = 4; fp32 at the 256 levels
and around the 255 rounding boundaries, infinities, zeros and subnormals against the restated expression on the CPU.
"""
import itertools
import os

import numpy as np
import pytest
import torch

import loop_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 768.0  # (representable in bf16)
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}
GUIDANCE = 7.5
# (guidance, x0_in, noise period of one frame, in place)
MATH_MODES = [(True, False, False, False), (False, False, True, False), (False, True, False, True),
              (True, False, True, True), (True, True, False, False)]


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def coeffs():
    """sqrt_beta, sqrt_alpha, c_x0, c_xt, sigma of timestep 601 as the fp32 values the C ABI receives"""
    from fresco_amd.loop import _coefficients
    return [float(np.float32(c)) for c in _coefficients(M.Scheduler(), [601])[0][:5]]


def view(n, dtype, gen=None, scale=1.0):
    """n elements one element behind a 16-byte boundary, a sentinel on either side: (buffer, view)"""
    buf = torch.full((n + 2,), SENTINEL, dtype=dtype, device=DEV)
    if gen is not None:
        buf[1:n + 1] = (scale * torch.randn(n, generator=gen, dtype=torch.float64)).to(dtype).to(DEV)
    v = buf[1:n + 1]
    assert v.data_ptr() % 16 == v.element_size()
    return buf, v


def intact(buf):
    return float(buf[0]) == SENTINEL and float(buf[-1]) == SENTINEL


def code(dtype):
    from fresco_amd import _lib
    return {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16, torch.float32: _lib.F32}[dtype]


def ptr(t):
    return None if t is None else t.data_ptr()


def run_case(lib, coeffs, dtype, frames, fe, mode, restore_on, record_on, copies, gen):
    guided, with_x0, frame_period, in_place = mode
    sb, sa, c0, c1, sigma = coeffs
    n = frames * fe
    xt_buf, xt = view(n, dtype, gen)
    eps_buf, eps = view(2 * n if guided else n, dtype, gen)
    x0_buf, x0 = view(n, dtype, gen, 3.0) if with_x0 else (None, None)
    nz_buf, noise = view(fe if frame_period else n, dtype, gen)
    rs_buf, restore = view(2 * fe, dtype, gen) if restore_on else (None, None)
    out_buf, out = (xt_buf, xt) if in_place else view(n, dtype)
    mi_buf, mi = view(copies * n, dtype) if copies else (None, None)
    rc_buf, record = view(2 * fe, dtype) if record_on else (None, None)

    d = lambda t: t.double().cpu()  # noqa: E731
    X, E, Z = d(xt), d(eps), d(noise)
    Z = Z.repeat(frames) if frame_period else Z
    if with_x0:
        x0_ref = d(x0)
        mass = abs(c0) * x0_ref.abs()
    else:
        eu = E[:n]
        if guided:
            ec = E[n:]
            e = eu + GUIDANCE * (ec - eu)
            emass = eu.abs() + GUIDANCE * (ec.abs() + eu.abs())
        else:
            e, emass = eu, eu.abs()
        x0_ref = (X - sb * e) / sa
        mass = abs(c0) * (X.abs() + sb * emass) / sa
    ref = (c0 * x0_ref + c1 * X) + sigma * Z
    mass = mass + (c1 * X).abs() + (sigma * Z).abs()

    want32 = None
    if dtype == torch.float32:  # the two-kernel route on the same inputs, before xt may be overwritten
        x0_two = torch.empty(n, dtype=dtype, device=DEV)
        if with_x0:
            x0_two.copy_(x0)
        else:
            rc = lib.fresco_ddpm_x0(ptr(xt), ptr(eps), ptr(eps[n:]) if guided else None, ptr(x0_two), None, n, GUIDANCE, sb, sa,
                                    code(dtype), None)
            assert rc == 0
        want32 = torch.empty(n, dtype=dtype, device=DEV)
        assert lib.fresco_ddpm_prev(ptr(x0_two), ptr(xt), ptr(noise), ptr(want32), n, noise.numel(), c0, c1, sigma, code(dtype),
                                    None) == 0

    rc = lib.loop_update(ptr(xt), ptr(eps), ptr(x0), ptr(noise), ptr(restore), ptr(out), ptr(mi), ptr(record), frames, fe,
                         n if guided else 0, noise.numel(), copies or 1, GUIDANCE, sb, sa, c0, c1, sigma, code(dtype), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    tag = (str(dtype), frames, fe, mode, restore_on, record_on, copies)
    for b in (xt_buf, eps_buf, x0_buf, nz_buf, rs_buf, out_buf, mi_buf, rc_buf):
        assert b is None or intact(b), tag

    lo = 0
    if restore_on:
        lo = 2 * fe
        assert torch.equal(out[:lo], restore), tag
    got = out[lo:]
    err = (d(got) - ref[lo:]).abs()
    bound = UNIT[dtype] * ref[lo:].abs() + 16 * 2.0 ** -24 * mass[lo:] + TINY[dtype]
    assert bool((err <= bound).all()), (tag, float((err / bound).max()))
    if want32 is not None:
        assert torch.equal(got, want32[lo:]), tag
    if copies:
        assert torch.equal(mi[:n], out) and (copies == 1 or torch.equal(mi[n:], out)), tag
    if record_on:
        assert torch.equal(record[:fe], out[:fe]) and torch.equal(record[fe:], out[(frames - 1) * fe:]), tag
    return float((err / bound).max()) if err.numel() else 0.0


@pytest.mark.parametrize("frames", [1, 2, 3])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
def test_loop_update(lib, coeffs, dtype, frames):
    gen = torch.Generator().manual_seed(100 * frames + len(str(dtype)))
    worst = 0.0
    for fe in (4, 36, 256, 1020):
        for mode, restore_on, record_on, copies in itertools.product(MATH_MODES, (False, True), (False, True), (0, 1, 2)):
            if restore_on and frames < 2:
                continue
            worst = max(worst, run_case(lib, coeffs, dtype, frames, fe, mode, restore_on, record_on, copies, gen))
    print("%s frames %d: worst error %.3f of the bound" % (dtype, frames, worst))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
def test_loop_update_at_three_frames_of_49152(lib, coeffs, dtype):
    gen = torch.Generator().manual_seed(7)
    worst = run_case(lib, coeffs, dtype, 3, 49152, (True, False, False, False), True, True, 2, gen)
    print("%s 3 x 49152: worst error %.3f of the bound" % (dtype, worst))


def frames_of(lib, x):
    n, C, H, W = x.shape
    out = torch.full((n * H * W * C + 2,), 99, dtype=torch.uint8, device=DEV)
    assert lib.loop_image_to_frames(x.data_ptr(), out[1:].data_ptr(), n, C, H, W, code(x.dtype), None) == 0
    torch.cuda.synchronize()
    assert int(out[0]) == 99 and int(out[-1]) == 99
    return out[1:-1].view(n, H, W, C).cpu().numpy()


def test_image_to_frames_on_every_fp16_pattern(lib):
    lg = np.load(os.path.join(ROOT, "tests", "golden", M.GOLDEN_FILE))
    table, nan = lg["u8_table"], lg["u8_nan"]
    count = 3 * 128 * 171
    idx = np.concatenate([np.arange(65536), np.arange(65536 - (count - 65536), 65536)])  # the tail repeated
    x = torch.from_numpy(idx.astype(np.uint16).view(np.float16).reshape(1, 3, 128, 171).copy()).to(DEV)
    got = frames_of(lib, x).transpose(0, 3, 1, 2).reshape(-1)
    keep = ~nan[idx]
    assert np.array_equal(got[keep], table[idx][keep])
    assert not got[~keep].any()  # a NaN writes 0


@pytest.mark.parametrize("C", [1, 4])
def test_image_to_frames_channel_counts(lib, C):
    gen = torch.Generator().manual_seed(C)
    for dtype in (torch.float16, torch.float32):
        buf, v = view(2 * C * 5 * 7, dtype, gen, 0.8)
        x = v.view(2, C, 5, 7)
        assert np.array_equal(frames_of(lib, x), M.image_to_frames_model(x.cpu()))
        assert intact(buf)


def test_image_to_frames_fp32_levels_and_boundaries(lib):
    f32 = np.float32
    levels = (2.0 * np.arange(256) / 255.0 - 1.0).astype(f32)
    edges = (2.0 * (np.arange(255) + 0.5) / 255.0 - 1.0).astype(f32)
    around = [edges]
    up, down = edges, edges
    for _ in range(2):
        up, down = np.nextafter(up, f32(np.inf)), np.nextafter(down, f32(-np.inf))
        around += [up, down]
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0, 1.5, -1.5, 3e38, -3e38], f32)
    vals = np.concatenate([levels] + around + [special])
    vals = np.concatenate([vals, np.zeros(-len(vals) % 3, f32)])
    x = torch.from_numpy(vals.reshape(1, 3, 1, -1).copy())
    want = M.image_to_frames_model(x)
    assert np.array_equal(frames_of(lib, x.to(DEV)), want)
    assert set(np.unique(want)) == set(range(256))
