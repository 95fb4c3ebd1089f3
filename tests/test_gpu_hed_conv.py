"""Each of the HED detector's 3 x 3 convolutions alone (fresco_fn_gemm, csrc/flownet.hip) against a float64 convolution,
at the channel widths of the network and on the kernel forms a 512 x 512 frame takes: the window-in-LDS form up to 16
channel chunks (cin = 512, K = 4608) and four column blocks (cout = 512), the XCD-aware workgroup order's main branch
(eight row blocks and more) with and without a tail, and the im2col form at the same widths.

A convolution is driven exactly as fresco_amd/hed.py::_sides_native drives it: weight planes from
fnweights.WeightPlanes().get(param, "conv", pad), activation planes from ops.fn_prep (the first convolution's from
ops.hed_input, 3 channels padded to 32), bias and ReLU in the epilogue, fp32 rows out (a block's last convolution) or
operand planes only (the others), under ops.fn_range_guard.

Inputs: activations relu(N(0, 1)) * 60 with every 7th pixel scaled by 1e-3 (their lo planes matter), peak about 300 of the
1015 the planes hold at scale 64; weights 0.9 sqrt(2 / fan_in) N(0, 1); biases 0.1 N(0, 1).  The first convolution reads
uint8 frames minus hed_model.NORM.

Bounds, per output element, both the project's own:
  * tests/test_gpu_flownet.py's bar for fp32-accumulated products of (hi, lo) planes: |err| <= 4e-6 S + 1e-6 with
    S = conv(|x|, |w|) + |b|;
  * planes-only runs add tests/test_gpu_hed.py's plane bound, (2^-21 |ref * scale| + 2^-25) / scale.
Every case prints its worst error / bound and, next to it, the same ratio for a CPU fp32 F.conv2d of the same operands.

Measured on an MI355X, worst error / bound over the 13 cases: fp32 rows 0.041 - 0.071, planes only 0.044 - 0.070, the
CPU fp32 convolution 0.010 - 0.046; the runs at scales (32, 16) give the figures of scale 64.  A scratch build without the
a_lo * w_hi product fails all 26 tests (ratios of 11 and more).  DESIGN.md section 12 has the table per case.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hed_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (cin, cout, n, H, W).  Window-in-LDS form: the smallest maps of whole 16 x 16 patches
PATCH_CASES = [
    (3, 64, 2, 16, 32),       # the first convolution, from hed_input planes; BN = 64; one channel chunk
    (64, 64, 2, 16, 16),
    (64, 128, 2, 32, 16),
    (128, 128, 1, 16, 16),
    (128, 256, 1, 16, 16),
    (256, 256, 2, 16, 16),
    (256, 512, 2, 16, 32),
    (512, 512, 2, 16, 16),    # 16 chunks, four column blocks
    (256, 512, 8, 16, 16),    # eight row blocks: the XCD order's main branch, no tail
    (512, 512, 9, 16, 16),    # nine: the main branch plus one tail row block, four column blocks
]
# im2col form at the same widths (maps that are not whole patches)
IM2COL_CASES = [
    (512, 512, 2, 8, 8),      # M = 128: less than one row block
    (512, 512, 3, 4, 4),
    (256, 512, 1, 9, 11),
]
CASES = PATCH_CASES + IM2COL_CASES
# the cases that also run with the planes of the lowered-scale remedy (a_scale != out_scale)
SCALED_CASES = {c for c in CASES if c[:2] == (256, 512)} | {(512, 512, 2, 16, 16)}


def _case_id(c):
    return "%dto%d_%dx%dx%d" % c


@functools.lru_cache(maxsize=None)
def _problem(case):
    """operands of a case and its float64 results, computed once: dict of CPU tensors (left unchanged by the tests)"""
    cin, cout, n, H, W = case
    g = torch.Generator().manual_seed(1000 * cin + cout + 17 * n + H + W)
    frames = None
    if cin == 3:
        frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8)
        norm = torch.tensor(M.NORM, dtype=torch.float32)
        rows = (frames.double() - norm.double()).reshape(n * H * W, 3)
    else:
        rows = torch.randn(n * H * W, cin, generator=g).clamp_min(0) * 60.0
        rows[::7] *= 1e-3
        rows = rows.double()  # the fp32 values the GPU is given, exactly
    w = (0.9 * (2.0 / (9 * cin)) ** 0.5 * torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)).float()
    b = (0.1 * torch.randn(cout, generator=g, dtype=torch.float64)).float()
    x = rows.reshape(n, H, W, cin).permute(0, 3, 1, 2).contiguous()
    ref = F.relu(F.conv2d(x, w.double(), b.double(), padding=1))
    S = F.conv2d(x.abs(), w.double().abs(), None, padding=1) + b.double().abs().view(1, -1, 1, 1)
    lib32 = F.relu(F.conv2d(x.float(), w, b, padding=1)).double()
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(n * H * W, cout).numpy()  # noqa: E731
    return dict(frames=frames, rows=rows.float(), w=w, b=b, ref=to_rows(ref), S=to_rows(S), lib32=to_rows(lib32),
                peak=float(x.abs().max()), out_peak=float(ref.max()))


def _convolve(case, want_f32, a_scale, out_scale):
    """one convolution as _sides_native runs it -> (fp32 rows or None, (hi, lo) or None), the guard's verdict"""
    from fresco_amd import ops
    from fresco_amd.fnweights import WeightPlanes
    cin, cout, n, H, W = case
    p = _problem(case)
    wts = WeightPlanes()
    weight = p["w"].to(DEV)
    bias = p["b"].to(DEV)
    with ops.fn_range_guard(torch.device(DEV)) as guard:
        if cin == 3:
            xs = ops.hed_input(p["frames"].to(DEV), torch.tensor(M.NORM, dtype=torch.float32, device=DEV), scale=a_scale)
        else:
            _, xs = ops.fn_prep(p["rows"].to(DEV), ld=cin, scale=a_scale)
        wp = wts.get(weight, "conv", 32 if cin == 3 else None)
        assert wp[0].shape == (cout, 9 * max(cin, 32))
        out, planes = ops.fn_gemm(xs, wp, cout, wp[0].shape[1], bias=bias, act=1, conv=(n, H, W, 3, 3, 1, 1),
                                  want_f32=want_f32, want_split=not want_f32, a_scale=a_scale, out_scale=out_scale)
    return out, planes, guard.tripped() or wts.out_of_range


def _np64(t):
    return t.detach().to("cpu", torch.float64).numpy()


def _scales(case):
    return [(64.0, 64.0)] + ([(32.0, 16.0)] if case in SCALED_CASES else [])


def _report(case, what, got, bound):
    p = _problem(case)
    err = np.abs(got - p["ref"])
    lib = np.abs(p["lib32"] - p["ref"])
    bar = 4e-6 * p["S"] + 1e-6
    print("%s %s: max |d| %.3g, worst error / bound %.3f (CPU fp32 conv2d against the product bar: %.3f); input peak %.0f, "
          "output peak %.0f" % (_case_id(case), what, err.max(), (err / bound).max(), (lib / bar).max(), p["peak"],
                                p["out_peak"]))
    assert got.shape == p["ref"].shape and np.all(np.isfinite(got))
    assert np.all(err <= bound), (what, float(err.max()), float((err / bound).max()))


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_fp32_rows_match_the_float64_convolution(case):
    """the form of a block's last convolution: fp32 rows for the side projection and the pooling"""
    p = _problem(case)
    assert p["peak"] < 1015.0 / 2  # the inputs leave room at scale 64 (and twice that at 32)
    for a_scale, out_scale in _scales(case):
        out, planes, tripped = _convolve(case, True, a_scale, out_scale)
        assert planes is None and out.dtype == torch.float32 and not tripped
        _report(case, "fp32 rows, scales (%g, %g)" % (a_scale, out_scale), _np64(out), 4e-6 * p["S"] + 1e-6)
        again, _, _ = _convolve(case, True, a_scale, out_scale)
        assert torch.equal(again, out)  # the same bits on every run


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_planes_only_match_the_float64_convolution(case):
    """the form of every other convolution: the epilogue leaves the next layer's operand planes and nothing else"""
    p = _problem(case)
    for a_scale, out_scale in _scales(case):
        out, planes, tripped = _convolve(case, False, a_scale, out_scale)
        assert out is None and not tripped
        hi, lo = planes
        assert hi.dtype == torch.float16 and lo.dtype == torch.float16 and hi.shape == p["ref"].shape == lo.shape
        got = (_np64(hi) + _np64(lo)) / out_scale
        bound = 4e-6 * p["S"] + 1e-6 + (2.0 ** -21 * np.abs(p["ref"] * out_scale) + 2.0 ** -25) / out_scale
        _report(case, "planes only, scales (%g, %g)" % (a_scale, out_scale), got, bound)
        _, again, _ = _convolve(case, False, a_scale, out_scale)
        assert torch.equal(again[0], hi) and torch.equal(again[1], lo)
