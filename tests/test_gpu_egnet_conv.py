"""The convolution forms the EGNet detector adds to fresco_fn_gemm (csrc/flownet.hip), each alone against a float64
convolution: 1 x 1 convolutions as plain products, 1 x 1 / stride 2 (kh = kw = 1 on the im2col form), 3 x 3 with dilation 2
and padding 2 (ResNet layer4; new in this kernel), and the merge layers' 5 x 5 and 7 x 7 on the im2col form, up to
K = 49 * 512 = 25088.

A convolution is driven as tests/test_gpu_hed_conv.py drives its cases and as fresco_amd/egnet.py::TUN_bone._conv runs it:
weight planes from fnweights.WeightPlanes().get(param, "conv"), activation planes from ops.fn_prep, bias and ReLU in the
epilogue, fp32 rows out or operand planes only, under ops.fn_range_guard.

Inputs: activations relu(N(0, 1)) * 60 with every 7th pixel scaled by 1e-3 (their lo planes matter); weights
0.9 sqrt(2 / fan_in) N(0, 1); biases 0.1 N(0, 1).

Bounds, per output element, those of tests/test_gpu_hed_conv.py: |err| <= 4e-6 S + 1e-6 with S = conv(|x|, |w|) + |b|;
planes-only runs add the plane bound (2^-21 |ref * scale| + 2^-25) / scale.  Every case prints its worst error / bound and
the same ratio for a CPU fp32 F.conv2d of the same operands.

The 16 x 16 dilated case is a map of whole 16 x 16 patches: with dilation 1 it would take the window-in-LDS form, whose
window holds the taps of dilation 1 only -- taking it here would miss the bound by orders of magnitude.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (cin, cout, n, H, W, k, stride, pad, dilation)
CASES = [
    (2048, 512, 1, 3, 3, 1, 1, 0, 1),     # 1 x 1 as a plain product: K = 2048
    (512, 2048, 2, 5, 4, 1, 1, 0, 1),     # ... 16 column blocks
    (256, 128, 2, 9, 9, 1, 2, 0, 1),      # 1 x 1 / stride 2: 9 -> 5
    (512, 1024, 1, 6, 8, 1, 2, 0, 1),     # ... even sizes: the last row and column are never read
    (512, 512, 2, 5, 5, 3, 1, 2, 2),      # 3 x 3, dilation 2: every window on a border
    (512, 512, 1, 3, 3, 3, 1, 2, 2),      # ... only the centre tap and the corners' diagonal taps inside
    (512, 512, 1, 16, 16, 3, 1, 2, 2),    # ... whole patches: must not take the window-in-LDS form
    (128, 128, 1, 16, 16, 5, 1, 2, 1),    # 5 x 5: whole patches, im2col form (the patch form is 3 x 3 only)
    (512, 512, 1, 5, 7, 5, 1, 2, 1),
    (128, 128, 2, 8, 8, 7, 1, 3, 1),      # 7 x 7
    (512, 512, 1, 3, 3, 7, 1, 3, 1),      # ... K = 25088, 784 chunks
]


def _case_id(c):
    return "%dto%d_%dx%dx%d_k%ds%dp%dd%d" % c


@functools.lru_cache(maxsize=None)
def _problem(case):
    """operands of a case and its float64 results, computed once: dict of CPU tensors (left unchanged by the tests)"""
    cin, cout, n, H, W, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(1000 * cin + cout + 17 * n + H + W + 7 * k + dil)
    rows = torch.randn(n * H * W, cin, generator=g).clamp_min(0) * 60.0
    rows[::7] *= 1e-3
    w = (0.9 * (2.0 / (k * k * cin)) ** 0.5 * torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)).float()
    b = (0.1 * torch.randn(cout, generator=g, dtype=torch.float64)).float()
    x = rows.double().reshape(n, H, W, cin).permute(0, 3, 1, 2).contiguous()
    kw = dict(stride=stride, padding=pad, dilation=dil)
    ref = F.relu(F.conv2d(x, w.double(), b.double(), **kw))
    S = F.conv2d(x.abs(), w.double().abs(), None, **kw) + b.double().abs().view(1, -1, 1, 1)
    lib32 = F.relu(F.conv2d(x.float(), w, b, **kw)).double()
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, cout).numpy()  # noqa: E731
    return dict(rows=rows, w=w, b=b, ref=to_rows(ref), S=to_rows(S), lib32=to_rows(lib32), peak=float(x.abs().max()),
                out_peak=float(ref.max()), out_hw=tuple(ref.shape[2:]))


def _convolve(case, want_f32, a_scale=64.0, out_scale=64.0):
    from fresco_amd import ops
    from fresco_amd.fnweights import WeightPlanes
    cin, cout, n, H, W, k, stride, pad, dil = case
    p = _problem(case)
    wts = WeightPlanes()
    weight, bias = p["w"].to(DEV), p["b"].to(DEV)
    assert ops.conv_out_size(H, W, k, k, stride, pad, dil) == p["out_hw"]
    with ops.fn_range_guard(torch.device(DEV)) as guard:
        _, xs = ops.fn_prep(p["rows"].to(DEV), ld=cin, scale=a_scale)
        wp = wts.get(weight, "conv")
        assert wp[0].shape == (cout, k * k * cin)
        conv = None if (k == 1 and stride == 1) else (n, H, W, k, k, stride, pad, dil)
        out, planes = ops.fn_gemm(xs, wp, cout, wp[0].shape[1], bias=bias, act=1, conv=conv, want_f32=want_f32,
                                  want_split=not want_f32, a_scale=a_scale, out_scale=out_scale)
    return out, planes, guard.tripped() or wts.out_of_range


def _np64(t):
    return t.detach().to("cpu", torch.float64).numpy()


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
    p = _problem(case)
    assert p["peak"] < 1015.0 / 2
    out, planes, tripped = _convolve(case, True)
    assert planes is None and out.dtype == torch.float32 and not tripped
    _report(case, "fp32 rows", _np64(out), 4e-6 * p["S"] + 1e-6)
    again, _, _ = _convolve(case, True)
    assert torch.equal(again, out)  # the same bits on every run


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_planes_only_match_the_float64_convolution(case):
    p = _problem(case)
    for a_scale, out_scale in ((64.0, 64.0), (32.0, 16.0)):
        out, planes, tripped = _convolve(case, False, a_scale, out_scale)
        assert out is None and not tripped
        hi, lo = planes
        assert hi.dtype == torch.float16 and lo.dtype == torch.float16 and hi.shape == p["ref"].shape == lo.shape
        got = (_np64(hi) + _np64(lo)) / out_scale
        bound = 4e-6 * p["S"] + 1e-6 + (2.0 ** -21 * np.abs(p["ref"] * out_scale) + 2.0 ** -25) / out_scale
        _report(case, "planes only, scales (%g, %g)" % (a_scale, out_scale), got, bound)


def test_dilation_one_in_the_tuple_is_the_seven_member_form():
    """an 8th member of 1 changes nothing: the same bits as the 7-member tuple every existing caller passes"""
    from fresco_amd import ops
    from fresco_amd.fnweights import WeightPlanes
    g = torch.Generator().manual_seed(3)
    rows = (torch.randn(2 * 16 * 16, 64, generator=g).clamp_min(0) * 60.0).to(DEV)
    weight = (0.06 * torch.randn(64, 64, 3, 3, generator=g)).to(DEV)
    _, xs = ops.fn_prep(rows, ld=64)
    wp = WeightPlanes().get(weight, "conv")
    a, _ = ops.fn_gemm(xs, wp, 64, 576, act=1, conv=(2, 16, 16, 3, 3, 1, 1))
    b, _ = ops.fn_gemm(xs, wp, 64, 576, act=1, conv=(2, 16, 16, 3, 3, 1, 1, 1))
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.fn_gemm(xs, wp, 64, 576, conv=(2, 16, 16, 3, 3, 1, 1, 0))
