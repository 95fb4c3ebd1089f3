"""tests/conv_ref.py, the float64 reference the GPU tests of vae_conv trust, against torch.nn.functional.conv2d in float64: one
small shape per form the kernel is called in.  The two differ only in summation order, so they agree to 1e-12 of the result's
largest magnitude; `mass` is compared with the same convolution on |x| and |w|.  conv_bar is checked against its formula."""
import pytest
import torch
import torch.nn.functional as F

from conv_ref import E, H11, check, conv_bar, conv_ref

REL = 1e-12


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _operands(n, Hs, Ws, cin, cout, k, seed):
    x = (_randn(n, Hs, Ws, cin, seed=seed) * 1.5).half()
    x[-1] = x[-1] * 0.5 + 1.0
    w = (_randn(cout, cin, k, k, seed=seed + 1) * (2.0 / (cin * k * k)) ** 0.5).half()
    return x, w


def _conv2d(x_nhwc, w, up2):
    """NHWC in, NHWC out, float64, zero padding k // 2 decided in the upsampled plane"""
    x = x_nhwc.double().permute(0, 3, 1, 2)
    if up2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w.double(), padding=w.shape[2] // 2).permute(0, 2, 3, 1)


FORMS = {
    # name: (n, Hs, Ws, cin, cout, ksize, up2): odd planes, several images, cout no multiple of anything
    "3x3": (2, 5, 7, 32, 12, 3, False),
    "3x3_up2": (2, 3, 5, 32, 12, 3, True),
    "1x1_per_image": (3, 4, 5, 64, 20, 1, False),
    "1x1_flat_rows": (1, 37, 1, 64, 20, 1, False),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_reference_equals_conv2d(form):
    n, Hs, Ws, cin, cout, k, up2 = FORMS[form]
    x, w = _operands(n, Hs, Ws, cin, cout, k, seed=sum(map(ord, form)))
    ref, mass = conv_ref(x, w, up2)
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    assert ref.shape == mass.shape == (n, H, W, cout) and ref.dtype == mass.dtype == torch.float64
    want, want_mass = _conv2d(x, w, up2), _conv2d(x.abs(), w.abs(), up2)
    for name, a, b in (("result", ref, want), ("mass", mass, want_mass)):
        rel = float((a - b).abs().max() / b.abs().max())
        print("conv_ref %s %s: |ref - conv2d| / max |conv2d| = %.2e" % (form, name, rel))
        assert rel <= REL, (form, name, rel)
    assert bool((mass >= ref.abs() * (1 - 1e-12)).all())      # sum |x| |w| bounds |sum x w|


def test_flat_rows_are_the_per_image_rows():
    """n = 1, H = M, W = 1 over all images' rows is the per-image 1 x 1 call on the same rows, and both are x W^T"""
    x, w = _operands(2, 7, 1, 64, 20, 1, seed=3)
    per_image, _ = conv_ref(x, w, False)
    flat, mass = conv_ref(x.reshape(1, 14, 1, 64), w, False)
    assert torch.equal(flat.reshape(2, 7, 1, 20), per_image)
    prod = x.double().reshape(14, 64) @ w.double().reshape(20, 64).t()
    assert float((flat.reshape(14, 20) - prod).abs().max() / prod.abs().max()) <= REL
    assert mass.shape == (1, 14, 1, 20)


def test_a_wrong_border_or_tap_order_is_seen():
    """the comparison above is not blind: a reference that wraps the border, or takes the taps transposed, misses 1e-12"""
    x, w = _operands(1, 5, 7, 32, 12, 3, seed=4)
    ref, _ = conv_ref(x, w, False)
    scale = float(ref.abs().max())
    wrapped = F.conv2d(F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="circular"), w.double()).permute(0, 2, 3, 1)
    transposed, _ = conv_ref(x, w.transpose(2, 3).contiguous(), False)
    assert float((wrapped - ref).abs().max()) / scale > 1e-3
    assert float((transposed - ref).abs().max()) / scale > 1e-3
    assert float((wrapped - ref)[:, 1:-1, 1:-1].abs().max()) / scale <= REL           # only the border differs


def test_bar_is_the_stated_formula():
    mass, ref = torch.tensor([[2.0, 0.0]], dtype=torch.float64), torch.tensor([[-3.0, 0.0]], dtype=torch.float64)
    bar16, bar32 = conv_bar(288, mass, ref), conv_bar(288, mass, ref, fp32=True)
    assert E == 2.0 ** -24 and H11 == 2.0 ** -11
    assert torch.equal(bar32, 288 * E * mass + 1e-6)
    assert torch.equal(bar16, 288 * E * mass + 1e-6 + H11 * ref.abs())
    assert float(bar16[0, 1]) == 1e-6                                                 # the floor where both terms vanish


def test_check_fails_on_an_excess_a_nan_and_a_shape(capsys):
    ref = torch.zeros(2, 3, dtype=torch.float64)
    bound = torch.full((2, 3), 1e-3, dtype=torch.float64)
    check("ok", ref + 5e-4, ref, bound)
    assert "ok: worst error / bound 0.500" in capsys.readouterr().out
    for bad in (ref + 2e-3, torch.full((2, 3), float("nan"), dtype=torch.float64), torch.zeros(3, 2, dtype=torch.float64)):
        with pytest.raises(AssertionError):
            check("bad", bad, ref, bound)
