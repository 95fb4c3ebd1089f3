"""The float64 reference of vae_conv and its bar, shared by the tests that compare the kernel element by element
(test_gpu_vae.py, test_gpu_conv_unet_forms.py).  tests/test_conv_ref_cpu.py checks the reference itself against
torch.nn.functional.conv2d.

The bar (e = 2^-24, one fp32 rounding): the fp16 operands are exact, so
    |got - ref| <= K e sum |x| |w| + 2^-11 |ref| + 1e-6        (fp32 output: without the 2^-11 term),
the worst case of K fp32 additions plus one output rounding.
"""
import numpy as np
import torch
import torch.nn.functional as F

E = 2.0 ** -24
H11 = 2.0 ** -11


def conv_ref(x, w, up2):
    """x (n, Hs, Ws, cin) fp16, w (cout, cin, k, k) fp16 -> (float64 result, sum |x| |w|), both (n, H, W, cout):
    im2col (F.unfold) and one float64 product"""
    x64 = x.double().permute(0, 3, 1, 2)
    if up2:
        x64 = x64.repeat_interleave(2, 2).repeat_interleave(2, 3)
    n, _, H, W = x64.shape
    k = w.shape[2]
    w64 = w.double().reshape(w.shape[0], -1)
    outs = []
    for xx, ww in ((x64, w64), (x64.abs(), w64.abs())):
        cols = F.unfold(xx, k, padding=k // 2) if k == 3 else xx.reshape(n, -1, H * W)
        outs.append((ww @ cols).transpose(1, 2).reshape(n, H, W, -1))
    return outs


def conv_bar(K, mass, ref, fp32=False):
    """K e sum |x| |w| + 2^-11 |ref| + 1e-6; fp32 output: without the 2^-11 term.  `ref` is the whole float64 result, bias
    and residual included: the one output rounding is relative to it"""
    bar = K * E * mass + 1e-6
    return bar if fp32 else bar + H11 * ref.abs()


def check(name, got, ref, bound):
    got, ref, bound = (t.detach().to("cpu", torch.float64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
                       for t in (got, ref, bound))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    print("%s: worst error / bound %.3f" % (name, float((err / bound).max())))
    assert np.isfinite(got).all() and np.all(err <= bound), name
