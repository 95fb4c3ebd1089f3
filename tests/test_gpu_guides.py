"""Guide kernels (fresco_edge_guide, fresco_warp_nearest) against restatements: the edge guide against numpy
cv2.filter2D semantics (reflect-101, saturation), the nearest warp against torch-CPU grid_sample(nearest, zeros,
align_corners=True) at pixel + flow with flow_utils' fp32 normalise step.  The blend kernel's mask warp shares the
warp's code; tests/test_gpu_blend.py pins its outputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fresco_amd import FrescoHipError
from fresco_amd import ebsynth as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LAPLACE = np.array([[0, -1, 0], [-1, 4, -1], [0, -1, 0]], np.int64)


def edge_model(img):
    """cv2.filter2D(img, -1, LAPLACE): correlation, BORDER_REFLECT_101, saturate_cast to uint8 (exact integers)"""
    h, w = img.shape[:2]
    ys = np.concatenate([[1], np.arange(h), [h - 2]]) if h > 1 else np.zeros(h + 2, np.int64)
    xs = np.concatenate([[1], np.arange(w), [w - 2]]) if w > 1 else np.zeros(w + 2, np.int64)
    pad = img.astype(np.int64)[ys][:, xs]
    acc = np.zeros(img.shape, np.int64)
    for dy in range(3):
        for dx in range(3):
            acc += LAPLACE[dy, dx] * pad[dy:dy + h, dx:dx + w]
    return np.clip(acc, 0, 255).astype(np.uint8)


def warp_model(img, flow):
    """flow_calc.warp(img, flow, 'nearest') on torch CPU: img uint8 (h, w, c), flow float32 (2, h, w)"""
    h, w = img.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    f = torch.from_numpy(flow)
    cx, cy = xs.float() + f[0], ys.float() + f[1]
    grid = torch.stack([2 * cx / (w - 1) - 1, 2 * cy / (h - 1) - 1], -1)[None]
    x = torch.from_numpy(img).permute(2, 0, 1)[None].float()
    out = F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=True)
    return out[0].permute(1, 2, 0).to(torch.uint8).numpy()


@pytest.mark.parametrize("hwc", [(2, 2, 3), (3, 3, 1), (2, 7, 3), (7, 2, 1), (17, 31, 3), (33, 20, 4), (64, 48, 3)])
def test_edge_guide_equals_filter2d(hwc):
    rng = np.random.default_rng(sum(hwc))
    n = 3
    imgs = rng.integers(0, 256, (n,) + hwc).astype(np.uint8)
    imgs[0, ::2, ::2] = 255  # saturates high
    imgs[0, 1::2, 1::2] = 0
    imgs[1] = 0
    imgs[1, hwc[0] // 2] = 255  # one bright row: +1020 on it, -255 next to it: both ends saturate
    got = E.edge_guide(torch.from_numpy(imgs).to(DEV)).cpu().numpy()
    for b in range(n):
        np.testing.assert_array_equal(got[b], edge_model(imgs[b]))
    one = E.edge_guide(torch.from_numpy(imgs[2]).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(one, edge_model(imgs[2]))
    assert (got[0] == 255).any() and (got[0] == 0).any()


def tie_flow(rng, h, w):
    """flows that hit exact half-pixel ties, integer shifts, out-of-range and large values"""
    f = rng.integers(-8, 9, (2, h, w)).astype(np.float32) * np.float32(0.5)
    f[:, : h // 4] += np.float32(0.25) * rng.integers(-3, 4, (2, h // 4, w)).astype(np.float32)
    f[0, -1] = 1e4
    f[1, :, -1] = -3e3
    f[:, h // 2, : w // 2] = np.float32(w + 0.5)
    return f


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", [(2, 2), (9, 13), (40, 33), (64, 64)])
def test_warp_nearest_equals_grid_sample(c, hw):
    h, w = hw
    rng = np.random.default_rng(h * 100 + w + c)
    n = 3
    imgs = rng.integers(0, 256, (n, h, w, c)).astype(np.uint8)
    flows = np.stack([tie_flow(rng, h, w) for _ in range(n)])
    got = E.warp_nearest(torch.from_numpy(imgs).to(DEV), torch.from_numpy(flows).to(DEV)).cpu().numpy()
    for b in range(n):
        np.testing.assert_array_equal(got[b], warp_model(imgs[b], flows[b]))
    one = E.warp_nearest(torch.from_numpy(imgs[1]).to(DEV), torch.from_numpy(flows[1][None]).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(one, warp_model(imgs[1], flows[1]))


def test_refused_shapes():
    x = torch.zeros((1, 1, 5, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(FrescoHipError):
        E.edge_guide(x)
    with pytest.raises(FrescoHipError):
        E.edge_guide(torch.zeros((4, 4, 17), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        E.warp_nearest(torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV),
                       torch.zeros((2, 4, 5), dtype=torch.float32, device=DEV))
