"""GPU parity of the tap-resize kernels (csrc/resize.hip) with the numpy restatement of OpenCV's rules
(tests/resize_model.py), bit for bit: INTER_LANCZOS4 on exact and fractional factors, frames smaller than the tap window, a
slightly shrinking side, the factor-2 limit and the accumulator's extremes; INTER_AREA's enlarging rule with a copied, a
shrinking and a growing side; a source off alignment; then resize_frames / resize_image / get_keyframe_ind end to end on
geometries of every branch, the last against the golden recorded from the unmodified reference
(tests/golden/make_keyframe_small_golden.py).  The kernel launches one workgroup per tile and does not cap its grid, so there
is no grid-stride case.  tests/test_resize_cpu.py shows that these inputs tell the rule variants apart."""
import os

import numpy as np
import pytest
import torch

import keyframe_model as KM
import resize_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "keyframe_small_golden.npz")))


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), int(np.abs(got.astype(int) - want).max()))


# ---- the kernels
@pytest.mark.parametrize("name", sorted(R.TAPS_CASES))
def test_resize_equals_the_model(name):
    from fresco_amd import ops
    method, n, H0, W0, H, W, _ = R.TAPS_CASES[name]
    src = R.taps_input(name)
    want = R.resize_taps(src, H, W, method)
    got = ops.resize_taps_u8(torch.from_numpy(src).to(DEV), H, W, method)
    assert got.shape == (n, H, W, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    _same(got.cpu().numpy(), want, name)
    if name == "lanczos_fractional":  # values clamped at both ends were among them
        v = (R.lanczos_raw(src, H, W) + (1 << 21)) >> 22
        assert (v < 0).any() and (v > 255).any() and (want == 0).any() and (want == 255).any()


@pytest.mark.parametrize("name", ["lanczos_odd_rows", "linear_odd_rows"])
def test_resize_reads_a_source_off_alignment(name):
    """a batch that starts at an odd byte of its buffer gives the same bits"""
    from fresco_amd import ops
    method, n, H0, W0, H, W, _ = R.TAPS_CASES[name]
    src = R.taps_input(name)
    buf = torch.zeros(src.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(src).to(DEV).reshape(-1)
    view = buf[1:].view(n, H0, W0, 3)
    assert view.data_ptr() % 4 == 1
    _same(ops.resize_taps_u8(view, H, W, method).cpu().numpy(), R.resize_taps(src, H, W, method), name)


def test_lanczos_accumulator_extremes():
    """255 under the positive coefficient products of the pixel with the largest positive mass, and under the negative ones
    of the pixel with the largest negative mass: the 32-bit sums nearest to overflow that this geometry can produce"""
    from fresco_amd import ops
    frame, (ya, xa, top), (yb, xb, bottom) = R.adversarial(45, 80, 64, 128)
    assert top + (1 << 21) < 2 ** 31 and top > 2 ** 30 and bottom < 0
    want = R.resize_lanczos4(frame, 64, 128)
    got = ops.resize_taps_u8(torch.from_numpy(frame).to(DEV), 64, 128, ops.RESIZE_LANCZOS4).cpu().numpy()
    _same(got, want, "adversarial")
    assert got[0, ya, xa, 0] == 255 and got[0, yb, xb, 0] == 0


def test_a_side_that_shrinks_by_more_than_two_is_refused():
    from fresco_amd import FrescoHipError, ops
    method, n, H0, W0, H, W = R.REFUSED_CASE
    x = torch.zeros(n, H0, W0, 3, dtype=torch.uint8, device=DEV)
    for m in (ops.RESIZE_LANCZOS4, ops.RESIZE_LINEAR_AREA):
        with pytest.raises(FrescoHipError, match="EUNSUPPORTED"):
            ops.resize_taps_u8(x, H, W, m)
    assert ops.resize_taps_u8(x[:, :128], H, W, method).shape == (n, H, W, 3)  # exactly 2 is taken


def test_two_runs_agree_bit_for_bit():
    from fresco_amd import ops
    for name in ("lanczos_three_frames", "linear_copy_axis"):
        method, n, H0, W0, H, W, _ = R.TAPS_CASES[name]
        src = torch.from_numpy(R.taps_input(name)).to(DEV)
        assert torch.equal(ops.resize_taps_u8(src, H, W, method), ops.resize_taps_u8(src, H, W, method))


def test_the_table_cache_keeps_methods_and_geometries_apart():
    from fresco_amd import ops
    src = R.taps_input("linear_odd_rows")
    x = torch.from_numpy(src).to(DEV)
    for _ in range(2):
        for method in (ops.RESIZE_LINEAR_AREA, ops.RESIZE_LANCZOS4):
            for H, W in ((64, 128), (48, 80)):
                _same(ops.resize_taps_u8(x, H, W, method).cpu().numpy(), R.resize_taps(src, H, W, method), (method, H, W))
    assert len(ops._TAP_TABLES) <= ops._TAP_TABLES_MAX


# ---- the Python surface
@pytest.mark.parametrize("how", sorted(R.SMALL_DISPATCH))
def test_resize_frames_and_resize_image_take_every_branch(how):
    import fresco_amd
    (n, H0, W0), (H, W) = R.SMALL_DISPATCH[how]
    src = KM.textured(n, H0, W0, 60 + sorted(R.SMALL_DISPATCH).index(how))
    want = R.resize_reference(src, 64)
    assert want.shape == (n, H, W, 3)
    x = torch.from_numpy(src).to(DEV)
    got = fresco_amd.resize_frames(x, 64, enlarge=True)
    assert got.is_cuda
    _same(got.cpu().numpy(), want, how)
    one = fresco_amd.resize_image(src[-1], 64)
    assert isinstance(one, np.ndarray)
    _same(one, want[-1], how)
    if how == "area":
        _same(fresco_amd.resize_frames(x, 64).cpu().numpy(), want, how)
    else:  # without the keyword the same input still raises
        with pytest.raises(NotImplementedError, match="LANCZOS" if how.startswith("lanczos") else "enlarges a side"):
            fresco_amd.resize_frames(x, 64)


@pytest.mark.parametrize("name", sorted(R.SMALL_GOLDEN_CASES))
def test_get_keyframe_ind_returns_the_golden_keys(name, golden):
    import fresco_amd
    seed, n, H0, W0, mininterv, maxinterv = golden[name + "_args"].tolist()
    assert (seed, n, H0, W0, mininterv, maxinterv) == R.SMALL_GOLDEN_CASES[name]
    frames = KM.synthetic_frames(seed, n, H0, W0)
    keys, resized = fresco_amd.get_keyframe_ind(frames, mininterv=mininterv, maxinterv=maxinterv, return_frames=True)
    assert list(keys) == golden[name + "_keys"].tolist(), name
    assert keys == fresco_amd.get_keyframe_ind(iter(frames), mininterv=mininterv, maxinterv=maxinterv)
    H, W = golden[name + "_size"].tolist()
    assert resized.is_cuda and resized.shape == (n, H, W, 3) and resized.dtype == torch.uint8
    _same(resized[:2].cpu().numpy(), R.resize_reference(frames[:2], 512), name)
    curve = fresco_amd.frame_errors(fresco_amd.keyframe._frame_chunks(frames, n), 512)  # against the reference's fp32 mse_loss
    ref = golden[name + "_err"]
    assert curve.shape == ref.shape and curve[0] == 0
    assert np.all(np.abs(curve[1:] - ref[1:]) <= 1e-4 * ref[1:])
