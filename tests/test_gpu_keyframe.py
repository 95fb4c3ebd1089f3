"""GPU parity of the key-frame kernels (csrc/keyframe.hip) with the numpy restatement of OpenCV's rules
(tests/keyframe_model.py), bit for bit: the area resize on integer, fractional and unit factors, the blurred squared
differences on frames from 5 x 5 up to several ragged tiles, with a carried frame and past 2^32, and get_keyframe_ind end to
end on the synthetic frames of the golden recorded from the unmodified reference (tests/golden/make_keyframe_golden.py).
tests/test_keyframe_cpu.py shows that these inputs tell the rule variants apart."""
import os

import numpy as np
import pytest
import torch

import keyframe_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "keyframe_golden.npz")))


@pytest.fixture(scope="module")
def golden_frames(golden):
    return M.synthetic_frames(int(golden["seed"]), int(golden["frames"]))


@pytest.fixture(scope="module")
def error_inputs():
    return M.error_inputs()


def _sums(frames, carry=None):
    from fresco_amd import ops
    out = ops.frame_sq_diffs(torch.from_numpy(frames).to(DEV), None if carry is None else torch.from_numpy(carry).to(DEV))
    assert out.dtype == torch.int64 and out.shape == (len(frames),)
    return out.cpu().tolist()


# ---- resize
@pytest.mark.parametrize("name", sorted(M.RESIZE_CASES))
def test_resize_equals_the_model(name):
    from fresco_amd import ops
    n, H0, W0, H, W, _ = M.RESIZE_CASES[name]
    src = M.resize_input(name)
    want = M.resize_area(src, H, W)
    got = ops.resize_area_u8(torch.from_numpy(src).to(DEV), H, W)
    assert got.shape == (n, H, W, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (name, int((got != want).sum()), int(np.abs(got.astype(int) - want).max()))


def test_resize_reads_an_unaligned_source_bytewise():
    """a batch that starts at an odd byte of its buffer: no 32-bit reads, the same bits"""
    from fresco_amd import ops
    n, H0, W0, H, W, _ = M.RESIZE_CASES["odd_rows"]
    src = M.resize_input("odd_rows")
    buf = torch.zeros(src.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(src).to(DEV).reshape(-1)
    view = buf[1:].view(n, H0, W0, 3)
    assert view.data_ptr() % 4 == 1
    for (h, w) in ((H, W), (15, 11)):  # the tables, and the 3 x 7 box
        assert np.array_equal(ops.resize_area_u8(view, h, w).cpu().numpy(), M.resize_area(src, h, w))


def test_resize_refusals():
    import fresco_amd
    from fresco_amd import FrescoHipError, ops
    x = torch.zeros(1, 64, 80, 3, dtype=torch.uint8, device=DEV)
    for H, W in ((65, 80), (64, 81), (128, 160)):
        with pytest.raises(FrescoHipError, match="EUNSUPPORTED"):
            ops.resize_area_u8(x, H, W)
    with pytest.raises(NotImplementedError, match="LANCZOS"):
        fresco_amd.resize_frames(torch.zeros(1, 270, 480, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError, match="enlarges a side"):
        fresco_amd.resize_frames(torch.zeros(1, 600, 500, 3, dtype=torch.uint8, device=DEV), 500)


def test_resize_frames_and_resize_image_follow_resize_size():
    import fresco_amd
    src = M.textured(2, 150, 200, 31)
    H, W, k = M.resize_size(150, 200, 128)
    assert (H, W) == (128, 192) and k < 1
    want = M.resize_area(src, H, W)
    got = fresco_amd.resize_frames(torch.from_numpy(src).to(DEV), 128)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    one = fresco_amd.resize_image(src[1], 128)
    assert isinstance(one, np.ndarray) and one.dtype == np.uint8 and np.array_equal(one, want[1])


# ---- errors
@pytest.mark.parametrize("name", ["5x5", "ragged", "identical", "saturated", "single", "narrow", "five"])
def test_sums_equal_the_model(name, error_inputs):
    frames = error_inputs[name]
    want = M.sq_diffs(frames)
    got = _sums(frames)
    assert got == want, (name, got, want)
    if name == "identical":
        assert got == [0, 0]
    if name == "saturated":
        assert got[1] == 160 * 144 * 3 * 255 * 255 > 2 ** 32
    if name == "single":
        assert got == [0]
    if name in ("5x5", "ragged"):
        assert len(got) >= 2 and got[1] > 0


def test_chunks_carry_the_last_frame(error_inputs):
    import fresco_amd
    five = error_inputs["five"]
    whole = _sums(five)
    parts = _sums(five[:2]) + _sums(five[2:4], carry=five[1]) + _sums(five[4:], carry=five[3])
    assert parts == whole == M.sq_diffs(five)
    H, W = five.shape[1:3]
    curve = fresco_amd.frame_errors(five)
    assert curve.shape == (5,) and np.array_equal(curve, M.error_curve(whole, H, W))
    for chunks in ([five[:2], five[2:4], five[4:]], [torch.from_numpy(five[:3]).to(DEV), five[3:]], [five[i] for i in range(5)]):
        assert np.array_equal(fresco_amd.frame_errors(chunks), curve)


def test_two_runs_agree_bit_for_bit(error_inputs):
    from fresco_amd import ops
    frames = torch.from_numpy(error_inputs["ragged"]).to(DEV)
    carry = torch.from_numpy(error_inputs["identical"][0]).to(DEV)
    a, b = ops.frame_sq_diffs(frames, carry), ops.frame_sq_diffs(frames, carry)
    assert torch.equal(a, b) and a[0] == 0  # (the carry is the first frame)
    src = torch.from_numpy(M.resize_input("three_frames")).to(DEV)
    assert torch.equal(ops.resize_area_u8(src, 64, 128), ops.resize_area_u8(src, 64, 128))


def test_error_refusals():
    from fresco_amd import FrescoHipError, ops
    for shape in ((2, 4, 9, 3), (2, 9, 4, 3)):
        with pytest.raises(FrescoHipError, match="sides >= 5"):
            ops.frame_sq_diffs(torch.zeros(shape, dtype=torch.uint8, device=DEV))


# ---- end to end
@pytest.mark.parametrize("name", sorted(M.GOLDEN_CASES))
def test_get_keyframe_ind_returns_the_golden_keys(name, golden, golden_frames):
    import fresco_amd
    served, reported, lastframen, mininterv, maxinterv = golden[name + "_args"].tolist()
    source = golden_frames[:min(served, reported)]
    keys = fresco_amd.get_keyframe_ind(iter(source), lastframen, mininterv, maxinterv)
    assert list(keys) == golden[name + "_keys"].tolist(), name
    if mininterv != maxinterv:  # the curve itself, against the reference's fp32 mse_loss
        curve = fresco_amd.frame_errors(fresco_amd.keyframe._frame_chunks(source, max(1, lastframen)), 512)
        ref = golden[name + "_err"]
        assert curve.shape == ref.shape and curve[0] == 0
        assert np.all(np.abs(curve[1:] - ref[1:]) <= 1e-4 * ref[1:])


def test_get_keyframe_ind_hands_back_the_resized_frames(golden, golden_frames):
    import fresco_amd
    frames = golden_frames[:34]  # two chunks
    keys, resized = fresco_amd.get_keyframe_ind(frames, mininterv=5, maxinterv=20, return_frames=True)
    assert keys == fresco_amd.get_keyframe_ind(torch.from_numpy(frames).to(DEV), mininterv=5, maxinterv=20)
    assert resized.is_cuda and resized.shape == (34, 512, 576, 3) and resized.dtype == torch.uint8
    for i in (0, 31, 32, 33):
        assert np.array_equal(resized[i].cpu().numpy(), M.resize_area(frames[i], 512, 576)), i
    keys, resized = fresco_amd.get_keyframe_ind(frames, 34, 5, 5, return_frames=True)
    assert keys == list(range(0, 34, 5)) and resized.shape == (34, 512, 576, 3)


def test_forty_frames_take_two_chunks_and_one_download(golden, golden_frames, monkeypatch):
    """no host loop over frames beyond the chunking: 40 frames are two uploads, two resize calls, two error calls and one
    device-to-host copy"""
    import fresco_amd
    from fresco_amd import keyframe, ops
    calls = dict(resize=[], errors=[], cpu=0, cuda=[])
    real_resize, real_errors, real_cpu, real_cuda = ops.resize_area_u8, ops.frame_sq_diffs, torch.Tensor.cpu, torch.Tensor.cuda

    def resize(frames, H, W):
        calls["resize"].append(len(frames))
        return real_resize(frames, H, W)

    def errors(frames, carry=None):
        calls["errors"].append((len(frames), carry is not None))
        return real_errors(frames, carry)

    def cpu(self, *a, **k):
        calls["cpu"] += 1
        return real_cpu(self, *a, **k)

    def cuda(self, *a, **k):
        calls["cuda"].append(len(self))
        return real_cuda(self, *a, **k)

    monkeypatch.setattr(keyframe.ops, "resize_area_u8", resize)
    monkeypatch.setattr(keyframe.ops, "frame_sq_diffs", errors)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    monkeypatch.setattr(torch.Tensor, "cuda", cuda)
    keys = fresco_amd.get_keyframe_ind(iter(golden_frames), mininterv=5, maxinterv=20)
    assert keys == golden["ordinary_keys"].tolist()
    assert calls == dict(resize=[32, 8], errors=[(32, False), (8, True)], cpu=1, cuda=[32, 8])
