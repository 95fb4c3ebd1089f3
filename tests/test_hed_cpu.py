"""The HED annotator without a GPU: parameter names against the reference's, the helper's restatement of the detector's
post-processing against records of the unmodified reference (tests/golden/hed_golden.npz, hed_wide_golden.npz), the host-side logic of the
public interface, the C ABI, and argument checks that must raise before anything is launched."""
import os
import re
import types

import numpy as np
import pytest
import torch

import hed_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fresco_hed_input", "fresco_hed_side_pool", "fresco_hed_fuse")


@pytest.fixture(scope="module")
def hed_golden():
    return M.load_golden(os.path.join(ROOT, "tests", "golden"))


def test_both_golden_files_record_one_network():
    """the state-dict names, shapes and the weights' sha256 of the two files are the same"""
    a, b = (np.load(os.path.join(ROOT, "tests", "golden", name)) for name in M.GOLDEN_FILES)
    for k in ("param_names", "param_shapes", "weights_sha256"):
        assert np.array_equal(a[k], b[k]), k
    assert not (set(a.files) & set(b.files)) - {"param_names", "param_shapes", "weights_sha256"}


def test_state_dict_names_are_the_references(hed_golden):
    import fresco_amd
    net = fresco_amd.ControlNetHED_Apache2()
    sd = net.state_dict()
    assert list(sd.keys()) == [str(s) for s in hed_golden["param_names"]]
    assert ["x".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in hed_golden["param_shapes"]]
    assert M.param_shapes() == {k: tuple(v.shape) for k, v in sd.items()}
    net.load_state_dict(M.standin_state_dict())  # strict: nothing missing, nothing unexpected
    assert M.weights_digest() == str(hed_golden["weights_sha256"])


@pytest.mark.parametrize("case", M.CASES + M.WIDE_CASES, ids=M.case_key)
def test_inputs_are_the_ones_the_reference_saw(hed_golden, case):
    fr = M.frames(case)
    assert fr.dtype == np.uint8 and fr.shape == case + (3,)
    assert M.digest(fr) == str(hed_golden[M.case_key(case) + "_sha256"])


@pytest.mark.parametrize("case", M.CASES + M.WIDE_CASES, ids=M.case_key)
def test_fuse_restatement_reproduces_the_reference_map(hed_golden, case):
    n, H, W = case
    for f in range(M.GOLDEN_FRAMES[case]):
        p32, p64, l32, l64, u8 = M.golden_sides(hed_golden, case, f)
        assert [p.shape for p in p32] == M.level_sizes(H, W)
        mean, edge = M.fuse_u8(p32, H, W)
        assert np.array_equal(mean, l32)
        assert np.array_equal(edge, u8)
        # what the GPU tests rest on: the reference's own fp32-vs-fp64 distance is small and nonzero, the sigmoid is not
        # saturated, and the guard band is thin
        assert 0 < np.abs(l32 - l64).max() < 5e-6
        assert len(np.unique(u8)) >= 64
        assert M.guard_band(l64).mean() <= M.GUARD_CAP


def test_module_forward_is_the_reference_network_on_library_ops(hed_golden):
    """the module's own forward (what the range fallback and library_ops run) against the reference's fp32 projections"""
    import fresco_amd
    case = (1, 72, 88)
    net = fresco_amd.ControlNetHED_Apache2().eval()
    net.load_state_dict(M.standin_state_dict())
    x = torch.from_numpy(M.frames(case)[0].copy()).float().permute(2, 0, 1)[None]
    with torch.no_grad():
        out = net(x)
    p32 = M.golden_sides(hed_golden, case, 0)[0]
    for a, b in zip(out, p32):
        assert tuple(a.shape[2:]) == b.shape and np.abs(a[0, 0].numpy() - b).max() <= 1e-5


def test_frames_and_condition_host_logic():
    from fresco_amd import hed
    fr = M.frames((2, 64, 64))
    t = hed.check_frames([fr[0], fr[1]])
    assert t.dtype == torch.uint8 and tuple(t.shape) == (2, 64, 64, 3) and np.array_equal(t.numpy(), fr)
    assert tuple(hed.check_frames(fr[0]).shape) == (1, 64, 64, 3)
    assert hed.check_frames(torch.from_numpy(fr)) .data_ptr() == torch.from_numpy(fr).data_ptr()
    with pytest.raises(TypeError):
        hed.check_frames([fr[0].astype(np.float32)])
    with pytest.raises(TypeError):
        hed.check_frames(torch.zeros(1, 64, 64, 3))
    with pytest.raises(ValueError):
        hed.check_frames([fr[0], fr[1][:32]])
    with pytest.raises(ValueError):
        hed.check_frames(torch.zeros(1, 3, 64, 64, dtype=torch.uint8))
    with pytest.raises(ValueError):
        hed.check_frames(torch.zeros(1, 8, 64, 3, dtype=torch.uint8))  # level 5 would be empty
    with pytest.raises(ValueError):
        hed.check_frames([])
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        assert hed.condition_dtype(dt) is dt
    with pytest.raises(TypeError):
        hed.condition_dtype(torch.uint8)
    with pytest.raises(TypeError):
        hed.condition_dtype(torch.float64)


def test_detector_construction_and_patching(tmp_path):
    import fresco_amd
    for n in ("HEDdetector", "ControlNetHED_Apache2", "DoubleConvBlock", "patch_hed"):
        assert n in fresco_amd.__all__ and hasattr(fresco_amd, n)
    with pytest.raises(FileNotFoundError, match="ControlNetHED.pth"):
        fresco_amd.HEDdetector()
    with pytest.raises(FileNotFoundError, match="downloads nothing"):
        fresco_amd.HEDdetector(str(tmp_path / "ControlNetHED.pth"))
    net = fresco_amd.ControlNetHED_Apache2(max_frames=3)
    det = fresco_amd.HEDdetector(network=net)
    assert det.netNetwork is net and not net.training
    assert net.max_frames == 3  # max_frames=None keeps the module's own value ...
    assert fresco_amd.HEDdetector(network=net, max_frames=5).netNetwork.max_frames == 5  # ... a given one is applied
    with pytest.raises(ValueError):
        fresco_amd.HEDdetector(network=net, max_frames=0)
    with pytest.raises(fresco_amd.FrescoHipError):  # CPU frames, CPU network: no fallback
        det.detect_batch([M.frames((1, 64, 128))[0]])
    with pytest.raises(TypeError):
        det.control_image([M.frames((1, 64, 128))[0]], torch.int8)
    stand_in = types.ModuleType("annotator.hed")
    stand_in.HEDdetector = object
    assert fresco_amd.patch_hed(stand_in) is stand_in and stand_in.HEDdetector is fresco_amd.HEDdetector
    with pytest.raises(ValueError):
        fresco_amd.ControlNetHED_Apache2(split_scales=(64, 64, 48, 64, 64))  # not a power of two
    with pytest.raises(ValueError):
        fresco_amd.ControlNetHED_Apache2(split_scales=(64, 64))
    assert fresco_amd.ControlNetHED_Apache2(split_scales=(64, 32, 32, 16, 16)).split_scales == (64.0, 32.0, 32.0, 16.0, 16.0)


def test_capi_symbols():
    from fresco_amd import _lib
    header = open(os.path.join(ROOT, "include", "fresco_hip.h")).read()
    lib = _lib.load()
    for n in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
        assert n in _lib.SIGNATURES and getattr(lib, n) is not None


def test_capi_rejects_bad_arguments_on_the_host():
    """null pointers and unsupported shapes return before any launch: no GPU is touched"""
    from fresco_amd import _lib
    lib = _lib.load()
    p = 4096  # a non-null, 16-byte aligned address that is never dereferenced
    assert lib.fresco_hed_input(0, p, p, p, 1, 16, 16, 64.0, 0, 0) == -1
    assert lib.fresco_hed_input(p, p, p + 8, p, 1, 16, 16, 64.0, 0, 0) == -1       # plane not 16-byte aligned
    assert lib.fresco_hed_input(p, p, p, p, 1, 16, 16, 0.0, 0, 0) == -1
    assert lib.fresco_hed_input(p, p, p, p, 8, 32768, 32768, 64.0, 0, 0) == -2     # n H W >= 2^31
    assert lib.fresco_hed_side_pool(p, p, p, 0, 0, 0, 1, 16, 16, 64, 64.0, 0, 0) == -1   # neither output
    assert lib.fresco_hed_side_pool(p, p, p, p, p, 0, 1, 16, 16, 64, 64.0, 0, 0) == -1   # one plane of the pair
    assert lib.fresco_hed_side_pool(p, p, p, p, p, p, 1, 16, 16, 96, 64.0, 0, 0) == -2   # C outside the list
    assert lib.fresco_hed_side_pool(p, p, p, p, p, p, 1, 1, 16, 64, 64.0, 0, 0) == -2    # nothing to pool
    assert lib.fresco_hed_side_pool(p + 4, p, p, p, p, p, 1, 16, 16, 64, 64.0, 0, 0) == -1
    assert lib.fresco_hed_fuse(p, p, p, p, 0, p, 0, 0, _lib.F32, 1, 16, 16, 0) == -1
    assert lib.fresco_hed_fuse(p, p, p, p, p, p, 0, 0, _lib.F32, 1, 15, 64, 0) == -2     # level 5 would be empty
    assert lib.fresco_hed_fuse(p, p, p, p, p, p, 0, p, 7, 1, 16, 16, 0) == -1            # unknown condition dtype


def test_wrappers_raise_on_the_host():
    from fresco_amd import FrescoHipError, ops
    f32 = lambda *s: torch.zeros(*s)  # noqa: E731
    with pytest.raises(TypeError):
        ops.hed_input(torch.zeros(1, 16, 16, 3), f32(3))
    with pytest.raises(ValueError):
        ops.hed_input(torch.zeros(1, 3, 16, 16, dtype=torch.uint8), f32(3))
    with pytest.raises(FrescoHipError):  # everything else is right: stopped at the device check
        ops.hed_input(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), f32(3))
    with pytest.raises(TypeError):
        ops.hed_side_pool(torch.zeros(256, 64, dtype=torch.float16), 1, 16, 16, f32(64))
    with pytest.raises(ValueError):
        ops.hed_side_pool(f32(256, 128)[:, :64], 1, 16, 16, f32(64))  # not contiguous
    with pytest.raises(FrescoHipError):
        ops.hed_side_pool(f32(256, 64), 1, 16, 16, f32(64))
    with pytest.raises(ValueError):
        ops.hed_fuse([f32(1, 16, 16)] * 4)
    with pytest.raises(TypeError):
        ops.hed_fuse([f32(1, 16, 16).double()] + [f32(1, 16 >> k, 16 >> k) for k in range(1, 5)])
    with pytest.raises(FrescoHipError):
        ops.hed_fuse([f32(1, 16 >> k, 16 >> k) for k in range(5)])
    with pytest.raises(ValueError):
        ops._split_scale(48.0)
