"""FreeU without a GPU: the numpy float64 model (tests/freeu_model.py: the closed form the kernels implement, and the
backbone scaling) against records of the unmodified reference (tests/golden/freeu_golden.npz), and the Python surface."""
import os
import re
import types

import numpy as np
import pytest
import torch

import freeu_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("Fourier_filter", "register_free_upblock2d", "register_free_crossattn_upblock2d", "apply_freeu")


@pytest.fixture(scope="module")
def freeu_golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "freeu_golden.npz")))


def _pow2(*sides):
    return all(n & (n - 1) == 0 for n in sides)


def _check(model, gold, key, scale, pow2):
    """model (float64) vs the golden's float64 record (1e-12 relative) and, where kept, its fp32 record (1e-6 max|x|).
    On a plane whose sides are not both powers of two the reference casts its input to float32 before the FFT
    (free_lunch_utils.py:33-35), whatever dtype it was given: its float64 record is then an fp32 computation and is held
    to the fp32 bound."""
    g64 = gold[key + "_f64"]
    assert model.shape == g64.shape, key
    err = np.abs(model - g64).max()
    print("%s: |model - ref64| = %.3g" % (key, err))
    assert err <= (1e-12 if pow2 else 1e-6) * scale, (key, err)
    if key + "_f32" in gold:
        err32 = np.abs(model - gold[key + "_f32"].astype(np.float64)).max()
        print("%s: |model - ref32| = %.3g (max|x| %.3g)" % (key, err32, scale))
        assert err32 <= 1e-6 * scale, (key, err32)


@pytest.mark.parametrize("shape", M.FOURIER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_closed_form_matches_the_reference_filter(freeu_golden, shape):
    x = M.fourier_input(shape)
    assert M.digest(x) == str(freeu_golden["fourier_%s_sha256" % "x".join(map(str, shape))])
    assert np.array_equal(x.astype(np.float16).astype(np.float64), x)  # exact in fp16 ...
    assert np.array_equal(torch.from_numpy(x).bfloat16().double().numpy(), x)  # ... and in bf16
    for s in M.FOURIER_SCALES:
        _check(M.fourier_model(x, s), freeu_golden, M.fourier_key(shape, s), np.abs(x).max(), _pow2(*shape[2:]))
    assert np.array_equal(M.fourier_model(x, 1.0), x)


def _fft_filter64(x, scale):
    """free_lunch_utils.py:25-52 with threshold = 1 restated on float64 tensors (the reference itself would cast a plane
    whose sides are not powers of two to float32 first); the mask holds `scale` in fp32, as the reference's does"""
    xf = torch.fft.fftshift(torch.fft.fftn(torch.from_numpy(x), dim=(-2, -1)), dim=(-2, -1))
    H, W = x.shape[2:]
    mask = torch.ones(x.shape, dtype=torch.float32)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = scale
    xf = torch.fft.ifftshift(xf * mask.double(), dim=(-2, -1))
    return torch.fft.ifftn(xf, dim=(-2, -1)).real.numpy()


@pytest.mark.parametrize("shape", M.FOURIER_TILED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_closed_form_matches_a_float64_fft_past_the_golden_shapes(shape):
    """the shapes the GPU tests hold to fourier_model alone: 1e-12 max|x|, the bar of the golden's float64 records"""
    x = M.fourier_input(shape)
    assert np.array_equal(x.astype(np.float16).astype(np.float64), x)
    assert np.array_equal(torch.from_numpy(x).bfloat16().double().numpy(), x)
    for s in M.FOURIER_SCALES + [1.0]:
        err = np.abs(M.fourier_model(x, s) - _fft_filter64(x, s)).max()
        print("%s s=%g: |model - fft64| = %.3g" % (shape, s, err))
        assert err <= 1e-12 * np.abs(x).max(), (shape, s, err)


@pytest.mark.parametrize("size", M.BLOCK_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", list(M.BLOCK_CONFIGS))
def test_model_blocks_match_the_reference_forwards(freeu_golden, name, size):
    C, outs, _ = M.BLOCK_CONFIGS[name]
    hidden, skips = M.block_inputs(name, size)
    m = M.model_block(name, size)
    p2 = _pow2(*size[1:])
    for kind in M.BLOCK_KINDS:
        key = M.block_key(kind, name, size)
        assert M.digest(hidden, *skips) == str(freeu_golden[key + "_sha256"])
        stage = C
        for k, t in enumerate(m["resnet_in"]):
            kept = M.kept_of(name, stage, t.shape[1])
            _check(t[:, kept], freeu_golden, "%s_in%d" % (key, k), np.abs(t).max(), p2)
            stage = outs[k]
        _check(m["out"][:, M.kept_of(name, stage, stage)], freeu_golden, key + "_out", np.abs(m["out"]).max(), p2)
        _check(m["hidden_after"][:, M.kept_of(name, C, C)], freeu_golden, key + "_hidden", np.abs(hidden).max(), True)
    # the reference changed the incoming tensor exactly where FreeU acts
    changed = bool(np.any(m["hidden_after"] != hidden))
    assert changed == (C in (1280, 640))


def test_backbone_inputs_bound_the_cancellation():
    for case in M.BACKBONE_CASES + M.BACKBONE_TILED_CASES:
        x = M.backbone_input(case)
        assert M.mean_map_condition(x), case
        m = x.mean(axis=1)
        assert len({round(float(v), 3) for v in m.mean(axis=(1, 2))}) == case[0]  # every sample its own mean


def test_package_exports_the_reference_names():
    import fresco_amd
    for n in NAMES + ("patch_free_lunch",):
        assert callable(getattr(fresco_amd, n)), n
        assert n in fresco_amd.__all__


def test_threshold_other_than_one_is_not_implemented():
    import fresco_amd
    with pytest.raises(NotImplementedError):
        fresco_amd.Fourier_filter(torch.zeros(1, 1, 4, 4), 2, 0.5)


def test_cpu_tensors_raise():
    import fresco_amd
    from fresco_amd import ops
    with pytest.raises(fresco_amd.FrescoHipError):
        fresco_amd.Fourier_filter(torch.zeros(1, 1, 4, 4), 1, 0.5)
    with pytest.raises(fresco_amd.FrescoHipError):
        ops.freeu_backbone(torch.zeros(1, 4, 4, 4), 2, 1.2)
    blk = M.make_block("UpBlock2D", "c640")
    fresco_amd.apply_freeu(M.StandInPipe([blk]), 1.2, 1.5, 0.9, 0.2)
    hidden, skips = M.block_inputs("c640", (1, 6, 10))
    with pytest.raises(fresco_amd.FrescoHipError):
        blk.forward(torch.from_numpy(hidden).half(), tuple(torch.from_numpy(s).half() for s in skips))


def test_training_checkpoint_branch_is_not_implemented():
    import fresco_amd
    blk = M.make_block("CrossAttnUpBlock2D", "c320")
    fresco_amd.register_free_crossattn_upblock2d(M.StandInPipe([blk]))
    blk.training = blk.gradient_checkpointing = True
    hidden, skips = M.block_inputs("c320", (1, 6, 10))
    with pytest.raises(NotImplementedError):
        blk.forward(torch.from_numpy(hidden), tuple(torch.from_numpy(s) for s in skips))


def test_plain_concat_blocks_run_anywhere():
    """320 hidden channels: no FreeU, so the registered forward is torch.cat + the block's own modules -- also on the CPU"""
    import fresco_amd
    for kind, reg in (("UpBlock2D", fresco_amd.register_free_upblock2d),
                      ("CrossAttnUpBlock2D", fresco_amd.register_free_crossattn_upblock2d)):
        r = M.run_block(reg, kind, "c320", (2, 4, 4), torch.float64)
        m = M.model_block("c320", (2, 4, 4))
        for a, b in zip(r["resnet_in"], m["resnet_in"]):
            assert np.array_equal(a.numpy(), b)
        assert np.array_equal(r["out"].numpy(), m["out"])
        blk = r["block"]
        assert (blk.b1, blk.b2, blk.s1, blk.s2) == (1.2, 1.5, 0.9, 0.2)


def test_patch_free_lunch_rebinds_all_four_names():
    import fresco_amd
    flu = types.ModuleType("free_lunch_utils")
    for n in NAMES:
        setattr(flu, n, object())
    flu.isinstance_str = sentinel = object()
    assert fresco_amd.patch_free_lunch(flu) is flu
    for n in NAMES:
        assert getattr(flu, n) is getattr(fresco_amd, n), n
    assert flu.isinstance_str is sentinel


def test_apply_freeu_touches_both_block_kinds_only():
    import fresco_amd

    class Other:
        pass

    blocks = [M.make_block("UpBlock2D", "c320"), M.make_block("CrossAttnUpBlock2D", "c320"), Other()]
    fresco_amd.apply_freeu(M.StandInPipe(blocks), 1.1, 1.2, 0.8, 0.3)
    for blk in blocks[:2]:
        assert (blk.b1, blk.b2, blk.s1, blk.s2) == (1.1, 1.2, 0.8, 0.3)
        assert "forward" in vars(blk)
    assert not hasattr(blocks[2], "b1") and not hasattr(blocks[2], "forward")


def test_entry_points_declared_bound_and_exported():
    from fresco_amd import _lib
    header = open(os.path.join(ROOT, "include", "fresco_hip.h")).read()
    lib = _lib.load()
    for n in ("fresco_freeu_workspace_bytes", "fresco_freeu_fourier", "fresco_freeu_backbone"):
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.SIGNATURES
        assert hasattr(lib, n)


def test_host_side_argument_checks():
    """every refusal answers before any HIP call, so they can be exercised without a GPU"""
    import ctypes
    from fresco_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p = (p + 255) // 256 * 256
    assert lib.fresco_freeu_workspace_bytes(16, 1280, 8, 8) > 0
    assert lib.fresco_freeu_workspace_bytes(1, 4, 1, 8) == 0
    assert lib.fresco_freeu_fourier(p, p + 1024, 16, 1, 1, 1, 16, 0.5, _lib.F16, None) == -2  # H < 2
    assert lib.fresco_freeu_fourier(p, p + 1024, 8, 1, 1, 4, 4, 0.5, _lib.F16, None) == -1  # batch stride < C H W
    assert lib.fresco_freeu_fourier(p + 1, p + 1024, 16, 1, 1, 4, 4, 0.5, _lib.F16, None) == -1  # misaligned
    assert lib.fresco_freeu_fourier(p, p + 1024, 16, 1, 1, 4, 4, 0.5, 7, None) == -1  # dtype
    assert lib.fresco_freeu_fourier(None, p, 16, 1, 1, 4, 4, 0.5, _lib.F16, None) == -1
    need = lib.fresco_freeu_workspace_bytes(1, 4, 4, 4)
    assert lib.fresco_freeu_backbone(p, None, 0, 1, 4, 5, 4, 4, 1.2, p + 2048, need, _lib.F16, None) == -1  # n_scaled > C
    assert lib.fresco_freeu_backbone(p, None, 0, 1, 4, 2, 4, 1, 1.2, p + 2048, need, _lib.F16, None) == -2  # W < 2
    assert lib.fresco_freeu_backbone(p, None, 0, 1, 4, 2, 4, 4, 1.2, p + 2048, need - 1, _lib.F16, None) == -3
    assert lib.fresco_freeu_backbone(p + 2, None, 0, 1, 4, 2, 4, 4, 1.2, p + 2048, need, _lib.F32, None) == -1  # misaligned
    assert lib.fresco_freeu_backbone(p, p, 64, 1, 4, 2, 4, 4, 1.2, p + 2048, need, _lib.F16, None) == -1  # cat == hidden
