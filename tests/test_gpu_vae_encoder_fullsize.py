"""The VAE encoder at the sizes a batch of 512 x 512 frames takes: what csrc/vae_enc.hip's streaming kernels and
fresco_amd/vae.py's encoder do past the small maps of tests/test_gpu_vae_encoder.py (the kernels both halves share --
GroupNorm, the attention's three arrangements -- are in tests/test_gpu_vae_fullsize.py, whose layout this file follows).
Every bar is one of tests/test_gpu_vae_encoder.py's, unchanged, and every comparison prints its worst error / bar.

  A  the streaming kernels past one pass of their grid-stride loop (2048 blocks of 256 threads: work item 524 288 and later
     run in a later pass): smallest convenient shapes with a ragged second pass, random data per image, the last image
     scaled and shifted, every element compared, a second run bit-equal.
       vaeenc_input    images (3, 3, 420, 417): exact bits and zero pad channels, as test_input_is_exact has it
       vaeenc_moments  (2, 513, 512): test_moments_match_float64's bar
       vaeenc_sample   parameters (3, 8, 210, 209) at both scales: test_sample_matches_float64_on_both_sides_of_the_clamp's bar
                       and its six hand-made elements on both sides of both clamp ends, once in the first pass and once in
                       the second
  C  the encoder end to end on vae_encoder_model.FULLSIZE_CASES against tests/golden/vae_encoder_fullsize_golden.npz
     (tests/golden/make_vae_encoder_fullsize_golden.py; test_gpu_vae_encoder.py's rule, 4 x recorded noise x peak): images
     (2, 192, 192) -- GroupNorm past one pass at C = 128 (192^2), attention at L = 576 with two images -- and the real
     (1, 512, 512): eight passes at C = 128, 4096 tokens.  A second call gives the same bits, and each frame encoded alone
     gives exactly the parameters it has inside the batch.

Measured on an MI355X, worst error / bar: see MEASURED below; DESIGN.md section 18 has the table.  What the single-pass
scratch build gave here: MUTANT of tests/test_gpu_vae_fullsize.py.
"""
import numpy as np
import pytest
import torch

import test_gpu_vae_encoder as VE
import vae_encoder_model as EM
from test_gpu_vae_encoder import E, H11, _check, encoder, vae16  # noqa: F401  (the last two: fixtures, built once for this module)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE_PASS = 2048 * 256  # work items of one pass of a streaming kernel's grid-stride loop (STREAM_MAX_BLOCKS blocks of 256)

MEASURED = """
A  vaeenc_input exact at cpad 32 and 8, vaeenc_moments 0.997, vaeenc_sample 0.997 (scale 1) and 0.988 (scale 0.18215)
C  vaeenc_2x192x192: taps 0.098 - 0.168, parameters 0.201 (PyTorch's fp16 module 0.169 - 0.473);  vaeenc_1x512x512: taps
   0.087 - 0.147, parameters 0.197 (0.124 - 0.300);  frames alone: bit-equal, every tap too
The file's 7 tests took 4.2 s: 2.1 s the 512 x 512 case with PyTorch's module beside it (5.1 s in a second run), 1.3 s the module fixtures, 0.5 s
the 192 x 192 case, the kernel tests 0.04 s and less each.
"""


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------
# A. streaming kernels past one grid pass
# ---------------------------------------------------------------------------------------------------------------
def test_input_past_one_grid_pass():
    from fresco_amd import ops
    n, H, W = 3, 420, 417
    assert ONE_PASS < n * H * W < 2 * ONE_PASS  # 525 420 pixels
    img = _randn(n, 3, H, W, seed=H)
    img[-1] = img[-1] * 0.5 + 1.0
    img = img.half().to(DEV)
    for cpad in (32, 8):
        out = ops.vaeenc_input(img, cpad=cpad)
        assert out.shape == (n, H, W, cpad) and out.dtype == torch.float16
        assert torch.equal(out[..., :3], img.permute(0, 2, 3, 1)) and not out[..., 3:].any(), cpad
        assert torch.equal(out, ops.vaeenc_input(img, cpad=cpad))


def test_moments_past_one_grid_pass():
    from fresco_amd import ops
    n, hh, ww = 2, 513, 512
    assert ONE_PASS < n * hh * ww < 2 * ONE_PASS  # 525 312 latent pixels
    h = (_randn(n, hh, ww, 8, seed=hh) * 3.0).to(DEV)
    h[-1] = h[-1] * 0.25 + 2.0
    wq, bq = (torch.eye(8) + 0.2 * _randn(8, 8, seed=1)).to(DEV), (0.1 * _randn(8, seed=2)).to(DEV)
    got = ops.vaeenc_moments(h, wq, bq)
    assert got.shape == (n, 8, hh, ww) and got.dtype == torch.float16
    ref = torch.einsum("oc,nhwc->nohw", wq.double(), h.double()) + bq.double()[None, :, None, None]
    mass = torch.einsum("oc,nhwc->nohw", wq.double().abs(), h.double().abs())
    _check("moments 2x513x512", got, ref, H11 * ref.abs() + 16 * E * mass + 1e-7)
    assert torch.equal(got, ops.vaeenc_moments(h, wq, bq))


# logvar below, at and above the clamp's edges, with the noise and mean of test_sample_matches_float64_on_both_sides_of_the_clamp
HAND_MADE = ((-40.0, 8.0, 0.0), (-30.0, 8.0, 0.0), (0.0, 1.5, -0.75), (20.0, 0.5, 3.0), (25.0, 0.5, 3.0), (25.0, -0.5, 0.0))


@pytest.mark.parametrize("scale", [1.0, 0.18215])
def test_sample_past_one_grid_pass_on_both_sides_of_the_clamp(scale):
    from fresco_amd import ops
    n, hh, ww = 3, 210, 209
    assert ONE_PASS < n * 4 * hh * ww < 2 * ONE_PASS  # 526 680 latent elements
    params = torch.cat([_randn(n, 4, hh, ww, seed=3) * 2.0, _randn(n, 4, hh, ww, seed=4) * 3.0 - 2.0], 1)
    params[-1] = params[-1] * 0.5 + 0.25
    params = params.half()
    noise = _randn(n, 4, hh, ww, seed=5).half()
    # the six elements twice: in the first pass (image 0, channel i % 4, row i) and in the second (image 2, channel 3, row 200 + i)
    spots = [(0, i % 4, i, 2 * i) for i in range(6)] + [(n - 1, 3, 200 + i, 2 * i) for i in range(6)]
    for (b, c, y, x), (lv, nz, mean) in zip(spots, HAND_MADE + HAND_MADE):
        params[b, 4 + c, y, x], noise[b, c, y, x], params[b, c, y, x] = lv, nz, mean
    flat = [((b * 4 + c) * hh + y) * ww + x for b, c, y, x in spots]
    assert max(flat[:6]) < ONE_PASS <= min(flat[6:])
    got = ops.vaeenc_sample(params.to(DEV), noise.to(DEV), scale)
    assert got.shape == noise.shape and got.dtype == torch.float16
    mean, logvar = params[:, :4].double(), params[:, 4:].double().clamp(-30.0, 20.0)
    spread = torch.exp(0.5 * logvar) * noise.double()
    ref = float(np.float32(scale)) * (mean + spread)
    _check("sample 3x8x210x209 scale %g" % scale, got, ref, H11 * ref.abs() + 8 * E * (mean.abs() + spread.abs()) + 1e-7)
    for i, s in enumerate(spots):
        print("  hand-made element %d at %s: got %.6g, float64 %.6g" % (i % 6, s, float(got[s]), float(ref[s])))
    for first in (0, 6):  # the clamp at -30 keeps exp(-15) 8 = 2.4e-6, the clamp at 20 keeps exp(10) / 2 = 11013 inside fp16
        assert float(got[spots[first]]) > 1e-6 * scale and float(got[spots[first + 4]]) > 1000 * scale
    assert torch.equal(got, ops.vaeenc_sample(params.to(DEV), noise.to(DEV), scale))


# ---------------------------------------------------------------------------------------------------------------
# C. end to end, past one pass and past one tile
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return EM.load_golden(VE.GOLDEN, EM.FULLSIZE_GOLDEN_FILE)


@pytest.mark.parametrize("case", EM.FULLSIZE_CASES, ids=EM.case_key)
def test_encoder_matches_the_fullsize_record(case, gold, vae16, encoder):  # noqa: F811
    """vaeenc_1x512x512 took 2.1 s and 5.1 s in two runs on an MI355X, PyTorch's fp16 module beside it included"""
    VE.encoder_against_record(case, gold, vae16, encoder)


def test_a_frame_encoded_alone_has_the_parameters_it_has_in_the_batch(encoder):  # noqa: F811
    case = EM.FULLSIZE_CASES[0]
    assert case[0] == 2
    x = EM.images(case).to(DEV)
    taps = {}
    params = encoder.encode(x, taps=taps).latent_dist.parameters
    for i in range(case[0]):
        alone = {}
        assert torch.equal(encoder.encode(x[i:i + 1], taps=alone).latent_dist.parameters, params[i:i + 1]), "frame %d" % i
        for t in EM.TAPS:
            assert torch.equal(alone[t], taps[t][i:i + 1]), (i, t)
