"""What tests/test_gpu_vae_fullsize.py and tests/test_gpu_vae_encoder_fullsize.py rely on in their records
(tests/golden/vae_fullsize_golden.npz, tests/golden/vae_encoder_fullsize_golden.npz), without a GPU: keys, shapes, positive
noise, peaks under ACT_LIMIT, and that the cases are past one grid pass and one attention tile where the GPU tests say they
are.  The float64 model is NOT run again at these sizes: test_vae_cpu.py and test_vae_encoder_cpu.py reproduce the small
records, and the makers of the full-size ones run the same record() on other cases."""
import os

import numpy as np
import torch

import vae_encoder_model as EM
import vae_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ONE_PASS = 2048 * 256  # STREAM_MAX_BLOCKS blocks of 256 threads (csrc/common.h)
CT_BM = 128            # rows of a tile of the convolution (csrc/conv_tile.h)


def _thinned_shape(n, H, W, C):
    return M.thin(np.zeros((n, H, W, C), np.int8)).shape


def _noise_and_peak(gold, key, taps):
    noise, peak = gold[key + "_noise"], gold[key + "_peak"]
    assert noise.shape == peak.shape == (len(taps) + 1,)
    assert (noise > 0).all() and (noise < 0.01).all() and (peak > 0).all() and (peak < M.ACT_LIMIT).all()


def test_the_cases_are_past_one_pass_and_one_tile():
    assert EM.FULLSIZE_CASES == [(n, 8 * h, 8 * w) for n, h, w in M.FULLSIZE_CASES]
    n, h, w = M.FULLSIZE_CASES[0]
    assert n == 2 and h * w > CT_BM and (h * w) % CT_BM  # two images, several row tiles of attention, the last one ragged
    # vae_gn_apply_kernel's items per image, P C / 8: a ragged later pass at every width of the decoder ...
    for P, C in ((64 * h * w, 128), (64 * h * w, 256), (16 * h * w, 512)):
        assert P * C // 8 > ONE_PASS and (P * C // 8) % ONE_PASS, (P, C)
    # ... and at the encoder's first width (its 256-wide maps are 96^2 here: inside one pass)
    assert 64 * h * w * 128 // 8 > ONE_PASS
    assert M.FULLSIZE_CASES[1] == (1, 64, 64)  # the real frame: 4096 tokens, eight passes at C = 128
    assert 512 * 512 * 128 // 8 == 8 * ONE_PASS


def test_the_decoder_record_holds_what_the_gpu_tests_rely_on():
    path = os.path.join(GOLDEN, M.FULLSIZE_GOLDEN_FILE)
    assert os.path.getsize(path) < (1 << 20)
    gold = M.load_golden(GOLDEN, M.FULLSIZE_GOLDEN_FILE)
    widths = {"conv_in": (1, 512), "mid": (1, 512), "up0": (2, 512), "up1": (4, 512), "up2": (8, 256), "up3": (8, 128),
              "norm_out": (8, 128)}
    assert tuple(widths) == M.TAPS
    for case in M.FULLSIZE_CASES:
        key = M.case_key(case)
        n, h, w = case
        _noise_and_peak(gold, key, M.TAPS)
        assert 0 < float(gold[key + "_u8_share"]) < 0.25
        # the whole uint8 image only where it is small: the real frame's would be 786 432 bytes that do not compress
        assert (key + "_image_u8" in gold) == (case == M.FULLSIZE_CASES[0])
        if key + "_image_u8" in gold:
            assert gold[key + "_image_u8"].shape == (n, 8 * h, 8 * w, 3) and gold[key + "_image_u8"].dtype == np.uint8
        assert gold[key + "_image"].dtype == np.float64
        assert gold[key + "_image"].shape == M.thin_image(np.zeros((n, 3, 8 * h, 8 * w), np.int8)).shape
        for t, (f, C) in widths.items():
            rec = gold["%s_%s" % (key, t)]
            assert rec.dtype == np.float64 and rec.shape == _thinned_shape(n, f * h, f * w, C), (key, t, rec.shape)
        lat = M.latents(case)
        assert lat.shape == (n, 4, h, w) and lat.dtype == torch.float16
    assert len(gold) == sum(len(M.TAPS) + 4 + (case == M.FULLSIZE_CASES[0]) for case in M.FULLSIZE_CASES)
    assert M.load_golden(GOLDEN).keys() == M.load_golden(GOLDEN, M.GOLDEN_FILE).keys()  # the default stays the small record
    assert not set(gold) & set(M.load_golden(GOLDEN))


def test_the_encoder_record_holds_what_the_gpu_tests_rely_on():
    path = os.path.join(GOLDEN, EM.FULLSIZE_GOLDEN_FILE)
    assert os.path.getsize(path) < (1 << 20)
    gold = EM.load_golden(GOLDEN, EM.FULLSIZE_GOLDEN_FILE)
    widths = {"conv_in": (1, 128), "down0": (2, 128), "down1": (4, 256), "down2": (8, 512), "down3": (8, 512), "mid": (8, 512),
              "norm_out": (8, 512)}
    assert tuple(widths) == EM.TAPS
    for case in EM.FULLSIZE_CASES:
        key = EM.case_key(case)
        n, H, W = case
        _noise_and_peak(gold, key, EM.TAPS)
        params = gold[key + "_parameters"]
        assert params.dtype == np.float64 and params.shape == (n, 8, H // 8, W // 8)
        assert -30 < params[:, 4:].min() and params[:, 4:].max() < 20
        for t, (f, C) in widths.items():
            rec = gold["%s_%s" % (key, t)]
            assert rec.dtype == np.float64 and rec.shape == _thinned_shape(n, H // f, W // f, C), (key, t, rec.shape)
        img = EM.images(case)
        assert img.shape == (n, 3, H, W) and img.dtype == torch.float16 and float(img.abs().max()) < 1.6
        assert float(img.float().std()) > 0.2
    assert len(gold) == len(EM.FULLSIZE_CASES) * (len(EM.TAPS) + 3)
    assert EM.load_golden(GOLDEN).keys() == EM.load_golden(GOLDEN, EM.GOLDEN_FILE).keys()
    assert not set(gold) & set(EM.load_golden(GOLDEN))
