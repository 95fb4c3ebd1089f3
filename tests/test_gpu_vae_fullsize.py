"""The VAE decoder at the sizes a batch of 512 x 512 frames takes: the forms of csrc/vae.hip, of vae_conv's per-image
weight matrices and of fresco_amd/vae.py's decoder that the small maps of tests/test_gpu_vae.py never reach (the encoder's
own kernels: tests/test_gpu_vae_encoder_fullsize.py).  Every bar is one of tests/test_gpu_vae.py's or tests/conv_ref.py's,
unchanged, and every comparison prints its worst error / bar.

  A  the streaming kernels past one pass of their grid-stride loop.  stream_blocks caps a grid at 2048 blocks of 256 threads
     (STREAM_MAX_BLOCKS): work item 524 288 and later run in a later pass.  Smallest convenient shapes with a ragged second
     pass, random data per image, the last image scaled and shifted, every element compared, a second run bit-equal.
       vae_groupnorm  C = 128 at (2, 129, 255), C = 256 at (2, 129, 128), C = 512 at (2, 65, 127), with and without SiLU:
                      test_gpu_vae.py's GroupNorm bound through its own helper; also 33 to 129 chunks in the statistics pass
       vae_input      latents (2, 4, 513, 512): the post_quant_conv bound of test_conv_ragged_channels_and_the_nchw_image,
                      channels 4 .. 31 zero
  B  the three arrangements of the mid block's attention on vae_conv with several row and column tiles per image AND
     several images -- Q K^T (cout = L, fp32, ldo = Lp), V^T = W_v x^T (x_img_stride 0, per-row bias, ldo = Lp), P V
     (K = Lp) -- with test_conv_per_image_weights_in_both_attention_arrangements' references and conv_bar (K = C, C, Lp):
       (n, L, C) = (3, 130, 512)   Lp 160: two ragged row tiles and two ragged column tiles per image, a grid of 12
       (2, 160, 512)               L = Lp: no pad columns
       (1, 4096, 512)              the real form: 32 x 32 tiles, 128 ring steps in P V; float64 references on the GPU
     Images differ in scale and offset.  scores and vt are written through `out=` into buffers with sentinel guard rows;
     scores starts as NaN and stays NaN in columns >= L, vt's pad columns stay zero, a second run gives the same bits.
     Then the chain of _attention: Q K^T -> vae_softmax -> P V on the kernel's own V^T, against a float64 softmax attention
     on the same fp16 q, k, v.  Its bar is the sum of the parts' bars, each carried to the output:
        conv_bar(Lp) of the P V call on its own operands
        + sum_j (softmax's bar 2^-11 p_j + 8 e on the logits the kernel read  +  p_j (exp(2 scale d) - 1)) |v_j|,
     d the largest conv_bar(C) of the row's logits: a softmax whose logits move by at most scale d moves by at most that
     factor.  No constant is new.
  C  the decoder end to end on vae_model.FULLSIZE_CASES against tests/golden/vae_fullsize_golden.npz
     (tests/golden/make_vae_fullsize_golden.py; test_gpu_vae.py's rule, 4 x recorded noise x peak, and its uint8 rule where
     the whole uint8 image is recorded): latents (2, 24, 24) -- GroupNorm past one pass at C = 128 and 256 (192^2) and C = 512
     (96^2), attention at L = 576 with two images -- and the real (1, 64, 64): 4096 tokens, eight passes at C = 128.  A second
     call gives the same bits, and each frame decoded alone gives exactly the bits it has inside the batch.

Measured on an MI355X, worst error / bar: see MEASURED below; DESIGN.md section 17 has the table.

A scratch build in which every grid-stride loop of vae.hip and vae_enc.hip runs a single pass passes every kernel test of
tests/test_gpu_vae.py and tests/test_gpu_vae_encoder.py, fails one end-to-end record in each (160 x 224, through GroupNorm
at 128 channels) and fails every test of A and C here: see MUTANT below.
"""
import pytest
import torch

import test_gpu_conv_unet_forms as U
import test_gpu_vae as V
import vae_model as M
from conv_ref import E, H11, check, conv_bar
from test_gpu_vae import decoder, vae16  # noqa: F401  (fixtures, built once for this module)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE_PASS = 2048 * 256  # work items of one pass of a streaming kernel's grid-stride loop (STREAM_MAX_BLOCKS blocks of 256)

MEASURED = """
A  vae_groupnorm 0.992 - 0.996 (as at the small sizes: the fp16 rounding of the result is most of the bar), vae_input 0.997
B  (3, 130, 512): Q K^T 0.012, V^T 0.807, P V 0.977, chain 0.282;  (2, 160, 512): 0.008, 0.818, 0.975, 0.285;
   (1, 4096, 512): 0.005, 0.812, 0.664, 0.117 -- 0.31 s for the whole case
C  vae_2x24x24: taps 0.118 - 0.155, image 0.140 (PyTorch's fp16 module 0.217 - 0.571), uint8 never 2 apart, 10.106 % one
   apart (allowed 22.153 %);  vae_1x64x64: taps 0.080 - 0.139, image 0.190;  frames alone: bit-equal, every tap too
The file's 13 tests took 11 s: 7.5 s of them PyTorch's module at (2, 24, 24) (4.1 s in a second run), 0.7 s the first
GroupNorm case, the kernel tests 0.3 s and less each.
"""

# What the single-pass scratch build (see the module docstring) gave on an MI355X.  What a later pass should have written
# is whatever the allocator left there, NaN included.
MUTANT = """
tests/test_gpu_vae.py: 28 passed, 1 failed; tests/test_gpu_vae_encoder.py: 17 passed, 1 failed.  Every kernel test passes.
The two failures are the 160 x 224 records, whose 128-channel GroupNorm has 573 440 items per image:
  test_decoder_matches_the_record[vae_1x20x28]          up2 11.5, up3 27.5, image 449 x the bar
  test_encoder_matches_the_record[vaeenc_1x160x224]     down0 122, parameters 142 x the bar
so the loop of vae_gn_apply_kernel was seen before, in one kernel, at one width, through an end-to-end bar; the loops of
vae_input, vaeenc_input, vaeenc_moments and vaeenc_sample and GroupNorm at 256 and 512 channels were not.
tests/test_gpu_vae_fullsize.py: 10 failed, 3 passed --
  test_groupnorm_past_one_grid_pass                     C = 128: worst error / bound 3.5e+06 and 3.3e+05; C = 256: 3.6e+04,
                                                        1.8e+04; C = 512: 2.0e+04, 1.4e+04
  test_input_past_one_grid_pass                         2.0e+03
  test_decoder_matches_the_fullsize_record              vae_2x24x24: up2, up3, norm_out and the image NaN; vae_1x64x64: up1 175 x
                                                        the bar, NaN from up2 on
  test_a_frame_decoded_alone_has_the_bits_it_has_in_the_batch   frame 0 differs
  B passes (vae_conv and vae_softmax have no such loop).
tests/test_gpu_vae_encoder_fullsize.py: 7 failed, 0 passed --
  test_input_past_one_grid_pass                         fails at cpad 32: what pass two should have written is not the image
  test_moments_past_one_grid_pass                       NaN
  test_sample_past_one_grid_pass_on_both_sides_of_the_clamp   NaN (scale 1), 4.6e+06 (scale 0.18215)
  test_encoder_matches_the_fullsize_record              vaeenc_2x192x192: NaN from down0 on; vaeenc_1x512x512: down0 146,
                                                        parameters 134 x the bar
  test_a_frame_encoded_alone_has_the_parameters_it_has_in_the_batch   frame 0 differs
The NaN taps of vae_2x24x24 and vaeenc_2x192x192 got past `max(worst)[0] <= 1.0`, the form the record comparison had: max()
over (ratio, name) pairs steps over a NaN that is not the first entry.  The comparison now asks every ratio to be <= 1.
"""


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------
# A. streaming kernels past one grid pass
# ---------------------------------------------------------------------------------------------------------------
GN_SHAPES = {128: (2, 129, 255), 256: (2, 129, 128), 512: (2, 65, 127)}


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("C", sorted(GN_SHAPES), ids=lambda c: "C%d" % c)
def test_groupnorm_past_one_grid_pass(C, silu):
    """vae_gn_apply_kernel strides per image over P C / 8 items; the statistics pass takes P / 256 = 33 to 129 chunks, which
    gn_finish_kernel adds up"""
    n, H, W = GN_SHAPES[C]
    assert ONE_PASS < H * W * C // 8 < 2 * ONE_PASS  # 526 320, 528 384, 528 320 per image: a ragged second pass
    V._groupnorm_against_float64(n, H, W, C, silu)  # every element; image 1 scaled and shifted; a second run's bits


def test_input_past_one_grid_pass():
    from fresco_amd import ops
    n, h, w = 2, 513, 512
    assert ONE_PASS < n * h * w < 2 * ONE_PASS  # 525 312 latent pixels
    z = _randn(n, 4, h, w, seed=21)
    z[-1] = z[-1] * 0.5 + 1.0
    z = z.half().to(DEV)
    wq, bq = (torch.eye(4) + 0.2 * _randn(4, 4, seed=22)).to(DEV), (0.1 * _randn(4, seed=23)).to(DEV)
    xin = ops.vae_input(z, wq, bq)
    assert xin.shape == (n, h, w, 32) and xin.dtype == torch.float16 and not xin[..., 4:].any()
    pq = torch.einsum("oc,nchw->nhwo", wq.double(), z.double()) + bq.double()
    mass = torch.einsum("oc,nchw->nhwo", wq.double().abs(), z.double().abs()) + bq.double().abs()
    check("post_quant_conv (2, 4, 513, 512)", xin[..., :4], pq, 8 * E * mass + H11 * pq.abs() + 1e-6)
    assert torch.equal(xin, ops.vae_input(z, wq, bq))


# ---------------------------------------------------------------------------------------------------------------
# B. the three attention arrangements with several tiles per image
# ---------------------------------------------------------------------------------------------------------------
ATTENTION_SHAPES = {"n3_L130": (3, 130, 512), "n2_L160_no_pad": (2, 160, 512), "real_L4096": (1, 4096, 512)}


def _each_image_differs(t):
    """image i scaled by 1 - i / 4 and shifted by i / 2, in place: a wrong image stride shows"""
    for i in range(1, t.shape[0]):
        t[i] = t[i] * (1.0 - 0.25 * i) + 0.5 * i
    return t


def _twice_into_guarded(name, rows, ld, dtype, fill, cout, call):
    """call(out) twice, each time into the live rows of a fresh (G + rows + G, ld) buffer: the guard rows hold a sentinel,
    the live rows `fill`.  -> the first run's live rows, after the guards' check, the check that columns >= cout still
    hold `fill`, and the second run's bits"""
    G = U._guard_rows(ld)
    bufs = []
    for _ in range(2):
        buf = torch.full((G + rows + G, ld), U.SENTINEL, dtype=dtype, device=DEV)
        buf[G:G + rows] = fill
        out = buf[G:G + rows]
        assert call(out).data_ptr() == out.data_ptr()
        bufs.append(buf)
    for buf in bufs:
        assert bool((buf[:G] == U.SENTINEL).all()) and bool((buf[G + rows:] == U.SENTINEL).all()), name + ": guard rows"
        pad = buf[G:G + rows, cout:]
        assert bool((torch.isnan(pad) if fill != fill else pad == fill).all()), name + ": columns beyond cout"
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(bufs[0].view(ints), bufs[1].view(ints)), name + ": a second run differs"
    return bufs[0][G:G + rows]


@pytest.mark.parametrize("shape", sorted(ATTENTION_SHAPES))
def test_attention_arrangements_with_several_tiles_per_image(shape):
    """real_L4096 took 0.31 s on an MI355X with its float64 references on the GPU (V^T included)"""
    from fresco_amd import _lib, ops
    n, L, C = ATTENTION_SHAPES[shape]
    Lp = (L + 31) // 32 * 32
    scale = float(C) ** -0.5
    seed = sum(map(ord, shape))
    q = _each_image_differs(_randn(n, L, C, seed=seed)).half().to(DEV)
    k = _each_image_differs(_randn(n, L, C, seed=seed + 1)).half().to(DEV)
    h = _each_image_differs(_randn(n, L, C, seed=seed + 2)).half().to(DEV)
    wv = (_randn(C, C, seed=seed + 3) * C ** -0.5).half().to(DEV)
    bv = _randn(C, seed=seed + 4).to(DEV)

    # Q K^T
    scores = _twice_into_guarded("Q K^T " + shape, n * L, Lp, torch.float32, float("nan"), L, lambda out: ops.vae_conv(
        q, k, None, n, L, 1, C, L, 1, out_kind=_lib.VAE_OUT_F32, w_img_stride=L * C, ldo=Lp, out=out))
    ref_s = q.double() @ k.double().transpose(1, 2)
    bar_s = conv_bar(C, q.double().abs() @ k.double().abs().transpose(1, 2), ref_s, fp32=True)
    check("Q K^T " + shape, scores.view(n, L, Lp)[..., :L], ref_s, bar_s)

    # V^T = W_v x^T + b_v per row
    vt = _twice_into_guarded("V^T " + shape, n * C, Lp, torch.float16, 0.0, L, lambda out: ops.vae_conv(
        wv, h, bv, n, C, 1, C, L, 1, x_img_stride=0, w_img_stride=L * C, bias_rows=True, ldo=Lp, out=out)).view(n, C, Lp)
    ref = (h.double() @ wv.double().t() + bv.double()).transpose(1, 2)
    mass = (h.double().abs() @ wv.double().abs().t()).transpose(1, 2)
    check("V^T " + shape, vt[..., :L], ref, conv_bar(C, mass, ref))
    vt64 = vt.double().transpose(1, 2)  # (n, Lp, C), the pad rows zero

    # P V on hand-made probabilities
    p = torch.zeros(n, L, Lp, dtype=torch.float16)
    p[..., :L] = torch.softmax(_each_image_differs(_randn(n, L, L, seed=seed + 5)) * 3.0, -1).half()
    p = p.to(DEV)
    o = ops.vae_conv(p, vt, None, n, L, 1, Lp, C, 1, w_img_stride=C * Lp)
    ref = p.double() @ vt64
    check("P V " + shape, o.view(n, L, C), ref, conv_bar(Lp, p.double() @ vt64.abs(), ref))
    assert torch.equal(o, ops.vae_conv(p, vt, None, n, L, 1, Lp, C, 1, w_img_stride=C * Lp))

    # the chain of _attention on these q, k and the kernel's V^T (the bar: see the module docstring)
    p_hat = ops.vae_softmax(scores, L, scale, ld_out=Lp)
    assert p_hat.shape == (n * L, Lp) and not p_hat[:, L:].any()
    o = ops.vae_conv(p_hat, vt, None, n, L, 1, Lp, C, 1, w_img_stride=C * Lp)
    p_hat = p_hat.view(n, L, Lp).double()
    grow = torch.expm1(2.0 * scale * bar_s.amax(-1, keepdim=True))
    p_true = torch.softmax(ref_s * scale, -1)
    p_read = torch.softmax(scores.view(n, L, Lp)[..., :L].double() * scale, -1)
    bar_p = H11 * p_read + 8 * E + p_true * grow
    bar = conv_bar(Lp, p_hat @ vt64.abs(), p_hat @ vt64) + bar_p @ vt64[:, :L].abs()
    check("softmax(Q K^T / sqrt C) V " + shape, o.view(n, L, C), p_true @ vt64[:, :L], bar)


# ---------------------------------------------------------------------------------------------------------------
# C. end to end, past one pass and past one tile
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return M.load_golden(V.GOLDEN, M.FULLSIZE_GOLDEN_FILE)


@pytest.mark.parametrize("case", M.FULLSIZE_CASES, ids=M.case_key)
def test_decoder_matches_the_fullsize_record(case, gold, vae16, decoder):  # noqa: F811
    """PyTorch's fp16 module is printed beside ours at (2, 24, 24) only: its first call takes 7.8 s there and 17.5 s at
    (1, 64, 64) on an MI355X (ours: 0.01 s), and nothing is asserted on it.  Measured: 7.5 s and 4.1 s in two runs for (2, 24, 24), under 3 s for (1, 64, 64)"""
    small = case == M.FULLSIZE_CASES[0]
    assert (M.case_key(case) + "_image_u8" in gold) == small
    V.decoder_against_record(case, gold, vae16 if small else None, decoder)


def test_a_frame_decoded_alone_has_the_bits_it_has_in_the_batch(decoder):  # noqa: F811
    case = M.FULLSIZE_CASES[0]
    assert case[0] == 2
    z = M.latents(case).to(DEV)
    taps = {}
    img = decoder.decode(z, taps=taps).sample
    for i in range(case[0]):
        alone = {}
        assert torch.equal(decoder.decode(z[i:i + 1], taps=alone).sample, img[i:i + 1]), "frame %d" % i
        for t in M.TAPS:
            assert torch.equal(alone[t], taps[t][i:i + 1]), (i, t)
