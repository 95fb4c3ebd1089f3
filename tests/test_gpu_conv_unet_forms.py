"""vae_conv (csrc/vae.hip on csrc/conv_tile.h) in the forms the UNet calls it in, element by element against float64 on the same
operands (tests/conv_ref.py), and its two neighbours of csrc/unet_tf.hip past what test_gpu_unet_transformer.py reaches:

  (a) 3 x 3 at the resnet widths (cin 320 .. 2560, up to 720 ring steps), plain, without a bias, with bias + residual;
  (b) the 8-byte-store epilogue on a ragged last column tile: a half-live tile, nbv = 1, a 32-channel block live in part,
      each with and without bias and residual, and into an `out` of row stride cout + 8 whose residual has that stride too;
  (c) the flat-row 1 x 1 calls (n = 1, H = M, W = 1) of the transformer and of the attention processor;
  (d) conv_tile.h's deal of the workgroups to the XCDs, over grids of 1 .. 45 workgroups;
  (e) unet_layernorm where a wave takes a second row (rows = 4 x 2048 + 5);
  (f) unet_geglu at K = 1280.

Rules of (a) - (d).  EVERY output element is compared.  The output is a buffer of this file: NaN where the kernel has to write,
a sentinel in guard rows before and after it and in the guard columns beyond cout, all unchanged afterwards.  The bias is the
head of a longer buffer whose tail is NaN, and a residual's guard columns are NaN: a read beyond cout, or at another row
stride, that reaches the output shows.  The last image (of flat rows: the last image's rows) is scaled and shifted, so bleed
across images shows.  A second run into a second such buffer gives the same bits.  Inputs are N(0, 1.5), weights
sqrt(2 / K) N(0, 1) rounded to fp16 once.

Bars: none is new.  vae_conv: conv_ref.conv_bar, K e sum |x| |w| + 2^-11 |ref| + 1e-6 with e = 2^-24 (test_gpu_vae.py's);
unet_layernorm and unet_geglu: test_gpu_unet_transformer.py's.  Every comparison prints its ratio to the bar.
"""
import functools

import pytest
import torch

from conv_ref import E, H11, check, conv_bar, conv_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -1234.0
NAN = float("nan")
CT_BM, CT_BN, CT_TH, CT_TW = 128, 128, 8, 16          # conv_tile.h's tile: pixels, channels, and the pixels' 8 x 16 plane


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


def _operands(n, Hs, Ws, cin, cout, k, seed, images=None):
    """x (n, Hs, Ws, cin) and w (cout, cin, k, k), fp16 on the GPU; `images`: how many images the flat rows of an n = 1 call
    hold (the last one's rows are the ones scaled and shifted)"""
    x = (_randn(n, Hs, Ws, cin, seed=seed) * 1.5).half()
    if images is None:
        x[-1] = x[-1] * 0.5 + 1.0
    else:
        assert n == 1 and Ws == 1 and Hs % images == 0
        x[0, Hs - Hs // images:] = x[0, Hs - Hs // images:] * 0.5 + 1.0
    w = (_randn(cout, cin, k, k, seed=seed + 1) * (2.0 / (cin * k * k)) ** 0.5).half()
    return x.to(DEV), w.to(DEV)


def _bias(cout, seed):
    """cout fp32 values at the head of a buffer whose other 128 are NaN"""
    buf = torch.full((cout + CT_BN,), NAN)
    buf[:cout] = _randn(cout, seed=seed)
    return buf.to(DEV)[:cout]


def _residual(rows, cout, ldo, seed):
    """(rows, ldo) fp16: N(0, 2) in the first cout columns, NaN in the guard columns"""
    buf = torch.full((rows, ldo), NAN, dtype=torch.float16)
    buf[:, :cout] = (_randn(rows, cout, seed=seed) * 2.0).half()
    return buf.to(DEV)


def _guard_rows(ldo):
    """at least a column tile's width of elements on either side, and an offset that keeps the rows 16-byte aligned"""
    return 4 * ((CT_BN + 4 * ldo - 1) // (4 * ldo)) + 4


def _run(name, x, wp, geom, ref, mass, bias=None, residual=None, pad=0):
    """vae_conv twice into guarded NaN buffers of row stride cout + pad -> the first run's live columns, (rows, cout), after
    the full comparison with ref [+ bias] [+ residual], the guards' check and the second run's bits"""
    from fresco_amd import ops
    n, H, W, cin, cout, k, up2 = geom
    rows, ldo, K = n * H * W, cout + pad, cin * k * k
    G = _guard_rows(ldo)
    want = ref.reshape(rows, cout)
    if bias is not None:
        want = want + bias.double()
    if residual is not None:
        assert residual.shape == (rows, ldo)
        want = want + residual[:, :cout].double()
    bufs = []
    for _ in range(2):
        buf = torch.full((G + rows + G, ldo), SENTINEL, dtype=torch.float16, device=DEV)
        buf[G:G + rows, :cout] = NAN
        out = buf[G:G + rows]
        got = ops.vae_conv(x, wp, bias, n, H, W, cin, cout, k, up2=up2, residual=residual, ldo=ldo, out=out)
        assert got.data_ptr() == out.data_ptr()
        bufs.append(buf)
    live = bufs[0][G:G + rows]
    check(name, live[:, :cout], want, conv_bar(K, mass.reshape(rows, cout), want))
    for buf in bufs:
        assert bool((buf[:G] == SENTINEL).all()) and bool((buf[G + rows:] == SENTINEL).all()), name + ": guard rows"
        assert bool((buf[G:G + rows, cout:] == SENTINEL).all()), name + ": guard columns"
    assert torch.equal(bufs[0].view(torch.int16), bufs[1].view(torch.int16)), name + ": a second run differs"
    return live[:, :cout]


def _pack(w):
    from fresco_amd.vae import pack_conv_weight
    return pack_conv_weight(w)


# ---------------------------------------------------------------------------------------------------------------
# (a) 3 x 3 at the resnet widths
# ---------------------------------------------------------------------------------------------------------------
RESNET_SHAPES = {
    # name: (n, Hs, Ws, cin, cout, up2)
    # three column tiles, the third half live (wn 1 dead); two images; 8 x 12 is one tile, ragged in x
    "c320_two_images": (2, 8, 12, 320, 320, False),
    # 9 x 17: 2 x 2 tiles, a one-row, a one-column and a one-pixel tile; 30 chunks
    "c960_edge_tiles": (1, 9, 17, 960, 320, False),
    # five whole column tiles, 60 chunks, two tiles ragged in y
    "c1920_five_column_tiles": (1, 10, 14, 1920, 640, False),
    # K = 23040: 80 chunks, 720 ring steps
    "c2560_K23040": (1, 8, 8, 2560, 320, False),
    # five images of one tile each x five column tiles: 25 workgroups, T % 8 = 1
    "c320_five_images": (5, 8, 8, 320, 640, False),
    # the Upsample2D form: 4 x 6 -> 8 x 12 (one tile, ragged in x), two images, five column tiles
    "up2_c640": (2, 4, 6, 640, 640, True),
}


@functools.lru_cache(maxsize=None)
def _resnet_case(shape):
    """operands and the float64 reference of one shape, computed once and shared by its three variants (never written to)"""
    n, Hs, Ws, cin, cout, up2 = RESNET_SHAPES[shape]
    x, w = _operands(n, Hs, Ws, cin, cout, 3, _seed(shape))
    ref, mass = conv_ref(x, w, up2)
    return x, _pack(w), ref, mass


@pytest.mark.parametrize("variant", ["plain", "no_bias", "bias_residual"])
@pytest.mark.parametrize("shape", sorted(RESNET_SHAPES))
def test_a_3x3_at_the_resnet_widths(shape, variant):
    n, Hs, Ws, cin, cout, up2 = RESNET_SHAPES[shape]
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    x, wp, ref, mass = _resnet_case(shape)
    seed = _seed(shape)
    bias = None if variant == "no_bias" else _bias(cout, seed + 2)
    res = _residual(n * H * W, cout, cout, seed + 3) if variant == "bias_residual" else None
    _run("(a) 3x3 %s %s" % (shape, variant), x, wp, (n, H, W, cin, cout, 3, up2), ref, mass, bias, res)


# ---------------------------------------------------------------------------------------------------------------
# (b) ragged column tiles on the 8-byte-store path
# ---------------------------------------------------------------------------------------------------------------
def _last_tile_live_blocks(cout):
    """(nbv of wn 0, nbv of wn 1) in the last column tile: conv_tile.h's ct_live_blocks, C's division"""
    co0 = (cout + CT_BN - 1) // CT_BN * CT_BN - CT_BN
    return tuple(min(max(int((cout - co0 - 64 * wn + 31) / 32), 0), 2) for wn in (0, 1))


RAGGED_COUT = {
    # cout: (nbv of wn 0, nbv of wn 1) of the last column tile
    36: (2, 0),    # wn 0's second block holds channels 32 .. 35 only; wn 1 dead
    96: (2, 1),    # nbv = 1 in wn 1
    100: (2, 2),   # wn 1's second block holds channels 96 .. 99 only
    160: (1, 0),   # second tile: nbv = 1 in wn 0, wn 1 dead
    288: (1, 0),   # third tile: the same after two whole tiles
    320: (2, 0),   # the UNet's width: third tile half live
}
RAGGED_FORMS = {"3x3": (1, 9, 17, 3), "1x1": (1, 150, 1, 1)}      # (n, H, W, ksize); cin = 64


@pytest.mark.parametrize("form", sorted(RAGGED_FORMS))
@pytest.mark.parametrize("cout", sorted(RAGGED_COUT))
def test_b_ragged_column_tile_with_vector_stores(cout, form):
    assert cout % 4 == 0 and (cout + 8) % 4 == 0                   # the 8-byte-store path, at both row strides
    assert _last_tile_live_blocks(cout) == RAGGED_COUT[cout]
    if cout in (36, 100):
        assert cout % 32 == 4                                      # ends inside a 32-channel block
    if cout in (96, 288):
        assert 1 in RAGGED_COUT[cout]
    if cout in (160, 320):
        assert RAGGED_COUT[cout][1] == 0                           # a dead wave
    n, H, W, k = RAGGED_FORMS[form]
    cin = 64
    seed = _seed("%s_%d" % (form, cout))
    x, w = _operands(n, H, W, cin, cout, k, seed)
    ref, mass = conv_ref(x, w, False)
    wp, bias = _pack(w), _bias(cout, seed + 2)
    for pad in (0, 8):
        res = _residual(n * H * W, cout, cout + pad, seed + 3)
        for use_bias in (True, False):
            for use_res in (False, True):
                name = "(b) %s cout=%d ldo=%d%s%s" % (form, cout, cout + pad, " + bias" if use_bias else "", " + residual" if use_res else "")
                _run(name, x, wp, (n, H, W, cin, cout, k, False), ref, mass, bias if use_bias else None, res if use_res else None, pad)


# ---------------------------------------------------------------------------------------------------------------
# (c) the flat-row 1 x 1 forms of the transformer and the attention processor
# ---------------------------------------------------------------------------------------------------------------
FLAT_FORMS = {
    # name: (images, rows per image, K, cout, bias, residual)
    "proj_in_proj_out": (2, 96, 320, 320, True, True),            # M 192: two row tiles, the second half full; third column tile half live
    "ff_net_2": (1, 129, 5120, 320, True, True),                  # 160 ring steps; M 129: one row in the second tile
    "to_out": (2, 33, 1280, 1280, True, False),                   # M 66, ten whole column tiles
}


@pytest.mark.parametrize("form", sorted(FLAT_FORMS))
def test_c_flat_rows(form):
    images, L, K, cout, use_bias, use_res = FLAT_FORMS[form]
    M = images * L
    seed = _seed(form)
    x, w = _operands(1, M, 1, K, cout, 1, seed, images=images)
    ref, mass = conv_ref(x, w, False)
    bias = _bias(cout, seed + 2) if use_bias else None
    res = _residual(M, cout, cout, seed + 3) if use_res else None
    _run("(c) flat rows %s M=%d K=%d cout=%d" % (form, M, K, cout), x, _pack(w), (1, M, 1, K, cout, 1, False), ref, mass, bias, res)


def test_c_fused_qkv_is_three_projections():
    """to_q | to_k | to_v at width 1280: one call on the three weight matrices stacked, read back as three column slices of
    row stride 3840, each against its own projection's float64 reference"""
    from fresco_amd import ops
    B, L, K, N = 2, 33, 1280, 1280
    M = B * L
    x, w0 = _operands(1, M, 1, K, N, 1, _seed("qkv"), images=B)
    ws = [w0] + [(_randn(N, K, 1, 1, seed=_seed("qkv") + 10 + i) * (2.0 / K) ** 0.5).half().to(DEV) for i in range(2)]
    refs = [conv_ref(x, w, False) for w in ws]
    wp = torch.cat([_pack(w) for w in ws], 0)
    assert wp.shape == (3 * N, K) and wp.is_contiguous()
    ref, mass = (torch.cat([r[i] for r in refs], -1) for i in range(2))
    got = _run("(c) to_q|to_k|to_v fused", x, wp, (1, M, 1, K, 3 * N, 1, False), ref, mass)
    out = ops.vae_conv(x.view(M, K), wp, None, 1, M, 1, K, 3 * N, 1).view(B, L, 3 * N)     # the processor's own call
    assert torch.equal(out.view(M, 3 * N), got)
    for i, name in enumerate(("to_q", "to_k", "to_v")):
        part = out[..., i * N:(i + 1) * N]
        assert part.shape == (B, L, N) and part.stride() == (L * 3 * N, 3 * N, 1)
        r, m = (t.reshape(B, L, N) for t in refs[i])
        check("(c) fused slice %s" % name, part, r, conv_bar(K, m, r))


def test_c_text_kv_flat_and_per_image_give_the_same_bits():
    """the text's to_k | to_v, K 768 -> 2560 on 2 x 77 rows: the flat call (154 rows: two row tiles, the second holding rows of
    both images' tail) and the per-image call (n = 2, H = 77: one row tile per image) add each element's K products in the
    same order, so they give the same bits; the transformer relies on the flat form"""
    B, L, K, cout = 2, 77, 768, 2560
    x, w = _operands(1, B * L, 1, K, cout, 1, _seed("text_kv"), images=B)
    ref, mass = conv_ref(x, w, False)
    wp = _pack(w)
    flat = _run("(c) text to_k|to_v flat", x, wp, (1, B * L, 1, K, cout, 1, False), ref, mass)
    per_image = _run("(c) text to_k|to_v per image", x.view(B, L, 1, K), wp, (B, L, 1, K, cout, 1, False), ref, mass)
    assert torch.equal(flat.view(torch.int16), per_image.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------
# (d) the workgroup deal
# ---------------------------------------------------------------------------------------------------------------
DEAL_PLANES = {1: (7, 13), 2: (8, 17), 3: (17, 11), 7: (8, 105), 17: (130, 9)}      # plane tiles: H x W of the 3 x 3 form
DEAL_ROWS = {1: 1, 2: 129, 3: 300, 7: 800, 17: 2100}                               # row tiles: M of the 1 x 1 form (M = 1 too)
DEAL_COUT = {1: 128, 2: 256, 3: 320}                                               # column tiles
DEAL_EXTRA = [(1, 7, 1), (1, 17, 1)]   # (n, tiles, column tiles): 7 and 17 are no product of the sweep's factors
DEAL_T = {1, 3, 7, 8, 9, 15, 17, 45}


def _deal_cases(k):
    sweep = [(n, tiles, ct) for n in (1, 2, 3, 5) for tiles in (1, 2, 3) for ct in (1, 2, 3)]
    for n, tiles, ct in sweep + DEAL_EXTRA:
        H, W = DEAL_PLANES[tiles] if k == 3 else (DEAL_ROWS[tiles], 1)
        yield n, H, W, DEAL_COUT[ct]


def _grid(n, H, W, cout, k):
    """T as the host computes it (conv_tile.h's ct_grid): n x tiles x ceil(cout / 128)"""
    tiles = ((H + CT_TH - 1) // CT_TH) * ((W + CT_TW - 1) // CT_TW) if k == 3 else (H * W + CT_BM - 1) // CT_BM
    return n * tiles * ((cout + CT_BN - 1) // CT_BN)


def test_d_sweep_covers_the_grids():
    for k in (1, 3):
        seen = {_grid(n, H, W, cout, k) for n, H, W, cout in _deal_cases(k)}
        assert DEAL_T <= seen, (k, sorted(DEAL_T - seen))
        assert any(T < 8 for T in seen) and any(T > 8 and T % 8 for T in seen) and any(T % 8 == 0 for T in seen)
    for tiles, (H, W) in DEAL_PLANES.items():
        assert _grid(1, H, W, 128, 3) == tiles
    for tiles, M in DEAL_ROWS.items():
        assert _grid(1, M, 1, 128, 1) == tiles


@pytest.mark.parametrize("k", [3, 1], ids=["3x3", "1x1"])
def test_d_every_tile_is_dealt_once(k):
    """cin 32, one chunk: the output starts as NaN, so a tile that no workgroup takes stays NaN, and one that lands in another
    tile's place (or an image's, or a column tile's) misses its reference"""
    cin = 32
    for n, H, W, cout in _deal_cases(k):
        T = _grid(n, H, W, cout, k)
        seed = _seed("deal%d_%d_%d_%d_%d" % (k, n, H, W, cout))
        x, w = _operands(n, H, W, cin, cout, k, seed)
        if n > 2:
            x[1] = x[1] * 0.25 - 2.0                                # a third kind of image
        ref, mass = conv_ref(x, w, False)
        _run("(d) deal %dx%d n=%d %dx%d cout=%d T=%d" % (k, k, n, H, W, cout, T), x, _pack(w), (n, H, W, cin, cout, k, False),
             ref, mass, _bias(cout, seed + 2))


# ---------------------------------------------------------------------------------------------------------------
# (e) unet_layernorm past one trip of its row loop
# ---------------------------------------------------------------------------------------------------------------
UL_MAX_BLOCKS, UL_WAVES = 2048, 4                                                   # unet_tf.hip's grid limit, waves per workgroup
LN_ROWS = UL_WAVES * UL_MAX_BLOCKS + 5


@pytest.mark.parametrize("C", [64, 320, 1280], ids=lambda c: "C%d_NP%d" % (c, (c + 511) // 512))
def test_e_layernorm_second_trip_of_the_row_loop(C):
    """8197 rows on the full grid of 2048 workgroups x 4 waves: waves 0 .. 4 take a second row (8192 .. 8196) with the gamma and
    beta they loaded for their first.  Row 8192, the first of the second trip, and the last row each have statistics of their
    own.  Bar: test_gpu_unet_transformer.py's, 16 e ((|x| + |mean|) rstd |gamma| + |beta|) + 1e-6 + 2^-11 |y|."""
    from fresco_amd import ops
    rows, eps = LN_ROWS, 1e-5
    first_of_second_trip = UL_WAVES * UL_MAX_BLOCKS
    assert (rows + UL_WAVES - 1) // UL_WAVES > UL_MAX_BLOCKS and first_of_second_trip < rows - 1
    gamma, beta = (_randn(C, seed=C + 1) * 0.5 + 1.0).to(DEV), _randn(C, seed=C + 2).to(DEV)
    x, r = _randn(rows, C, seed=C + 3) * 2.0 + 0.5, _randn(rows, C, seed=C + 4) * 1.5
    x[-1] = x[-1] * 0.125 - 6.0
    x[first_of_second_trip] = x[first_of_second_trip] * 3.0 + 4.0
    x, r = x.half().to(DEV), r.half().to(DEV)
    keep_x, keep_r = x.clone(), r.clone()
    for use_r in (False, True):
        xs = x.double() + (r.double() if use_r else 0.0)
        mean = xs.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(xs.var(-1, unbiased=False, keepdim=True) + eps)
        ref = (xs - mean) * rstd * gamma.double() + beta.double()
        bar = 16 * E * ((xs.abs() + mean.abs()) * rstd * gamma.double().abs() + beta.double().abs()) + 1e-6 + H11 * ref.abs()
        rounded = (x.float() + r.float()).half() if use_r else x
        for want_sum in (False, True):
            res = ops.unet_layernorm(x, gamma, beta, eps, residual=r if use_r else None, want_sum=want_sum)
            y, total = res if want_sum else (res, None)
            assert y.dtype == torch.float16 and y.shape == x.shape and y.is_contiguous()
            check("(e) layernorm C=%d rows=%d%s%s" % (C, rows, " + r" if use_r else "", " + sum_out" if want_sum else ""), y, ref, bar)
            if want_sum:
                assert torch.equal(total.view(torch.int16), rounded.view(torch.int16))           # x + r rounded ONCE
            again = ops.unet_layernorm(x, gamma, beta, eps, residual=r if use_r else None, want_sum=want_sum)
            assert torch.equal(y.view(torch.int16), (again[0] if want_sum else again).view(torch.int16))
            if want_sum:
                assert torch.equal(again[1].view(torch.int16), rounded.view(torch.int16))
    assert torch.equal(x, keep_x) and torch.equal(r, keep_r)                                     # the inputs are left unchanged


# ---------------------------------------------------------------------------------------------------------------
# (f) unet_geglu at K = 1280
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M_, inner", [(33, 640), (129, 5120)], ids=["M33_inner640", "M129_inner5120"])
def test_f_geglu_at_K1280(M_, inner):
    """40 ring steps; the reference, the bar, the both-tails assertion and the second run are test_gpu_unet_transformer.py's"""
    from test_gpu_unet_transformer import _geglu_against_float64
    assert M_ * inner >= 127 * 32                                   # the size from which the both-tails assertion is made
    _geglu_against_float64(M_, 1280, inner)
