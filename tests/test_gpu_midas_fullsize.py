"""The MiDaS detector past one grid pass and on the kernel forms a batch of 512 x 512 frames takes: the code paths of
csrc/midas.hip, csrc/pool3s2.h, of fresco_fn_gemm's / fresco_attn_f32's MiDaS-only forms and of fresco_amd/midas.py that the
small maps of tests/test_gpu_midas.py never reach.  Helpers and bars are those of tests/test_gpu_midas.py, imported and
unchanged; every comparison prints its worst error / bar; every input is seeded and every image of a batch has data of its
own.

  A  the streaming kernels past one pass of their grid-stride loop.  The grid is capped at 2048 blocks of 256 threads
     (STREAM_MAX_BLOCKS): everything past ONE_PASS = 524 288 work items runs in a later pass.  Smallest convenient shapes
     with a ragged second pass: midas_input, midas_groupnorm at all five widths (fp32, planes, far-border planes, plain and
     with residual; C = 128 and 512 also at the small shape), midas_pool, midas_tokens / midas_head_merge /
     midas_rowbias_gelu at L = 1025 (the 512 x 512 token count) with n = 3.  midas_layernorm (no such loop) at 769
     workgroups and at the widths 4, 260, 1020, 1024: one piece, a second round with one live lane, a last round four lanes
     short, every round full; each output alone bit-equal to the both-outputs run.
  B  the shared kernels in MiDaS's forms: q | k | v as one product with out_blocks = 36 at nine row blocks, every block
     bit-equal to a separate 64-column product; the chain product -> (head n, L, 64) views -> ops.attention_f32 at
     L = 1025 -> ops.midas_head_merge against the float64 Attention.forward arithmetic (from x, W and b, so the stacked
     weight order and the batch = head x n + image contract are part of it); the two readout gathers through a_rows
     (M = 3 and M = 3072 from one plane pair); fc1 with the GELU epilogue, planes only, and fc2 at K = 3072; the head's
     128 -> 32 3 x 3 and its 32 -> 1 product inside a poisoned buffer; layer 4's 768 -> 768 3 x 3 stride 2.
     Bar: 2^-20 sum |x| |w| + 1e-6 against float64 products of the same fp32 operands, planes + 2^-21 |y| (+ 2^-25).
  C  the tail: a minmax pass in which every thread reads one or two pixels, with the extremes placed where a skipped
     stride or a partial of the wrong frame changes every output value; two frames of 726 x 724 (the tail kernel's own
     second pass); the smallest legal sides; fp16, bf16 and fp32 conditions throughout.
  D  the range flag of every MiDaS producer (in range: silent; one value past 65000 / scale in the LAST row: raised; NaN:
     raised; no planes asked for: silent) and the detector's recomputation on library ops that the flag drives.
  E  eight 160 x 192 frames through the native detector: midas_input, the stem's GroupNorm apply and stage 0's C = 256
     apply take two passes.  max_frames = 1 keeps every kernel inside one pass and must give the same bits; the last frame
     is compared with DPTDepthModel.forward in float64 on the CPU at |got - f64| <= 4 x e_ref x peak per tap, e_ref the
     same module's fp32-vs-float64 distance computed here (taps at full width: the float64 forward of one frame takes
     under a second on the CPU).  forward() hands its taps out as fp32, so the float64 taps are rounded once (2^-24 |tap|, far
     below e_ref); the depth is compared in full float64.

Measured on an MI355X, worst error / bar (MEASURED below has every figure, DESIGN.md section 16 the table): A 0.015 - 0.150
and input 0.988 (its bar is the two roundings themselves), pool / tokens / head merge equal; B 0.062 - 0.293; C equal; E taps
0.167 - 0.283, depth 0.202, the batch bit-equal to frame-by-frame passes.  D found midas_pool silent on a NaN; fixed in
csrc/pool3s2.h.  A scratch build in which every grid-stride loop of midas.hip and pool3s2.h makes a single pass passes
tests/test_gpu_midas.py whole and fails here; with midas_minmax_kernel reading one pixel per thread as well, the old file
fails its two largest uint8-map cases and the new minmax tests fail too: see MUTANT below.
"""
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import midas_model as M
import test_gpu_egnet_conv as C
import test_gpu_midas as T
from test_gpu_midas import E, SCALE, _check, _conv_bound, _groupnorm_against_float64, _planes64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE_PASS = 2048 * 256  # work items of one pass of a streaming kernel's grid-stride loop (STREAM_MAX_BLOCKS blocks of 256 threads)
FN_BM = 256            # rows of a row block of fresco_fn_gemm
PLANE_FLOOR = 2.0 ** -25

# worst error / bar on an MI355X, 49 passed in 11 s
MEASURED = """
A  input 0.988 (the bar is the two roundings themselves), the same bits on a second run
   groupnorm past one pass, five widths x (plain, residual): fp32 0.115 - 0.150, planes 0.107 - 0.149, far-border planes equal
   groupnorm C = 128, 512 at (2, 18, 30): fp32 0.115 - 0.128, planes 0.107 - 0.149
   pool: fp32 equal to F.max_pool2d, planes 0.249; tokens equal; head merge equal, planes 0.250
   readout: fp32 0.075, planes 0.105; with another image's bias row every pass-two row would miss by 3.2e5 x the bar or more
   layernorm (3075, 768) 0.088; C = 4: 0.015, 260: 0.054, 1020: 0.029 (planes 0.036), 1024: 0.035 (planes 0.046); the
   single-output runs bit-equal to the both-outputs run
B  q | k | v in 36 blocks 0.230, 0 values differ from 36 separate 64-column products
   attention chain (max |ref| 9.65): fp32 0.062, planes 0.062; a swapped head and image order would miss by 4.9e4 x the bar
   readout gathers: cls rows (M = 3) 0.114, grid rows (M = 3072) 0.192
   fc1 + GELU, planes only 0.180; fc2 at K = 3072 0.293
   head 128 -> 32: fp32 rows 0.243, planes only 0.212 (a CPU fp32 conv2d: 0.019); 32 -> 1: 0.178, 0 guard floats overwritten
   layer 4's stride-2 convolution 0.132, last row 0.113, last column 0.116, planes 0.127
C  every depth-image, normal-image and condition value equal, at 3 x 160 x 192, 2 x 726 x 724, (2, 2, 2), (1, 2, 64),
   (1, 64, 2), for fp16, bf16 and fp32; without one of the placed extremes 94 - 100 % of that frame's depth image would change
D  every producer: silent in range, raised by one value in the last row and by a NaN, silent without planes.  midas_pool did
   NOT raise its flag on a NaN before this file (fmaxf drops it; csrc/pool3s2.h now ORs the NaN test of every value it reads
   into the flag).  The detector with a 2^14 decoder scale: one warning, 0 depth values differ from the library-ops run
E  batched vs max_frames = 1: 0 depth, depth-image and normal-image values differ; frame 7 against float64: stem 0.167,
   stage0 0.223, stage1 0.193, stage2 0.240, tokens0 0.224, tokens8 0.238, tokens11 0.248, layer3 0.254, layer4 0.240,
   path_4 0.257, path_3 0.257, path_2 0.236, path_1 0.283, depth 0.202 (e_ref 5e-7 - 9e-6 of the peak); tail equal
"""

# What two scratch builds gave on an MI355X (outputs past the first pass are never written there: the figures are those of
# whatever the allocator left).  Both leave outputs unwritten and fault nothing; both were built before the pool's NaN flag.
MUTANT = """
1. every grid-stride `for` of midas.hip and pool3s2.h a single pass (idx += total), midas_minmax_kernel as it is:
   tests/test_gpu_midas.py: 33 passed.
   tests/test_gpu_midas_fullsize.py: 19 failed, 3 errors, 27 passed --
     test_input_past_one_grid_pass                    worst error / bound 5.6e6
     test_groupnorm_past_one_grid_pass (all ten)      fp32 worst error / bound 6.3e5 - 5.2e6
     test_pool_past_one_grid_pass                     32 768 of 2 129 920 fp32 values differ from F.max_pool2d
     test_tokens_at_1025_tokens                       264 448 values differ
     test_head_merge_at_1025_tokens                   264 448 values differ
     test_readout_row_bias_at_1024_rows_per_image     worst error / bound 5.1e5
     test_tail_past_one_grid_pass (three dtypes)      the second-pass pixels of both maps
     test_range_flag_of_every_midas_producer[pool]    the NaN (the old pool, not the mutation)
     the three tests of E: the batched run trips the range flag on unwritten planes (a RuntimeWarning, an error there)
   passing: the (2, 18, 30) GroupNorm cases and LayerNorm (no such loop), B (planes from ops.fn_prep), the minmax and
   smallest-side tail tests, D.
2. the same plus one read per thread in midas_minmax_kernel (i += HW):
   tests/test_gpu_midas.py: 2 failed, 31 passed -- test_uint8_maps_match_the_record at 1 x 192 x 256 and 1 x 256 x 320
   (49 152 and 81 920 pixels for 16 384 minmax threads: largest difference 8 and 22).  The kernel test at 40 x 56 passes;
   the end-to-end record does see this one.
   tests/test_gpu_midas_fullsize.py: 24 failed, 24 passed (tokens and head merge were one test then) -- the failures of 1, and
     test_tail_minmax_where_every_thread_strides (three dtypes)  30 592 of 30 720 depth values and 5 800 normals of frame 0
     test_tail_past_one_grid_pass                                460 095 of 525 624 depth values of frame 0
     test_batch_of_eight_equals_frame_by_frame                   122 880 depth values of 245 760 differ
     test_last_frame_of_the_batch_matches_float64                stem at 4.7e5 x the bar
     test_tail_of_the_native_depth                               9 729 depth-image values of frame 1
"""

_gpu, _np64 = T._gpu, T._np64
gold, detector = T.gold, T.detector  # the module-scoped fixtures of tests/test_gpu_midas.py: the detector with stand-in weights


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------
# A. streaming kernels past one grid pass
# ---------------------------------------------------------------------------------------------------------------
def test_input_past_one_grid_pass():
    """x / 127.5 - 1 within one fp32 rounding of each of the two operations: |q| e + |r| e <= (|ref| + 1) e + |ref| e"""
    from fresco_amd import ops
    n, H, W = 2, 296, 300
    assert ONE_PASS < n * H * W * 3 < 2 * ONE_PASS  # 532 800
    assert (n * H * W - 2 * W) * 3 > ONE_PASS       # the last two rows of the last image lie in pass two
    x = np.random.RandomState(H * W).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    x[0, 0, :256, 2] = np.arange(256)    # all 256 byte values in pass one ...
    x[1, -2, -256:, 1] = np.arange(256)  # ... and in pass two
    x[1, -1, -1] = (0, 255, 128)
    got = ops.midas_input(_gpu(x))
    assert got.shape == (n, H, W, 3) and got.dtype == torch.float32
    ref = x.astype(np.float64) / 127.5 - 1.0
    bound = 2 * E * np.abs(ref) + E
    _check("input %s" % ((n, H, W),), _np64(got), ref, bound)
    last = got[1, -1, -1].cpu().numpy()
    assert last[0] == -1.0 and last[1] == 1.0 and abs(float(last[2]) - ref[1, -1, -1, 2]) <= bound[1, -1, -1, 2]
    assert torch.equal(ops.midas_input(_gpu(x)), got)  # the same bits on every run


GN_SHAPES = {64: (2, 130, 128), 128: (2, 92, 90), 256: (2, 66, 64), 512: (2, 46, 45), 1024: (2, 33, 32)}


@pytest.mark.parametrize("C_", sorted(GN_SHAPES), ids=lambda c: "C%d_cpg%d" % (c, c // 32))
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
def test_groupnorm_past_one_grid_pass(C_, residual):
    """fp32, planes and far-border planes (the pitch arithmetic ((img plane_h + py) plane_w + px) on second-pass pixels: the
    border row and column zero, the interior equal to the unbordered planes)"""
    n, H, W = GN_SHAPES[C_]
    assert ONE_PASS < n * H * W * (C_ // 4) < 2 * ONE_PASS
    _groupnorm_against_float64(n, H, W, C_, residual)


@pytest.mark.parametrize("C_", [128, 512], ids=lambda c: "C%d_cpg%d" % (c, c // 32))
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
def test_groupnorm_bottleneck_mid_widths_at_the_small_shape(C_, residual):
    """the mid widths of stages 1 and 2 (cpg 4 and 16) at tests/test_gpu_midas.py's shape: no stride involved"""
    _groupnorm_against_float64(2, 18, 30, C_, residual)


def test_pool_past_one_grid_pass():
    from fresco_amd import ops
    n, H, W = 2, 260, 256
    assert ONE_PASS < n * (H // 2) * (W // 2) * (64 // 4) < 2 * ONE_PASS  # 532 480
    x = -(_randn(n, H, W, 64, seed=H * W).abs() * 40.0 + 0.5)  # negative everywhere: padding must never win
    x[1] = x[1] * 0.125 - 3.0
    want = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1), value=float("-inf")), 3, 2).permute(0, 2, 3, 1).contiguous()
    assert want.shape == (n, H // 2, W // 2, 64) and float(want.max()) < 0
    out, planes = ops.midas_pool(x.to(DEV), want_f32=True)
    print("pool %s: %d of %d fp32 values differ from F.max_pool2d" % ((n, H, W), int((out.cpu() != want).sum()), want.numel()))
    assert torch.equal(out.cpu(), want)
    ref = want.double().numpy()
    _check("pool %s planes" % ((n, H, W),), _planes64(planes).reshape(ref.shape), ref, 2.0 ** -21 * np.abs(ref) + PLANE_FLOOR)
    none, again = ops.midas_pool(x.to(DEV))
    assert none is None and torch.equal(again[0], planes[0]) and torch.equal(again[1], planes[1])


def test_tokens_at_1025_tokens():
    n, L, C_ = 3, 1025, 768
    assert ONE_PASS < n * L * (C_ // 4) < 2 * ONE_PASS  # 590 400
    T._tokens_equal(n, L, C_)


def test_head_merge_at_1025_tokens():
    n, L, heads = 3, 1025, 12
    assert ONE_PASS < n * L * heads * 16 < 2 * ONE_PASS  # 590 400
    T._head_merge_equal(n, L, heads)


def test_readout_row_bias_at_1024_rows_per_image():
    """three images, bias rows 6 apart: pass two holds rows of the last image only, and their result lies within the bar of
    GELU(x + row 2) while GELU(x + row 0) and GELU(x + row 1) miss it by orders of magnitude in every such row"""
    n, rows, C_ = 3, 1024, 768
    assert ONE_PASS < n * rows * (C_ // 4) < 2 * ONE_PASS   # 589 824
    x, rb, out, ref, bound = T._readout_against_float64(n, rows, C_, spread=6.0)
    first = -(-ONE_PASS // (C_ // 4))  # the first row that lies in pass two as a whole
    assert (n - 1) * rows < first < n * rows
    got = _np64(out)[first:]
    assert np.all(np.abs(got - ref[first:]) <= bound[first:])
    for other in range(n - 1):
        wrong = F.gelu(x[first:].double() + rb[other].double()).numpy()
        miss = np.abs(wrong - ref[first:]).max(1) / bound[first:].max(1)
        print("readout pass two: with image %d's row the result would miss by %.3g x the bar at the least" % (other, miss.min()))
        assert miss.min() > 100.0


LN_CASES = [(3075, 768), (5, 4), (5, 260), (5, 1020), (5, 1024)]


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: "M%d_C%d" % c)
def test_layernorm_rows_and_widths(case):
    """(3075, 768): 769 workgroups, the last with three rows.  C = 4: one 16-byte piece; 260: a second round with one live lane;
    1020: the last round four lanes short; 1024: every round full.  The bar's 2^-18 term was derived for 768 adds and is
    looser for the narrow widths."""
    from fresco_amd import ops
    (x, gamma, beta), y, planes = T._layernorm_against_float64(*case)
    xg, gg, bg = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    only, none = ops.midas_layernorm(xg, gg, bg, eps=1e-6, want_f32=True, want_split=False)
    assert none is None and torch.equal(only, y)
    none, split = ops.midas_layernorm(xg, gg, bg, eps=1e-6, want_f32=False, want_split=True)
    assert none is None and torch.equal(split[0], planes[0]) and torch.equal(split[1], planes[1])


# ---------------------------------------------------------------------------------------------------------------
# B. the shared kernels in MiDaS's forms
# ---------------------------------------------------------------------------------------------------------------
def _weight_planes(w):
    from fresco_amd import ops
    return ops.fn_prep(w.to(DEV).contiguous(), scale=ops.FN_W_SCALE)[1]


def _guarded_gemm(*args, **kw):
    from fresco_amd import ops
    with ops.fn_range_guard(torch.device(DEV)) as guard:
        res = ops.fn_gemm(*args, **kw)
    assert not guard.tripped()
    return res


def _product_bar(x64, w64):
    return (2.0 ** -20 * (x64.abs() @ w64.abs().t()) + 1e-6).numpy()


@pytest.fixture(scope="module")
def qkv():
    """the stacked q | k | v product of a transformer block as DPTDepthModel._block runs it, n = 2 images of L = 1025 tokens,
    with its float64 result; image 1's rows lie well apart from image 0's.  Computed once."""
    from fresco_amd import ops
    n, L, K, N = 2, 1025, 768, 2304
    x = _randn(n * L, K, seed=36)
    x[L:] = x[L:] * 2.0 + 1.5
    w, b = _randn(N, K, seed=37) * 0.03, _randn(N, seed=38) * 0.1
    _, xp = ops.fn_prep(x.to(DEV))
    wp = _weight_planes(w)
    out, none = _guarded_gemm(xp, wp, N, K, bias=b.to(DEV), out_blocks=36)
    assert none is None
    ref = x.double() @ w.double().t() + b.double()
    return dict(n=n, L=L, K=K, N=N, x=x, w=w, b=b, xp=xp, wp=wp, out=out, ref=ref, bar=_product_bar(x.double(), w.double()))


def test_qkv_as_36_column_blocks(qkv):
    """M = 2050: nine row blocks -- eight in the XCD-ordered branch and one tail block; 36 column blocks of 64"""
    Mr, K = qkv["n"] * qkv["L"], qkv["K"]
    assert -(-Mr // FN_BM) == 9
    out = qkv["out"]
    assert out.shape == (36, Mr, 64) and out.dtype == torch.float32
    ref = qkv["ref"].reshape(Mr, 36, 64).permute(1, 0, 2).numpy()
    bar = qkv["bar"].reshape(Mr, 36, 64).transpose(1, 0, 2)
    _check("q | k | v in 36 blocks", _np64(out), ref, bar)
    differ = 0
    for j in range(36):
        wj = (qkv["wp"][0][64 * j:64 * j + 64], qkv["wp"][1][64 * j:64 * j + 64])
        sep, _ = _guarded_gemm(qkv["xp"], wj, 64, K, bias=qkv["b"][64 * j:64 * j + 64].to(DEV))
        assert sep.shape == (Mr, 64)
        differ += int((sep != out[j]).sum())
    print("q | k | v in 36 blocks: %d values differ from 36 separate 64-column products" % differ)
    assert differ == 0


def test_attention_chain_keeps_the_head_and_image_order(qkv):
    """product -> (heads n, L, 64) views -> attention_f32 -> head_merge, against Attention.forward's arithmetic in float64 up to
    (not including) proj.  L = 1025: one token past eight query blocks, one key past a whole tile."""
    from fresco_amd import ops
    n, L, heads = qkv["n"], qkv["L"], 12
    out = qkv["out"]
    q, k, v = (out[i * heads:(i + 1) * heads].view(heads * n, L, 64) for i in range(3))  # as DPTDepthModel._block does
    o = ops.attention_f32(q, k, v, 0.125)
    merged, planes = ops.midas_head_merge(o, n, want_f32=True, want_split=True)
    q64, k64, v64 = qkv["ref"].reshape(n, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    attn = ((q64 @ k64.transpose(-2, -1)) * 64 ** -0.5).softmax(dim=-1)
    ref = (attn @ v64).transpose(1, 2).reshape(n * L, heads * 64).numpy()
    bar = 2e-5 * max(1.0, float(np.abs(ref).max()))
    assert merged.shape == ref.shape
    _check("attention chain fp32 (max |ref| %.2f)" % np.abs(ref).max(), _np64(merged), ref, np.full_like(ref, bar))
    _check("attention chain planes", _planes64(planes), ref, bar + 2.0 ** -21 * np.abs(ref))
    # batch = image x heads + head in place of head x n + image: what a swapped order would hand on
    r4 = ref.reshape(n, L, heads, 64)
    b = np.arange(heads)[None, :] * n + np.arange(n)[:, None]  # (image, head) -> batch
    swapped = np.stack([np.stack([r4[b[i, h] // heads, :, b[i, h] % heads] for h in range(heads)], 1) for i in range(n)])
    miss = float(np.abs(swapped - r4).max()) / bar
    print("attention chain: a swapped head and image order would miss by %.3g x the bar" % miss)
    assert miss > 1000.0


def test_readout_gathers_through_row_tables():
    """ProjectReadout's two products from ONE (3 x 1025, 768) plane pair: the cls rows (M = 3, far below a row block) with the
    bias, and the grid rows in image order (M = 3072)"""
    from fresco_amd import ops
    n, L, K = 3, 1025, 768
    tok = _randn(n * L, K, seed=40) * 1.5
    tok[::L] = tok[::L] * 2.0 + 3.0  # the cls rows: unlike every grid row
    w_cls, w_tok, b = _randn(K, K, seed=41) * K ** -0.5, _randn(K, K, seed=42) * K ** -0.5, _randn(K, seed=43) * 0.1
    r = torch.arange(n * L, dtype=torch.int32, device=DEV).view(n, L)
    cls_rows, grid_rows = r[:, 0].contiguous(), r[:, 1:].reshape(-1).contiguous()
    _, tp = ops.fn_prep(tok.to(DEV))
    row, _ = _guarded_gemm(tp, _weight_planes(w_cls), K, K, bias=b.to(DEV), a_rows=cls_rows)
    g, _ = _guarded_gemm(tp, _weight_planes(w_tok), K, K, a_rows=grid_rows)
    assert row.shape == (n, K) and g.shape == (n * (L - 1), K)
    t64 = tok.double().view(n, L, K)
    _check("readout cls rows (M = 3)", _np64(row), (t64[:, 0] @ w_cls.double().t() + b.double()).numpy(),
           _product_bar(t64[:, 0], w_cls.double()))
    grid64 = t64[:, 1:].reshape(-1, K)
    _check("readout grid rows (M = 3072)", _np64(g), (grid64 @ w_tok.double().t()).numpy(), _product_bar(grid64, w_tok.double()))


def test_mlp_gelu_epilogue_and_k_3072():
    """fc1: K = 768, N = 3072, act = 2 (erf GELU), planes only; fc2: K = 3072, N = 768 on those planes"""
    from fresco_amd import ops
    Mr, K, N = 2050, 768, 3072
    x = _randn(Mr, K, seed=50)
    x[1025:] = x[1025:] * 1.5 - 0.5
    w1, b1 = _randn(N, K, seed=51) * (2.0 / K) ** 0.5, _randn(N, seed=52) * 0.1
    w2, b2 = _randn(K, N, seed=53) * N ** -0.5, _randn(K, seed=54) * 0.1
    _, xp = ops.fn_prep(x.to(DEV))
    none, hp = _guarded_gemm(xp, _weight_planes(w1), N, K, bias=b1.to(DEV), act=2, want_f32=False, want_split=True)
    assert none is None and hp[0].shape == (Mr, N) and hp[0].dtype == torch.float16
    pre = x.double() @ w1.double().t() + b1.double()
    ref = (0.5 * pre * (1.0 + torch.erf(pre * 0.5 ** 0.5))).numpy()
    h64 = _planes64(hp)
    _check("fc1 + GELU, planes only", h64, ref, _product_bar(x.double(), w1.double()) + 2.0 ** -21 * np.abs(ref))
    out, _ = _guarded_gemm(hp, _weight_planes(w2), K, N, bias=b2.to(DEV))
    h64 = torch.from_numpy(h64)
    _check("fc2 at K = 3072", _np64(out), (h64 @ w2.double().t() + b2.double()).numpy(), _product_bar(h64, w2.double()))


HEAD3 = (128, 32, 2, 40, 56, 3, 1, 1, 1)  # (cin, cout, n, H, W, k, stride, pad, dilation) of tests/test_gpu_egnet_conv.py
GUARD, POISON = 4096, -12345.0


def test_head_convolutions_and_the_one_column_product():
    """output_conv[2] (128 -> 32, 3 x 3, ReLU) as fp32 rows and as planes only, then output_conv[4] (32 -> 1, ReLU, fp32 only)
    from those planes: one output column, K = 32, written through out_f32 into the middle of a poisoned buffer -- "column
    blocks past N read the zero page and store nothing" """
    from fresco_amd import ops
    p = C._problem(HEAD3)
    bar = 2.0 ** -20 * p["S"] + 1e-6
    out, planes, tripped = C._convolve(HEAD3, True)
    assert planes is None and not tripped
    C._report(HEAD3, "fp32 rows", C._np64(out), bar)
    out, planes, tripped = C._convolve(HEAD3, False, SCALE, SCALE)
    assert out is None and not tripped
    a64 = _planes64(planes)
    C._report(HEAD3, "planes only", a64, bar + 2.0 ** -21 * np.abs(p["ref"]))

    Mr = a64.shape[0]
    w = (_randn(1, 32, seed=60).abs() * 32 ** -0.5)
    a64 = torch.from_numpy(a64)
    b = torch.tensor([-round(float((a64 @ w.double().t()).median()), 2)])  # the ReLU cuts about half of the column
    ref = F.relu(a64 @ w.double().t() + b.double()).numpy()
    assert (ref == 0).mean() > 0.1 and (ref > 0).mean() > 0.1
    buf = torch.full((Mr + 2 * GUARD,), POISON, dtype=torch.float32, device=DEV)
    got, none = _guarded_gemm(planes, _weight_planes(w), 1, 32, bias=b.to(DEV), act=1, want_f32=True, want_split=False,
                              out_f32=buf[GUARD:GUARD + Mr].view(Mr, 1))
    assert none is None and got.shape == (Mr, 1)
    host = buf.cpu()
    touched = int((host[:GUARD] != POISON).sum() + (host[GUARD + Mr:] != POISON).sum())
    print("32 -> 1 on %d rows: %d guard floats overwritten" % (Mr, touched))
    _check("head 32 -> 1", host[GUARD:GUARD + Mr].double().numpy()[:, None], ref, _product_bar(a64, w.double()))
    assert touched == 0


def test_layer4_stride2_conv_on_a_token_grid():
    """act_postprocess4[4]: 768 -> 768, 3 x 3, stride 2, symmetric padding 1, bias, no activation, fp32 rows and planes"""
    from fresco_amd import ops
    n, H, W, Cn = 2, 8, 6, 768
    x = _randn(n * H * W, Cn, seed=70) * 2.0
    x[H * W:] = x[H * W:] * 0.5 + 1.0
    w, b = _randn(Cn, Cn, 3, 3, seed=71) * (9 * Cn) ** -0.5, _randn(Cn, seed=72) * 0.1
    _, xp = ops.fn_prep(x.to(DEV))
    wp = _weight_planes(w.permute(0, 2, 3, 1).reshape(Cn, -1))
    got, planes = _guarded_gemm(xp, wp, Cn, 9 * Cn, bias=b.to(DEV), conv=(n, H, W, 3, 3, 2, 1), want_f32=True, want_split=True)
    x64, w64 = x.double().view(n, H, W, Cn).permute(0, 3, 1, 2), w.double()
    ref = F.conv2d(x64, w64, b.double(), 2, padding=1).permute(0, 2, 3, 1).numpy()
    assert ref.shape == (n, 4, 3, Cn)
    bound = _conv_bound(x64, w64, 2, (1, 1, 1, 1))
    got = _np64(got).reshape(ref.shape)
    _check("layer 4 conv", got, ref, bound)
    _check("layer 4 conv last row", got[:, -1], ref[:, -1], bound[:, -1])
    _check("layer 4 conv last column", got[:, :, -1], ref[:, :, -1], bound[:, :, -1])
    _check("layer 4 conv planes", _planes64(planes).reshape(ref.shape), ref, bound + 2.0 ** -21 * np.abs(ref))


# ---------------------------------------------------------------------------------------------------------------
# C. the tail
# ---------------------------------------------------------------------------------------------------------------
COND_DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def _minmax_frames():
    """three frames of 160 x 192 = 30 720 pixels: the 16 384 threads of a frame's minmax pass read one or two each.
    frame 0: minimum at the very last pixel, maximum at pixel 16 384, the first one of the second stride; frame 1: both in
    the first row, a much larger range; frame 2: maximum at the last pixel"""
    H, W = 160, 192
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    rs = np.random.RandomState(11)
    f0 = (12.0 + 3.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 0.2 * rs.rand(H, W)).astype(np.float32)
    f0.reshape(-1)[-1] = 2.0
    f0.reshape(-1)[16384] = 31.0
    f1 = (800.0 + 300.0 * np.cos(xx / 11.0 + yy / 5.0) + 20.0 * rs.rand(H, W)).astype(np.float32)
    f1[0, 5], f1[0, 150] = -500.0, 4000.0
    f2 = (5.0 + 0.02 * yy + 0.01 * xx + 0.5 * rs.rand(H, W)).astype(np.float32)
    f2[40:70, 30:90] = 4.0
    f2.reshape(-1)[-1] = 40.0
    return np.stack([f0, f1, f2])


@pytest.mark.parametrize("dtype", COND_DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_tail_minmax_where_every_thread_strides(dtype):
    d = _minmax_frames()
    HW = d[0].size
    assert 64 * 256 < HW < 2 * 64 * 256
    assert d[0].argmin() == HW - 1 and d[0].argmax() == 16384 and d[1].argmin() < 192 and d[1].argmax() < 192
    assert d[2].argmax() == HW - 1 and np.ptp(d[1]) > 100 * np.ptp(d[0])
    dimg, _ = T._tail_against_numpy(d, dtype)
    # each extreme moves the whole map: without it (the next value in its place) most depth values change
    for f, idx in ((0, HW - 1), (0, 16384), (2, HW - 1)):
        e = d[f].copy()
        e.reshape(-1)[idx] = np.median(e)
        changed = float((M.tail(e)[0] != dimg[f].cpu().numpy()).mean())
        print("tail minmax: without frame %d's extreme at pixel %d, %.0f %% of its depth image would change" % (f, idx, 100 * changed))
        assert changed > 0.5


def _big_tail_frames():
    """two frames of 726 x 724 = 525 624 pixels: 1 336 of each frame's pixels run in the tail kernel's second pass.  Smooth,
    plus noise, plus a region below bg_th; the second frame's last rows and column carry a pattern of their own"""
    H, W = 726, 724
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    rs = np.random.RandomState(13)
    f0 = (6.0 + 4.0 * np.sin(xx / 37.0) * np.cos(yy / 29.0) + 0.05 * rs.standard_normal((H, W))).astype(np.float32)
    f0[100:300, 200:500] = 0.5
    f1 = (30.0 + 0.02 * xx + 0.03 * yy + 2.0 * rs.rand(H, W)).astype(np.float32)
    f1[400:500, 50:350] = 12.0
    f1[-2, :] = (20.0 + 25.0 * (np.arange(W) * 7 % 23) / 23.0).astype(np.float32)
    f1[-1, :] = (20.0 + 25.0 * (np.arange(W) ** 2 % 97) / 97.0).astype(np.float32)
    f1[:, -1] = (15.0 + 40.0 * (np.arange(H) % 13) / 13.0).astype(np.float32)
    return np.stack([f0, f1])


@pytest.mark.parametrize("dtype", COND_DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_tail_past_one_grid_pass(dtype):
    d = _big_tail_frames()
    assert ONE_PASS < d[0].size < 2 * ONE_PASS
    dimg, nimg = T._tail_against_numpy(d, dtype)
    dn, nn = dimg.cpu().numpy(), nimg.cpu().numpy()
    assert (dn[0, 100:300, 200:500] == 0).all() and (nn[0, 102:298, 202:498] == (127, 127, 255)).all()  # below bg_th: masked
    assert len(np.unique(dn[1, -1])) > 8 and len(np.unique(nn[1, -1].reshape(-1, 3), axis=0)) > 8  # pass two is no constant


@pytest.mark.parametrize("shape", [(2, 2, 2), (1, 2, 64), (1, 64, 2)], ids=lambda s: "%dx%dx%d" % s)
def test_tail_at_the_smallest_sides(shape):
    """H or W = 2: reflect-101 folds row -1 and row 2 onto the other row"""
    d = (3.0 + 10.0 * np.random.RandomState(sum(shape)).rand(*shape)).astype(np.float32)
    for dtype in COND_DTYPES:
        _, nimg = T._tail_against_numpy(d, dtype)
    if max(shape[1:]) > 2:  # (on a 2 x 2 frame every tap pair folds onto one pixel: all gradients are zero)
        assert len(np.unique(nimg.cpu().numpy().reshape(-1, 3), axis=0)) > 1


# ---------------------------------------------------------------------------------------------------------------
# D. range flags
# ---------------------------------------------------------------------------------------------------------------
BIG = 1016.0  # 1016 * 64 = 65024 > 65000


def _flag_groupnorm(far_border):
    from fresco_amd import ops
    n, H, W, Cn = 2, 18, 30, 64
    x = (_randn(n, H, W, Cn, seed=80) * 3.0).to(DEV)
    gamma, beta = torch.ones(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    res = _randn(n, H, W, Cn, seed=81).to(DEV)
    big = res.clone()
    big[-1, -1, -1, -1] = 2000.0  # relu(norm + 2000) > 1016: exactly one output value, the last one
    nan = x.clone()
    nan[-1, -1, -1, -1] = float("nan")  # a NaN in the input reaches every output of its group (no ReLU: fmaxf drops a NaN)

    def run(x_, res_, want_split=True, relu=False):
        return ops.midas_groupnorm(x_, gamma, beta, relu=relu, residual=res_, want_f32=not want_split, want_split=want_split,
                                   far_border=far_border and want_split)
    return run, dict(ok=(x, res), big=(x, big), nan=(nan, None))


def _flag_pool():
    from fresco_amd import ops
    x = (_randn(2, 20, 24, 64, seed=82) * 40.0).to(DEV)
    big = x.clone()
    big[-1, -1, -1, -1] = BIG
    nan = x.clone()
    nan[-1, -1, -1, -1] = float("nan")
    return (lambda x_, want_split=True: ops.midas_pool(x_)), dict(ok=(x,), big=(big,), nan=(nan,))


def _flag_layernorm():
    """the last row holds one outlier: its normalised value is about sqrt(767) = 27.7, times gamma = 40 on that channel"""
    from fresco_amd import ops
    Mr, Cn = 37, 768
    x = _randn(Mr, Cn, seed=83).to(DEV)
    gamma, beta = torch.ones(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    gamma[5] = 40.0
    big = x.clone()
    big[-1, 5] = 1e4
    nan = x.clone()
    nan[-1, 5] = float("nan")

    def run(x_, want_split=True):
        return ops.midas_layernorm(x_, gamma, beta, want_f32=not want_split, want_split=want_split)
    return run, dict(ok=(x,), big=(big,), nan=(nan,))


def _flag_head_merge():
    from fresco_amd import ops
    n, heads, L = 2, 12, 25
    o = (_randn(heads * n, L, 64, seed=84) * 20.0).to(DEV)
    big = o.clone()
    big[-1, -1, -1] = BIG  # the last head of the last image's last token: the last value of the last output row
    nan = o.clone()
    nan[-1, -1, -1] = float("nan")

    def run(o_, want_split=True):
        return ops.midas_head_merge(o_, n, want_f32=not want_split, want_split=want_split)
    return run, dict(ok=(o,), big=(big,), nan=(nan,))


def _flag_rowbias_gelu():
    from fresco_amd import ops
    n, rows, Cn = 3, 24, 768
    x, rb = (_randn(n * rows, Cn, seed=85) * 2.0).to(DEV), (_randn(n, Cn, seed=86) * 2.0).to(DEV)
    big = x.clone()
    big[-1, -1] = BIG + 20.0  # GELU(t) = t out here, and |bias| stays far below 20
    nan = x.clone()
    nan[-1, -1] = float("nan")

    def run(x_, want_split=True):
        return ops.midas_rowbias_gelu(x_, rb, rows, want_f32=not want_split, want_split=want_split)
    return run, dict(ok=(x,), big=(big,), nan=(nan,))


PRODUCERS = {"groupnorm": lambda: _flag_groupnorm(False), "groupnorm_far_border": lambda: _flag_groupnorm(True),
             "pool": _flag_pool, "layernorm": _flag_layernorm, "head_merge": _flag_head_merge,
             "rowbias_gelu": _flag_rowbias_gelu}


@pytest.mark.parametrize("name", sorted(PRODUCERS))
def test_range_flag_of_every_midas_producer(name):
    """silent in range; raised by ONE value past 65000 / scale in the last row (a flag OR that only the first wave performs
    would miss it); raised by a NaN; silent when no planes are asked for (midas_pool always writes planes)"""
    from fresco_amd import ops
    run, data = PRODUCERS[name]()
    dev = torch.device(DEV)
    with ops.fn_range_guard(dev) as guard:
        _, planes = run(*data["ok"])
    assert not guard.tripped()
    assert float(planes[0].float().abs().max()) < 64000.0
    with ops.fn_range_guard(dev) as guard:
        _, planes = run(*data["big"])
    assert guard.tripped(), "one value past the range"
    hi = planes[0].float().abs()  # 65000 is 64992 in fp16
    assert int((hi >= 64000.0).sum()) == 1  # exactly one value saturated ...
    if name != "groupnorm_far_border":      # ... in the last row (there the last rows are the zero border)
        assert float(hi.reshape(-1, hi.shape[-1])[-1].max()) >= 64000.0
    with ops.fn_range_guard(dev) as guard:
        run(*data["nan"])
    assert guard.tripped(), "a NaN"
    if name != "pool":
        for key in ("big", "nan"):
            with ops.fn_range_guard(dev) as guard:
                out, none = run(*data[key], want_split=False)
            assert none is None and out is not None and not guard.tripped(), key


def test_detector_recomputes_on_library_ops_when_a_stage_overflows(detector):
    """the decoder's planes written with 2^14 hold |x| < 4: its producers raise the flag, depth() warns once and hands back
    the library-ops result.  PyTorch's own convolutions are not bit-stable from call to call on this GPU by default (two
    library-ops runs of these frames differ in 11 700 of 12 288 depth values, in the last digits, from stage 1 on), so the
    comparison runs under torch.backends.cudnn.deterministic, where they are."""
    import fresco_amd
    net = fresco_amd.DPTDepthModel(split_scales=(64, 64, 64, 2.0 ** 14))
    net.load_state_dict(detector.model.state_dict(), strict=True)
    net = net.float().to(DEV).eval()
    fr = _gpu(M.frames((2, 64, 96)))
    saved, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        with pytest.warns(RuntimeWarning, match="left the range") as rec:
            first = net.depth(fr)
        assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1 and net._warned
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            second = net.depth(fr)  # recomputed again, silently
        net.library_ops = True
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            lib = net.depth(fr)
    finally:
        torch.backends.cudnn.deterministic = saved
    print("overflowing decoder: %d and %d depth values differ from the library-ops run"
          % (int((first != lib).sum()), int((second != lib).sum())))
    assert torch.equal(first, lib) and torch.equal(second, lib)
    assert not detector.model._warned


# ---------------------------------------------------------------------------------------------------------------
# E. a batch that strides inside the detector
# ---------------------------------------------------------------------------------------------------------------
BATCH = (8, 160, 192)
REF_FRAME = BATCH[0] - 1


@pytest.fixture(scope="module")
def batch_run(detector):
    """(frames, taps, depth, depth images, normal images) of ONE batched native run, warnings as errors"""
    fr = _gpu(M.frames(BATCH))
    taps = {}
    assert detector.model.max_frames >= BATCH[0]  # one chunk
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no range trip: the native path computed this
        depth = detector.model.depth(fr, taps)
        dimg, nimg = detector.detect_batch(fr)
    return fr, taps, depth, dimg, nimg


def test_batch_of_eight_equals_frame_by_frame(detector, batch_run):
    """batched: midas_input, the stem's GroupNorm apply and stage 0's C = 256 apply take two passes; one frame per pass stays
    inside one pass of every kernel, so this pins the later passes against the first"""
    n, H, W = BATCH
    assert ONE_PASS < n * H * W * 3 < 2 * ONE_PASS                       # midas_input: 737 280
    assert ONE_PASS < n * (H // 2) * (W // 2) * (64 // 4) < 2 * ONE_PASS   # the stem's GroupNorm apply: 983 040
    assert ONE_PASS < n * (H // 4) * (W // 4) * (256 // 4) < 2 * ONE_PASS  # stage 0's C = 256 apply: 983 040
    assert H * W * 3 < ONE_PASS and (H // 2) * (W // 2) * 16 < ONE_PASS
    fr, _, depth, dimg, nimg = batch_run
    saved, detector.model.max_frames = detector.model.max_frames, 1
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            depth1 = detector.model.depth(fr)
            dimg1, nimg1 = detector.detect_batch(fr)
    finally:
        detector.model.max_frames = saved
    print("%s batched vs max_frames = 1: %d depth values, %d depth-image and %d normal-image values differ"
          % (M.case_key(BATCH), int((depth1 != depth).sum()), int((dimg1 != dimg).sum()), int((nimg1 != nimg).sum())))
    assert torch.equal(depth1, depth) and torch.equal(dimg1, dimg) and torch.equal(nimg1, nimg)


def test_last_frame_of_the_batch_matches_float64(detector, batch_run):
    """|got - f64| <= 4 x e_ref x peak for every tap at full width and for the depth; e_ref x peak = max |fp32 - f64| of this
    package's module on the CPU (the golden file's rule with the noise computed here)"""
    import fresco_amd
    fr, taps, depth, _, _ = batch_run
    assert list(taps) == list(M.TAPS)
    n32 = fresco_amd.DPTDepthModel()
    n32.load_state_dict({k: v.cpu() for k, v in detector.model.state_dict().items()}, strict=True)
    n32 = n32.float().eval()
    n64 = copy.deepcopy(n32).double()
    one = fr[REF_FRAME:REF_FRAME + 1].cpu().numpy()
    runs = []
    with torch.no_grad():
        for net, dtype in ((n32, torch.float32), (n64, torch.float64)):
            t = {}
            d = net(M.network_input(one, dtype), t)
            runs.append([t[name].double().numpy() for name in M.TAPS] + [d.double().numpy()])
    worst = []
    for name, f32, f64 in zip(M.TAPS + ("depth",), *runs):
        got = _np64(depth if name == "depth" else taps[name])
        assert got.shape[0] == BATCH[0], (name, got.shape)
        got = got[REF_FRAME:REF_FRAME + 1]
        assert got.shape == f64.shape, (name, got.shape, f64.shape)
        peak = float(np.abs(f64).max())
        noise = float(np.abs(f32 - f64).max())
        ratio = float(np.abs(got - f64).max()) / (4 * noise)
        print("%s frame %d %-8s |got - f64| / (4 x e_ref %.2e x peak %.3g) = %.3f" % (M.case_key(BATCH), REF_FRAME, name,
                                                                                    noise / peak, peak, ratio))
        worst.append((ratio, name))
    assert max(worst)[0] <= 1.0, max(worst)


def test_tail_of_the_native_depth(batch_run):
    _, _, depth, dimg, nimg = batch_run
    d2, n2 = T._tail_against_numpy(depth.cpu().numpy(), torch.float16)
    assert torch.equal(d2, dimg) and torch.equal(n2, nimg)
