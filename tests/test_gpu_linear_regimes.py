"""The fused projection kernel (fresco_linear, fp16 and bf16) against an fp64 product of the same 16-bit operands, in every
loop regime of the kernel: one feature tile per workgroup (the only regime tests/test_gpu_linear.py reaches), several tiles
(in-loop weight staging, the 3-slot ring wrapping, the output cursor moving from one output to the next inside a workgroup),
splits that begin inside an output, run across two or three outputs, a last split shorter than the others, and the LDS plan
at its last byte.  Which regime a shape lands in is asked of the library (fresco_linear_plan), never assumed: a case whose
shape stops landing in the regime it is named for fails and has to move its M.

The bar is derived, not measured.  p = 11 (fp16) or 8 (bf16); A = |x| |W|^T + |b| in fp64.  Products of two 16-bit numbers
are exact in fp32; any fp32 summation order of K of them plus the bias errs by at most E = K u A; the one rounding to the
output type adds at most 2^-p |s|.  So, per element,

    |out - ref| <= 2^-p (|ref| + E) + E + 2^-25           (2^-25: half an fp16 subnormal step)

u is the unit roundoff of the MFMA's fp32 accumulation: U = 2^-24 (round to nearest) holds on the MI355X.  It was settled by
putting torch's own matmul (the library, not the kernel under test) through the same bar at the two variant shapes below:
its worst |err| / bar is 0.877 (fp16, K = 320), 0.746 (fp16, K = 640), 0.971 (bf16, K = 320), 0.949 (bf16, K = 640), nowhere
over the bar, so the truncating value 2^-23 is not needed; test_library_matmul_meets_the_same_bar keeps that check.

Every output is a view into one buffer prefilled with a NaN bit pattern, with 3 rows below row M - 1 and 8 columns between
and behind the outputs: after a launch every fence element still holds the pattern and no output element does.  An exact
case (operands in {-1, 0, 1}, integer biases: every sum is an integer both types hold) needs no bar at all, and launches of
the same rows in two different regimes must agree bit for bit (per element the accumulation order depends on K alone)."""
import functools

import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
P = {torch.float16: 11, torch.bfloat16: 8}
DTYPES = [torch.float16, torch.bfloat16]
SENTINEL = 0x7FAD  # a NaN in fp16 and in bf16
FENCE_ROWS, FENCE_COLS = 3, 8
M_MAX = 65536


def _name(dt):
    return "fp16" if dt == torch.float16 else "bf16"


# ---- inputs: generated once on the CPU, moved once, never written ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _x(K, dt, exact=False):
    g = synth.gen(1000 + K + exact)
    if exact:
        x = torch.randint(-1, 2, (M_MAX, K), generator=g) * (torch.rand(M_MAX, K, generator=g) < 0.375)
        return x.to(dt).to(DEV)  # (P(nonzero) = 2/3 * 3/8 = 1/4)
    return torch.randn(M_MAX, K, generator=g).to(dt).to(DEV)


@functools.lru_cache(maxsize=None)
def _wb(K, N, nw, dt, exact=False):
    """(weights, biases): nw tensors each, separately allocated"""
    g = synth.gen(2000 + K + N + nw + exact)
    if exact:
        W = torch.randint(-1, 2, (nw * N, K), generator=g) * (torch.rand(nw * N, K, generator=g) < 0.375)
        b = torch.randint(-8, 9, (nw * N,), generator=g)
    else:
        W = torch.randn(nw * N, K, generator=g) / K ** 0.5
        b = torch.randn(nw * N, generator=g)
    Ws = [w.to(dt).contiguous().to(DEV) for w in W.chunk(nw, 0)]
    bs = [t.to(dt).contiguous().to(DEV) for t in b.chunk(nw, 0)]
    return Ws, bs


# ---- which regime a shape lands in: asked of the library -----------------------------------------------------------
def _regime(nw, M, N, K):
    import fresco_amd.ops as ops
    rc, row_blocks, splits, tps = ops.linear_plan(nw, M, N, K)
    assert rc == 0, rc
    nF, tpo = nw * N // 64, N // 64
    rng = [(s * tps, min(nF, (s + 1) * tps)) for s in range(splits)]
    assert rng[-1][1] == nF and rng[-1][0] < nF
    return dict(row_blocks=row_blocks, splits=splits, tps=tps, steps=tps * (K // 160),
                straddle=[s for s, (a, b) in enumerate(rng) if a // tpo != (b - 1) // tpo],
                mid=[s for s, (a, b) in enumerate(rng) if a % tpo],
                last=rng[-1][1] - rng[-1][0],
                spans=max((b - 1) // tpo - a // tpo + 1 for a, b in rng))


def _fmt(r):
    return "grid %d x %d, tps %d (%d steps), last split %d, straddling %s, begin mid-output %s, outputs per split <= %d" % (
        r["row_blocks"], r["splits"], r["tps"], r["steps"], r["last"], r["straddle"], r["mid"][:4], r["spans"])


def _assert_regime(r, need):
    for key, want in need.items():
        if key in ("tps", "splits", "spans", "last"):
            assert r[key] == want, (key, want, r)
        elif key == "min_tps":
            assert r["tps"] >= want, (key, want, r)
        elif key in ("straddle", "mid"):
            assert bool(r[key]) == want, (key, want, r)
        elif key == "short_last":
            assert (r["last"] < r["tps"]) == want, (key, want, r)
        else:
            raise KeyError(key)


# ---- poisoned, fenced outputs ---------------------------------------------------------------------------------------
def _fenced(M, N, nw, dt):
    buf = torch.full((M + FENCE_ROWS, nw * (N + FENCE_COLS)), SENTINEL, dtype=torch.int16, device=DEV).view(dt)
    return buf, [buf[:M, j * (N + FENCE_COLS):j * (N + FENCE_COLS) + N] for j in range(nw)]


def _check_fences(buf, M, N, nw):
    bits = buf.view(torch.int16).clone()
    for j in range(nw):
        o = bits[:M, j * (N + FENCE_COLS):j * (N + FENCE_COLS) + N]
        left = int((o == SENTINEL).sum())
        assert left == 0, "output %d: %d elements were never written" % (j, left)
        o.fill_(SENTINEL)
    touched = int((bits != SENTINEL).sum())
    assert touched == 0, "%d fence elements (rows >= M or the 8 columns behind an output) were written" % touched


def _launch(x, Ws, bs, dt, x_rows=None):
    import fresco_amd.ops as ops
    M = x.shape[0] if x_rows is None else x_rows.numel()
    N, nw = Ws[0].shape[0], len(Ws)
    buf, outs = _fenced(M, N, nw, dt)
    got = ops.linear(x, Ws, bs, outs=outs, x_rows=x_rows)
    assert all(g is o for g, o in zip(got, outs))
    _check_fences(buf, M, N, nw)
    return buf, outs


# ---- the reference and the bar ---------------------------------------------------------------------------------------
def _ref_chunks(x, Ws, bs):
    """(r0, r1, [(ref, A)] per output), fp64 on the device, 8192 rows at a time"""
    Wd = [W.double() for W in Ws]
    for r0 in range(0, x.shape[0], 8192):
        xs = x[r0:r0 + 8192].double()
        xa = xs.abs()
        res = []
        for W, b in zip(Wd, bs or [None] * len(Ws)):
            ref, A = xs @ W.t(), xa @ W.abs().t()
            if b is not None:
                ref, A = ref + b.double(), A + b.double().abs()
            res.append((ref, A))
        yield r0, r0 + xs.shape[0], res


def _worst_fraction(x, Ws, bs, outs, dt, u=U):
    """max over all elements of |out - ref| / bar, and the number of elements over the bar"""
    K, p = x.shape[1], P[dt]
    worst = torch.zeros((), dtype=torch.float64, device=DEV)
    over = torch.zeros((), dtype=torch.int64, device=DEV)
    for r0, r1, res in _ref_chunks(x, Ws, bs):
        for (ref, A), o in zip(res, outs):
            E = K * u * A
            bar = 2.0 ** -p * (ref.abs() + E) + E + 2.0 ** -25
            frac = torch.nan_to_num((o[r0:r1].double() - ref).abs() / bar, nan=float("inf"))
            worst = torch.maximum(worst, frac.max())
            over += (frac > 1.0).sum()
    return float(worst), int(over)


def _check(what, x, Ws, bs, outs, dt, regime=None):
    worst, over = _worst_fraction(x, Ws, bs, outs, dt)
    print("%s %s: plan %s; worst |err| / bar = %.3f" % (what, _name(dt), _fmt(regime) if regime else "-", worst))
    assert worst <= 1.0, "%s: worst |err| / bar = %.3f, %d elements over the bar" % (what, worst, over)


# ---- the regimes ----------------------------------------------------------------------------------------------------
# (name, K, N, nw, M, bias, what the plan must say); the long walks carry biases (bias_s + j * N + col over many cursor
# steps), the short ones do not (the kernel skips the bias read altogether): the variants below mix them
CASES = [
    ("one-tile", 320, 320, 3, 1000, False, dict(tps=1)),
    ("two-tiles-ring-wraps", 320, 320, 3, 4700, False, dict(tps=2, straddle=True, short_last=True, last=1)),
    ("three-tiles-mid-output", 320, 320, 3, 13100, False, dict(tps=3, straddle=True, mid=True)),
    ("eight-tiles-ragged", 320, 320, 3, 32769, True, dict(tps=8, splits=2, last=7, straddle=True, spans=2)),
    ("one-split-three-outputs", 320, 320, 3, 65281, True, dict(tps=15, splits=1, spans=3)),
    ("k640-two-tiles", 640, 640, 3, 2400, False, dict(tps=2)),
    ("k640-straddle", 640, 640, 3, 6500, False, dict(tps=3, straddle=True, mid=True)),
    ("k640-two-outputs-short-last", 640, 640, 2, 8500, False, dict(tps=3, last=2, straddle=True)),
    ("k640-one-split", 640, 640, 3, 65535, True, dict(tps=30, splits=1, spans=3)),
    ("to-out", 320, 320, 1, 65536, True, dict(tps=5, splits=1, spans=1)),
    ("n64-cursor-every-tile", 320, 64, 3, 45000, True, dict(tps=2, splits=2, spans=2)),
    ("lds-last-byte-1x2048", 320, 2048, 1, 3000, False, dict(tps=2)),
    ("lds-last-byte-2x1024", 320, 1024, 2, 3000, False, dict(tps=2)),
]
# the multi-tile cases the variants below are applied to: (K, N, nw, M)
V320 = (320, 320, 3, 4700)   # tps 2: split 2 straddles out0 | out1
V640 = (640, 640, 3, 6500)   # tps 3: straddling, splits beginning inside an output


def _variant(shape):
    K, N, nw, M = shape
    r = _regime(nw, M, N, K)
    _assert_regime(r, dict(min_tps=2, straddle=True))
    return K, N, nw, M, r


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("name,K,N,nw,M,bias,need", CASES, ids=[c[0] for c in CASES])
def test_regime(name, K, N, nw, M, bias, need, dt):
    r = _regime(nw, M, N, K)
    _assert_regime(r, need)
    if nw * N == 2048:
        import fresco_amd.ops as ops
        assert ops.linear_plan(nw, M, N + 64, K)[0] != 0  # one more tile of bias does not fit
    x = _x(K, dt)[:M]
    Ws, bs = _wb(K, N, nw, dt)
    bs = bs if bias else None
    _, outs = _launch(x, Ws, bs, dt)
    _check(name, x, Ws, bs, outs, dt, r)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [V320, V640], ids=["k320", "k640"])
@pytest.mark.parametrize("which", [(0, 1, 2), (1,), (0, 2)], ids=["all", "mid-only", "outer-only"])
def test_bias_on_outputs_of_a_multi_tile_split(shape, which, dt):
    K, N, nw, M, r = _variant(shape)
    x = _x(K, dt)[:M]
    Ws, bs = _wb(K, N, nw, dt)
    bs = [b if j in which else None for j, b in enumerate(bs)]
    _, outs = _launch(x, Ws, bs, dt)
    _check("bias on %s" % (which,), x, Ws, bs, outs, dt, r)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [V320, V640], ids=["k320", "k640"])
@pytest.mark.parametrize("layout", ["reversed", "apart"])
def test_weight_placement(shape, layout, dt):
    """W1 - W0 and W2 - W0 negative (the three weights carved out of one buffer in reverse address order), and positive
    with an unrelated tensor in between"""
    K, N, nw, M, r = _variant(shape)
    x = _x(K, dt)[:M]
    Ws, bs = _wb(K, N, nw, dt)
    gap = 1024 + 8  # elements: keeps every weight 16-byte aligned
    pool = torch.full((nw * (N * K + gap),), 3.0e4, dtype=dt, device=DEV)  # what a wrong slab address would read
    order = list(reversed(range(nw))) if layout == "reversed" else list(range(nw))
    placed = [None] * nw
    for slot, j in enumerate(order):
        w = pool[slot * (N * K + gap):slot * (N * K + gap) + N * K].view(N, K)
        w.copy_(Ws[j])
        placed[j] = w
    ptrs = [w.data_ptr() for w in placed]
    assert ptrs == sorted(ptrs, reverse=(layout == "reversed")) and all(p % 16 == 0 for p in ptrs)
    _, outs = _launch(x, placed, bs, dt)
    _check("weights %s" % layout, x, Ws, bs, outs, dt, r)
    _, same = _launch(x, Ws, bs, dt)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(outs, same))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [V320, V640], ids=["k320", "k640"])
def test_gathered_rows_multi_tile(shape, dt):
    """an unsorted table with repeats, shorter than x, bit-equal to gathering first"""
    K, N, nw, M, r = _variant(shape)
    Mx = M + 1500
    x = _x(K, dt)[:Mx]
    rows = torch.randint(0, M + 300, (M,), generator=synth.gen(K)).to(torch.int32)
    assert len(set(rows.tolist())) < M and not bool((rows[1:] >= rows[:-1]).all()) and int(rows.max()) < Mx - 1
    rows = rows.to(DEV)
    Ws, bs = _wb(K, N, nw, dt)
    _, outs = _launch(x, Ws, bs, dt, x_rows=rows)
    xs = x.index_select(0, rows.long())
    _check("gathered", xs, Ws, bs, outs, dt, r)
    _, plain = _launch(xs, Ws, bs, dt)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(outs, plain))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [V320, V640], ids=["k320", "k640"])
def test_strided_input_multi_tile(shape, dt):
    """x is a column slice of a tensor twice as wide (row stride 2K); the other half would poison the sums"""
    K, N, nw, M, r = _variant(shape)
    wide = torch.full((M, 2 * K), 3.0e4, dtype=dt, device=DEV)
    x = wide[:, K:]
    x.copy_(_x(K, dt)[:M])
    assert x.stride(0) == 2 * K
    Ws, bs = _wb(K, N, nw, dt)
    _, outs = _launch(x, Ws, bs, dt)
    _check("strided x", x, Ws, bs, outs, dt, r)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("K,N,base", [(320, 320, 4608), (640, 640, 2304)], ids=["k320", "k640"])
@pytest.mark.parametrize("rem", [1, 31, 33, 255])
def test_ragged_last_row_block_multi_tile(K, N, base, rem, dt):
    """M mod 256 = rem: at 1 and 31 whole waves of the last workgroup lie beyond M; the 3 fence rows catch their stores"""
    M, nw = base + rem, 3
    assert M % 256 == rem
    r = _regime(nw, M, N, K)
    _assert_regime(r, dict(min_tps=2))
    x = _x(K, dt)[:M]
    Ws, bs = _wb(K, N, nw, dt)
    _, outs = _launch(x, Ws, bs, dt)
    _check("M %% 256 = %d" % rem, x, Ws, bs, outs, dt, r)


# ---- no bar at all ---------------------------------------------------------------------------------------------------
EXACT = [(320, 320, 3, 65281, dict(tps=15, splits=1)), (640, 640, 3, 65535, dict(tps=30, splits=1)),
         (320, 64, 3, 45000, dict(tps=2, spans=2))]


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("K,N,nw,M,need", EXACT, ids=["tps15", "tps30", "n64"])
def test_exact_integers(K, N, nw, M, need, dt):
    """x, W in {-1, 0, 1} (nonzero with probability 1/4), integer biases in [-8, 8]: every partial sum is a small integer,
    exact in fp32 in any order and exact in fp16 / bf16 up to 256 -- the output equals the reference, whatever the order"""
    r = _regime(nw, M, N, K)
    _assert_regime(r, need)
    x = _x(K, dt, True)[:M]
    Ws, bs = _wb(K, N, nw, dt, True)
    _, outs = _launch(x, Ws, bs, dt)
    peak = 0.0
    for r0, r1, res in _ref_chunks(x, Ws, bs):
        for (ref, _), o in zip(res, outs):
            peak = max(peak, float(ref.abs().max()))
            assert peak <= 256
            assert torch.equal(o[r0:r1], ref.to(dt)), "rows %d..%d differ" % (r0, r1)
    print("exact %s K=%d N=%d: plan %s; max|ref| = %g" % (_name(dt), K, N, _fmt(r), peak))


# ---- the result of a row does not depend on the regime its launch lands in --------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_rows_do_not_depend_on_the_regime(dt):
    K, N, nw = 320, 320, 3
    Ws, bs = _wb(K, N, nw, dt)
    X = _x(K, dt)
    _assert_regime(_regime(nw, 65281, N, K), dict(tps=15, splits=1))
    _assert_regime(_regime(nw, 1000, N, K), dict(tps=1))
    _, big = _launch(X[:65281], Ws, bs, dt)
    _, small = _launch(X[:1000], Ws, bs, dt)
    for a, b in zip(big, small):
        assert torch.equal(a[:1000].view(torch.int16), b.view(torch.int16))
    # the rows of the last row block of the ragged eight-tile launch, launched alone (one tile per split)
    _assert_regime(_regime(nw, 32769, N, K), dict(tps=8))
    _assert_regime(_regime(nw, 1, N, K), dict(tps=1))
    _, big = _launch(X[:32769], Ws, bs, dt)
    _, small = _launch(X[32768:32769], Ws, bs, dt)
    for a, b in zip(big, small):
        assert torch.equal(a[32768:].view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("K,N,M,tps", [(320, 320, 65281, 15), (640, 640, 65535, 30)], ids=["k320", "k640"])
def test_one_split_launch_is_deterministic(K, N, M, tps, dt):
    """twice, not in a loop: a ring wait one slab short shows here before it shows as an error"""
    nw = 3
    _assert_regime(_regime(nw, M, N, K), dict(tps=tps, splits=1))
    Ws, bs = _wb(K, N, nw, dt)
    x = _x(K, dt)[:M]
    first, _ = _launch(x, Ws, bs, dt)
    second, _ = _launch(x, Ws, bs, dt)
    assert torch.equal(first.view(torch.int16), second.view(torch.int16))


# ---- the bar itself: the library's GEMM of the same operands must meet it -----------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [V320, V640], ids=["k320", "k640"])
def test_library_matmul_meets_the_same_bar(shape, dt):
    """not the kernel under test: torch's own matmul through the bar, which is how U was settled"""
    K, N, nw, M = shape
    x = _x(K, dt)[:M]
    Ws, _ = _wb(K, N, nw, dt)
    outs = [x @ W.t() for W in Ws]
    _check("torch.matmul", x, Ws, None, outs, dt)


# ---- linear_supported answers what the kernel answers --------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_linear_raises_exactly_where_linear_supported_says_no(dt):
    import fresco_amd
    import fresco_amd.ops as ops
    M = 8
    launched = refused = 0
    for K in (320, 640, 256):
        x = torch.ones(M, K, dtype=dt, device=DEV)
        for N in (64, 320, 640, 672, 704, 1024, 1088, 2048, 2112, 100):
            W = torch.ones(N, K, dtype=dt, device=DEV)
            for nw in (1, 2, 3):
                ok = ops.linear_supported(K, N, dt, nw)
                assert ok == (ops.linear_plan(nw, M, N, K)[0] == 0)
                assert ok == (K in (320, 640) and N % 64 == 0 and nw * N <= 2048), (K, N, nw)
                outs = [torch.full((M, N), SENTINEL, dtype=torch.int16, device=DEV).view(dt) for _ in range(nw)]
                if ok:
                    ops.linear(x, [W] * nw, None, outs=outs)
                    assert all(bool((o.float() == K).all()) for o in outs), (K, N, nw)
                    launched += 1
                else:
                    with pytest.raises(fresco_amd.FrescoHipError):
                        ops.linear(x, [W] * nw, None, outs=outs)
                    # refused before any launch: nothing was written
                    assert all(bool((o.view(torch.int16) == SENTINEL).all()) for o in outs), (K, N, nw)
                    refused += 1
    torch.cuda.synchronize()
    assert launched == 2 * (7 + 5 + 3) and refused == 90 - launched
