"""FreeU on the GPU: the closed-form Fourier filter, the backbone scaling + concat, and the registered block forwards,
against float64 records of the unmodified reference (tests/golden/freeu_golden.npz) and the float64 model that
tests/test_freeu_cpu.py pins to them (tests/freeu_model.py).

Bounds.  Filter: |y - y64| <= half an ulp of the storage type at |y64| (2^-11 relative for fp16, 2^-8 for bf16, nothing for
fp32) + 6e-6 max|x| over the plane -- seven tree-reduced fp32 sums at log2(HW) 2^-24 <= 14 * 6e-8 each, times a
coefficient of at most max|x|.  Backbone: half an ulp + 1e-5 |x|, on inputs whose channel-mean map has a range of at
least half its largest magnitude (checked), which bounds the cancellation in (m - min) / (max - min).
"""
import os

import numpy as np
import pytest
import torch

import freeu_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}
CANARY = -77.0


@pytest.fixture(scope="module")
def freeu_golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "freeu_golden.npz")))


def _gpu(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _np64(t):
    return t.detach().to("cpu", torch.float64).numpy()


def _assert_within(got, ref, bound, what):
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: max |d| = %.3g, worst error / bound = %.3f" % (what, float(err.max()) if err.size else 0.0, ratio))
    assert np.all(np.isfinite(got)), what
    assert np.all(err <= bound), (what, float(err.max()), ratio)


def _fourier_bound(ref, x, dtype_name):
    return M.half_ulp(ref, dtype_name) + 6e-6 * np.abs(x).max(axis=(2, 3), keepdims=True)


def _backbone_bound(ref, x_abs, dtype_name):
    return M.half_ulp(ref, dtype_name) + 1e-5 * x_abs


# ---------------------------------------------------------------------------------------------------------------
# Fourier filter
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", M.FOURIER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fourier_filter_matches_the_float64_reference(freeu_golden, shape, dtype_name):
    import fresco_amd
    x = M.fourier_input(shape)
    xg = _gpu(x, DTYPES[dtype_name])
    assert np.array_equal(_np64(xg), x)  # the GPU sees the values the reference saw
    for s in M.FOURIER_SCALES:
        ref = freeu_golden[M.fourier_key(shape, s) + "_f64"]
        y = fresco_amd.Fourier_filter(xg, 1, s)
        assert y.dtype == xg.dtype and y.shape == xg.shape
        _assert_within(_np64(y), ref, _fourier_bound(ref, x, dtype_name), "%s %s s=%g" % (shape, dtype_name, s))
        assert torch.equal(y, fresco_amd.Fourier_filter(xg, 1, s))  # same bits on every run
    assert torch.equal(fresco_amd.Fourier_filter(xg, 1, 1.0), xg)
    assert torch.equal(xg, _gpu(x, DTYPES[dtype_name]))  # the input is left alone


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", M.FOURIER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fourier_filter_writes_only_its_slices(shape, dtype_name):
    from fresco_amd import ops
    B, C, H, W = shape
    dt = DTYPES[dtype_name]
    xg = _gpu(M.fourier_input(shape), dt)
    for s in (0.2, 1.0):
        buf = torch.full((B, 2 * C * H * W), CANARY, dtype=dt, device=DEV)
        out = buf[:, :C * H * W].view(B, C, H, W)
        assert out.data_ptr() == buf.data_ptr() and (B == 1 or out.stride(0) == 2 * C * H * W)
        assert ops.freeu_fourier(xg, s, out=out) is out
        assert torch.equal(out, ops.freeu_fourier(xg, s))
        assert bool((buf[:, C * H * W:] == CANARY).all())
    # a non-contiguous input is made contiguous first
    xt = xg.transpose(2, 3)
    assert torch.equal(ops.freeu_fourier(xt, 0.2), ops.freeu_fourier(xt.contiguous(), 0.2))


_fourier_refs = {}


def _fourier_ref(shape, s):
    """fourier_model in float64, computed once per (shape, scale) and shared by the dtypes"""
    if (shape, s) not in _fourier_refs:
        _fourier_refs[shape, s] = M.fourier_model(M.fourier_input(shape), s)
    return _fourier_refs[shape, s]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", M.FOURIER_TILED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fourier_filter_on_every_kernel_form(shape, dtype_name):
    """planes past 1024 and 4096 elements, with packs and with single elements (freeu_model.FOURIER_TILED_SHAPES),
    against the float64 model; the output goes into a slice of a canary-filled buffer"""
    import fresco_amd
    from fresco_amd import ops
    B, C, H, W = shape
    dt = DTYPES[dtype_name]
    x = M.fourier_input(shape)
    xg = _gpu(x, dt)
    assert np.array_equal(_np64(xg), x)
    for s in M.FOURIER_SCALES:
        ref = _fourier_ref(shape, s)
        y = fresco_amd.Fourier_filter(xg, 1, s)
        assert y.dtype == xg.dtype and y.shape == xg.shape
        _assert_within(_np64(y), ref, _fourier_bound(ref, x, dtype_name), "%s %s s=%g" % (shape, dtype_name, s))
        assert torch.equal(y, fresco_amd.Fourier_filter(xg, 1, s))  # same bits on every run
        buf = torch.full((B, 2 * C * H * W), CANARY, dtype=dt, device=DEV)
        out = buf[:, :C * H * W].view(B, C, H, W)
        assert ops.freeu_fourier(xg, s, out=out) is out
        assert torch.equal(out, y) and bool((buf[:, C * H * W:] == CANARY).all())
    assert torch.equal(fresco_amd.Fourier_filter(xg, 1, 1.0), xg)
    assert torch.equal(xg, _gpu(x, DTYPES[dtype_name]))  # the input is left alone


def _views(B, chw, dt):
    """-> [(name, buffer, the (B, chw) view of it a test writes through)]: a view that starts one element into its buffer
    (no 16-byte alignment), and one whose batch stride is odd; canaries before, between and after the samples"""
    flat = torch.full((B * chw + 16,), CANARY, dtype=dt, device=DEV)
    rows = torch.full((B, chw + 3), CANARY, dtype=dt, device=DEV)
    return [("one element in", flat, flat[1:1 + B * chw].view(B, chw)), ("odd batch stride", rows, rows[:, :chw])]


def _canaries_intact(name, buf, B, chw):
    if name == "one element in":
        return bool((buf[:1] == CANARY).all()) and bool((buf[1 + B * chw:] == CANARY).all())
    return bool((buf[:, chw:] == CANARY).all())


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (2, 2, 48, 48), (2, 1, 72, 64)], ids=lambda s: "x".join(map(str, s)))
def test_fourier_filter_into_unaligned_and_odd_strided_views(shape, dtype_name):
    """H W is a multiple of the pack, the destination is not: the pointer half and the stride half of the `wide`
    predicate each send the call down the single-element path (planes of 64, 2304 and 4608 elements: all three kernels)"""
    from fresco_amd import ops
    B, C, H, W = shape
    dt = DTYPES[dtype_name]
    chw = C * H * W
    assert (H * W) % 8 == 0 and chw % 2 == 0
    x = M.fourier_input(shape)
    xg = _gpu(x, dt)
    for s in (0.2, 1.0):
        ref = _fourier_ref(shape, s)
        for name, buf, view in _views(B, chw, dt):
            out = view.view(B, C, H, W)
            if name == "one element in":
                assert out.data_ptr() % 16 == xg.element_size() and out.stride(0) == chw
            else:
                assert out.data_ptr() % 16 == 0 and out.stride(0) % 2 == 1
            assert ops.freeu_fourier(xg, s, out=out) is out
            _assert_within(_np64(out), ref, _fourier_bound(ref, x, dtype_name), "%s %s s=%g %s" % (shape, dtype_name, s, name))
            assert _canaries_intact(name, buf, B, chw), name
            if s == 1.0:
                assert torch.equal(out, xg)
            first = out.clone()
            ops.freeu_fourier(xg, s, out=out)
            assert torch.equal(out, first)


def test_copy_takes_a_second_grid_stride_trip():
    """scale = 1 on 129 x 128 x 256 fp16 elements: 2064 blocks' worth of 16-byte packs against the grid cap of 2048"""
    from fresco_amd import ops
    B, C, H, W = 1, 129, 128, 256
    chw = C * H * W
    x = (torch.arange(chw, device=DEV) % 2039).to(torch.float16).view(B, C, H, W)  # integers below 2048: exact in fp16
    buf = torch.full((chw + 64,), CANARY, dtype=torch.float16, device=DEV)
    out = buf[:chw].view(B, C, H, W)
    assert ops.freeu_fourier(x, 1.0, out=out) is out
    assert torch.equal(out, x) and bool((buf[chw:] == CANARY).all())


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_copy_of_an_odd_sample_size(dtype_name):
    """scale = 1 with C H W = 3465: the single-element copy kernel, 14 blocks per sample, into both kinds of view"""
    from fresco_amd import ops
    shape = (2, 3, 33, 35)
    B, chw = 2, 3 * 33 * 35
    dt = DTYPES[dtype_name]
    xg = _gpu(M.fourier_input(shape), dt)
    assert torch.equal(ops.freeu_fourier(xg, 1.0), xg)
    for name, buf, view in _views(B, chw, dt):
        out = view.view(shape)
        ops.freeu_fourier(xg, 1.0, out=out)
        assert torch.equal(out, xg) and _canaries_intact(name, buf, B, chw), name


def test_fourier_filter_refuses_what_is_not_built():
    import fresco_amd
    from fresco_amd import ops
    with pytest.raises(fresco_amd.FrescoHipError, match="EUNSUPPORTED"):
        ops.freeu_fourier(torch.zeros(1, 1, 1, 8, device=DEV), 0.5)
    with pytest.raises(NotImplementedError):
        fresco_amd.Fourier_filter(torch.zeros(1, 1, 4, 4, device=DEV), 2, 0.5)


# ---------------------------------------------------------------------------------------------------------------
# backbone
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backbone_refs():
    """float64 model outputs, computed once per (case, b)"""
    refs = {}
    for case in M.BACKBONE_CASES + M.BACKBONE_TILED_CASES:
        x = M.backbone_input(case)
        refs[case] = (x, {b: M.backbone_model(x, case[2], b) for b in M.BACKBONE_BS})
    return refs


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("case", M.BACKBONE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_backbone_scaling_and_concat(backbone_refs, case, dtype_name):
    _check_backbone(backbone_refs, case, dtype_name)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("case", M.BACKBONE_TILED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_backbone_on_planes_of_several_tiles(backbone_refs, case, dtype_name):
    """freeu_model.BACKBONE_TILED_CASES: every pixel tile must read its own slice of the mean map and of the channels"""
    _check_backbone(backbone_refs, case, dtype_name)


def _check_backbone(backbone_refs, case, dtype_name):
    from fresco_amd import ops
    B, C, n, H, W = case
    dt = DTYPES[dtype_name]
    x, refs = backbone_refs[case]
    assert M.mean_map_condition(x)
    means = x.mean(axis=(1, 2, 3))
    assert len(set(np.round(means, 3))) == B  # every sample has its own mean (and, by construction, range)
    extra = 3
    for b in M.BACKBONE_BS:
        hidden = _gpu(x, dt)
        cat = torch.full((B, C + extra, H, W), CANARY, dtype=dt, device=DEV)
        assert ops.freeu_backbone(hidden, n, b, cat=cat) is hidden
        _assert_within(_np64(hidden), refs[b], _backbone_bound(refs[b], np.abs(x), dtype_name),
                       "%s %s b=%g" % (case, dtype_name, b))
        x0 = _gpu(x, dt)
        assert torch.equal(hidden[:, n:], x0[:, n:])  # channels past the scaled half: untouched bits
        assert torch.equal(cat[:, :C], hidden)
        assert bool((cat[:, C:] == CANARY).all())
        alone = _gpu(x, dt)  # without a concat destination only hidden changes, to the same bits
        ops.freeu_backbone(alone, n, b)
        assert torch.equal(alone, hidden)
        again = _gpu(x, dt)
        cat2 = torch.empty_like(cat)
        ops.freeu_backbone(again, n, b, cat=cat2)
        assert torch.equal(again, hidden) and torch.equal(cat2[:, :C], cat[:, :C])


def test_backbone_constant_mean_map_is_not_repaired():
    """0 / 0 like the reference: the scaled channels turn non-finite, the others stay"""
    from fresco_amd import ops
    hidden = torch.ones(1, 4, 4, 4, dtype=torch.float16, device=DEV)
    ops.freeu_backbone(hidden, 2, 1.2)
    assert not bool(torch.isfinite(hidden[:, :2]).any())
    assert bool((hidden[:, 2:] == 1).all())


def test_site_writes_both_halves_of_the_concat(backbone_refs):
    """ops.freeu_site: the two calls land in one tensor -- the filter's output starts at channel C of it"""
    from fresco_amd import ops
    case = M.BACKBONE_CASES[2]
    x, refs = backbone_refs[case]
    B, C, n, H, W = case
    skip = M.fourier_input((B, 7, H, W))
    hidden, sk = _gpu(x, torch.float16), _gpu(skip, torch.float16)
    cat = ops.freeu_site(hidden, sk, n, 1.2, 0.9)
    assert cat.shape == (B, C + 7, H, W)
    alone = _gpu(x, torch.float16)
    ops.freeu_backbone(alone, n, 1.2)
    assert torch.equal(cat[:, :C], alone) and torch.equal(hidden, alone)
    assert torch.equal(cat[:, C:], ops.freeu_fourier(sk, 0.9))


# ---------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------
def _registers():
    import fresco_amd
    return {"UpBlock2D": fresco_amd.register_free_upblock2d, "CrossAttnUpBlock2D": fresco_amd.register_free_crossattn_upblock2d}


def _block_bound(ref, stage, skip, dtype_name="float16"):
    """per-element bound for a resnet input (B, stage + skip channels, H, W): the backbone bound on the hidden part
    (|x| >= |ref| / 1.5: the factor lies in [1, b] and b <= 1.5 here), the filter bound on the skip part"""
    bound = M.half_ulp(ref, dtype_name)
    bound[:, :stage] += 1e-5 * np.abs(ref[:, :stage]) / 1.5
    if skip is not None:
        bound[:, stage:] += 6e-6 * np.abs(skip).max(axis=(2, 3), keepdims=True)
    return bound


@pytest.mark.parametrize("size", M.BLOCK_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", list(M.BLOCK_CONFIGS))
@pytest.mark.parametrize("kind", M.BLOCK_KINDS)
def test_registered_forward_matches_the_reference_forward(freeu_golden, kind, name, size):
    C, outs, _ = M.BLOCK_CONFIGS[name]
    hidden, skips = M.block_inputs(name, size)
    r = M.run_block(_registers()[kind], kind, name, size, torch.float16, device=DEV)
    model = M.model_block(name, size)
    blk = r["block"]
    assert (blk.b1, blk.b2, blk.s1, blk.s2) == tuple(M.BLOCK_FACTORS[k] for k in ("b1", "b2", "s1", "s2"))
    key = M.block_key(kind, name, size)
    stage = C
    for k, t in enumerate(r["resnet_in"]):
        got, skip = _np64(t), skips[-1 - k]
        assert got.shape[1] == stage + M.SKIP_CH
        full = _block_bound(model["resnet_in"][k], stage, skip)
        kept = M.kept_of(name, stage, got.shape[1])
        ref = freeu_golden["%s_in%d_f64" % (key, k)]
        _assert_within(got[:, kept], ref, full[:, kept], "%s resnet %d vs golden" % (key, k))
        _assert_within(got, model["resnet_in"][k], full, "%s resnet %d vs model, every channel" % (key, k))
        if not M.site_of(stage):  # no FreeU at this width: a plain concat, exactly
            assert np.array_equal(got, model["resnet_in"][k])
        stage = outs[k]
    got = _np64(r["out"])
    kept = M.kept_of(name, stage, stage)
    _assert_within(got[:, kept], freeu_golden[key + "_out_f64"], _block_bound(model["out"], stage, None)[:, kept],
                   key + " output vs golden")
    _assert_within(got, model["out"], _block_bound(model["out"], stage, None), key + " output vs model")
    # the incoming tensor is scaled in place exactly where the reference scales it
    after = _np64(r["hidden_after"])
    kept = M.kept_of(name, C, C)
    bound = _block_bound(model["hidden_after"], C, None)
    _assert_within(after[:, kept], freeu_golden[key + "_hidden_f64"], bound[:, kept], key + " incoming hidden vs golden")
    _assert_within(after, model["hidden_after"], bound, key + " incoming hidden vs model")
    n = M.site_of(C)
    assert np.array_equal(after[:, n:], hidden[:, n:])
    assert bool(np.any(after[:, :n] != hidden[:, :n])) == bool(n)
    if kind == "CrossAttnUpBlock2D":
        assert [len(a.inputs) for a in blk.attentions] == [1] * len(outs)


def test_apply_freeu_registers_both_block_kinds():
    import fresco_amd
    size = (2, 4, 4)
    hidden, skips = M.block_inputs("c640", size)
    blocks = [M.make_block(kind, "c640") for kind in M.BLOCK_KINDS]
    fresco_amd.apply_freeu(M.StandInPipe(blocks), **M.BLOCK_FACTORS)
    for kind, blk in zip(M.BLOCK_KINDS, blocks):
        assert (blk.b1, blk.b2, blk.s1, blk.s2) == (1.2, 1.5, 0.9, 0.2)
        with torch.no_grad():
            out = blk.forward(_gpu(hidden, torch.float16), tuple(_gpu(s, torch.float16) for s in skips))
        r = M.run_block(_registers()[kind], kind, "c640", size, torch.float16, device=DEV)
        assert torch.equal(out, r["out"])
        for a, b in zip(blk.resnets, r["block"].resnets):
            assert torch.equal(a.inputs[0], b.inputs[0])


@pytest.mark.parametrize("kind", M.BLOCK_KINDS)
def test_channels_last_hidden_is_still_scaled_in_place(kind):
    size = (2, 4, 4)
    hidden, _ = M.block_inputs("c1280", size)
    a = M.run_block(_registers()[kind], kind, "c1280", size, torch.float16, device=DEV)
    b = M.run_block(_registers()[kind], kind, "c1280", size, torch.float16, device=DEV, channels_last=True)
    assert not b["hidden_after"].is_contiguous()
    assert torch.equal(a["hidden_after"], b["hidden_after"])
    assert not torch.equal(b["hidden_after"], _gpu(hidden, torch.float16))
    for x, y in zip(a["resnet_in"], b["resnet_in"]):
        assert torch.equal(x, y)
    assert torch.equal(a["out"], b["out"])
