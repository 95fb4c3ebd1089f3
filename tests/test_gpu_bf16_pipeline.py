"""A bf16 pipeline end to end: the attention processor on the bf16 kernels, the DDPM step, AdaIN, optimize_feature and
warp_tensor with bf16 tensors in and out.

Processor bar: t = max |err| / (rms(ref) + |ref|) <= 2^-6 against the oracle with bf16 storage rounding
(synth.oracle_attention(..., round_dtype=torch.bfloat16)).  The reference's own op sequence in bf16 (torch on the CPU) sits
at t = 0.65 - 0.99 x 2^-7 on these cases; the cap is twice its worst value because this path rounds at other points than
torch does.  Every test prints t."""
import copy
import sys
import warnings

import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
MODES = ["plain", "cf", "cf_temporal", "full"]
CASES = {"L3": (3, 128, "L3"), "L2": (3, 256, "L2")}  # HW = 256 in both


def _rms(x):
    return float(x.double().pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (N, R, layer) in CASES.items():
        c = synth.make_attention_case(N, R, layer, seed=3, dtype=BF)
        assert c["HW"] == 256
        out[name] = c
    return out


_REFS = {}


def _oracle(case, key, mode):
    if (key, mode) not in _REFS:
        _REFS[(key, mode)] = synth.oracle_attention(case, mode, round_dtype=BF)
    return _REFS[(key, mode)]


def _t(out, ref):
    out = out.double().cpu()
    ref = ref.double()
    return float(((out - ref).abs() / (_rms(ref) + ref.abs())).max())


def _proc(case, mode, native=True):
    import fresco_amd
    ctrl = synth.controller_for(case, mode, DEV, dtype=BF) if mode != "plain" else fresco_amd.AttentionControl()
    proc = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl)
    if not native:
        proc.native_bf16 = False
    attn = copy.deepcopy(case["attn"]).to(DEV).to(BF)
    return proc, attn


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layer", ["L3", "L2"])
def test_bf16_processor_parity(cases, layer, mode, monkeypatch):
    import fresco_amd
    import fresco_amd.ops as ops
    case = cases[layer]
    proc, attn = _proc(case, mode)
    assert fresco_amd.FRESCOAttnProcessor2_0.native_bf16 is True
    seen = []

    def spy(name):
        fn = getattr(ops, name)

        def wrapper(*a, **k):
            ts = []
            for x in list(a) + list(k.values()):
                for y in (x if isinstance(x, (list, tuple)) else [x]):
                    if torch.is_tensor(y) and y.is_floating_point():
                        ts.append(y.dtype)
            nw = (1 if torch.is_tensor(a[1]) else len(a[1])) if name == "linear" else None
            seen.append((name, ts, nw, k.get("x_rows") is not None))
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapper)

    for name in ("linear", "attention", "temporal_attention"):
        spy(name)
    with warnings.catch_warnings(record=True) as rec, torch.no_grad():
        warnings.simplefilter("always")
        out = proc(attn, case["hidden"].to(DEV))
    assert out.dtype == BF
    assert not [w for w in rec if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in rec]
    assert seen and all(dt == BF for _, ts, _, _ in seen for dt in ts), seen
    names = [s[0] for s in seen]
    assert "attention" in names and ("temporal_attention" in names) == (mode in ("cf_temporal", "full"))
    lin = [s for s in seen if s[0] == "linear"]
    if mode == "cf":  # cross-frame only: to_q in full, K | V of the selected rows in one gathered launch
        assert any(nw == 2 and rows for _, _, nw, rows in lin), lin
    else:             # q | k | v in ONE launch
        assert any(nw == 3 and not rows for _, _, nw, rows in lin), lin
    assert any(nw == 1 for _, _, nw, _ in lin), lin  # to_out
    t = _t(out, _oracle(case, layer, mode))
    print("bf16 processor %s %s: t = %.4f x 2^-6" % (layer, mode, t * 64))
    assert t <= 2.0 ** -6, t


@pytest.mark.parametrize("mode", ["cf", "cf_temporal"])
def test_bf16_processor_value_range(cases, mode):
    """to_v scaled by 2^18 and to_out by 2^-18 (exact in bf16): V leaves fp16's range (the rounding path of the parent
    commit gives inf here), the layer's output does not change."""
    case = dict(cases["L3"])
    a = copy.deepcopy(case["attn"])
    with torch.no_grad():
        a.to_v.weight.mul_(2.0 ** 18)
        a.to_out[0].weight.mul_(2.0 ** -18)
    case["attn"] = a
    proc, attn = _proc(case, mode)
    with warnings.catch_warnings(record=True) as rec, torch.no_grad():
        warnings.simplefilter("always")
        out = proc(attn, case["hidden"].to(DEV))
    assert not [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert out.dtype == BF and bool(torch.isfinite(out).all())
    t = _t(out, synth.oracle_attention(case, mode, round_dtype=BF))
    print("bf16 processor range %s: t = %.4f x 2^-6" % (mode, t * 64))
    assert t <= 2.0 ** -6, t


@pytest.mark.parametrize("mode", ["full", "cf"])
def test_bf16_processor_rounding_path_switch(cases, mode):
    """native_bf16 = False: the projections run as the modules' own GEMMs, q, k, v are rounded to fp16 for the kernels,
    one RuntimeWarning -- the bar of test_processor_other_activation_dtypes (2e-2 against the unrounded fp32 oracle)."""
    case = cases["L3"]
    proc, attn = _proc(case, mode, native=False)
    with pytest.warns(RuntimeWarning, match="rounded to fp16"), torch.no_grad():
        out = proc(attn, case["hidden"].to(DEV))
    assert out.dtype == BF
    ref32 = synth.oracle_attention(case, mode, round_dtype=None)
    err = (out.float().cpu() - ref32).abs()
    print("rounding path %s: max err %.3e" % (mode, float(err.max())))
    assert bool((err <= 2e-2 + 2e-2 * ref32.abs()).all()), float(err.max())


# ---- step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [False, True])
def test_bf16_step_equals_fp32_path_bit_for_bit(rep, monkeypatch):
    """The kernels are elementwise with fp32 arithmetic inside and one rounding at the store, so a bf16 result is the fp32
    path's result on the upcast inputs, rounded to bf16 -- bit for bit.  predict_x0 and step's x0 are checked that way
    directly.  step's second kernel reads x0 as stored (bf16, as the reference's dtype-agnostic torch step does), so the
    previous sample is compared with the fp32 kernel on the upcast of exactly that stored x0."""
    import fresco_amd
    S = sys.modules["fresco_amd.step"]  # `fresco_amd.step` itself is the function
    import make_step_golden as msg
    g = synth.gen(17)
    x = (torch.randn(6, 4, 16, 16, generator=g) * 1.3).to(BF)
    eps = torch.randn(6, 4, 16, 16, generator=g).to(BF)
    eps_t = torch.randn(6, 4, 16, 16, generator=g).to(BF)
    noise = torch.randn(6, 4, 16, 16, generator=g).to(BF).to(DEV)
    monkeypatch.setattr(S.torch, "randn", lambda *a, **k: noise.to(k.get("dtype", torch.float32)))
    dx, de, dt = x.to(DEV), eps.to(DEV), eps_t.to(DEV)

    x0b, eb = fresco_amd.predict_x0(dx, de, dt, guidance_scale=7.5, alpha_prod_t=0.37)
    x0f, ef = fresco_amd.predict_x0(dx.float(), de.float(), dt.float(), guidance_scale=7.5, alpha_prod_t=0.37)
    assert x0b.dtype == BF and eb.dtype == BF
    assert torch.equal(x0b, x0f.to(BF)) and torch.equal(eb, ef.to(BF))

    for t in (701, 1):
        prev_b, x0_b = fresco_amd.step(msg.P(), de, t, dx, None, repeat_noise=rep)
        assert prev_b.dtype == BF and x0_b.dtype == BF
        _, x0_f = fresco_amd.step(msg.P(), de.float(), t, dx.float(), None, repeat_noise=rep)
        assert torch.equal(x0_b, x0_f.to(BF))
        with monkeypatch.context() as m:
            m.setattr(S, "predict_x0", lambda *a, **k: (x0_b.float(), None))
            prev_f, _ = fresco_amd.step(msg.P(), de.float(), t, dx.float(), None, repeat_noise=rep)
        assert prev_f.dtype == torch.float32
        assert torch.equal(prev_b, prev_f.to(BF))


# ---- AdaIN --------------------------------------------------------------------------------------------------------------
def _ordered(t):
    """bf16 -> integers whose difference counts representable values in between"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def test_bf16_adain_and_mean_std():
    import fresco_amd
    g = synth.gen(23)
    c = (torch.randn(4, 64, 8, 8, generator=g) * 2 + 0.5).to(BF).to(DEV)
    s = (torch.randn(4, 64, 8, 8, generator=g) * 0.7 - 1).to(BF).to(DEV)
    out = fresco_amd.adaptive_instance_normalization(c, s)
    ref = fresco_amd.adaptive_instance_normalization(c.float(), s.float())
    assert out.dtype == BF and ref.dtype == torch.float32
    d = (_ordered(out) - _ordered(ref.to(BF))).abs().max()
    print("adain: max ulp distance", int(d))
    assert int(d) <= 1
    mean, std = fresco_amd.calc_mean_std(c)
    mref, sref = fresco_amd.calc_mean_std(c.float())
    assert mean.dtype == BF and std.dtype == BF and tuple(mean.shape) == (4, 64, 1, 1)
    assert int((_ordered(mean) - _ordered(mref.to(BF))).abs().max()) <= 1
    assert int((_ordered(std) - _ordered(sref.to(BF))).abs().max()) <= 1


# ---- optimize_feature / warp_tensor -----------------------------------------------------------------------------------------
def _check_vs_fp32(out, ref, what):
    assert out.dtype == BF and ref.dtype == torch.float32
    ref = ref.double().cpu()
    frac = float(((out.double().cpu() - ref).abs() / (2.0 ** -7 * (_rms(ref) + ref.abs()))).max())
    print("%s: worst |err| / bar = %.3f" % (what, frac))
    assert frac <= 1.0, (what, frac)


def test_bf16_optimize_feature_and_warp_tensor():
    """bf16 sample in, bf16 out, within 2^-7 (rms + |ref|) of the same call on the upcast fp32 sample (the fp32 working
    copies inside stay; only the last AdaIN / the final cast store bf16)"""
    import fresco_amd
    oc = synth.make_opt_case(4, 128, 8, 64, seed=1)
    x = oc["x"].to(BF).to(DEV)
    flows = [f.to(DEV) for f in oc["flows"]]
    occs = [o.to(DEV) for o in oc["occs"]]
    o_b = fresco_amd.optimize_feature(x, flows, occs, [oc["target"].to(DEV)], iters=2, unet_chunk_size=2)
    o_f = fresco_amd.optimize_feature(x.float(), flows, occs, [oc["target"].to(DEV)], iters=2, unet_chunk_size=2)
    _check_vs_fp32(o_b, o_f, "optimize_feature")
    w_b = fresco_amd.warp_tensor(x, flows, occs, oc["sal"].to(DEV), 2)
    w_f = fresco_amd.warp_tensor(x.float(), flows, occs, oc["sal"].to(DEV), 2)
    _check_vs_fp32(w_b, w_f, "warp_tensor")
