"""The frame-sharded attention branch in bf16 on ONE GPU (ranks emulated by threads, as test_gpu_sharded.py): bf16
activations run the branch in bf16 -- projections, exchange buffers, attention passes, fresco_temporal_pack /
_attn_packed_dt / _unpack around the trajectory all-to-all -- with no cast and no warning.

Bars: t = max |err| / (rms(ref) + |ref|) <= 2^-6 against the bf16 oracle for each rank's rows (the bf16 processor bar), and
max |sharded - single-GPU bf16| <= 4e-3: the fp16 test's 5e-4 scaled by the ulp ratio 2^3 (same kernels, same key
order)."""
import copy
import threading
import warnings

import pytest
import torch

import synth
from test_gpu_sharded import ThreadShard

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
_cases, _refs = {}, {}


def _case(N, R, layer, keep):
    key = (N, R, layer, keep)
    if key not in _cases:
        case = synth.make_attention_case(N, R, layer, seed=4, dtype=BF)
        if keep == "f1":
            case["cf_mask"][2:] = False
        _cases[key] = case
    return _cases[key]


def _oracle(N, R, layer, keep, mode):
    key = (N, R, layer, keep, mode)
    if key not in _refs:
        _refs[key] = synth.oracle_attention(_case(N, R, layer, keep), mode, round_dtype=BF)
    return _refs[key]


def _rms(x):
    return float(x.double().pow(2).mean().sqrt())


def _t(out, ref):
    out = out.double().cpu()
    ref = ref.double().cpu()
    return float(((out - ref).abs() / (_rms(ref) + ref.abs())).max())


def _run_ranks(case, mode, world, N, native=True):
    """-> [(local batch index, output)] per rank, {thread name: [RuntimeWarning messages]}"""
    import fresco_amd
    from fresco_amd.dist import FrameShard
    attn = copy.deepcopy(case["attn"]).to(DEV).to(BF)
    hidden = case["hidden"].to(DEV)
    slots = [None] * world
    barrier = threading.Barrier(world)
    outs, errs = [None] * world, []
    warned = {}

    def record(message, category, filename, lineno, file=None, line=None):  # runs in the thread that warned
        if issubclass(category, RuntimeWarning):
            warned.setdefault(threading.current_thread().name, []).append(str(message))

    def rank_fn(r):
        try:
            base = FrameShard(N, 2, r, world)
            sel = base.local_batch_index().to(DEV)
            ctrl = synth.controller_for(case, mode, DEV, dtype=BF)
            if mode == "full":  # the stored reference features are sharded like the hidden states
                ctrl.stored_attn["decoder_attn"] = [case["ref"].to(DEV).to(BF).index_select(0, sel)]
            proc = fresco_amd.FRESCOAttnProcessor2_0(2, ctrl)
            proc.native_bf16 = native
            proc.shard = ThreadShard(base, slots, barrier)
            with torch.no_grad():
                outs[r] = (sel, proc(attn, hidden.index_select(0, sel).contiguous()))
        except Exception as e:  # pragma: no cover
            errs.append(e)
            barrier.abort()

    with warnings.catch_warnings():
        warnings.simplefilter("always")
        warnings.showwarning = record
        ts = [threading.Thread(target=rank_fn, args=(r,), name="rank%d" % r) for r in range(world)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    assert not errs, errs
    torch.cuda.synchronize()
    return outs, warned


def _single(case, mode):
    import fresco_amd
    attn = copy.deepcopy(case["attn"]).to(DEV).to(BF)
    with torch.no_grad():
        out = fresco_amd.FRESCOAttnProcessor2_0(2, synth.controller_for(case, mode, DEV, dtype=BF))(attn, case["hidden"].to(DEV))
    torch.cuda.synchronize()
    return out


def _check(case, ref, mode, world, N, what):
    single = _single(case, mode)
    assert single.dtype == BF
    outs, warned = _run_ranks(case, mode, world, N)
    assert not warned, warned
    for sel, o in outs:
        assert o.dtype == BF
        t = _t(o, ref.index_select(0, sel.cpu()))
        d = float((o.float() - single.index_select(0, sel).float()).abs().max())
        print("sharded bf16 %s %s: t = %.4f x 2^-6, max |sharded - single| = %.3e" % (what, mode, t * 64, d))
        assert t <= 2.0 ** -6, (what, mode, t)
        assert d <= 4e-3, (what, mode, d)


@pytest.mark.parametrize("world,N,keep", [(2, 4, "all"), (4, 4, "all"), (2, 4, "f1")])
@pytest.mark.parametrize("mode", ["cf", "cf_temporal", "full", "temporal"])
def test_sharded_bf16_processor_equals_single_gpu(world, N, keep, mode):
    if keep != "all" and mode == "temporal":
        pytest.skip("the mask variants only touch the cross-frame pass")
    _check(_case(N, 128, "L3", keep), _oracle(N, 128, "L3", keep, mode), mode, world, N, "L3 world=%d %s" % (world, keep))


def test_sharded_bf16_head_dim_80_through_the_packed_temporal_entry():
    _check(_case(4, 256, "L2", "all"), _oracle(4, 256, "L2", "all", "cf_temporal"), "cf_temporal", 2, 4, "L2 world=2 all")


def test_sharded_bf16_rounding_path_switch():
    """native_bf16 = False: the branch rounds to fp16 as before, every rank's processor says so once, bf16 comes back"""
    case = _case(4, 128, "L3", "all")
    outs, warned = _run_ranks(case, "cf_temporal", 2, 4, native=False)
    assert sorted(warned) == ["rank0", "rank1"], warned
    assert all(any("rounded to fp16" in m for m in msgs) for msgs in warned.values()), warned
    ref32 = synth.oracle_attention(case, "cf_temporal", round_dtype=None)
    for sel, o in outs:
        assert o.dtype == BF
        r = ref32.index_select(0, sel.cpu())
        err = (o.float().cpu() - r).abs()
        # (the bar of the single-GPU rounding path, test_gpu_bf16_pipeline.py::test_bf16_processor_rounding_path_switch)
        assert bool((err <= 2e-2 + 2e-2 * r.abs()).all()), float(err.max())


def test_temporal_pack_unpack_bf16_round_trip():
    """pack -> (identity transport, world = 1) -> unpack reproduces q bit for bit: copies, no arithmetic"""
    import fresco_amd.ops as ops
    N, HW, C, chunk = 2, 64, 320, 2
    g = synth.gen(9)
    q, k, v = (torch.randn(chunk * N, HW, C, generator=g).to(BF).to(DEV) for _ in range(3))
    fwd_map = torch.stack([torch.randperm(HW, generator=g) for _ in range(N)]).to(DEV)
    buf = ops.temporal_pack(q, k, v, fwd_map, chunk, N, 0, 1)
    assert buf.dtype == BF and tuple(buf.shape) == (1, N, chunk, HW, 3 * C)
    # (the packed rows are q | k | v of the trajectory order: the same bits, moved)
    assert torch.equal(buf[0, 1, 0, :, C:2 * C].view(torch.int16), k[0 * N + 1][fwd_map[1]].view(torch.int16))
    out = ops.temporal_unpack(buf[..., :C].contiguous(), fwd_map, chunk, N, 0, 1)
    assert out.dtype == BF
    assert torch.equal(out.view(torch.int16), q.view(torch.int16))
