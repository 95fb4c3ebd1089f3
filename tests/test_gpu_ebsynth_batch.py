"""Batched Ebsynth (fresco_ebsynth_run_batch / ebsynth_run_batch): every member of a batch equals ebsynth_run on its
inputs and seed, bit for bit (image, E, NNF), over the branches of test_gpu_ebsynth_matrix.py (inputs built by its
case_inputs, under its exact-sum bound); seeds distinct and repeated, permuted batch order, refused arguments, and
repeatability."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from fresco_amd import FrescoHipError, _lib, ebsynth_run, ebsynth_run_batch
from fresco_amd import ebsynth as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_ebsynth_matrix import CASES, assert_exact_regime, case_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def members(name, n):
    """n problems of one case: the case's inputs with each problem's style / guides rolled and offset, so the
    problems differ, within the case's per-channel byte ranges (the exact regime holds for every member)."""
    ci = case_inputs(name)
    out = []
    for b in range(n):
        p = dict(ci)
        for k in ("ss", "sg", "tg"):
            a = ci[k]
            lo, hi = a.reshape(-1, a.shape[-1]).min(0), a.reshape(-1, a.shape[-1]).max(0)
            rolled = np.roll(a, (3 * b, 5 * b), axis=(0, 1)).astype(np.int64)
            p[k] = (lo + (rolled - lo + 7 * b) % (hi - lo + 1)).astype(np.uint8)
        if ci["mod"] is not None:
            p["mod"] = np.roll(ci["mod"], b, axis=1)
        out.append(p)
    return out


def single(p, seed):
    return ebsynth_run(gpu(p["ss"]), gpu(p["sg"]), gpu(p["tg"]),
                       target_modulation=None if p["mod"] is None else gpu(p["mod"]), style_weights=p["sw"],
                       guide_weights=p["gw"], seed=seed, return_nnf=True, **p["kw"])


def batch(ps, seeds):
    mod = None if ps[0]["mod"] is None else gpu(np.stack([p["mod"] for p in ps]))
    return ebsynth_run_batch(gpu(np.stack([p["ss"] for p in ps])), gpu(np.stack([p["sg"] for p in ps])),
                             gpu(np.stack([p["tg"] for p in ps])), target_modulation=mod, style_weights=ps[0]["sw"],
                             guide_weights=ps[0]["gw"], seeds=seeds, return_nnf=True, **ps[0]["kw"])


def assert_member(got, b, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g[b].cpu().numpy(), w.cpu().numpy())


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_batch_members_equal_single_calls(name, n):
    ps = members(name, n)
    for p in ps:
        assert_exact_regime(p["kw"].get("patch_size", 5), p["ss"], p["sg"], p["tg"], p["sw"], p["gw"], p["mod"])
    seeds = [11 + 13 * b for b in range(n)]
    got = batch(ps, seeds)
    for b in range(n):
        assert_member(got, b, single(ps[b], seeds[b]))


def test_repeated_seeds_and_permuted_order():
    name = "rw1_modulation"
    ps = members(name, 4)
    seeds = [5, 5, 9, 5]
    got = batch(ps, seeds)
    for b in range(4):
        assert_member(got, b, single(ps[b], seeds[b]))
    same = batch([ps[0]] * 3, [5, 5, 6])  # one problem twice with one seed: equal; another seed: differs
    for g in same:
        np.testing.assert_array_equal(g[0].cpu().numpy(), g[1].cpu().numpy())
    assert not torch.equal(same[2][0], same[2][2])
    perm = [2, 0, 3, 1]
    got_p = batch([ps[k] for k in perm], [seeds[k] for k in perm])
    for g, gp in zip(got, got_p):
        np.testing.assert_array_equal(gp.cpu().numpy(), g[perm].cpu().numpy())


def test_second_run_is_bit_identical():
    ps = members("rw2_modulation_weighted_extra_pass", 3)
    a, b = batch(ps, [1, 2, 3]), batch(ps, [1, 2, 3])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refused_before_any_launch():
    """n = 0, n above the cap and a short workspace are refused with the outputs untouched."""
    lib = _lib.load()
    ps = members("rw1_16ch_weighted", 2)
    p = ps[0]
    (sh, sw_, ns), (th, tw, ng) = p["ss"].shape, p["tg"].shape
    n_ok = 2
    need = lib.fresco_ebsynth_batch_workspace_bytes(n_ok, ns, ng, sw_, sh, tw, th, 5, -1, 0)
    assert need == E.batch_workspace_bytes(n_ok, ns, ng, (sh, sw_), (th, tw))
    assert need > lib.fresco_ebsynth_batch_workspace_bytes(1, ns, ng, sw_, sh, tw, th, 5, -1, 0) > 0
    assert lib.fresco_ebsynth_batch_workspace_bytes(1, ns, ng, sw_, sh, tw, th, 5, -1, 0) == \
        lib.fresco_ebsynth_workspace_bytes(ns, ng, sw_, sh, tw, th, 5, -1, 0)
    assert lib.fresco_ebsynth_batch_workspace_bytes(0, ns, ng, sw_, sh, tw, th, 5, -1, 0) == 0
    assert lib.fresco_ebsynth_batch_workspace_bytes(E.MAX_BATCH + 1, ns, ng, sw_, sh, tw, th, 5, -1, 0) == 0
    nmax = E.MAX_BATCH + 1
    ss = gpu(np.stack([p["ss"]] * nmax))
    sg = gpu(np.stack([p["sg"]] * nmax))
    tg = gpu(np.stack([p["tg"]] * nmax))
    out = torch.full((nmax, th, tw, ns), 77, dtype=torch.uint8, device=DEV)
    err = torch.full((nmax, th, tw), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    c = _lib._c
    swa, gwa = (c.c_float * ns)(*p["sw"]), (c.c_float * ng)(*p["gw"])
    levels = E.max_pyramid_levels((sh, sw_), (th, tw), 5)
    it = (c.c_int * levels)(*([2] * levels))
    stop = (c.c_int * levels)(*([5] * levels))
    seeds = (c.c_uint64 * nmax)(*range(nmax))

    def call(n, nbytes):
        return lib.fresco_ebsynth_run_batch(n, ss.data_ptr(), sg.data_ptr(), tg.data_ptr(), None, swa, gwa, ns, ng,
                                            sw_, sh, tw, th, 3500.0, 5, 2, levels, it, it, stop, 0, seeds, None,
                                            out.data_ptr(), err.data_ptr(), ws.data_ptr(), nbytes, None)

    torch.cuda.synchronize()
    assert call(0, need) == -1
    assert call(-3, need) == -1
    assert call(E.MAX_BATCH + 1, need) == -2
    assert call(n_ok, need - 1) == -3
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((err == 7.0).all())
    with pytest.raises(ValueError):
        ebsynth_run_batch(ss[:2], sg[:2], tg[:2], seeds=[1, 2, 3])
    with pytest.raises(FrescoHipError):
        ebsynth_run_batch(ss, sg, tg)  # 65 problems
    assert call(n_ok, need) == 0
    torch.cuda.synchronize()
    want = ebsynth_run_batch(ss[:2], sg[:2], tg[:2], style_weights=p["sw"], guide_weights=p["gw"],
                             vote_mode="weighted", search_vote_iters=2, patchmatch_iters=2, seeds=[0, 1])
    assert torch.equal(out[:2], want[0]) and torch.equal(err[:2], want[1])
