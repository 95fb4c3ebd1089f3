"""The sequential correspondence model of tests/mapping_model.py against the oracle's argsort restatement on every input
family the GPU test uses (grid-resolution tensors, scale 1, flow pre-divided), and three checks that the families can
tell the model from a copy that is wrong in one rule: half-away rounding, a >= replacement rule, another error sum."""
import pytest
import torch

import mapping_model as M
from oracle import fresco_oracle as O

CASES = M.cases()


@pytest.mark.parametrize("case", CASES, ids=M.case_id)
def test_model_equals_oracle(case):
    flow, occ, frames = M.inputs(case)
    N = case[3]
    maps, unl = [], []
    for i in range(N - 1):
        m, u = M.pair_loop(flow[i], occ[i], frames[i:i + 2], 1.0)
        mo, uo = O.single_mapping_ind(flow[i:i + 1], occ[i:i + 1], frames[i:i + 2], 1.0)
        assert torch.equal(m, mo) and torch.equal(u, uo), i
        maps.append(m)
        unl.append(u)
    fwd, bwd, mask = M.chain_loop(maps, unl, N, hw=case[1] * case[2])
    fo, bo, mo = O.mapping_ind(flow, occ, frames, 1.0)
    assert torch.equal(fwd, fo[:, 0]) and torch.equal(bwd, bo[:, 0]) and torch.equal(mask, mo[:, 0])


@pytest.mark.parametrize("fill_in", [False, True])
@pytest.mark.parametrize("H,W", [(3, 5), (31, 33), (33, 37)])
def test_chain_case_mask_is_the_block_split_on_the_chosen_trajectories(H, W, fill_in):
    flow, occ, frames, expect, chosen = M.chain_case(H, W, seed=H, fill_in=fill_in)
    fwd, bwd, mask = M.model(flow, occ, frames, 1.0)
    assert torch.equal(mask, expect)
    fo, bo, mo = O.mapping_ind(flow, occ, frames, 1.0)
    assert torch.equal(fwd, fo[:, 0]) and torch.equal(bwd, bo[:, 0]) and torch.equal(mask, mo[:, 0])
    # the pair-3 split sits on exactly the chosen trajectories
    split3 = ~mask[:, 3, 4]
    assert torch.equal(split3.nonzero()[:, 0], chosen)
    if not fill_in:  # nothing else is broken: every other row is all ones
        rest = torch.ones(H * W, dtype=torch.bool)
        rest[chosen] = False
        assert bool(mask[rest].all())
    else:  # some chosen trajectories came through a fill-in source of pair 1
        assert bool((~mask[chosen, 1, 2]).any()) and bool(mask[chosen, 1, 2].any())


def _differs(name, grids, **wrong):
    n = 0
    for H, W in grids:
        flow, occ, frames = M.family(name, H, W, 2, seed=H)
        a = M.pair_loop(flow[0], occ[0], frames, 1.0)
        b = M.pair_loop(flow[0], occ[0], frames, 1.0, **wrong)
        n += int(not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])))
    return n == len(grids)


GR = [(31, 33), (33, 37), (45, 47)]


def test_half_integer_family_separates_half_away_rounding():
    assert _differs("half", GR, rounding="away")


@pytest.mark.parametrize("where", ["one", "row", "few"])
def test_tie_family_separates_a_greater_or_equal_rule(where):
    assert _differs("collapse_%s_q3" % where, GR, replace="ge")


@pytest.mark.parametrize("where", ["one", "row", "few"])
def test_near_tie_family_separates_the_other_error_sum(where):
    assert _differs("collapse_%s_near" % where, GR, esum="right")


def test_near_tie_family_has_a_zero_against_a_denormal():
    """source 0 (error denormal) meets the last source (error exactly 0) on one target: the later one wins; flushing the
    denormal to zero would keep source 0"""
    flow, occ, frames = M.family("collapse_few_near", 31, 33, 2, seed=1)
    m, _ = M.pair_loop(flow[0], occ[0], frames, 1.0)
    W = 33
    t = int(flow[0, 1, 0, 0]) * W + int(flow[0, 0, 0, 0])
    assert int(m[t]) == 31 * 33 - 1
    d = frames[1, :, 0, 0] - frames[0].reshape(3, -1)[:, t]
    e = float((d * d).sum() / 3)
    assert 0.0 < e < 1.17e-38
