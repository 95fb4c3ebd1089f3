"""fresco_mapping_ind at the shapes and inputs where it can go wrong, bit for bit against the sequential model of
tests/mapping_model.py (the reference's own loop, src/flow_utils.py:84-101, restated; not the argsort oracle).

The C entry is driven directly with grid-resolution tensors built by hand: grids below one 1024-thread pass, of exactly
one pass and ragged multi-pass ones (the block scan's carry and the second word of `keys`), N = 1, 2, 3, 9, scale 1 and
8, landings on .5 and on the borders, collapses onto one / a row of / hw/7 targets with tied, distinct and near-tied
colours, occlusion values at the threshold, non-finite flows, and a nine-frame chain broken at one pair only.  Every
element of fwd, bwd and mask is compared; every output is poisoned before the call.  The public wrappers are compared
with the oracle on non-square frames with given occlusions."""
import pytest
import torch

import mapping_model as M
from oracle import fresco_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(flow, occ, frames, scale, ws_fill):
    """flow (P,2,H,W) as the entry takes it (not yet divided by scale), occ (P,H,W), frames (N,3,H,W), all fp32 CPU"""
    from fresco_amd import _lib, ops
    lib = _lib.load()
    N, _, H, W = frames.shape
    hw = H * W
    if N == 1:  # no pair: the entry still wants non-null pointers
        flow, occ = torch.zeros(1, 2, H, W), torch.zeros(1, H, W)
    fl, oc, fr = flow.contiguous().to(DEV), occ.contiguous().to(DEV), frames.contiguous().to(DEV)
    fwd = torch.full((N, hw), -7, dtype=torch.int64, device=DEV)
    bwd = torch.full((N, hw), -7, dtype=torch.int64, device=DEV)
    mask = torch.full((hw, N, N), 7, dtype=torch.uint8, device=DEV)
    nbytes = lib.fresco_mapping_workspace_bytes(N, H, W)
    ws = torch.full((max(nbytes, 256),), ws_fill, dtype=torch.uint8, device=DEV)
    rc = lib.fresco_mapping_ind(fl.data_ptr(), oc.data_ptr(), fr.data_ptr(), fwd.data_ptr(), bwd.data_ptr(),
                                mask.data_ptr(), ws.data_ptr(), ws.numel(), N, H, W, float(scale), ops._stream())
    _lib.check(rc, "fresco_mapping_ind")
    return fwd.cpu(), bwd.cpu(), mask.cpu()


def _check(flow_grid, occ, frames, scale, expect_mask=None):
    N, _, H, W = frames.shape
    hw = H * W
    flow = flow_grid * scale
    want = M.model(flow, occ, frames, scale)
    got = _run(flow, occ, frames, scale, 0xAB)
    again = _run(flow, occ, frames, scale, 0x00)
    for a, b in zip(got, again):  # two runs, different scratch contents: equal bits
        assert torch.equal(a, b)
    fwd, bwd, mask = got
    assert int(mask.max()) <= 1
    assert torch.equal(fwd, want[0]) and torch.equal(bwd, want[1]) and torch.equal(mask.bool(), want[2])
    ar = torch.arange(hw)
    for f in range(N):
        assert torch.equal(torch.sort(fwd[f])[0], ar)
        assert torch.equal(fwd[f][bwd[f]], ar)
    if expect_mask is not None:
        assert torch.equal(mask.bool(), expect_mask)
    return fwd, bwd, mask.bool()


@pytest.mark.parametrize("case", M.cases(), ids=M.case_id)
def test_mapping_ind_equals_the_loop_model(case):
    name, H, W, N, scale = case
    flow, occ, frames = M.inputs(case)
    fwd, bwd, mask = _check(flow, occ, frames, scale)
    hw = H * W
    ident = torch.arange(hw).expand(N, hw)
    if name == "all_occluded":  # identity, everything unlinked: every pair splits every mask row
        want = torch.eye(N, dtype=torch.bool).expand(hw, N, N)
        assert torch.equal(fwd, ident) and torch.equal(mask, want)
    if name == "zero_flow" or N == 1:
        assert torch.equal(fwd, ident) and torch.equal(bwd, ident) and bool(mask.all())


@pytest.mark.parametrize("fill_in", [False, True])
@pytest.mark.parametrize("H,W,scale", [(31, 33, 8.0), (33, 37, 1.0), (45, 47, 8.0)])
def test_chain_broken_at_one_pair_only(H, W, scale, fill_in):
    """N = 9, mirror-image pairs (bijections), the sources of a chosen set of trajectories occluded at pair 3: the mask is
    the exact {<= 3} x {> 3} block split on exactly those trajectories (mapping_model.chain_case; with fill_in some of them
    reach pair 3 through a fill-in source of pair 1 and carry that pair's split too)"""
    flow, occ, frames, expect, chosen = M.chain_case(H, W, seed=H, fill_in=fill_in)
    _, _, mask = _check(flow, occ, frames, scale, expect_mask=expect)
    assert torch.equal((~mask[:, 3, 4]).nonzero()[:, 0], chosen)


@pytest.mark.parametrize("Hf,Wf,scale", [(100, 180, 8.0), (256, 448, 8.0), (256, 448, 16.0), (72, 40, 4.0)])
def test_public_wrappers_nonsquare_given_occlusions(Hf, Wf, scale):
    """get_mapping_ind / get_single_mapping_ind / cross_frame_masks against the oracle on non-square frames (100 x 180: sizes
    the scale does not divide), with GIVEN occlusions: the comparison is unconditional"""
    import fresco_amd
    N = 4
    g = torch.Generator().manual_seed(int(Hf + Wf + scale))
    base = torch.tensor([5.0, -3.0]).view(1, 2, 1, 1)
    flows = base + 2.0 * torch.randn(N, 2, Hf, Wf, generator=g)
    occs = (torch.rand(N, Hf, Wf, generator=g) < 0.2).float()
    imgs = (torch.rand(N, 3, Hf, Wf, generator=g) * 4).floor() / 4
    h, w = int(Hf // scale), int(Wf // scale)
    fm, bm, tm = fresco_amd.get_mapping_ind(flows.to(DEV), occs.to(DEV), imgs.to(DEV), scale=scale)
    fo, bo, to_ = O.mapping_ind(flows, occs, imgs, scale=scale)
    assert tuple(fm.shape) == (N, 1, h * w)
    assert torch.equal(fm.cpu(), fo) and torch.equal(bm.cpu(), bo) and torch.equal(tm.cpu(), to_)
    m, unl = fresco_amd.get_single_mapping_ind(flows[1:2].to(DEV), occs[1:2].to(DEV), imgs[1:3].to(DEV), scale)
    mo, uo = O.single_mapping_ind(flows[1:2], occs[1:2], imgs[1:3], scale)
    assert torch.equal(m.cpu(), mo) and torch.equal(unl.cpu(), uo)
    assert bool(uo.any()) and not bool(uo.all())
    ms = fresco_amd.cross_frame_masks(occs.to(DEV), scales=(scale, 2 * scale))
    for a, b in zip(ms, O.cross_frame_masks(occs, scales=(scale, 2 * scale))):
        assert torch.equal(a.cpu(), b)
