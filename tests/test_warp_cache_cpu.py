"""The derived-tensor cache of fresco_amd/warp.py (`_cached`, `_derived`, `invalidate_cache`) on CPU tensors with a counting
`build`: a stale hit would make every later warp_tensor / optimize_feature of a run use another batch's resized flows.
The key is (kind, extra) + (data_ptr, shape, version counter, device) per source; an entry also holds weak references to its
sources, so that a new tensor at a recycled address misses."""
import gc

import numpy as np
import pytest
import torch

from fresco_amd import warp


@pytest.fixture(autouse=True)
def _clean_cache():
    warp.invalidate_cache()
    yield
    warp.invalidate_cache()


class Build:
    """build() for _cached: counts its calls and returns a fresh object each time"""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return ("value", self.calls)


def _srcs(n=4):
    return tuple(torch.zeros(2, 3) + i for i in range(n))


def test_same_sources_hit():
    b = Build()
    srcs = _srcs()
    v1 = warp._cached("flow_occ", srcs, (8, True), b)
    v2 = warp._cached("flow_occ", srcs, (8, True), b)
    v3 = warp._cached("flow_occ", tuple(srcs), (8, True), b)  # (a new tuple of the same tensor objects)
    assert v1 is v2 and v1 is v3 and b.calls == 1 and len(warp._derived) == 1


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_in_place_update_of_any_source_misses(which):
    b = Build()
    srcs = _srcs()
    v1 = warp._cached("flow_occ", srcs, (8, True), b)
    srcs[which].add_(1)
    v2 = warp._cached("flow_occ", srcs, (8, True), b)
    assert b.calls == 2 and v2 is not v1 and v2 == ("value", 2)
    assert warp._cached("flow_occ", srcs, (8, True), b) is v2 and b.calls == 2


def test_other_extra_or_kind_misses_and_keeps_both():
    b = Build()
    srcs = _srcs()
    v_dil = warp._cached("flow_occ", srcs, (8, True), b)
    v_plain = warp._cached("flow_occ", srcs, (8, False), b)
    v_h = warp._cached("flow_occ", srcs, (16, True), b)
    v_kind = warp._cached("saliency", srcs, (8, True), b)
    assert b.calls == 4 and len(warp._derived) == 4
    assert warp._cached("flow_occ", srcs, (8, True), b) is v_dil
    assert warp._cached("flow_occ", srcs, (8, False), b) is v_plain
    assert warp._cached("flow_occ", srcs, (16, True), b) is v_h
    assert warp._cached("saliency", srcs, (8, True), b) is v_kind
    assert b.calls == 4


def test_other_shape_or_order_misses():
    b = Build()
    t, u = torch.zeros(2, 6), torch.ones(2, 6)
    warp._cached("k", (t, u), 0, b)
    warp._cached("k", (u, t), 0, b)
    warp._cached("k", (t.view(3, 4), u), 0, b)  # same pointer and version counter, other shape
    assert b.calls == 3


def test_new_tensor_at_the_same_address_misses():
    """torch.from_numpy over one numpy buffer gives distinct tensor objects with the same data_ptr, shape, version (0) and
    device: the key is equal, only the weak reference tells them apart -- both while the first tensor lives and after it died
    (the recycled-address case)."""
    b = Build()
    buf = np.zeros((2, 3), dtype=np.float32)
    other = torch.ones(2, 3)
    t1 = torch.from_numpy(buf)
    ptr = t1.data_ptr()
    v1 = warp._cached("k", (t1, other), 0, b)
    t2 = torch.from_numpy(buf)
    assert t2 is not t1 and t2.data_ptr() == ptr and t2.shape == t1.shape and t2._version == t1._version
    v2 = warp._cached("k", (t2, other), 0, b)  # t1 alive
    assert b.calls == 2 and v2 is not v1
    del t1, t2
    gc.collect()
    t3 = torch.from_numpy(buf)
    assert t3.data_ptr() == ptr and t3._version == 0
    v3 = warp._cached("k", (t3, other), 0, b)  # the first owners of that address are dead
    assert b.calls == 3 and v3 is not v2
    assert warp._cached("k", (t3, other), 0, b) is v3 and b.calls == 3


def test_inference_mode_tensors_are_never_stored():
    b = Build()
    with torch.inference_mode():
        t = torch.zeros(2, 3)
    normal = torch.ones(2, 3)
    assert warp._version_of(t) is None and warp._version_of(normal) == 0
    warp._cached("k", (normal,), 0, b)
    before = len(warp._derived)
    v1 = warp._cached("k", (t, normal), 0, b)
    v2 = warp._cached("k", (normal, t), 0, b)
    v3 = warp._cached("k", (t, normal), 0, b)
    assert b.calls == 4 and v1 is not v3 and v2 is not v3
    assert len(warp._derived) == before == 1


def test_dead_source_drops_its_entry_on_the_next_miss():
    b = Build()
    keep = _srcs(2)
    dying = _srcs(2)
    warp._cached("k", keep, 0, b)
    warp._cached("k", dying, 0, b)
    warp._cached("k", (keep[0], dying[1]), 1, b)  # one dead source of two is enough
    assert len(warp._derived) == 3
    del dying
    gc.collect()
    warp._cached("k", keep, 0, b)  # a hit: sweeps nothing
    assert len(warp._derived) == 3 and b.calls == 3
    other = _srcs(1)
    warp._cached("k", other, 0, b)  # a miss: both entries with a dead source go
    assert b.calls == 4 and len(warp._derived) == 2
    assert warp._cached("k", keep, 0, b) == ("value", 1) and b.calls == 4


def test_34th_live_entry_clears_the_table():
    b = Build()
    live = [torch.zeros(1) + i for i in range(34)]
    for i in range(33):
        warp._cached("k", (live[i],), 0, b)
        assert len(warp._derived) == i + 1
    assert warp._cached("k", (live[0],), 0, b) == ("value", 1) and b.calls == 33  # 33 live entries: all still served
    warp._cached("k", (live[33],), 0, b)
    assert b.calls == 34 and len(warp._derived) == 1
    warp._cached("k", (live[0],), 0, b)  # gone with the rest
    assert b.calls == 35 and len(warp._derived) == 2


def test_data_copy_is_not_seen_until_invalidate_cache():
    """the documented hole: `t.data.copy_()` writes the storage without bumping t's version counter"""
    b = Build()
    srcs = _srcs()
    v1 = warp._cached("flow_occ", srcs, (8, True), b)
    ver = srcs[1]._version
    srcs[1].data.copy_(torch.full((2, 3), 7.0))
    assert float(srcs[1][0, 0]) == 7.0 and srcs[1]._version == ver
    assert warp._cached("flow_occ", srcs, (8, True), b) is v1 and b.calls == 1  # stale
    warp.invalidate_cache()
    assert len(warp._derived) == 0
    v2 = warp._cached("flow_occ", srcs, (8, True), b)
    assert b.calls == 2 and v2 is not v1


def test_prep_flow_occ_keys_on_height_and_dilate(monkeypatch):
    """_prep_flow_occ's own key: the four flow / occlusion tensors plus (feature height, with_dilate)"""
    calls = []
    monkeypatch.setattr(warp, "_prep_flow_occ_build", lambda h, fl, oc, d: calls.append((h, d)) or (h, d))
    flows, occs = list(_srcs(2)), list(_srcs(2))
    assert warp._prep_flow_occ(8, flows, occs, True) == (8, True)
    assert warp._prep_flow_occ(8, flows, occs, True) == (8, True)
    assert warp._prep_flow_occ(8, flows, occs, False) == (8, False)
    assert warp._prep_flow_occ(16, flows, occs, True) == (16, True)
    assert calls == [(8, True), (8, False), (16, True)]
    occs[0].mul_(0)
    assert warp._prep_flow_occ(8, flows, occs, True) == (8, True)
    assert calls[-1] == (8, True) and len(calls) == 4
