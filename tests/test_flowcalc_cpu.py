"""fresco_amd.flowcalc without a GPU: the library's new symbols, the padder arithmetic and the sizes refused before any
launch, pair scheduling (which pairs per chain, which files, swapped-pair sharing), existing files left alone, the files
written through the caller module's cv2 as the reference writes them, and patch_flow_calc."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import fresco_amd
from fresco_amd import _lib, flowcalc as FC, propagate as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import video_blend_standins as S  # noqa: E402


class NoModel(torch.nn.Module):
    """a flow model that must not run"""

    def forward_normalised(self, *a, **k):
        raise AssertionError("the network ran")


def test_library_exports_the_flowcalc_entry_points():
    assert "fresco_flowcalc_input" in _lib.SIGNATURES and "fresco_flowcalc_output" in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert hasattr(lib, "fresco_flowcalc_input") and hasattr(lib, "fresco_flowcalc_output")
    header = open(os.path.join(os.path.dirname(HERE), "include", "fresco_hip.h")).read()
    assert "int fresco_flowcalc_input(" in header and "int fresco_flowcalc_output(" in header


def test_package_exports():
    assert fresco_amd.FlowCalc is FC.FlowCalc and fresco_amd.patch_flow_calc is FC.patch_flow_calc


def _input_padder(h, w, factor=8):
    """utils.utils.InputPadder(mode='sintel')._pad, restated"""
    pad_ht = (((h // factor) + 1) * factor - h) % factor
    pad_wd = (((w // factor) + 1) * factor - w) % factor
    return [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]


@pytest.mark.parametrize("h,w", [(96, 128), (123, 171), (512, 512), (17, 33), (2, 2), (8, 9), (720, 1280)])
def test_padder_arithmetic(h, w):
    l, r, t, b = _input_padder(h, w)
    assert FC.padding(h, w) == (t, b, l, r)
    assert FC.padded_size(h, w) == (h + t + b, w + l + r)
    x = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w)
    padded = torch.nn.functional.pad(x, [l, r, t, b], mode="replicate")
    assert tuple(padded.shape[-2:]) == FC.padded_size(h, w)


def test_golden_pads():
    assert FC.padding(96, 128) == (0, 0, 0, 0)
    assert FC.padding(123, 171) == (2, 3, 2, 3) and FC.padded_size(123, 171) == (128, 176)


@pytest.mark.parametrize("h,w", [(1, 64), (64, 1), (64, 72), (72, 64), (100, 100), (8, 8)])
def test_refused_sizes(h, w):
    with pytest.raises(ValueError):
        FC.check_size(h, w)


@pytest.mark.parametrize("h,w", [(16, 16), (96, 128), (123, 171), (512, 512), (720, 1280)])
def test_accepted_sizes(h, w):
    FC.check_size(h, w)


def _frames(n, h=96, w=128, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]


def test_refused_before_any_launch(tmp_path):
    fc = FC.FlowCalc(flow_model=NoModel(), cv2=S.cv2)
    fr = _frames(2)
    with pytest.raises(ValueError, match="different sizes"):
        fc.get_flows([fr[0], fr[1][:64]], [(0, 1)], [str(tmp_path / "f.npy")])
    with pytest.raises(ValueError, match="windows"):
        fc.get_flows(_frames(2, 100, 100), [(0, 1)], [str(tmp_path / "f.npy")])
    with pytest.raises(ValueError, match="uint8"):
        fc.get_flow(fr[0].astype(np.float32), fr[1], str(tmp_path / "f.npy"))
    with pytest.raises(ValueError, match="outside"):
        fc.get_flows(fr, [(0, 2)], [None])
    assert not os.listdir(tmp_path)


def test_schedule_shares_swapped_pairs():
    pairs = [(0, 1), (1, 2), (2, 3), (3, 2), (2, 1), (1, 0), (1, 2)]
    forwards, plan = FC.schedule(pairs, share=True)
    assert forwards == [(0, 1), (1, 2), (2, 3)]
    assert plan == [(0, False), (1, False), (2, False), (2, True), (1, True), (0, True), (1, False)]
    forwards, plan = FC.schedule(pairs, share=False)
    assert forwards == [(0, 1), (1, 2), (2, 3), (3, 2), (2, 1), (1, 0)]
    assert plan == [(k, False) for k in range(6)] + [(1, False)]


def test_video_blend_chains_share_all_but_the_ends():
    """the driver's pairs for an interval of length L: forward chain (k, k+1), backward chain (k+1, k); every
    backward pair but the one at each end is the swap of a forward pair"""
    base = "/nonexistent"
    vs = S.VideoSequence.__new__(S.VideoSequence)
    vs.base, vs.key_ind, vs.input_dir = base, [0, 5, 9], base + "/video"
    vs.key_dir, vs.tmp_dir, vs.n_seq = base + "/keys", base + "/tmp", 2
    chains = [P.Chain(vs, i, fwd) for i in range(vs.n_seq) for fwd in (True, False)]
    slot, pairs, saves = {}, [], []
    for c in chains:
        for j in range(c.interval - 1):
            for p in c.inputs[j:j + 2]:
                slot.setdefault(p, len(slot))
            pairs.append((slot[c.inputs[j]], slot[c.inputs[j + 1]]))
            saves.append(os.path.basename(c.flows[j]))
    # interval 0..5: forward flows of 0->1 .. 3->4 into flow_f_0000..0003, backward 5->4 .. 2->1 into flow_b_0005..0002
    assert saves[:8] == ["flow_f_%04d.npy" % k for k in range(4)] + ["flow_b_%04d.npy" % k for k in (5, 4, 3, 2)]
    forwards, plan = FC.schedule(pairs)
    shared = [saves[r] for r, (_, sw) in enumerate(plan) if sw]
    assert shared == ["flow_b_%04d.npy" % k for k in (4, 3, 2)] + ["flow_b_%04d.npy" % k for k in (8, 7)]
    assert len(forwards) == len(pairs) - 5


def test_existing_files_are_neither_recomputed_nor_rewritten(tmp_path):
    fr = _frames(3)
    paths = [str(tmp_path / ("flow_%d.npy" % k)) for k in range(2)]
    want = []
    for p in paths:
        f = np.random.default_rng(len(want)).standard_normal((1, 2, 96, 128)).astype(np.float32)
        np.save(p, f)
        S.cv2.imwrite(os.path.splitext(p)[0] + ".png", np.zeros((96, 128, 1), np.int64))
        want.append(f)
    snap = lambda: {p.name: (p.stat().st_mtime_ns, p.read_bytes()) for p in tmp_path.iterdir()}  # noqa: E731
    before = snap()
    fc = FC.FlowCalc(flow_model=NoModel(), cv2=S.cv2)
    got = fc.get_flows(fr, [(0, 1), (1, 0)], paths)
    for g, w in zip(got, want):
        assert isinstance(g, torch.Tensor) and np.array_equal(g.numpy(), w)
    assert np.array_equal(fc.get_flow(fr[0], fr[1], paths[0]).numpy(), want[0])
    assert np.array_equal(fc.get_mask(fr[0], fr[1], paths[0]), np.zeros((96, 128), np.uint8))
    assert snap() == before and fc.stats["forwards"] == 0


def test_files_go_through_the_modules_cv2_as_the_reference_writes_them(tmp_path):
    calls = []
    cv2 = types.SimpleNamespace(imwrite=lambda path, arr: calls.append((path, np.array(arr))) or True)
    flow = np.random.default_rng(0).standard_normal((1, 2, 5, 7)).astype(np.float32)
    occ = (np.arange(35).reshape(5, 7) % 3 == 0).astype(np.uint8) * 255
    path = str(tmp_path / "flow_f_0003.npy")
    FC.write_outputs(cv2, path, flow, occ)
    saved = np.load(path)
    assert saved.dtype == np.float32 and saved.shape == (1, 2, 5, 7) and np.array_equal(saved, flow)
    # flow_utils: bwd_occ.cpu().permute(1, 2, 0).to(torch.long).numpy() * 255
    ref = torch.from_numpy(occ != 0).float()[None].permute(1, 2, 0).to(torch.long).numpy() * 255
    (p, arr), = calls
    assert p == str(tmp_path / "flow_f_0003.png")
    assert arr.dtype == ref.dtype == np.int64 and arr.shape == ref.shape == (5, 7, 1) and np.array_equal(arr, ref)
    assert not os.path.exists(p)  # nothing written around the module's cv2


def test_patch_flow_calc_rebinds_both_names(monkeypatch):
    guide = types.SimpleNamespace(read_flow=S.read_flow, read_mask=S.read_mask, flow_calc="reference")
    monkeypatch.setitem(sys.modules, "blender.guide", guide)
    vb = types.SimpleNamespace(cv2=S.cv2, flow_calc="reference")
    fc = FC.FlowCalc(flow_model=NoModel())
    assert FC.patch_flow_calc(vb, fc) is vb
    assert vb.flow_calc is fc and guide.flow_calc is fc and fc.cv2 is S.cv2


def test_warp_modes_other_than_nearest_raise():
    fc = FC.FlowCalc(flow_model=NoModel())
    with pytest.raises(NotImplementedError, match="nearest"):
        fc.warp(np.zeros((4, 4, 3), np.uint8), torch.zeros(1, 2, 4, 4), "bilinear")
    with pytest.raises(NotImplementedError, match="nearest"):
        fc.warp(np.zeros((4, 4, 3), np.uint8), torch.zeros(1, 2, 4, 4))
