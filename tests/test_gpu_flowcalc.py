"""fresco_amd.flowcalc on the GPU.

1. fresco_flowcalc_input is bit-identical to torch's replicate pad + GMFlow.forward's normalisation on the device.
2. fresco_flowcalc_output: masks bit-identical to fresco_amd.forward_backward_consistency_check of the unpadded flows,
   flows an exact copy of the unpadded slice, the swapped outputs the same check with the roles exchanged.
3. Against tests/golden/flowcalc_golden.npz (make_flowcalc_golden.py: the reference's FlowCalc.get_flow on CPU with the
   closed-form stand-in weights): flows within tests/test_gmflow.py's bar for stand-in weights, masks disagreeing only
   at pixels within twice the case's flow error of the threshold, the saved files of the reference's shape and dtype.
4. get_flows, batched and shared, against a per-call get_flow loop on the same model; a shared (k+1, k) against running
   (k+1, k) itself.
5. The stage: propagate.run_ebsynth on the stand-in video with patch_flow_calc and a stand-in-weight FlowCalc.
"""
import hashlib
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import closed_form as cf
from fresco_amd import flowcalc as FC, propagate as P
from fresco_amd import forward_backward_consistency_check

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import video_blend_standins as S  # noqa: E402
from test_gpu_guides import warp_model  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "flowcalc_golden.npz")
CASES = {"a": (96, 128), "b": (123, 171)}


@pytest.fixture(scope="module")
def model():
    import fresco_amd.gmflow as G
    m = G.GMFlow(**FC.CONFIG).eval()
    sd = m.state_dict()
    m.load_state_dict({k: cf.gmflow_param(k, tuple(v.shape)) for k, v in sd.items()})
    return m.cuda()


def frames_of(h, w, n=2):
    """as make_flowcalc_golden.frames_of: closed-form frames rounded to uint8 HWC"""
    return [f.permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).numpy().copy() for f in cf.gmflow_frames(n, h, w)]


def epe(a, b):
    return (torch.as_tensor(a).float() - torch.as_tensor(b).float()).pow(2).sum(-3).sqrt()


def torch_input(frame, dev="cuda"):
    """what FlowCalc.get_flow + GMFlow.forward compute on the device for one image"""
    x = torch.from_numpy(frame).permute(2, 0, 1).float()[None].to(dev)
    t, b, l, r = FC.padding(*frame.shape[:2])
    x = F.pad(x, [l, r, t, b], mode="replicate")
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
    return (x / 255.0 - mean) / std


def margin(fwd, bwd):
    """|bwd + warp(fwd, bwd)| - (0.01 (|fwd| + |bwd|) + 0.5), geometry.py's operations in torch: (B, H, W)"""
    b, _, h, w = bwd.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=bwd.device), torch.arange(w, device=bwd.device), indexing="ij")
    g = torch.stack((xs, ys), 0).float()[None] + bwd
    grid = torch.stack((2 * g[:, 0] / (w - 1) - 1, 2 * g[:, 1] / (h - 1) - 1), -1)
    warped = F.grid_sample(fwd, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    diff = torch.norm(bwd + warped, dim=1)
    return diff - (0.01 * (torch.norm(fwd, dim=1) + torch.norm(bwd, dim=1)) + 0.5)


class RecordingCv2:
    def __init__(self):
        self.writes = {}

    def imwrite(self, path, arr):
        self.writes[path] = np.array(arr)
        return S.cv2.imwrite(path, arr)

    def __getattr__(self, name):
        return getattr(S.cv2, name)


# ---------------------------------------------------------------------------------------------------------------------
# 1. input
@pytest.mark.parametrize("hw", list(CASES.values()))
@pytest.mark.parametrize("npairs", [1, 16])
def test_input_is_torchs_pad_and_normalise(hw, npairs):
    h, w = hw
    rng = np.random.default_rng(npairs + h)
    frames = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(5)]
    frames[0][:] = np.arange(256, dtype=np.uint8)[np.arange(h * w * 3) % 256].reshape(h, w, 3)  # every byte value
    first = rng.integers(0, 5, npairs)
    second = rng.integers(0, 5, npairs)
    first[0], second[0] = 0, 0  # one frame on both sides of a pair, and (with 16 pairs) in several pairs
    dev_frames = torch.from_numpy(np.stack(frames)).cuda()
    got = FC.flowcalc_input(dev_frames, first, second)
    want = torch.cat([torch_input(frames[i]) for i in list(first) + list(second)], 0)
    assert got.shape == want.shape == (2 * npairs, 3) + FC.padded_size(h, w)
    assert torch.equal(got, want), float((got - want).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 2. output
def _flows(P_, hp, wp, kind, seed):
    """(2P, 2, hp, wp): forward fields, then backward fields that undo them up to a perturbation of about the
    threshold, so that both outcomes of the check occur; a band of rows points far outside the image"""
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        # half-pixel values constant over 16 x 16 blocks (ties of the bilinear taps), per-pixel noise on a quarter
        blk = torch.randint(-6, 7, (P_, 2, hp // 16 + 1, wp // 16 + 1), generator=g).float() * 0.5
        fwd = blk.repeat_interleave(16, 2).repeat_interleave(16, 3)[:, :, :hp, :wp].contiguous()
        fwd += 0.2 * torch.randn(P_, 2, hp, wp, generator=g) * (torch.rand(P_, 1, hp, wp, generator=g) < 0.25)
        pert = 0.4 * torch.randn(P_, 2, hp, wp, generator=g)
    else:
        fwd = cf.flow(P_, hp, wp, 1.0)  # smooth, closed form
        _, _, i, j = cf._grid(P_, 2, hp, wp)
        pert = (0.6 * torch.sin(0.3 * i + 0.7 * j + 1.3 * torch.arange(2).view(1, 2, 1, 1))).float()
    bwd = -fwd + pert
    fwd[:, :, 4:6] *= 40.0
    return torch.cat([fwd, bwd], 0)


@pytest.mark.parametrize("hw", list(CASES.values()) + [(45, 30)])
@pytest.mark.parametrize("kind", ["random", "closed"])
def test_output_is_unpad_and_consistency_check(hw, kind):
    h, w = hw
    hp, wp = FC.padded_size(h, w)
    t, _, l, _ = FC.padding(h, w)
    P_ = 3
    flows = _flows(P_, hp, wp, kind, h + w).cuda()
    bf, bo, ff, fo = FC.flowcalc_output(flows, h, w, swapped=True)
    bf1, bo1 = FC.flowcalc_output(flows, h, w, swapped=False)
    fwd = flows[:P_, :, t:t + h, l:l + w].contiguous()
    bwd = flows[P_:, :, t:t + h, l:l + w].contiguous()
    focc, bocc = forward_backward_consistency_check(fwd, bwd)
    assert torch.equal(bf, bwd) and torch.equal(ff, fwd) and torch.equal(bf1, bwd)
    assert bo.dtype == torch.uint8 and set(torch.unique(bo).tolist()) <= {0, 255}
    assert torch.equal(bo, (bocc * 255).to(torch.uint8)) and torch.equal(bo1, bo)
    assert torch.equal(fo, (focc * 255).to(torch.uint8))
    # the swapped pair's own check: roles exchanged
    focc2, bocc2 = forward_backward_consistency_check(bwd, fwd)
    assert torch.equal(fo, (bocc2 * 255).to(torch.uint8)) and torch.equal(bo, (focc2 * 255).to(torch.uint8))
    frac = float((bo != 0).float().mean())
    print("flowcalc_output %s %dx%d: occluded fraction %.3f" % (kind, h, w, frac))
    assert 0.05 < frac < 0.95 and 0.05 < float((fo != 0).float().mean()) < 0.95


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the reference
@pytest.mark.parametrize("tag", list(CASES))
def test_get_flow_matches_the_reference(tag, model, tmp_path):
    g = np.load(GOLDEN)
    h, w = CASES[tag]
    fr = frames_of(h, w)
    assert hashlib.sha256(np.stack(fr).tobytes()).hexdigest() == str(g["frames_sha256_" + tag])
    cv2 = RecordingCv2()
    fc = FC.FlowCalc(flow_model=model, cv2=cv2)
    for order, (i, j) in (("ab", (0, 1)), ("ba", (1, 0))):
        key = "%s_%s" % (tag, order)
        path = str(tmp_path / ("flow_%s.npy" % key))
        ret = fc.get_flow(fr[i], fr[j], path)
        assert ret.is_cuda and tuple(ret.shape) == (1, 2, h, w)
        saved = np.load(path)
        ref = g["flow_" + key]
        assert saved.dtype == ref.dtype == np.dtype(str(g["npy_dtype"])) and saved.shape == ref.shape
        assert np.array_equal(saved, ret.cpu().numpy())
        e = epe(saved, ref)
        emax, emean = float(e.max()), float(e.mean())
        mask = cv2.writes[str(tmp_path / ("flow_%s.png" % key))]
        assert str(mask.dtype) == str(g["mask_dtype"]) and str(mask.shape[2:]) == str(g["mask_shape_suffix"])
        assert mask.shape == (h, w, 1)
        dis = (mask[..., 0] != 0) != (g["mask_" + key][..., 0] != 0)
        m = g["margin_" + key].astype(np.float32)
        print("get_flow %s: EPE vs the reference max %.4f mean %.5f px; mask disagreement %.4f (max |margin| there %.3g)"
              % (key, emax, emean, float(dis.mean()), float(np.abs(m[dis]).max()) if dis.any() else 0.0))
        assert emax < 0.15 and emean < 0.05, (emax, emean)
        assert float(dis.mean()) <= 0.01
        assert np.all(np.abs(m[dis]) < 2 * emax)
        # read back: nothing computed, read_flow's tensor
        before = fc.stats["forwards"]
        back = fc.get_flow(fr[i], fr[j], path)
        assert fc.stats["forwards"] == before and not back.is_cuda and np.array_equal(back.numpy(), saved)
        gm = fc.get_mask(fr[i], fr[j], path)
        assert gm.dtype == np.uint8 and np.array_equal(gm != 0, mask[..., 0] != 0)


def test_warp_nearest_is_the_reference(model):
    rng = np.random.default_rng(5)
    fc = FC.FlowCalc(flow_model=model)
    h, w = 37, 53
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    flow = (rng.integers(-8, 9, (2, h, w)) * 0.5).astype(np.float32)
    flow[0, :4] = 3.0 * w
    got = fc.warp(img, torch.from_numpy(flow)[None], "nearest")
    assert got.dtype == np.uint8 and np.array_equal(got, warp_model(img, flow))
    m = rng.random((h, w)) < 0.3
    gm = fc.warp(m, torch.from_numpy(flow)[None], "nearest")
    assert gm.dtype == np.bool_ and np.array_equal(gm, warp_model(m.astype(np.uint8)[..., None], flow)[..., 0] != 0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. batched and shared against the per-call loop
def chain_pairs(n):
    """video_blend's forward chain over frames 0..n-1 and the backward chain back"""
    return [(k, k + 1) for k in range(n - 1)] + [(k + 1, k) for k in reversed(range(n - 1))]


def _loop(model, frames, pairs, base):
    os.makedirs(base)
    fc = FC.FlowCalc(flow_model=model, max_pairs=1, share=False, cv2=S.cv2)
    paths = [os.path.join(base, "flow_%02d.npy" % r) for r in range(len(pairs))]
    for (a, b), p in zip(pairs, paths):
        fc.get_flow(frames[a], frames[b], p)
    assert fc.stats["forwards"] == len(pairs)
    return paths


def _margins(model, frames, pairs):
    """per pair, the consistency margin of its own bidirectional forward (reference padder, GMFlow.forward)"""
    out = []
    for a, b in pairs:
        x0, x1 = (torch.from_numpy(frames[k]).permute(2, 0, 1).float()[None].cuda() for k in (a, b))
        t, bb, l, r = FC.padding(*frames[a].shape[:2])
        x0, x1 = (F.pad(x, [l, r, t, bb], mode="replicate") for x in (x0, x1))
        fl = model(x0, x1, attn_splits_list=[2], corr_radius_list=[-1], prop_radius_list=[-1],
                   pred_bidir_flow=True)["flow_preds"][-1]
        h, w = frames[a].shape[:2]
        fl = fl[:, :, t:t + h, l:l + w]
        out.append(margin(fl[:1].contiguous(), fl[1:].contiguous())[0].cpu().numpy())
    return out


def assert_same_outputs(paths, want_paths, margins, exact=True):
    """flows within 1e-3 px EPE and masks differing only where |margin| < 1e-2 -- and, since batching and sharing turned
    out bit-identical to the per-call loop on an MI355X (the network's kernels are batch-invariant and its transformer
    symmetric in the two images), identical files when `exact`"""
    worst = 0.0
    for p, q, m in zip(paths, want_paths, margins):
        a, b = np.load(p), np.load(q)
        e = float(epe(a, b).max())
        worst = max(worst, e)
        assert e < 1e-3, (p, e)
        ma, mb = S.read_mask(p), S.read_mask(q)
        dis = (ma != 0) != (mb != 0)
        assert np.all(np.abs(m[dis]) < 1e-2), (p, float(np.abs(m[dis]).max()))
        if exact:
            assert np.array_equal(a, b) and np.array_equal(ma, mb), (p, e, int(dis.sum()))
    return worst


@pytest.mark.parametrize("max_pairs,share", [(4, True), (16, True), (3, False)])
def test_get_flows_batched_and_shared_match_the_per_call_loop(model, tmp_path, max_pairs, share):
    frames = frames_of(123, 171, n=5)
    pairs = chain_pairs(5)
    want = _loop(model, frames, pairs, str(tmp_path / "loop"))
    os.makedirs(tmp_path / "batch")
    paths = [str(tmp_path / "batch" / ("flow_%02d.npy" % r)) for r in range(len(pairs))]
    fc = FC.FlowCalc(flow_model=model, max_pairs=max_pairs, share=share, cv2=S.cv2)
    ret = fc.get_flows(frames, pairs, paths)
    n_fwd = len(FC.schedule(pairs, share)[0])
    assert fc.stats["pairs"] == n_fwd and fc.stats["forwards"] == -(-n_fwd // max_pairs)
    assert n_fwd == (4 if share else 8)
    for r, p in zip(ret, paths):
        assert not r.is_cuda and tuple(r.shape) == (1, 2, 123, 171) and np.array_equal(r.numpy(), np.load(p))
    assert FC.FlowCalc(flow_model=model, max_pairs=max_pairs, share=share).get_flows(
        frames, pairs, paths, return_flows=False) is None
    margins = _margins(model, frames, pairs)
    worst = assert_same_outputs(paths, want, margins)
    _, plan = FC.schedule(pairs, share)
    shared = [r for r, (_, sw) in enumerate(plan) if sw]
    assert len(shared) == (4 if share else 0)
    # shared (k+1, k) against running (k+1, k) itself: the same bars
    assert_same_outputs([paths[r] for r in shared], [want[r] for r in shared], [margins[r] for r in shared])
    identical = all(np.array_equal(np.load(p), np.load(q)) for p, q in zip(paths, want))
    print("get_flows max_pairs %d share %s: max EPE vs the per-call loop %.2e px, bit-identical %s"
          % (max_pairs, share, worst, identical))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the stage
@pytest.fixture
def guide_module(monkeypatch):
    gm = types.SimpleNamespace(read_flow=S.read_flow, read_mask=S.read_mask, flow_calc=None)
    monkeypatch.setitem(sys.modules, "blender.guide", gm)
    return gm


def _stage(base, fc, **kw):
    S.make_video(base, S.KEY_IND, h=32, w=48)
    vs = S.VideoSequence(base, S.KEY_IND)
    vb = types.SimpleNamespace(cv2=S.cv2, flow_calc=types.SimpleNamespace(get_flow=S.get_flow))
    FC.patch_flow_calc(vb, fc)
    P.patch_run_ebsynth(vb, **kw)
    vb.run_ebsynth(vs)
    return vs


def test_stage_runs_on_flowcalc(model, tmp_path, guide_module):
    fc = FC.FlowCalc(flow_model=model, max_pairs=16, share=True)
    base = str(tmp_path / "run")
    stats = {}
    vs = _stage(base, fc, stats=stats)
    assert guide_module.flow_calc is fc
    # KEY_IND [0, 3, 7]: 2 + 2 + 3 + 3 pairs, 1 + 2 of them shared
    assert fc.stats["pairs"] == 7 and fc.stats["forwards"] == 1
    ref_fc = FC.FlowCalc(flow_model=model, max_pairs=1, share=False)
    ref_base = str(tmp_path / "ref")
    _stage(ref_base, ref_fc, synth=S.answer_all)
    assert ref_fc.stats["forwards"] == 10
    flows = sorted(f for f in os.listdir(vs.tmp_dir) if f.endswith(".npy"))
    assert len(flows) == 10 and flows == sorted(f for f in os.listdir(os.path.join(ref_base, "tmp")) if f.endswith(".npy"))
    frames = [S.imread(os.path.join(base, "video", "%04d.png" % t)) for t in range(S.KEY_IND[-1] + 1)]
    pairs = [(k, k + 1) if f.startswith("flow_f") else (k, k - 1) for f in flows for k in [int(f[7:11])]]
    assert_same_outputs([os.path.join(vs.tmp_dir, f) for f in flows], [os.path.join(ref_base, "tmp", f) for f in flows],
                        _margins(model, frames, pairs))
    # the rest of the stage completed: every output frame and its error map
    for i in range(vs.n_seq):
        for fwd in (True, False):
            for out in vs.get_output_sequence(i, fwd):
                assert os.path.exists(out)
    # existing flow files are left byte-identical and nothing is recomputed
    tmp = vs.tmp_dir
    before = {f: (os.stat(os.path.join(tmp, f)).st_mtime_ns, open(os.path.join(tmp, f), "rb").read())
              for f in os.listdir(tmp) if f.endswith((".npy", ".png"))}
    fc2 = FC.FlowCalc(flow_model=model, max_pairs=16)
    _stage(base, fc2, synth=S.answer_all)
    assert fc2.stats["forwards"] == 0
    after = {f: (os.stat(os.path.join(tmp, f)).st_mtime_ns, open(os.path.join(tmp, f), "rb").read())
             for f in os.listdir(tmp) if f.endswith((".npy", ".png"))}
    assert after == before
