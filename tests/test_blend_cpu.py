"""CPU tests of the video_blend backend (fresco_amd.blend): the numpy model against the golden and against itself, the
argument checks and workspace sizes that need no GPU, the kernels' register budgets, and patch_video_blend's rebinding."""
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import blend_model as M  # noqa: E402
import make_blend_golden as G  # noqa: E402

from fresco_amd import FrescoHipError, _lib  # noqa: E402
from fresco_amd import blend as B  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "blend_golden.npz")


def golden_frames():
    """(name, case, golden dict, model dict with the DCT solve) for every golden frame, interval masks chained"""
    z = np.load(GOLDEN)
    out, prev = [], None
    for name, case in G.cases().items():
        assert str(z[name + "_sha256"]) == G.digest(case), "%s: regenerated inputs differ from the golden's" % name
        res = G.run_case(name, case, prev if name.startswith("interval_") else None, solver="dct")
        prev = z[name + "_mask"]
        out.append((name, case, {k: z["%s_%s" % (name, k)] for k in ("mask", "hist_lab", "poisson_lab")}, res))
    return out


def poisson_bars(got, ref, x=None):
    """Poisson bars in Lab bytes: at most 1 LSB anywhere, and at least 99.5 % equal per channel.  Against the
    reference's lsqr (x: the float64 exact solution + mean) the 99.5 % counts the pixels whose truncation is well
    defined, x at least 2e-3 from an integer: where x is an integer lsqr's noise of either sign decides it.  Returns
    the per-channel equal fractions over all pixels and over the counted ones."""
    d = np.abs(got.astype(int) - ref.astype(int))
    assert d.max() <= 1, int(d.max())
    keep = np.ones(d.shape, bool) if x is None else np.abs(x - np.round(x)) >= 2e-3
    eq = [float((d[..., c] == 0).mean()) for c in range(3)]
    eq_kept = [float((d[..., c][keep[..., c]] == 0).mean()) if keep[..., c].any() else 1.0 for c in range(3)]
    assert min(eq_kept) >= 0.995, (eq, eq_kept)
    return eq, eq_kept


def test_model_reproduces_golden():
    for name, case, g, res in golden_frames():
        assert np.array_equal(res["mask"], g["mask"]), name
        assert np.array_equal(res["hist_lab"], g["hist_lab"]), name


def _plain_histogram_blend_lab(a, b, min_error, weight1, weight2):
    """histogram_blend.blend as the model stated it before the zero-std rule: no constant channel is looked for"""
    a, b, m = M.bgr_to_lab(a), M.bgr_to_lab(b), M.bgr_to_lab(min_error)
    t_mean = np.ones([3], np.float32) * M.T_MEAN
    t_std = np.ones([3], np.float32) * M.T_STD

    def tr(img, means, stds, tm, ts):
        return (img.astype(np.float32) - means.reshape(1, 1, 3)) * ts.reshape(1, 1, 3) / stds.reshape(1, 1, 3) + \
            tm.reshape(1, 1, 3)

    A = tr(a, a.mean(axis=(0, 1)), a.std(axis=(0, 1)), t_mean, t_std)
    B_ = tr(b, b.mean(axis=(0, 1)), b.std(axis=(0, 1)), t_mean, t_std)
    ab = (A * weight1 + B_ * weight2 - M.T_MEAN) / 0.5 + M.T_MEAN
    return tr(ab, ab.mean(axis=(0, 1)), ab.std(axis=(0, 1)), m.mean(axis=(0, 1)), m.std(axis=(0, 1)))


def test_zero_std_rule_leaves_other_inputs_bit_identical():
    """no golden case has a constant channel, and there the model's values equal the plain formula's in every bit"""
    for name, case, g, res in golden_frames():
        me = M.min_error_image(case["oa"], case["ob"], res["mask"])
        for w in ((1 - case["weight1"], case["weight1"]), (0.7, 0.6)):
            if 0.0 in w:
                continue  # a weight of 0 with no constant channel: covered below, ab varies through the other image
            got = M.histogram_blend_values(case["oa"], case["ob"], me, *w)
            want = _plain_histogram_blend_lab(case["oa"], case["ob"], me, *w)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, w)
    case = G.cases()["odd"]
    me = M.min_error_image(case["oa"], case["ob"], case["prev_mask"])
    for w in ((1.0, 0.0), (0.0, 1.0)):
        assert np.array_equal(M.histogram_blend_values(case["oa"], case["ob"], me, *w),
                              _plain_histogram_blend_lab(case["oa"], case["ob"], me, *w)), w


def test_zero_std_rule_on_constant_channels():
    """a channel with std 0 transfers to the target mean, without a division by zero (numpy warnings are errors here)"""
    import warnings
    case = G.cases()["odd"]
    oa, ob, mask = case["oa"], case["ob"], case["prev_mask"]
    g_a, g_b = np.repeat(oa[..., 1:2], 3, -1), np.repeat(ob[..., 1:2], 3, -1)
    flat = np.ascontiguousarray(np.broadcast_to(np.asarray((40, 120, 200), np.uint8), oa.shape))
    assert M.constant_channels(M.bgr_to_lab(g_a)).tolist() == [False, True, True]
    assert M.constant_channels(M.bgr_to_lab(flat)).tolist() == [True, True, True]
    assert not M.constant_channels(M.bgr_to_lab(oa)).any()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        # grey + grey: a and b of the blend are the min-error image's mean, 128; L is what the plain formula gives
        me = M.min_error_image(g_a, g_b, mask)
        lab = M.histogram_blend_lab(g_a, g_b, me, 0.6, 0.4)
        assert (lab[..., 1:] == 128).all()
        with np.errstate(all="ignore"):
            plain = _plain_histogram_blend_lab(g_a, g_b, me, 0.6, 0.4)
        assert np.array_equal(M.histogram_blend_values(g_a, g_b, me, 0.6, 0.4)[..., 0], plain[..., 0])
        # grey + colour: a's a / b channels sit at 128 after the first transfer, so the blend follows b alone and equals
        # the transfer of b onto the min-error statistics
        me = M.min_error_image(g_a, ob, mask)
        got = M.histogram_blend_values(g_a, ob, me, 0.6, 0.4)
        only_b = M.histogram_blend_values(ob, ob, me, 0.0, 1.0)
        assert np.abs(got[..., 1:] - only_b[..., 1:]).max() < 1e-3
        # flat + texture: weight 0 on the texture leaves a constant blend -> the min-error mean in every value
        me = M.min_error_image(flat, ob, mask)
        lab_me = M.bgr_to_lab(me)
        v = M.histogram_blend_values(flat, ob, me, 1.0, 0.0)
        assert np.array_equal(v, np.broadcast_to(lab_me.mean(axis=(0, 1)), v.shape))
        # weight on the texture: the blend follows it in all three channels
        v = M.histogram_blend_values(flat, ob, me, 0.6, 0.4)
        assert np.abs(v - M.histogram_blend_values(ob, ob, me, 0.0, 1.0)).max() < 1e-3
        # equal images: correlation 1, the blend returns Lab(oa)
        assert np.array_equal(M.histogram_blend_lab(oa, oa, oa, 0.6, 0.4), M.bgr_to_lab(oa))
        res = M.blend_frame(g_a, g_b, case["d1"], case["d2"], 0.4, mask, case["flow"])
        assert (res["poisson_lab"][..., 1:] == 128).all() and np.isfinite(res["image"].astype(float)).all()


def test_dct_solve_equals_lsqr_on_golden():
    """The exact DCT solve against the reference-shaped lsqr (the golden) within the Poisson bars; before truncation
    the two agree to far below a grey level."""
    pytest.importorskip("scipy")
    report = []
    for name, case, g, res in golden_frames():
        hist = M.lab_to_bgr(res["hist_lab"])
        x_dct = M.poisson_solution(hist, case["oa"], case["ob"], res["mask"], solver="dct")
        x_lsqr = M.poisson_solution(hist, case["oa"], case["ob"], res["mask"], solver="lsqr")
        assert np.abs(x_dct - x_lsqr).max() < 5e-3, (name, float(np.abs(x_dct - x_lsqr).max()))
        eq, eq_kept = poisson_bars(res["poisson_lab"], g["poisson_lab"], x_dct)
        report.append("%s: max |x_dct - x_lsqr| %.1e, equal %s, well-defined equal %s"
                      % (name, np.abs(x_dct - x_lsqr).max(), np.round(eq, 4).tolist(), np.round(eq_kept, 4).tolist()))
    print("\n".join(report))


def test_dct_solve_is_the_normal_equations_solution():
    """x from the DCT solve satisfies (I + w^2 (Gx^T Gx + Gy^T Gy)) x = w^2 (Gx^T gx + Gy^T gy) + im to rounding"""
    rng = np.random.default_rng(3)
    h, w, wt = 9, 14, 2.5
    gx, gy, im = (rng.standard_normal((h, w)) * 20 for _ in range(3))
    gx[-1] = 0
    gy[:, -1] = 0
    x = M._solve_dct(gx, gy, im, wt)
    dx = np.zeros_like(x)
    dx[:-1] = x[:-1] - x[1:]
    dy = np.zeros_like(x)
    dy[:, :-1] = x[:, :-1] - x[:, 1:]

    def adj(g, axis):
        r = g.copy()
        if axis == 0:
            r[1:] -= g[:-1]
        else:
            r[:, 1:] -= g[:, :-1]
        return r

    lhs = x + wt * wt * (adj(dx, 0) + adj(dy, 1))
    rhs = im + wt * wt * (adj(gx, 0) + adj(gy, 1))
    assert np.abs(lhs - rhs).max() < 1e-9


def test_lab_round_trip_and_fixed_points():
    """Every colour of the cube: BGR -> Lab -> BGR -> Lab lands within 1 of its first Lab code.  (The BGR side does not
    round-trip: 8-bit Lab holds fewer colours than 8-bit BGR; 75 % of the cube comes back within 1.)"""
    v = np.arange(256, dtype=np.uint8)
    cube = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    lab = M.bgr_to_lab(cube)
    d = np.abs(M.bgr_to_lab(M.lab_to_bgr(lab)).astype(int) - lab.astype(int))
    assert d.max() <= 1 and (d == 0).mean() > 0.99, (int(d.max()), float((d == 0).mean()))
    assert np.array_equal(M.bgr_to_lab(np.array([[0, 0, 0]], np.uint8)), [[0, 128, 128]])
    assert np.array_equal(M.bgr_to_lab(np.array([[255, 255, 255]], np.uint8)), [[255, 128, 128]])
    for g in (1, 50, 128, 200, 254):
        lab = M.bgr_to_lab(np.array([[g, g, g]], np.uint8))
        assert tuple(lab[0, 1:]) == (128, 128), (g, lab)
        assert np.array_equal(M.lab_to_bgr(lab), [[g, g, g]]), (g, lab)
    assert np.array_equal(M.lab_to_bgr(np.array([[0, 128, 128]], np.uint8)), [[0, 0, 0]])
    assert np.array_equal(M.lab_to_bgr(np.array([[255, 128, 128]], np.uint8)), [[255, 255, 255]])


def test_error_mask_weights():
    d1 = np.array([[1.0, 2.0, 3.0]], np.float32)
    d2 = np.array([[2.0, 2.0, 2.0]], np.float32)
    assert np.array_equal(M.error_mask(d1, d2, 0.5, 0.5), [[0, 1, 1]])
    assert np.array_equal(M.error_mask(d1, d2, 0.0, 1.0), [[0, 0, 0]])
    assert np.array_equal(M.error_mask(d1, d2, 1.0, 0.0), [[1, 1, 1]])


def test_warp_model_matches_torch_grid_sample():
    import torch.nn.functional as F
    case = G.cases()["odd"]
    prev, flow = case["prev_mask"], case["flow"]
    h, w = prev.shape
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    grid = torch.stack([x, y]).float()[None] + torch.from_numpy(flow)
    g = torch.stack([2 * grid[:, 0] / (w - 1) - 1, 2 * grid[:, 1] / (h - 1) - 1], -1)
    ref = F.grid_sample(torch.from_numpy(prev).float()[None, None], g, mode="nearest", padding_mode="zeros",
                        align_corners=True)[0, 0].to(torch.uint8).numpy()
    assert np.array_equal(M.warp_nearest(prev, flow), ref)


def _img(h=8, w=8):
    return torch.zeros((h, w, 3), dtype=torch.uint8)


def test_argument_checks_need_no_gpu():
    a, d = _img(), torch.zeros((8, 8))
    with pytest.raises(FrescoHipError):  # CPU tensors
        B.blend_frame(a, a, d, d, 0.5)
    with pytest.raises(FrescoHipError):
        B.histogram_blend(a, a, a)
    with pytest.raises(FrescoHipError):
        B.poisson_fusion(a, a, a, torch.zeros((8, 8), dtype=torch.uint8))
    with pytest.raises(FrescoHipError):
        B.bgr_to_lab(a)
    with pytest.raises(ValueError):  # channels
        B.blend_frame(torch.zeros((8, 8, 4), dtype=torch.uint8), a, d, d, 0.5)
    with pytest.raises(ValueError):  # error map dtype
        B.blend_frame(a, a, d.double(), d, 0.5)
    with pytest.raises(ValueError):  # shape mismatch
        B.blend_frame(a, _img(8, 9), d, d, 0.5)
    with pytest.raises(ValueError):  # prev_mask without flow
        B.blend_frame(a, a, d, d, 0.5, prev_mask=torch.zeros((8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError):  # flow shape
        B.blend_frame(a, a, d, d, 0.5, torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((1, 2, 8, 7)))
    with pytest.raises(ValueError):
        B.blend_frame(a, a, d, d, 1.5)
    with pytest.raises(ValueError):
        B.poisson_fusion(a, a, a, torch.zeros((8, 8), dtype=torch.uint8), grad_weight=(1.0, 2.0))
    with pytest.raises(ValueError):
        B.blend_interval([a], [a], [d], [d], [None])
    with pytest.raises(ValueError):
        B.error_mask(d, d, 0.3, 0.3)


def _expected_ws(w, h):
    def al(x):
        return (x + 255) // 256 * 256
    n = w * h
    return al(32 * 8) + 3 * al(3 * n) + 2 * al(12 * n) + 2 * al(4 * h * h) + 2 * al(4 * w * w) + al(4 * h) + al(4 * w)


def test_workspace_bytes():
    lib = _lib.load()
    for w, h in ((512, 512), (96, 64), (53, 37), (2, 2), (4096, 4096), (4096, 2)):
        assert lib.fresco_blend_workspace_bytes(w, h) == _expected_ws(w, h), (w, h)
        assert B.workspace_bytes(h, w) == _expected_ws(w, h)
    for w, h in ((1, 512), (512, 1), (4097, 8), (8, 4097), (0, 0), (-3, 8)):
        assert lib.fresco_blend_workspace_bytes(w, h) == 0, (w, h)


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_blend_kernels_do_not_spill(tmp_path):
    """Every blend.hip kernel keeps to registers: no spills, no scratch (the listing method of test_kernel_resources)."""
    src = os.path.join(os.path.dirname(HERE), "fresco_amd", "csrc", "blend.hip")
    out = str(tmp_path / "blend.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                    "--cuda-device-only", "-c", src, "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=600)
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", open(out).read(), re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = (int(g("vgpr_spill_count")), int(g("private_segment_fixed_size")))
    names = " ".join(kernels)
    for k in ("blend_prep", "blend_rhs", "blend_tables", "blend_gemm", "blend_bgr2lab", "blend_lab2bgr"):
        assert k in names, (k, names)
    assert all(v == (0, 0) for v in kernels.values()), kernels


def test_patch_video_blend_rebinds_process_seq():
    vb = types.SimpleNamespace(process_seq=None, cv2=None, load_error=None, flow_calc=None)
    B.patch_video_blend(vb)
    assert callable(vb.process_seq) and vb.process_seq.__module__ == "fresco_amd.blend"
    with pytest.raises(ValueError, match="blend_histogram"):
        vb.process_seq(None, 0, blend_histogram=False)
