"""GPU tests of the video_blend backend (fresco_amd.blend, csrc/blend.hip) against the numpy model tests/blend_model.py,
torch's CPU grid_sample and the golden (tests/golden/blend_golden.npz, reference-shaped lsqr)."""
import os
import struct
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
from test_blend_cpu import golden_frames, poisson_bars  # noqa: E402

from fresco_amd import _lib  # noqa: E402
from fresco_amd import blend as B  # noqa: E402
from fresco_amd.ebsynth import write_error_bin  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def gpu(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dtype)


def cpu(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def lab_neighbour_ok(got_bgr, model_lab):
    """per pixel: got_bgr is the Lab -> BGR conversion of some Lab code within 1 of model_lab in every channel (what a
    1 LSB Lab difference can turn into after the final conversion); returns the fraction of pixels that differ"""
    got_bgr, model_lab = got_bgr.reshape(-1, 3), model_lab.reshape(-1, 3)
    want = M.lab_to_bgr(model_lab)
    diff = np.nonzero(np.any(got_bgr != want, -1))[0]
    if diff.size:
        steps = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3)
        cand = np.clip(model_lab[diff][:, None, :].astype(int) + steps[None], 0, 255).astype(np.uint8)
        ok = np.any(np.all(M.lab_to_bgr(cand) == got_bgr[diff][:, None, :], -1), -1)
        assert ok.all(), (int((~ok).sum()), diff[~ok][:5])
    return diff.size / len(got_bgr)


def all_codes(lo, hi):
    c = np.arange(lo, hi, dtype=np.int64)
    return np.stack([c & 255, (c >> 8) & 255, c >> 16], -1).astype(np.uint8)


def test_lab_conversions_over_all_colours():
    """BGR -> Lab over all 2^24 colours and Lab -> BGR over all 2^24 codes: within 1 LSB of the model, >= 99.99 %
    equal"""
    for name, gfn, mfn in (("bgr_to_lab", B.bgr_to_lab, M.bgr_to_lab), ("lab_to_bgr", B.lab_to_bgr, M.lab_to_bgr)):
        worst, neq, total = 0, 0, 0
        step = 1 << 22
        for lo in range(0, 1 << 24, step):
            x = all_codes(lo, lo + step)
            got = cpu(gfn(gpu(x))).astype(int)
            d = np.abs(got - mfn(x).astype(int))
            worst = max(worst, int(d.max()))
            neq += int((d != 0).sum())
            total += d.size
        print("%s: %d of %d values differ from the model (max %d)" % (name, neq, total, worst))
        assert worst <= 1 and neq <= 1e-4 * total, (name, worst, neq)


def test_error_mask_exact():
    rng = np.random.default_rng(5)
    d1 = (rng.integers(0, 50, (61, 77)) / 4).astype(np.float32)
    d2 = (rng.integers(0, 50, (61, 77)) / 4).astype(np.float32)
    d1[0, :4] = [np.inf, 0, np.nan, 1e30]
    for w1 in (0.0, 1.0, 0.5, 0.2, 1 / 3, 0.8):
        got = cpu(B.error_mask(gpu(d1), gpu(d2), w1, 1 - w1))
        assert np.array_equal(got, M.error_mask(d1, d2, w1, 1 - w1)), w1


def test_propagated_mask_equals_torch_grid_sample():
    """weight1 = 0 makes the error mask all 0, so the frame's mask is the warped previous mask alone.  It must equal
    CPU grid_sample(nearest) but where the unnormalised coordinate lies within 1e-4 of a .5 boundary (<= 0.1 %)."""
    import torch.nn.functional as F
    rng = np.random.default_rng(6)
    for h, w in ((72, 56), (37, 53), (256, 320)):
        prev = (rng.random((h, w)) < 0.4).astype(np.uint8)
        flow = G.flow_field(300 + h, h, w)
        flow[0, :, h // 4: h // 4 + 3] += rng.standard_normal((2, 3, w)).astype(np.float32) * 7
        z = np.zeros((h, w), np.float32)
        img = gpu(np.zeros((h, w, 3), np.uint8))
        _, got = B.blend_frame(img, img, gpu(z), gpu(z), 0.0, gpu(prev), gpu(flow), gradient=False)
        got = cpu(got)
        y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        grid = torch.stack([x, y]).float()[None] + torch.from_numpy(flow)
        xg, yg = 2 * grid[:, 0] / (w - 1) - 1, 2 * grid[:, 1] / (h - 1) - 1
        ref = F.grid_sample(torch.from_numpy(prev).float()[None, None], torch.stack([xg, yg], -1), mode="nearest",
                            padding_mode="zeros", align_corners=True)[0, 0].to(torch.uint8).numpy()
        ux, uy = ((xg + 1) / 2 * (w - 1))[0].numpy(), ((yg + 1) / 2 * (h - 1))[0].numpy()
        tie = (np.abs(ux - np.floor(ux) - 0.5) < 1e-4) | (np.abs(uy - np.floor(uy) - 0.5) < 1e-4)
        bad = got != ref
        print("%dx%d: %d mismatches, %d pixels near a .5 boundary" % (h, w, bad.sum(), tie.sum()))
        assert not (bad & ~tie).any(), np.argwhere(bad & ~tie)[:5]
        assert bad.mean() <= 1e-3
        assert np.array_equal(got, M.warp_nearest(prev, flow))  # the model's restatement, exactly


def test_histogram_blend_within_one_lsb():
    for name, case, g, res in golden_frames():
        me = M.min_error_image(case["oa"], case["ob"], g["mask"])
        w1 = case["weight1"]
        out, lab = B.histogram_blend(gpu(case["oa"]), gpu(case["ob"]), gpu(me), 1 - w1, 1 - (1 - w1), return_lab=True)
        want = M.histogram_blend_lab(case["oa"], case["ob"], me, 1 - w1, 1 - (1 - w1))
        d = np.abs(cpu(lab).astype(int) - want.astype(int))
        assert d.max() <= 1 and (d == 0).mean() >= 0.999, (name, int(d.max()), float((d == 0).mean()))
        assert np.array_equal(cpu(out), M.lab_to_bgr(cpu(lab))), name


def test_poisson_fusion_against_golden_and_model():
    report = []
    for name, case, g, res in golden_frames():
        hist = M.lab_to_bgr(g["hist_lab"])
        out, lab = B.poisson_fusion(gpu(hist), gpu(case["oa"]), gpu(case["ob"]), gpu(g["mask"]), return_lab=True)
        lab = cpu(lab)
        x = M.poisson_solution(hist, case["oa"], case["ob"], g["mask"], solver="dct")
        eq_g, kept_g = poisson_bars(lab, g["poisson_lab"], x)
        eq_m, _ = poisson_bars(lab, M.poisson_fusion_lab(hist, case["oa"], case["ob"], g["mask"]))
        assert np.array_equal(cpu(out), M.lab_to_bgr(lab)), name
        report.append("%s: equal vs golden %s (well-defined %s), vs DCT model %s" % (
            name, np.round(eq_g, 4).tolist(), np.round(kept_g, 4).tolist(), np.round(eq_m, 5).tolist()))
    print("\n".join(report))


def interval_512(n=4, seed=7):
    s = 512
    frames = [G.frame(seed + k, s, s) for k in range(n)]
    flows = [(G.smooth(seed + 50 + k, s, s, 2, 16).transpose(2, 0, 1)[None] / 1023.0 * 9 - 4.5 + 1 / 3)
             .astype(np.float32) for k in range(n - 1)]
    return frames, flows


def test_blend_interval_512_within_stage_bars():
    """The whole loop at 512^2.  Bars from the stage errors: the mask is exact (no flow lands on a .5 tie here);
    the histogram blend is within 1 Lab LSB at <= 0.1 % of values and the Poisson solve within 1 at <= 0.5 % per
    channel, so every pixel of the image must be the conversion of a Lab code within 1 of the model's, and at most
    3 x (0.5 + 0.1) % = 1.8 % of pixels may differ."""
    frames, flows = interval_512()
    n = len(frames)
    imgs = B.blend_interval([gpu(f["oa"]) for f in frames], [gpu(f["ob"]) for f in frames],
                            [gpu(f["d1"]) for f in frames], [gpu(f["d2"]) for f in frames], [gpu(f) for f in flows])
    ref = M.blend_interval([f["oa"] for f in frames], [f["ob"] for f in frames], [f["d1"] for f in frames],
                           [f["d2"] for f in frames], flows)
    prev = None
    for k in range(n):
        _, mask = B.blend_frame(gpu(frames[k]["oa"]), gpu(frames[k]["ob"]), gpu(frames[k]["d1"]),
                                gpu(frames[k]["d2"]), k / n, prev, gpu(flows[k - 1]) if k else None)
        assert np.array_equal(cpu(mask), ref[k]["mask"]), k
        prev = mask
        frac = lab_neighbour_ok(cpu(imgs[k]), ref[k]["poisson_lab"])
        print("frame %d: %.4f %% of pixels differ from the model" % (k, 100 * frac))
        assert frac <= 0.018, (k, frac)


def test_bit_reproducible():
    frames, flows = interval_512(n=2, seed=11)
    f = frames[1]
    args = (gpu(f["oa"]), gpu(f["ob"]), gpu(f["d1"]), gpu(f["d2"]), 0.5,
            gpu((np.arange(512 * 512).reshape(512, 512) % 3 == 0).astype(np.uint8)), gpu(flows[0]))
    a_img, a_mask = B.blend_frame(*args)
    b_img, b_mask = B.blend_frame(*args)
    assert torch.equal(a_img, b_img) and torch.equal(a_mask, b_mask)


def test_unsupported_sides_and_short_workspace_refused_before_launch():
    lib = _lib.load()
    s = 16
    img = torch.full((s, s, 3), 7, dtype=torch.uint8, device=DEV)
    d = torch.zeros((s, s), dtype=torch.float32, device=DEV)
    out = torch.full((s, s, 3), 77, dtype=torch.uint8, device=DEV)
    mask = torch.full((s, s), 77, dtype=torch.uint8, device=DEV)
    ws = torch.empty(B.workspace_bytes(s, s), dtype=torch.uint8, device=DEV)
    gw = (_lib._c.c_float * 3)(2.5, 0.5, 0.5)

    def call(w, h, nbytes):
        return lib.fresco_blend_frame(img.data_ptr(), img.data_ptr(), d.data_ptr(), d.data_ptr(), w, h, 0.5, None, None,
                                      B.GRADIENT, gw, mask.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)

    for w, h in ((1, s), (s, 1), (4097, 2), (2, 4097), (0, 0)):
        assert call(w, h, ws.numel()) == -2, (w, h)
    assert call(s, s, ws.numel() - 1) == -3
    assert lib.fresco_poisson_fusion(img.data_ptr(), img.data_ptr(), img.data_ptr(), mask.data_ptr(), 1, s, gw,
                                     out.data_ptr(), None, ws.data_ptr(), ws.numel(), None) == -2
    assert lib.fresco_histogram_blend(img.data_ptr(), img.data_ptr(), img.data_ptr(), s, s, 0.5, 0.5, out.data_ptr(),
                                      None, ws.data_ptr(), 10, None) == -3
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((mask == 77).all())  # nothing ran
    with pytest.raises(_lib.FrescoHipError):
        B.blend_frame(img[:1], img[:1], d[:1], d[:1], 0.5)
    assert call(s, s, ws.numel()) == 0  # the same buffers are fine at a supported size


# ---------------------------------------------------------------------------------------------------------------------
# patch_video_blend on stand-ins for cv2, VideoSequence, load_error and flow_calc
# ---------------------------------------------------------------------------------------------------------------------
class FakeCv2:
    """imread / imwrite of BGR uint8 arrays as .npy files next to the path"""

    @staticmethod
    def imwrite(path, img):
        np.save(path + ".npy", np.asarray(img))
        return True

    @staticmethod
    def imread(path):
        return np.load(path + ".npy")


class FakeSequence:
    """the parts of blender/video_sequence.py's VideoSequence that process_seq uses, output_format '%04d.jpg'"""

    def __init__(self, root, key_ind):
        self.root, self.key_ind = str(root), key_ind
        for d in ("video", "keys", "out_0", "out_1", "tmp", "blend"):
            os.makedirs(os.path.join(self.root, d), exist_ok=True)

    def p(self, d, i, ext="jpg"):
        return os.path.join(self.root, d, "%04d.%s" % (i, ext))

    def get_sequence_beg_id(self, i):
        return self.key_ind[i]

    def interval(self, i):
        return self.key_ind[i + 1] - self.key_ind[i]

    def get_key_img(self, i):
        return self.p("keys", self.key_ind[i])

    def get_input_sequence(self, i, is_forward=True):
        b, e = self.key_ind[i], self.key_ind[i + 1]
        return [self.p("video", j) for j in (range(b, e) if is_forward else range(e, b, -1))]

    def get_output_sequence(self, i, is_forward=True):
        b, e = self.key_ind[i], self.key_ind[i + 1]
        if is_forward:
            return [self.p("out_%d" % i, j) for j in range(b, e)]
        return [self.p("out_%d" % (i + 1), j) for j in range(e, b, -1)]

    def get_flow_sequence(self, i, is_forward=True):
        b, e = self.key_ind[i], self.key_ind[i + 1]
        return [os.path.join(self.root, "tmp", "flow_f_%04d.npy" % j) for j in range(b, e - 1)]

    def get_blending_img(self, i):
        return self.p("blend", i)


def fake_load_error(bin_path, img_shape):
    """video_blend.load_error: int64 pixel count, then fp32 errors"""
    data = open(bin_path, "rb").read()
    assert struct.unpack("q", data[:8])[0] == img_shape[0] * img_shape[1]
    return np.frombuffer(data[8:], np.float32).reshape(img_shape[0], img_shape[1]).copy()


def test_patched_process_seq_end_to_end(tmp_path, capsys):
    h, w, beg, end = 40, 48, 0, 6
    seq = FakeSequence(tmp_path, [beg, end])
    cv2 = FakeCv2()
    key = G.image(500, h, w)
    cv2.imwrite(seq.get_key_img(0), key)
    fwd, bwd = {}, {}
    for j in range(beg, end + 1):
        cv2.imwrite(seq.p("video", j), G.image(600 + j, h, w))
    for k, path in enumerate(seq.get_output_sequence(0)):
        fwd[beg + k] = (G.image(700 + k, h, w), G.error_map(800 + k, h, w))
        cv2.imwrite(path, fwd[beg + k][0])
        write_error_bin(path.replace("jpg", "bin"), fwd[beg + k][1])
    for k, path in enumerate(seq.get_output_sequence(0, False)):
        j = end - k
        bwd[j] = (G.image(900 + k, h, w), G.error_map(1000 + k, h, w))
        cv2.imwrite(path, bwd[j][0])
        write_error_bin(path.replace("jpg", "bin"), bwd[j][1])
    flows = {}
    for j, path in enumerate(seq.get_flow_sequence(0)):
        flows[j] = G.flow_field(1100 + j, h, w)
        np.save(path, flows[j])
    flow_calc = types.SimpleNamespace(get_flow=lambda i1, i2, path: torch.from_numpy(np.load(path)))
    vb = types.SimpleNamespace(cv2=cv2, load_error=fake_load_error, flow_calc=flow_calc, process_seq=None)
    B.patch_video_blend(vb)
    vb.process_seq(seq, 0, True, True)
    assert "others:" in capsys.readouterr().out

    n = end - beg - 1
    ids = range(beg + 1, end)
    oas = [fwd[j][0] for j in ids]
    obs = [bwd[j][0] for j in ids]
    d1s = [fwd[j][1] for j in ids]
    d2s = [bwd[end - 1 - k][1] for k in range(n)]  # the kept quirk: frame beg+1+k gets the map of frame end-1-k
    ref = M.blend_interval(oas, obs, d1s, d2s, [flows[k] for k in range(1, n)])
    natural = M.blend_interval(oas, obs, d1s, [bwd[j][1] for j in ids], [flows[k] for k in range(1, n)])
    assert any(not np.array_equal(a["mask"], b["mask"]) for a, b in zip(ref, natural))  # the pairing is visible
    assert np.array_equal(cv2.imread(seq.get_blending_img(beg)), key)
    for k, j in enumerate(ids):
        got = cv2.imread(seq.get_blending_img(j))
        frac = lab_neighbour_ok(got, ref[k]["poisson_lab"])
        assert frac <= 0.018, (j, frac)
