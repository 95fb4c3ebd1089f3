"""Generate tests/golden/oracle_vs_reference_golden.npz: what the UNMODIFIED reference returns on the seeded random inputs
of tests/test_oracle_vs_reference.py (random flows, occlusions, features, several sizes).

Run in the build container only:  python tests/golden/make_oracle_vs_reference_golden.py
The inputs are not stored: the test rebuilds them from the seeds with `video` and `processor_inputs` below (torch's CPU
generator); `inputs/*` holds a float64 fingerprint of them, so that a changed random stream fails loudly there.

The flow_warp, warp_tensor, processor and optimize_feature outputs are stored on a grid of step q, an integer per element
(see `quantize`): the test loads them with `load`, which also returns q / 2 per array, and bounds |oracle - stored| by its
tolerance MINUS q / 2 -- so |oracle - reference| < tolerance holds as before.  q leaves room for the oracle's own distance
to the reference, which depends on the CPU's vector width: 0.8 x the tolerance for warp_tensor and the processor (at most
0.04 of it used), 0.1 x for flow_warp (up to 0.83 of it used by torch's scalar kernels), 5e-6 for optimize_feature (whose
bulk is bounded by a median of 1e-5).  The 0 / 1
masks are stored as uint8; everything else as the reference returned it.
"""
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FakeAttn  # noqa: E402

OUT = os.path.join(HERE, "oracle_vs_reference_golden.npz")

FLOW_WARP_CASES = [(3, 32, 1), (5, 48, 2)]                      # N, R, seed
WARP_TENSOR_FORMS = lambda R: ((6, R // 8, 2), (3, R, 1))        # C, h, chunk
MAPPING_CASES = [(3, 32, 3, 8.0), (4, 64, 4, 8.0), (4, 64, 5, 16.0)]  # N, R, seed, scale
PROCESSOR_CASES = [(2, 16, 6), (1, 40, 7), (4, 32, 8)]           # heads, C, seed
PROCESSOR_MODES = ["full", "cf_temporal", "cf", "temporal", "plain"]
OPT_CASES = [(12, 8, 9), (8, 6, 10)]                             # C, h, seed
ADAIN_SEEDS = [11, 12]
DILATE_KERNELS = (7, 13)


def video(N, R, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.tensor([2.0, -1.5]).view(1, 2, 1, 1)
    smooth = F.interpolate(torch.randn(N, 2, R // 8, R // 8, generator=g), size=(R, R), mode="bilinear", align_corners=True)
    bwd = base + 1.5 * smooth + 0.2 * torch.randn(N, 2, R, R, generator=g)
    fwd = -bwd + 0.1 * torch.randn(N, 2, R, R, generator=g)
    fo = (torch.rand(N, R, R, generator=g) < 0.15).float()
    bo = (torch.rand(N, R, R, generator=g) < 0.15).float()
    imgs = torch.rand(N, 3, R, R, generator=g) * 2 - 1
    sal = torch.rand(N, 1, R // 2, R // 2, generator=g)
    return dict(fwd=fwd, bwd=bwd, fo=fo, bo=bo, imgs=imgs, sal=sal, g=g)


def quantize(out, key, x, q):
    """stores x as k * q with integer k (|x - k q| <= q / 2): key + "#q", key + "#shape" and the four little-endian bytes of
    every int32 k as four planes, key + "#k" (uint8, (4, n)), which compress far better than interleaved bytes"""
    k = np.rint(x.double().numpy() / q)
    assert np.abs(k).max() < 2 ** 31
    out[key + "#q"], out[key + "#shape"] = np.float64(q), np.array(k.shape, dtype=np.int64)
    out[key + "#k"] = k.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4).T.copy()


def load(path=OUT):
    """-> (arrays as tensors, {key: q / 2} of the quantized ones); a quantized array comes back as float64 k * q"""
    raw = np.load(path)
    out, half = {}, {}
    for name in raw.files:
        key, _, part = name.partition("#")
        if not part:
            out[key] = torch.from_numpy(raw[name])
        elif part == "q":
            k = raw[key + "#k"].T.copy().view("<i4").reshape(tuple(raw[key + "#shape"]))
            out[key], half[key] = torch.from_numpy(k * float(raw[name])), float(raw[name]) / 2
    return out, half


def fingerprint(*tensors):
    return np.array([float(t.double().abs().sum()) for t in tensors])


def processor_inputs(heads, C, seed):
    N, R, scale = 4, 64, 8.0
    v = video(N, R, seed)
    g = v["g"]
    HW, B = (R // 8) ** 2, 2 * N
    W = [torch.randn(C, C, generator=g) / C ** 0.5 for _ in range(4)]
    hs, rf = torch.randn(B, HW, C, generator=g), torch.randn(B, HW, C, generator=g)
    o = F.interpolate(v["bo"][:-1].unsqueeze(1), scale_factor=1.0 / scale, mode="bilinear")
    cfm = torch.cat((o[0:1].reshape(1, -1) > -1, o.reshape(o.shape[0], -1) > 0.5), dim=0)
    return dict(v=v, scale=scale, W=W, attn=FakeAttn(C, heads, W), hs=hs, rf=rf, cfm=cfm)


def main():
    import _ref_harness

    torch.set_num_threads(8)
    dh, fu, geo, ut = _ref_harness.load_reference()
    out = {}
    with torch.no_grad():
        for N, R, seed in FLOW_WARP_CASES:
            key = "%d-%d-%d" % (N, R, seed)
            v = video(N, R, seed)
            x = torch.randn(N, 5, R, R, generator=v["g"])
            quantize(out, "flow_warp/" + key, geo.flow_warp(x, v["bwd"]), 0.1 * 2e-5)
            fp = [x]
            for (C, h, chunk) in WARP_TENSOR_FORMS(R):
                s = torch.randn(chunk * N, C, h, h, generator=v["g"])
                fp.append(s)
                quantize(out, "warp_tensor/%s/%d-%d-%d" % (key, C, h, chunk),
                         fu.warp_tensor(s, [v["fwd"], v["bwd"]], [v["fo"], v["bo"]], v["sal"], chunk), 0.8 * 5e-5)
            out["inputs/flow_warp/" + key] = fingerprint(v["fwd"], v["bwd"], v["sal"], *fp)
        for N, R, seed, scale in MAPPING_CASES:
            key = "%d-%d-%d-%g" % (N, R, seed, scale)
            v = video(N, R, seed)
            for j, t in enumerate(fu.get_mapping_ind(v["bwd"], v["bo"], v["imgs"], scale=scale)):
                out["mapping/%s/%d" % (key, j)] = t
            out["inputs/mapping/" + key] = fingerprint(v["bwd"], v["bo"], v["imgs"])
        for heads, C, seed in PROCESSOR_CASES:
            key = "%d-%d-%d" % (heads, C, seed)
            p = processor_inputs(heads, C, seed)
            v = p["v"]
            fm, bm, tm = fu.get_mapping_ind(v["bwd"], v["bo"], v["imgs"], scale=p["scale"])
            out["processor/%s/fwd_map" % key], out["processor/%s/tmask" % key] = fm, tm
            out["inputs/processor/" + key] = fingerprint(v["bwd"], v["bo"], v["imgs"], *p["W"], p["hs"], p["rf"])
            paras = {"fwd_mappings": [fm], "bwd_mappings": [bm], "interattn_masks": [tm]}
            for mode in PROCESSOR_MODES:
                ctl = dh.AttentionControl()
                proc = dh.FRESCOAttnProcessor2_0(2, ctl)
                if mode == "full":
                    ctl.enable_store()
                    proc(p["attn"], p["rf"])
                    ctl.disable_store()
                    ctl.enable_controller(interattn_paras=paras, attn_mask=[p["cfm"]])
                elif mode == "cf_temporal":
                    ctl.enable_interattn(paras)
                    ctl.enable_cfattn([p["cfm"]])
                elif mode == "cf":
                    ctl.enable_cfattn([p["cfm"]])
                elif mode == "temporal":
                    ctl.enable_interattn(paras)
                want = proc(p["attn"], p["hs"])
                quantize(out, "processor/%s/%s" % (key, mode), want, 0.8 * 1e-4 * max(1.0, float(want.abs().max())))
        for C, h, seed in OPT_CASES:
            key = "%d-%d-%d" % (C, h, seed)
            N, R = 4, 8 * h
            v = video(N, R, seed)
            x = torch.randn(2 * N, C, h, h, generator=v["g"])
            t = torch.randn(2 * N, C, h, h, generator=v["g"])
            vv = t.reshape(2 * N, C, h * h).transpose(1, 2)
            vv = vv / ((vv ** 2).sum(dim=2, keepdims=True) ** 0.5)
            corr = [torch.bmm(vv, vv.transpose(-1, -2)).float()]
            for iters in (1, 3):
                quantize(out, "optimize/%s/%d" % (key, iters),
                         dh.optimize_feature(x, [v["fwd"], v["bwd"]], [v["fo"], v["bo"]], corr, iters=iters), 5e-6)
            out["inputs/optimize/" + key] = fingerprint(v["fwd"], v["bwd"], v["fo"], v["bo"], x, t)
        for seed in ADAIN_SEEDS:
            v = video(4, 32, seed)
            g = v["g"]
            a, b = torch.randn(6, 7, 9, 5, generator=g), 2.0 * torch.randn(6, 7, 9, 5, generator=g) + 0.5
            out["adain/%d" % seed] = ut.adaptive_instance_normalization(a, b)
            fp = [v["fwd"], v["bwd"], a, b]
            for k in DILATE_KERNELS:
                m = (torch.rand(3, 1, 32, 32, generator=g) < 0.05).float()
                fp.append(m)
                dm = ut.Dilate(kernel_size=k, device="cpu")(m)
                assert ((dm == 0) | (dm == 1)).all()
                out["dilate/%d/%d" % (seed, k)] = dm.to(torch.uint8)
            fo, bo = geo.forward_backward_consistency_check(v["fwd"], v["bwd"])
            assert all(((t == 0) | (t == 1)).all() for t in (fo, bo))
            out["fbcheck/%d/fwd_occ" % seed], out["fbcheck/%d/bwd_occ" % seed] = fo.to(torch.uint8), bo.to(torch.uint8)
            out["inputs/adain/%d" % seed] = fingerprint(*fp)
    # an .npz that np.load reads like any other, LZMA- instead of deflate-compressed (0.7 instead of 0.8 MB)
    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in out.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, v.numpy() if torch.is_tensor(v) else np.asarray(v))
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
