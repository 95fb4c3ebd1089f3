"""CPU emulation of attn_flash_kernel's arithmetic (fp16 operands, exact fp32 products, P rounded to fp16, row sum from the
rounded P) with the softmax scale either FOLDED into the fp16 Q (one extra rounding of c*q per element) or applied EXACTLY
per score, against an fp64 softmax -- to measure what the fold costs in accuracy as a function of the kernel's own
criterion, the Cauchy-Schwarz logit bound  B = c |q| max|k|  (log2 units; the kernel folds while B <= FOLD_MAX).
Reports, per bound bucket, the worst  |O - ref| / (1e-3 + 1e-3 |ref|)  (the parity bar of tests/: must stay < 1).
    python tools/fold_margin.py
--dtype bf16: the same emulation with bf16 operands, bf16 P and m_run on the bf16 grid (the bf16 instantiations of
attn.hip), against the bf16 bar  2^-7 (rms(v) + |ref|)  of tests/test_gpu_bf16_attention.py; buckets start at bound 1, and
the test's 6 x N(0,1) key case is reported at its own shapes.  This is what attn_cfg.h's FoldCfg<bf16_t> quotes.
    python tools/fold_margin.py --dtype bf16
"""
import math
import torch

torch.manual_seed(0)
D, Lq, M = 40, 1024, 4237
LOG2E = 1.4426950408889634
DT = torch.float16   # element type of the emulated kernel (--dtype bf16: torch.bfloat16)
EDGES = [0, 8, 12, 16, 20, 24, 32, 48, 1e9]
BAR_NAME = "1e-3 bar"


def bar(ref, v):
    if DT == torch.float16:
        return 1e-3 + 1e-3 * ref.abs()
    return 2.0 ** -7 * (v.double().pow(2).mean().sqrt() + ref.abs())


def run(q, k, v, scale, fold):
    c = scale * LOG2E
    qd, kd, vd = q.double(), k.double(), v.double()
    ref = torch.softmax((qd @ kd.T) * scale, -1) @ vd
    if fold:
        qf = (q.float() * c).to(DT).double()            # the kernel: fp32 multiply, one rounding to the element type
        x = (qf @ kd.T).float()                          # MFMA: exact products, fp32 accumulation
    else:
        x = ((qd @ kd.T).float() * c)
    m = x.max(-1, keepdim=True).values.to(DT).float()    # reference point on the element type's grid
    p = torch.exp2(x - m).to(DT).double()                # P stored in the element type; the ones row sums the ROUNDED P
    o = (p @ vd) / p.sum(-1, keepdim=True)
    err = (o - ref).abs() / bar(ref, v)
    return err.max(dim=1).values                        # per query


def bound(q, k, scale):
    return scale * LOG2E * q.float().norm(dim=1) * k.float().norm(dim=1).max()


def report(name, q, k, v, scale):
    B = bound(q, k, scale)
    ef, ee = run(q, k, v, scale, True), run(q, k, v, scale, False)
    print("%s  (bound %.1f .. %.1f)" % (name, float(B.min()), float(B.max())))
    edges = EDGES
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (B > lo) & (B <= hi)
        if int(sel.sum()):
            print("   B in (%4g, %4g]: %5d queries   worst folded %.3f   worst exact %.3f   (of the %s)"
                  % (lo, hi, int(sel.sum()), float(ef[sel].max()), float(ee[sel].max()), BAR_NAME))


def sweeps():
    scale = 1 / math.sqrt(D)
    for gain in (0.5, 1.0, 1.5, 2.0, 3.0):
        q = (gain * torch.randn(Lq, D) * torch.linspace(0.5, 1.5, Lq).view(-1, 1)).to(DT)
        k, v = torch.randn(M, D).to(DT), torch.randn(M, D).to(DT)
        report("N(0,1) k, v; q gain %.1f" % gain, q, k, v, scale)
    # adversarial: every query has a few keys ALIGNED with it (logit = bound for those keys), values far apart
    for a in (1.0, 1.5, 2.0, 3.0):
        q = torch.randn(Lq, D).to(DT)
        k, v = torch.randn(M, D).to(DT), (3 * torch.randn(M, D)).to(DT)
        idx = torch.randint(0, M, (Lq, 2))
        k[idx[:, 0]] = (a * q.float()).to(DT)
        k[idx[:, 1]] = (a * q.float() * 0.98).to(DT)
        report("aligned keys x%.1f, |v| ~ 3" % a, q, k, v, scale)


def bf16_test_cases():
    """test_bf16_attention_large_logits (keys at 6 x N(0,1), (Lq, M) = (200, 333)) and the plain N(0,1) case beside it:
    worst error over 24 heads as a fraction of the bf16 bar, scale folded into a re-rounded bf16 Q vs kept exact"""
    for Dh in (40, 80):
        for kgain in (1.0, 6.0):
            sc = 1.0 / math.sqrt(Dh)
            wf = we = 0.0
            lo, hi = 1e9, 0.0
            for _ in range(24):
                q, k, v = torch.randn(200, Dh).to(DT), (kgain * torch.randn(333, Dh)).to(DT), torch.randn(333, Dh).to(DT)
                Bd = bound(q, k, sc)
                lo, hi = min(lo, float(Bd.min())), max(hi, float(Bd.max()))
                wf = max(wf, float(run(q, k, v, sc, True).max()))
                we = max(we, float(run(q, k, v, sc, False).max()))
            print("D=%d keys %g x N(0,1) (bound %.0f .. %.0f): worst folded %.2f   worst exact %.2f   (of the %s)"
                  % (Dh, kgain, lo, hi, wf, we, BAR_NAME))


def logit_range_cases():
    """the inputs of tests/test_gpu_attention.py::test_attention_logit_ranges, kernel decision rule included"""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import synth
    for Dh in (40, 80):
        for qgain in (1.0, 2.2, 6.0, 30.0):
            g = synth.gen(int(Dh * 10 + qgain))
            B_, H, Lq_, M_ = 2, 8, 256, 700
            C = H * Dh
            q = (torch.randn(B_, Lq_, C, generator=g) * qgain * torch.linspace(0.3, 1.5, Lq_).view(1, Lq_, 1)).to(DT)
            k = (torch.randn(B_, M_, C, generator=g) * torch.linspace(0.5, 1.6, M_).view(1, M_, 1)).to(DT)
            v = torch.randn(B_, M_, C, generator=g).to(DT)
            sc = 1.0 / math.sqrt(Dh)
            worst = {16.0: 0.0, 24.0: 0.0, 32.0: 0.0}
            for b in range(B_):
                for h in range(H):
                    qq, kk, vv = (t[b, :, h * Dh:(h + 1) * Dh] for t in (q, k, v))
                    Bd = bound(qq, kk, sc)
                    ef, ee = run(qq, kk, vv, sc, True), run(qq, kk, vv, sc, False)
                    for fm in worst:
                        # the kernel folds per WAVE (64 queries at D = 40): all of them must satisfy the criterion
                        rows = 64 if Dh == 40 else 32
                        ok = (Bd <= fm).view(-1, rows).all(1).repeat_interleave(rows)
                        worst[fm] = max(worst[fm], float(torch.where(ok, ef, ee).max()))
            print("logit_ranges D=%d qgain=%4.1f: worst error / bar at FOLD_MAX 16 / 24 / 32: %.3f / %.3f / %.3f"
                  % (Dh, qgain, worst[16.0], worst[24.0], worst[32.0]))


if __name__ == "__main__":
    import sys
    if "--dtype" in sys.argv and sys.argv[sys.argv.index("--dtype") + 1] == "bf16":
        DT = torch.bfloat16
        EDGES = [0, 1, 2, 4, 8, 16, 24, 32, 48, 1e9]
        BAR_NAME = "bf16 bar 2^-7 (rms v + |ref|)"
        sweeps()
        bf16_test_cases()
        sys.exit(0)
    if "ranges" not in sys.argv:
        sweeps()
    logit_range_cases()
