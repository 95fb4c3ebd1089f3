"""numpy restatement of Ebsynth's GPU algorithm (the reference's ebsynth_cuda.cu driver loop), vectorised over pixels.

Two schedules of the uniformity bookkeeping (Omega, the per-source-pixel patch coverage):
  omega="snapshot"  this repository's backend, bit for bit: every pass reads Omega from a pass-start snapshot plus the
                    pixel's own moves; other pixels' moves show from the next pass on; the random search runs all radii
                    in one pass.  The backend's patch error may be contracted to FMAs; with integer-valued weights
                    and patch^2 * sum_c w_c * range_c^2 < 2^24 every error and partial sum is an exact fp32 integer,
                    and the backend's NNF, E and image match this model exactly (tests/test_gpu_ebsynth.py,
                    tests/test_gpu_ebsynth_matrix.py).
  omega="live"      the reference GPU backend's ordering: Omega is updated after every candidate step and read live by
                    every pixel (all pixels advance in lockstep, one schedule the reference's concurrent atomics allow),
                    and each random-search radius is a pass of its own.
Random numbers are the backend's counter-based hash in both, so the two differ in the Omega schedule only.
"""
import numpy as np

F = np.float32
M32 = np.uint64(0xFFFFFFFF)


def hash64(seed, pixel, pss, step):
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (np.uint64(0x9E3779B97F4A7C15) * (pixel.astype(np.uint64) + np.uint64(1)))
        z = z + np.uint64(((pss << 32) | step) & ((1 << 64) - 1)) * np.uint64(0xD6E8FEB86659FD93)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def clamped(a, y, x):
    return a[np.clip(y, 0, a.shape[0] - 1), np.clip(x, 0, a.shape[1] - 1)]


def max_levels(sh, sw, th, tw, patch):
    mh, mw = min(sh, th), min(sw, tw)
    for level in range(32, -1, -1):
        f = F(2.0) ** F(-level)
        if min(int(F(mh) * f), int(F(mw) * f)) >= 2 * patch + 1:
            return level + 1
    return 0


def level_size(n, levels, level):
    return int(F(n) * F(2.0) ** F(-(levels - 1 - level)))


def resample(img, oh, ow):
    ih, iw = img.shape[:2]
    sc = F(iw) / F(ow)
    ys, xs = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    fx, fy = sc * xs.astype(F), sc * ys.astype(F)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    s, t = (fx - ix.astype(F))[..., None], (fy - iy.astype(F))[..., None]
    one = F(1.0)
    f = img.astype(F)
    v = ((one - s) * (one - t) * clamped(f, iy, ix) + s * (one - t) * clamped(f, iy, ix + 1)
         + (one - s) * t * clamped(f, iy + 1, ix) + s * t * clamped(f, iy + 1, ix + 1))
    return v.astype(np.uint8)


def random_nnf(th, tw, sh, sw, r, seed):
    h = hash64(seed, np.arange(th * tw), 0xFFFFFFFF, 0)
    x = r + (h & M32) % np.uint64(sw - 2 * r)
    y = r + (h >> np.uint64(32)) % np.uint64(sh - 2 * r)
    return np.stack([x, y], -1).astype(np.int64).reshape(th, tw, 2)


def upscale_nnf(prev, th, tw, sh, sw, patch):
    ph, pw = prev.shape[:2]
    ys, xs = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
    p = prev[np.clip(ys // 2, 0, ph - 1), np.clip(xs // 2, 0, pw - 1)]
    return np.stack([np.clip(p[..., 0] * 2 + xs % 2, patch, sw - patch - 1),
                     np.clip(p[..., 1] * 2 + ys % 2, patch, sh - patch - 1)], -1)


def vote(src_style, nnf, patch, err=None):
    th, tw = nnf.shape[:2]
    ns = src_style.shape[2]
    r = patch // 2
    ys, xs = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
    acc = np.zeros((th, tw, ns), F)
    wsum = np.zeros((th, tw), F)
    for py in range(-r, r + 1):
        for px in range(-r, r + 1):
            n = clamped(nnf, ys + py, xs + px)
            s = src_style[n[..., 1] - py, n[..., 0] - px].astype(F)
            w = np.ones((th, tw), F) if err is None else \
                F(1.0) / (F(1.0) + clamped(err, ys + py, xs + px) / F(patch * patch * ns))
            acc = acc + w[..., None] * s
            wsum = wsum + w
    return (acc / wsum[..., None]).astype(np.uint8)


def stop_mask(new, old, thr, patch):
    m = np.abs(new.astype(np.int32) - old).max(-1) >= thr
    h, w = m.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros_like(m)
    for py in range(-(patch // 2), patch // 2 + 1):
        for px in range(-(patch // 2), patch // 2 + 1):
            out |= clamped(m, ys + py, xs + px)
    return out


class Level:
    def __init__(self, ts, tg, ss, sg, mod, sw, gw, patch, lam):
        self.ts, self.tg, self.ss, self.sg, self.mod = ts, tg, ss, sg, mod
        self.sw, self.gw = np.asarray(sw, np.float64), np.asarray(gw, np.float64)
        self.patch, self.lam = patch, F(lam)
        self.th, self.tw = tg.shape[:2]
        self.sh, self.swid = ss.shape[:2]
        self.ob = (F(self.tw * self.th) / F(self.swid * self.sh)) * F(patch * patch)
        self.ys, self.xs = np.meshgrid(np.arange(self.th), np.arange(self.tw), indexing="ij")

    def error(self, c):
        """patch error of every target pixel against the source patch centred at c (th, tw, 2)"""
        r = self.patch // 2
        e = np.zeros((self.th, self.tw), np.float64)
        for py in range(-r, r + 1):
            ty = np.clip(self.ys + py, 0, self.th - 1)
            for px in range(-r, r + 1):
                tx = np.clip(self.xs + px, 0, self.tw - 1)
                sy, sx = c[..., 1] + py, c[..., 0] + px
                d = self.ts[ty, tx].astype(np.float64) - self.ss[sy, sx]
                e += (d * d * self.sw).sum(-1)
                d = self.tg[ty, tx].astype(np.float64) - self.sg[sy, sx]
                w = self.gw if self.mod is None else self.gw * (self.mod[ty, tx].astype(F) / F(255.0))
                e += (d * d * w).sum(-1)
        return e.astype(F)

    def window_sum(self, om, c):
        r = self.patch // 2
        ii = np.zeros((om.shape[0] + 1, om.shape[1] + 1), np.int64)
        ii[1:, 1:] = om.cumsum(0).cumsum(1)
        x0, y0, x1, y1 = c[..., 0] - r, c[..., 1] - r, c[..., 0] + r + 1, c[..., 1] + r + 1
        return ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]

    def overlap(self, a, b):
        p = self.patch
        return (np.maximum(0, p - np.abs(a[..., 0] - b[..., 0])) * np.maximum(0, p - np.abs(a[..., 1] - b[..., 1])))

    def occ(self, s):
        return (s.astype(F) / F(self.patch * self.patch)) / self.ob

    def omega_move(self, om, frm, to, sel):
        r = self.patch // 2
        for oy in range(-r, r + 1):
            for ox in range(-r, r + 1):
                np.add.at(om, (to[sel][:, 1] + oy, to[sel][:, 0] + ox), 1)
                np.add.at(om, (frm[sel][:, 1] + oy, frm[sel][:, 0] + ox), -1)


def omega_build(nnf, sh, sw, patch):
    om = np.zeros((sh, sw), np.int64)
    r = patch // 2
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            np.add.at(om, (nnf[..., 1].ravel() + oy, nnf[..., 0].ravel() + ox), 1)
    return om


class Pass:
    """One propagation or random-search pass over every active pixel."""

    def __init__(self, L, om, nnf, E, active, omega):
        self.L, self.om, self.live = L, om, omega == "live"
        self.snap = om.copy()
        self.n0 = nnf.copy()
        self.nbest = nnf.copy()
        self.ebest = E.copy()
        self.active = active
        self.accepts = np.zeros(active.shape, np.int64)
        self.cur_occ = self.occ_at(self.n0)

    def occ_at(self, c):
        L = self.L
        if L.lam == 0:
            return np.zeros(c.shape[:2], F)
        if self.live:
            return L.occ(L.window_sum(self.om, c))
        return L.occ(L.window_sum(self.snap, c) - L.overlap(c, self.n0) + L.overlap(c, self.nbest))

    def try_(self, c, valid):
        L = self.L
        c = np.where(valid[..., None], c, self.nbest)
        if self.live:
            self.cur_occ = self.occ_at(self.nbest)
        new_occ = self.occ_at(c)
        cur = self.ebest + L.lam * self.cur_occ
        e = L.error(c)
        acc = valid & (e + L.lam * new_occ < cur)
        if L.lam != 0:
            L.omega_move(self.om, self.nbest, c, acc)
        self.nbest = np.where(acc[..., None], c, self.nbest)
        self.ebest = np.where(acc, e, self.ebest)
        self.accepts += acc
        if not self.live:
            self.cur_occ = np.where(acc, self.occ_at(self.nbest), self.cur_occ)


def patchmatch(L, om, nnf, E, mask, iters, seed, pass_id, omega, stats):
    hp = L.patch // 2
    pix = (L.ys * L.tw + L.xs).ravel()
    for _ in range(iters):
        for jump in (4, 2, 1):
            P = Pass(L, om, nnf, E, mask, omega)
            for ox, oy in ((-jump, 0), (jump, 0), (0, -jump), (0, jump)):
                on = clamped(nnf, L.ys + oy, L.xs + ox)
                c = np.stack([on[..., 0] - ox, on[..., 1] - oy], -1)
                valid = mask & (c[..., 0] >= hp) & (c[..., 0] < L.swid - hp) & (c[..., 1] >= hp) & \
                    (c[..., 1] < L.sh - hp)
                P.try_(c, valid)
            stats["multi_accept"] += int((P.accepts >= 2).sum())
            nnf, E = P.nbest, P.ebest
        radii = []
        r = 1
        while r < max(L.swid, L.sh) // 2:
            radii.append(r)
            r *= 2
        groups = [radii] if omega == "snapshot" else [[r] for r in radii]
        for grp in groups:
            P = Pass(L, om, nnf, E, mask, omega)
            for r in grp:
                step = r.bit_length() - 1
                nb = P.nbest
                xmin, xmax = np.maximum(nb[..., 0] - r, hp), np.minimum(nb[..., 0] + r, L.swid - 1 - hp)
                ymin, ymax = np.maximum(nb[..., 1] - r, hp), np.minimum(nb[..., 1] + r, L.sh - 1 - hp)
                h = hash64(seed, pix, pass_id, step).reshape(L.th, L.tw)
                cx = xmin + ((h & M32) % (xmax - xmin + 1).astype(np.uint64)).astype(np.int64)
                cy = ymin + ((h >> np.uint64(32)) % (ymax - ymin + 1).astype(np.uint64)).astype(np.int64)
                P.try_(np.stack([cx, cy], -1), mask)
            nnf, E = P.nbest, P.ebest
        pass_id += 1
    return nnf, L.error(nnf), pass_id


def per_level(v, levels):
    if isinstance(v, (list, tuple)):
        if len(v) != levels:
            raise ValueError("%d per-level values given for %d pyramid levels" % (len(v), levels))
        return [int(x) for x in v]
    return [int(v)] * levels


def run(ss, sg, tg, mod=None, sw=None, gw=None, uniformity=3500.0, patch=5, vote_mode="plain", levels=-1,
        svi=6, pmi=4, stop=5, extra_pass_3x3=False, seed=0, omega="snapshot", stats=None):
    """The whole pyramid; returns (image, E, NNF).  The per-level arguments svi, pmi and stop take an int (every level)
    or one value per level, coarse first, like ebsynth_run."""
    sh, swd, ns = ss.shape
    th, tw, ng = tg.shape
    sw = [1.0 / ns] * ns if sw is None else sw
    gw = [1.0 / ng] * ng if gw is None else gw
    top = max_levels(sh, swd, th, tw, patch)
    levels = top if levels == -1 else min(levels, top)
    stats = {"multi_accept": 0} if stats is None else stats
    svi, pmi, stop = (per_level(v, levels) for v in (svi, pmi, stop))
    pass_id = 0
    nnf = None
    for level in range(levels):
        fine = level == levels - 1
        lsh, lsw = level_size(sh, levels, level), level_size(swd, levels, level)
        lth, ltw = level_size(th, levels, level), level_size(tw, levels, level)
        if fine:
            lss, lsg, ltg, lmod = ss, sg, tg, mod
        else:
            lss, lsg, ltg = resample(ss, lsh, lsw), resample(sg, lsh, lsw), resample(tg, lth, ltw)
            lmod = None if mod is None else resample(mod, lth, ltw)
        nnf = random_nnf(lth, ltw, lsh, lsw, patch // 2, seed) if level == 0 else \
            upscale_nnf(nnf, lth, ltw, lsh, lsw, patch)
        E = np.zeros((lth, ltw), F)
        om = omega_build(nnf, lsh, lsw, patch)
        ts = None
        for p in range(2 if (fine and extra_pass_3x3) else 1):
            pat, lam = (patch, uniformity) if p == 0 else (3, 0.0)
            ts = vote(lss, nnf, pat)
            mask = np.ones((lth, ltw), bool)
            for v in range(svi[level]):
                L = Level(ts, ltg, lss, lsg, lmod, sw, gw, pat, lam)
                if pmi[level] > 0:
                    E = L.error(nnf)
                    nnf, E, pass_id = patchmatch(L, om, nnf, E, mask, pmi[level], seed, pass_id, omega, stats)
                else:
                    E = L.error(nnf)
                new = vote(lss, nnf, pat, E if vote_mode == "weighted" else None)
                if v < svi[level] - 1:
                    mask = stop_mask(new, ts, stop[level], pat)
                ts = new
    return ts, E, nnf
