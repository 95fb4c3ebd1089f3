"""Sequential model of the FLATTEN correspondence path (src/flow_utils.py:56-138), written from its description, and
the input families the mapping tests share.

pair_loop   one frame pair at grid resolution (what fresco_mapping_ind takes): float32 landings rounded half to even,
            sources visited in ascending order, an incumbent replaced only by a strictly smaller float32 colour error
            ((d0^2 + d1^2) + d2^2) / 3, losers unused, unlinked targets filled with the unused sources in ascending order.
chain_loop  fwd[i+1] = map_i[fwd[i]], bwd = inverse permutation, mask rows split where a trajectory meets an unlinked target.

The keyword switches of pair_loop (rounding / replace / esum) build the deliberately wrong copies the discrimination
checks need; nothing else uses them.

Families (family(name, H, W, N, seed) -> flow (P,2,H,W) in GRID units, occ (P,H,W), frames (N,3,H,W), P = N-1): the caller
multiplies the flow by the scale it hands to the kernel (a power of two: exact both ways).
"""
import numpy as np
import torch

F32 = np.float32


def _np(t, dtype):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=dtype)


def _round(v, rounding):
    if rounding == "even":
        return np.rint(v)
    assert rounding == "away"
    return np.copysign(np.floor(np.abs(v) + F32(0.5)), v)


def pair_loop(flow, occ, frames, scale, *, rounding="even", replace="gt", esum="left"):
    """flow (2,H,W) float32, channel 0 = x, 1 = y, not yet divided by scale; occ (H,W) (> 0.5 = occluded); frames
    (2,3,H,W) or (2,3,HW): frames[0] holds the targets, frames[1] the sources.  -> (mapping (HW,) int64, unlinked (HW,) bool)"""
    flow = _np(flow, F32)
    _, H, W = flow.shape
    hw = H * W
    occ = _np(occ, F32).reshape(hw)
    fr = _np(frames, F32).reshape(2, 3, hw)
    sc = F32(scale)
    gy = np.repeat(np.arange(H, dtype=F32), W)
    gx = np.tile(np.arange(W, dtype=F32), H)
    with np.errstate(all="ignore"):
        wy = _round(gy + flow[1].reshape(hw) / sc, rounding)
        wx = _round(gx + flow[0].reshape(hw) / sc, rounding)
        valid = (wy >= 0) & (wy < H) & (wx >= 0) & (wx < W) & ~(occ > F32(0.5))
        tgt = np.where(valid, wy * F32(W) + wx, 0).astype(np.int64)
    # float32 colour error of every source against its own landing (each product and sum rounded to float32)
    d = fr[1] - fr[0][:, tgt]
    sq = d * d
    if esum == "left":
        err = ((sq[0] + sq[1]) + sq[2]) / F32(3)
    else:
        assert esum == "right"
        err = (sq[0] + (sq[1] + sq[2])) / F32(3)
    assert err.dtype == F32
    mapping = [-1] * hw
    used = valid.tolist()
    tg, er = tgt.tolist(), err.tolist()  # float32 -> Python float is exact: comparisons are unchanged
    for s in range(hw):
        if not used[s]:
            continue
        t = tg[s]
        inc = mapping[t]
        if inc == -1:
            mapping[t] = s
        elif (er[inc] > er[s]) if replace == "gt" else (er[inc] >= er[s]):
            used[inc] = False
            mapping[t] = s
        else:
            used[s] = False
    unused = [s for s in range(hw) if not used[s]]
    unlinked = [m == -1 for m in mapping]
    it = iter(unused)
    for t in range(hw):
        if unlinked[t]:
            mapping[t] = next(it)
    assert next(it, None) is None
    return torch.tensor(mapping, dtype=torch.int64), torch.tensor(unlinked, dtype=torch.bool)


def chain_loop(maps, unlinked, N, hw=None):
    """maps / unlinked: the N-1 per-pair results of pair_loop.  -> fwd (N,hw) int64, bwd (N,hw) int64, mask (hw,N,N) bool.
    hw is needed only when N = 1 (no pair to take it from)."""
    if N > 1:
        hw = len(maps[0])
    fwd = [list(range(hw))]
    bwd = [list(range(hw))]
    mask = np.ones((hw, N, N), dtype=bool)
    for i in range(N - 1):
        m, u = [int(a) for a in maps[i]], [bool(a) for a in unlinked[i]]
        prev, nxt, inv = fwd[-1], [0] * hw, [0] * hw
        for p in range(hw):
            if u[prev[p]]:  # the trajectory of aligned pixel p breaks between frames i and i + 1
                mask[p, : i + 1, i + 1:] = False
                mask[p, i + 1:, : i + 1] = False
            nxt[p] = m[prev[p]]
            inv[nxt[p]] = p
        fwd.append(nxt)
        bwd.append(inv)
    return torch.tensor(fwd, dtype=torch.int64), torch.tensor(bwd, dtype=torch.int64), torch.from_numpy(mask)


def model(flow, occ, frames, scale):
    """all pairs + the chain: flow (P,2,H,W), occ (P,H,W), frames (N,3,H,W) -> fwd, bwd, mask as chain_loop"""
    frames = _np(frames, F32)
    N, _, H, W = frames.shape
    res = [pair_loop(flow[i], occ[i], frames[i:i + 2], scale) for i in range(N - 1)]
    return chain_loop([r[0] for r in res], [r[1] for r in res], N, hw=H * W)


# ------------------------------------------------------------------------------------------------------------------
# input families
# ------------------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1), (3, 5), (31, 33), (32, 32), (25, 41), (33, 37), (32, 56), (1, 1500), (1500, 1), (45, 47)]
COLLAPSE = ["collapse_%s_%s" % (a, b) for a in ("one", "row", "few") for b in ("q3", "distinct", "near")]
FAMILIES = ["half", "border"] + COLLAPSE + ["all_occluded", "zero_flow", "occ_values", "nonfinite"]


def _grid(H, W):
    gy = np.repeat(np.arange(H, dtype=F32).reshape(H, 1), W, 1)
    gx = np.repeat(np.arange(W, dtype=F32).reshape(1, W), H, 0)
    return gy, gx


def _to_flow(ly, lx, H, W):
    """the flow (2,H,W) (x first) that lands pixel (y, x) at (ly, lx); exact while |landing|, |grid| are small"""
    gy, gx = _grid(H, W)
    return np.stack([(lx - gx).astype(F32), (ly - gy).astype(F32)], 0)


def _colours(rng, kind, N, H, W):
    if kind == "q3":  # few distinct colours: many exactly equal errors, the earliest source must win
        return (rng.randint(0, 4, size=(N, 3, H, W)) / 3.0).astype(F32)
    if kind == "distinct":
        n = N * 3 * H * W
        return ((rng.permutation(n) + 1) / F32(n)).astype(F32).reshape(N, 3, H, W)
    assert kind == "near"  # 8-bit colours from a short bright range; family() plants the near-ties below them
    return (rng.randint(120, 136, size=(N, 3, H, W)).astype(F32) / F32(255)).astype(F32)


def _mirror_triple():
    """the first 8-bit colour (a, b, c), a < b < c < 64/255, with ((a^2 + b^2) + c^2) / 3 > ((c^2 + b^2) + a^2) / 3 in float32"""
    k = np.arange(1, 64, dtype=F32) / F32(255)
    q = k * k
    for i in range(len(k)):
        for j in range(i + 1, len(k)):
            for m in range(j + 1, len(k)):
                if ((q[i] + q[j]) + q[m]) / F32(3) > ((q[m] + q[j]) + q[i]) / F32(3):
                    return k[i], k[j], k[m]
    raise AssertionError("no such colour")


def family(name, H, W, N, seed=0):
    rng = np.random.RandomState(1000 + seed)
    P = max(N - 1, 0)
    hw = H * W
    occ = np.zeros((P, H, W), F32)
    frames = rng.rand(N, 3, H, W).astype(F32)
    flow = np.zeros((P, 2, H, W), F32)
    gy, gx = _grid(H, W)
    for i in range(P):
        if name == "half":
            # landings k or k + 0.5 per pixel and axis, k from -1 (-0.5 -> -0: valid) to the far border
            # (H - 0.5 -> H or H - 1 by the parity of H), a few beyond on either side
            ly = rng.randint(-2, H + 1, size=(H, W)).astype(F32) + F32(0.5) * rng.randint(0, 2, size=(H, W)).astype(F32)
            lx = rng.randint(-2, W + 1, size=(H, W)).astype(F32) + F32(0.5) * rng.randint(0, 2, size=(H, W)).astype(F32)
            ly[0, :] = rng.choice([-0.5, 0.5, H - 0.5, H - 1.5], size=W).astype(F32)
            lx[:, 0] = rng.choice([-0.5, 0.5, W - 0.5, W - 1.5], size=H).astype(F32)
            flow[i] = _to_flow(ly, lx, H, W)
        elif name == "border":
            ly = rng.choice(np.array([-1, 0, H - 1, H], F32), size=(H, W))
            lx = rng.choice(np.array([-1, 0, W - 1, W], F32), size=(H, W))
            inner = rng.rand(H, W) < 0.5
            ly = np.where(inner, rng.randint(0, H, size=(H, W)), ly).astype(F32)
            lx = np.where(rng.rand(H, W) < 0.5, rng.randint(0, W, size=(H, W)), lx).astype(F32)
            fl = _to_flow(ly, lx, H, W)
            # -0.5 - ulp is only representable as a landing from row / column 0 (0 + flow is exact there)
            below = np.nextafter(F32(-0.5), F32(-1))
            fl[1, 0, ::2] = below
            fl[0, ::2, 0] = below
            fl[1, 0, 1::4] = F32(-0.5)
            flow[i] = fl
        elif name.startswith("collapse"):
            _, where, col = name.split("_")
            if where == "one":
                t = rng.randint(0, hw, size=(H, W))[0, 0] * np.ones((H, W), np.int64)
            elif where == "row":
                t = rng.randint(0, H) * W + rng.randint(0, W, size=(H, W))
            else:
                t = rng.choice(rng.permutation(hw)[: max(hw // 7, 1)], size=(H, W))
            flow[i] = _to_flow((t // W).astype(F32), (t % W).astype(F32), H, W)
        elif name == "all_occluded":
            occ[i] = 1
            flow[i] = _to_flow(rng.randint(0, H, size=(H, W)).astype(F32), rng.randint(0, W, size=(H, W)).astype(F32), H, W)
        elif name == "zero_flow":
            pass
        elif name == "occ_values":
            vals = np.array([0.0, 0.5, np.nextafter(F32(0.5), F32(1)), 1.0], F32)
            occ[i] = rng.choice(vals, size=(H, W))
            ly = np.clip(gy + rng.randint(-1, 2, size=(H, W)), 0, H - 1)
            lx = np.clip(gx + rng.randint(-1, 2, size=(H, W)), 0, W - 1)
            flow[i] = _to_flow(ly.astype(F32), lx.astype(F32), H, W)
        elif name == "nonfinite":
            ly = np.clip(gy + rng.randint(-1, 2, size=(H, W)), 0, H - 1)
            lx = np.clip(gx + rng.randint(-1, 2, size=(H, W)), 0, W - 1)
            fl = _to_flow(ly.astype(F32), lx.astype(F32), H, W)
            bad = [np.nan, np.inf, -np.inf]
            for j, s in enumerate(rng.choice(hw, size=min(6, hw), replace=False)):
                y, x = divmod(int(s), W)
                fl[j % 2, y, x] = bad[j % 3]
                # a bilinear resize at factor 1 multiplies the right / lower neighbour by a zero weight: the pixels to the
                # left of and above a non-finite flow are occluded, so that they are invalid with or without that product
                occ[i, max(y - 1, 0):y + 1, max(x - 1, 0):x + 1] = 1
                occ[i, y, x] = 0
            flow[i] = fl
        else:
            raise KeyError(name)
    if name.startswith("collapse"):
        col = name.split("_")[2]
        frames = _colours(rng, col, N, H, W)
        if col == "near" and P >= 1 and hw >= 3:
            # an error of exactly 0 against a denormal one, the denormal first: the later, exact source must replace it.
            # No other colour of the source frame is 0, so nothing else reaches error 0 on this target.
            fl = flow[0]
            t = int(round(float(fl[1, 0, 0]))) * W + int(round(float(fl[0, 0, 0])))  # the landing of source 0

            def plant(s, tt, colour):  # source s of pair 0 lands on target tt, which is black
                y, x = divmod(s, W)
                fl[0, y, x], fl[1, y, x] = tt % W - x, tt // W - y
                frames[1, :, y, x] = colour
                frames[0, :, tt // W, tt % W] = 0

            plant(0, t, (1e-20, 0, 0))
            plant(hw - 1, t, (0, 0, 0))
            if hw >= 7:
                # a pair one float32 step apart in one channel, the larger first
                plant(1, (t + 1) % hw, (np.nextafter(F32(2.0 ** -10), F32(1)), 0, 0))
                plant(hw - 2, (t + 1) % hw, (F32(2.0 ** -10), 0, 0))
                # a colour and its mirror image, whose errors differ by the order of the sum alone, the larger first
                a, b, c = _mirror_triple()
                plant(2, (t + 2) % hw, (a, b, c))
                plant(hw - 3, (t + 2) % hw, (c, b, a))
    return torch.from_numpy(flow), torch.from_numpy(occ), torch.from_numpy(frames)


def chain_case(H, W, seed=0, fill_in=False, N=9, at=3):
    """N frames whose pairs are bijections (mirror images: every target linked, no fill-in) except that the sources of a
    chosen set of TRAJECTORIES are occluded at pair `at`.  -> flow, occ, frames, expected mask (hw,N,N), chosen set.

    fill_in: pair 1 also loses a set of sources, so its unlinked targets are filled in and some chosen trajectories reach
    pair `at` through a fill-in source.  (A fill-in source exists only where a target is unlinked, which breaks the same
    trajectory at that pair too: those trajectories carry the pair-1 split as well as the pair-`at` one.)"""
    rng = np.random.RandomState(2000 + seed)
    hw = H * W
    gy, gx = _grid(H, W)
    frames = rng.rand(N, 3, H, W).astype(F32)
    flow = np.zeros((N - 1, 2, H, W), F32)
    occ = np.zeros((N - 1, H, W), F32)
    perm = []  # perm[i][s] = target of source s at pair i
    for i in range(N - 1):
        ly, lx = (gy, F32(W - 1) - gx) if i % 2 == 0 else (F32(H - 1) - gy, gx)
        flow[i] = _to_flow(ly, lx, H, W)
        perm.append((ly * W + lx).astype(np.int64).reshape(hw))
    expect = np.ones((hw, N, N), dtype=bool)

    def split(p, i):
        expect[p, : i + 1, i + 1:] = False
        expect[p, i + 1:, : i + 1] = False

    early = np.zeros(0, np.int64)
    if fill_in:
        lost = np.sort(rng.choice(hw, size=max(hw // 5, 1), replace=False))  # occluded sources of pair 1
        occ[1].reshape(hw)[lost] = 1
    # walk the chain: pos[p] = pixel of trajectory p in frame i
    pos = np.arange(hw)
    for i in range(N - 1):
        inv = np.empty(hw, np.int64)
        inv[perm[i]] = np.arange(hw)  # inv[t] = the source that lands on target t
        src = inv[pos]
        if fill_in and i == 1:
            hit = np.isin(src, lost)  # targets whose only source is occluded: unlinked, filled in ascending order
            early = np.nonzero(hit)[0]
            tg = np.sort(pos[hit])
            fill = dict(zip(tg.tolist(), lost.tolist()))
            for p in early:
                split(p, 1)
                src[p] = fill[int(pos[p])]
        if i == at:
            chosen = np.sort(rng.choice(hw, size=max(hw // 3, 1), replace=False))
            if fill_in:  # at least some of the trajectories that came through a fill-in source
                chosen = np.union1d(chosen, early[::2])
            occ[at].reshape(hw)[src[chosen]] = 1
            # the occluded sources fill their own (now unlinked) targets in ascending order
            tg = np.sort(pos[chosen])
            fill = dict(zip(tg.tolist(), np.sort(src[chosen]).tolist()))
            for p in chosen:
                split(p, at)
                src[p] = fill[int(pos[p])]
        pos = src
    return (torch.from_numpy(flow), torch.from_numpy(occ), torch.from_numpy(frames), torch.from_numpy(expect),
            torch.from_numpy(chosen))


def cases():
    """(family, H, W, N, scale): every grid with the half-integer family, N in {1, 2, 3, 9} each on a grid below one
    1024-thread pass, on exactly one pass and on a ragged multi-pass grid; every family on a sub-1024 and on a ragged
    multi-pass grid, N and scale (1 or 8) in rotation."""
    out = []
    sweep = {1: [(3, 5), (32, 32), (25, 41)], 2: [(1, 1), (31, 33), (32, 32), (33, 37), (1, 1500)],
             3: [(3, 5), (32, 32), (32, 56), (1500, 1)], 9: [(31, 33), (32, 32), (25, 41), (45, 47)]}
    for N, grids in sweep.items():
        for j, (H, W) in enumerate(grids):
            out.append(("half", H, W, N, (1.0, 8.0)[(j + N) % 2]))
    small, ragged, Ns = [(3, 5), (31, 33)], [(25, 41), (33, 37), (32, 56), (45, 47)], [2, 3, 9, 2, 3]
    for j, name in enumerate(FAMILIES[1:]):
        out.append((name,) + small[j % 2] + (Ns[j % 5], (1.0, 8.0)[j % 2]))
        out.append((name,) + ragged[j % 4] + (Ns[(j + 2) % 5], (8.0, 1.0)[j % 2]))
    assert {c[1:3] for c in out} == set(GRIDS)
    return out


def case_id(c):
    return "%s-%dx%d-N%d-s%d" % c


def inputs(c):
    """the tensors of one entry of cases(): flow in grid units, occ, frames"""
    return family(c[0], c[1], c[2], c[3], seed=7 * c[1] + c[2] + c[3])
