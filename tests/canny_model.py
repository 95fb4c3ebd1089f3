"""A numpy restatement of the rules fresco_amd's Canny kernels reproduce: OpenCV's generic
Canny(src, low, high, apertureSize=3, L2gradient=False) on an 8-bit 3-channel image -- all integer, so every comparison
against it is for equality -- plus the inputs the tests share and the named rule variants that show those inputs can tell
the rules apart.  Agreement of this restatement with a real OpenCV is checked only where cv2 can be imported
(tests/test_canny_cpu.py).

union_hysteresis() is rule 5 once more, by the two union passes csrc/canny.hip makes (inside 32 x 32 tiles, then from
the tiles' border pixels), with named defects that each drop one link or one group of border pixels: they show which
class maps can tell a kernel with that defect from a right one."""
import math

import numpy as np

# (name, what it changes): classify(img, low, high, variant=name) applies exactly one of them
VARIANTS = (
    ("last_channel_on_ties", "the last channel of the largest magnitude wins, not the first"),
    ("replicated_magnitude_border", "the magnitude outside the image is the border's, not 0"),
    ("flipped_diagonal_sign", "the diagonal neighbours are taken on the other diagonal"),
    ("hv_second_strict", "m > instead of m >= on the second horizontal / vertical neighbour"),
    ("hv_first_nonstrict", "m >= instead of m > on the first horizontal / vertical neighbour"),
    ("diag_second_nonstrict", "m >= instead of m > on the second diagonal neighbour"),
    ("low_nonstrict", "m >= low instead of m > low"),
    ("high_nonstrict", "m >= high instead of m > high"),
)
VARIANT_NAMES = tuple(v[0] for v in VARIANTS)


def thresholds(low, high):
    """rule 1: floors, swapped when low > high"""
    low, high = int(math.floor(low)), int(math.floor(high))
    return (high, low) if low > high else (low, high)


def sobel(img):
    """rule 2: (H, W, 3) uint8 -> dx, dy (H, W, 3) int32; 3 x 3, BORDER_REPLICATE"""
    H, W = img.shape[:2]
    p = np.pad(img.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    s = lambda r, c: p[r:r + H, c:c + W]  # noqa: E731
    dx = (s(0, 2) + 2 * s(1, 2) + s(2, 2)) - (s(0, 0) + 2 * s(1, 0) + s(2, 0))
    dy = (s(2, 0) + 2 * s(2, 1) + s(2, 2)) - (s(0, 0) + 2 * s(0, 1) + s(0, 2))
    return dx, dy


def classify(img, low, high, variant=None):
    """rules 1-4: (H, W, 3) uint8 -> the class map (H, W) uint8: 0, 1 (weak), 2 (strong)"""
    assert variant is None or variant in VARIANT_NAMES, variant
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, (img.dtype, img.shape)
    low, high = thresholds(low, high)
    H, W = img.shape[:2]
    dx3, dy3 = sobel(img)
    mag3 = np.abs(dx3) + np.abs(dy3)
    if variant == "last_channel_on_ties":
        ch = 2 - np.argmax(mag3[:, :, ::-1], axis=2)
    else:
        ch = np.argmax(mag3, axis=2)  # the first of the largest
    pick = lambda a: np.take_along_axis(a, ch[:, :, None], axis=2)[:, :, 0]  # noqa: E731
    dx, dy, m = pick(dx3), pick(dy3), pick(mag3)
    M = np.pad(m, 1, mode="edge" if variant == "replicated_magnitude_border" else "constant")
    nb = lambda dr, dc: M[1 + dr:1 + dr + H, 1 + dc:1 + dc + W]  # noqa: E731
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    first = (lambda a, b: a >= b) if variant == "hv_first_nonstrict" else (lambda a, b: a > b)
    second = (lambda a, b: a > b) if variant == "hv_second_strict" else (lambda a, b: a >= b)
    dsecond = (lambda a, b: a >= b) if variant == "diag_second_nonstrict" else (lambda a, b: a > b)
    horiz = first(m, nb(0, -1)) & second(m, nb(0, 1))
    vert = first(m, nb(-1, 0)) & second(m, nb(1, 0))
    neg = (dx ^ dy) < 0  # s = -1
    if variant == "flipped_diagonal_sign":
        neg = ~neg
    # s = 1: (r - 1, c - 1) and (r + 1, c + 1); s = -1: (r - 1, c + 1) and (r + 1, c - 1)
    diag = np.where(neg, (m > nb(-1, 1)) & dsecond(m, nb(1, -1)), (m > nb(-1, -1)) & dsecond(m, nb(1, 1)))
    keep = np.where(y < t22, horiz, np.where(y > t67, vert, diag))
    keep &= (m >= low) if variant == "low_nonstrict" else (m > low)
    strong = (m >= high) if variant == "high_nonstrict" else (m > high)
    return np.where(keep, np.where(strong, 2, 1), 0).astype(np.uint8)


def hysteresis(cls):
    """rule 5: class map (H, W) or (n, H, W) -> uint8 0 / 255: the class 1 / 2 pixels of every 8-connected component of
    class 1 / 2 pixels that holds a class 2 pixel; a byte >= 3 counts as 0; frames are independent"""
    cls = np.asarray(cls)
    if cls.ndim == 3:
        return np.stack([hysteresis(c) for c in cls])
    H, W = cls.shape
    c = np.where(cls <= 2, cls, 0)
    cand = np.zeros((H + 2, W + 2), bool)
    cand[1:-1, 1:-1] = c > 0
    out = np.zeros((H + 2, W + 2), bool)
    stack = [(int(r) + 1, int(q) + 1) for r, q in zip(*np.nonzero(c == 2))]
    for r, q in stack:
        out[r, q] = True
    while stack:
        r, q = stack.pop()
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if cand[r + dr, q + dc] and not out[r + dr, q + dc]:
                    out[r + dr, q + dc] = True
                    stack.append((r + dr, q + dc))
    return out[1:-1, 1:-1].astype(np.uint8) * 255


def canny(img, low, high):
    return hysteresis(classify(img, low, high))


def canny_batch(frames, low, high):
    return np.stack([canny(f, low, high) for f in frames])


def classify_batch(frames, low, high):
    return np.stack([classify(f, low, high) for f in frames])


# ---- rule 5 as the kernels compute it
TILE = 32  # CANNY_T of csrc/canny.hip

# (name, what it leaves out): union_hysteresis(cls, variant=name) applies exactly one of them
UNION_DEFECTS = (
    ("tile_drop_w", "tile pass: no link to W"),
    ("tile_drop_nw", "tile pass: no link to NW"),
    ("tile_drop_n", "tile pass: no link to N (and, as in the kernel, nothing else where N is set)"),
    ("tile_drop_ne", "tile pass: no link to NE"),
    ("tile_ne_skipped_when_nw", "tile pass: NE only where NW is not set"),
    ("border_drop_w", "border pass: no link to W"),
    ("border_drop_nw", "border pass: no link to NW"),
    ("border_drop_n", "border pass: no link to N"),
    ("border_drop_ne", "border pass: no link to NE"),
    ("border_drop_first_row", "border pass: a tile's first row left out"),
    ("border_drop_first_column", "border pass: a tile's first column (below its first row) left out"),
    ("border_drop_last_column", "border pass: a tile's last column (below its first row) left out"),
    ("border_ne_not_across_corner", "border pass: a tile's top-right pixel does not link into the tile diagonally above"),
    ("border_nw_not_across_corner", "border pass: a tile's top-left pixel does not link into the tile diagonally above"),
)
UNION_DEFECT_NAMES = tuple(v[0] for v in UNION_DEFECTS)


def union_hysteresis(cls, variant=None):
    """rule 5 by the link rules of canny_tile_union_kernel and canny_border_union_kernel, in a plain union-find over the set
    pixels: inside a tile a pixel joins N alone where N is set, else NE, and NW or else W; then the pixels of every tile's first
    row, first column and last column join their four backward neighbours in the frame, across tiles.  The lower index is the
    root, frames stay apart (a frame's first row has nothing above it).  Equal to hysteresis() with no variant."""
    assert variant is None or variant in UNION_DEFECT_NAMES, variant
    cls = np.asarray(cls)
    if cls.ndim == 2:
        return union_hysteresis(cls[None], variant)[0]
    n, H, W = cls.shape
    T, HW = TILE, H * W
    flat = np.where(cls <= 2, cls, 0).reshape(-1)
    parent = {int(p): int(p) for p in np.flatnonzero(flat)}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def union(a, b):
        a, b = find(a), find(b)
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b

    where = []
    for p in parent:
        gy, gx = divmod(p % HW, W)
        where.append((p, gy, gx, gy % T, gx % T))
    for p, gy, gx, ly, lx in where:  # the tile pass
        q = p - W
        if ly > 0 and q in parent:
            if variant != "tile_drop_n":
                union(p, q)
            continue
        ne = ly > 0 and lx + 1 < T and gx + 1 < W and q + 1 in parent
        nw = ly > 0 and lx > 0 and q - 1 in parent
        if ne and variant != "tile_drop_ne" and not (nw and variant == "tile_ne_skipped_when_nw"):
            union(p, q + 1)
        if nw:
            if variant != "tile_drop_nw":
                union(p, q - 1)
        elif lx > 0 and p - 1 in parent and variant != "tile_drop_w":
            union(p, p - 1)
    for p, gy, gx, ly, lx in where:  # the border pass
        if ly == 0:
            if variant == "border_drop_first_row":
                continue
        elif lx == 0:
            if variant == "border_drop_first_column":
                continue
        elif lx == T - 1:
            if variant == "border_drop_last_column":
                continue
        else:
            continue
        if gx > 0 and p - 1 in parent and variant != "border_drop_w":
            union(p, p - 1)
        if gy > 0:
            q = p - W
            if (gx > 0 and q - 1 in parent and variant != "border_drop_nw"
                    and not (ly == 0 and lx == 0 and variant == "border_nw_not_across_corner")):
                union(p, q - 1)
            if q in parent and variant != "border_drop_n":
                union(p, q)
            if (gx + 1 < W and q + 1 in parent and variant != "border_drop_ne"
                    and not (ly == 0 and lx == T - 1 and variant == "border_ne_not_across_corner")):
                union(p, q + 1)
    lit = {find(int(p)) for p in np.flatnonzero(flat == 2)}
    out = np.zeros(n * HW, np.uint8)
    keep = [p for p in parent if find(p) in lit]
    out[keep] = 255
    return out.reshape(n, H, W)


# ---- inputs
def _box3(a, axis):
    p = np.pad(a, [(1, 1) if k == axis else (0, 0) for k in range(a.ndim)], mode="edge")
    sl = lambda o: tuple(slice(o, o + a.shape[k]) if k == axis else slice(None) for k in range(a.ndim))  # noqa: E731
    return (p[sl(0)] + p[sl(1)] + p[sl(2)]) / 3.0


def natural(n, H, W, std=10.0, seed=0):
    """(n, H, W, 3) uint8: per-channel N(0, 1) noise under three passes of a width-3 box filter per axis, scaled to standard
    deviation `std` around 128 and rounded.  At std 10 and thresholds 50 / 100 (std 20: 100 / 200) its gradients sit around
    the thresholds: weak and strong pixels, kept and dropped components, ties between channels (uniform noise is useless
    for that: every survivor is strong)."""
    out = []
    for i in range(n):
        f = np.random.RandomState(1000 * seed + i).standard_normal((H, W, 3))
        for _ in range(3):
            f = _box3(_box3(f, 0), 1)
        f = f / f.std() * std + 128.0
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return np.stack(out)


# (n, H, W, seed) of the natural batches; seeds for which every frame, at both settings below, holds the properties
# tests/test_canny_cpu.py asserts (every rule variant visible, weak pixels both kept and dropped)
NATURAL_CASES = ((1, 37, 53, 7), (3, 70, 75, 1), (2, 96, 160, 1), (1, 130, 67, 1))
# (standard deviation of the field, low, high)
NATURAL_SETTINGS = ((10.0, 50, 100), (20.0, 100, 200))


def natural_case(case, std):
    n, H, W, seed = case
    return natural(n, H, W, std, seed)


def case_id(case):
    return "%dx%dx%d" % tuple(case[:3])


def step_columns(H=6, W=8, at=4, value=100):
    img = np.zeros((H, W, 3), np.uint8)
    img[:, at:] = value
    return img


def step_rows(H=6, W=8, at=3, value=100):
    img = np.zeros((H, W, 3), np.uint8)
    img[at:] = value
    return img


def seed_last(c):
    """the map with its last set pixel in raster order made the strong one: in a one-component map the pixel farthest,
    along the labels, from the component's lowest index, which is where a union-find's root ends up"""
    c = np.array(c)
    p = np.flatnonzero(c)
    assert p.size
    c.reshape(-1)[p[-1]] = 2
    return c


def serpentine(H=70, W=75, seed=True):
    """even rows weak, joined alternately at the right and the left end; one strong pixel at (0, 0), or with
    seed="last" at the path's last pixel in raster order, or none"""
    c = np.zeros((H, W), np.uint8)
    c[0::2] = 1
    for k, r in enumerate(range(1, H, 2)):
        c[r, W - 1 if k % 2 == 0 else 0] = 1
    if seed == "last":
        return seed_last(c)
    if seed:
        c[0, 0] = 2
    return c


def line(H, W, vertical=False, seed="last"):
    """a weak line along the middle row (column) of the map, strong at its first pixel, its last one or nowhere"""
    c = np.zeros((H, W), np.uint8)
    if vertical:
        c[:, W // 2] = 1
    else:
        c[H // 2] = 1
    if seed == "last":
        return seed_last(c)
    if seed:
        c.reshape(-1)[np.flatnonzero(c)[0]] = 2
    return c


def spiral(H=70, W=75, seed="last"):
    """a one-pixel path from (0, 0) clockwise inwards, one empty pixel between its turns; strong at its inner end
    ("last"), at (0, 0) ("first") or nowhere"""
    c = np.zeros((H, W), np.uint8)
    inside = lambda r, q: 0 <= r < H and 0 <= q < W  # noqa: E731
    r, q, dr, dq = 0, 0, 0, 1
    c[0, 0] = 1
    while True:
        for _ in range(2):
            nr, nq, ar, aq = r + dr, q + dq, r + 2 * dr, q + 2 * dq
            if inside(nr, nq) and not c[nr, nq] and not (inside(ar, aq) and c[ar, aq]):
                break
            dr, dq = dq, -dr
        else:
            break
        r, q = nr, nq
        c[r, q] = 1
    if seed == "last":
        c[r, q] = 2
    elif seed:
        c[0, 0] = 2
    return c


def staircase(H=70, W=75):
    """a one-pixel diagonal across the map from a strong (0, 0): connected through corners only"""
    c = np.zeros((H, W), np.uint8)
    k = np.arange(min(H, W))
    c[k, k] = 1
    c[0, 0] = 2
    return c


def anti_staircase(H=70, W=75):
    """a one-pixel anti-diagonal from a strong (0, W - 1) down and to the left: every step is a NE link"""
    c = np.zeros((H, W), np.uint8)
    k = np.arange(min(H, W))
    c[k, W - 1 - k] = 1
    c[0, W - 1] = 2
    return c


def checkerboard(H=70, W=75):
    r, q = np.mgrid[:H, :W]
    c = ((r + q) % 2 == 0).astype(np.uint8)
    c[0, 0] = 2
    return c


def two_blobs(H=40, W=75):
    """two weak blobs one empty column apart (column 36), the left one seeded"""
    c = np.zeros((H, W), np.uint8)
    c[5:35, 3:36] = 1
    c[5:35, 37:70] = 1
    c[20, 10] = 2
    return c


def random_classes(n=2, H=130, W=150, p_weak=0.45, p_strong=0.002, seed=3):
    u = np.random.RandomState(seed).random_sample((n, H, W))
    return np.where(u < p_strong, 2, np.where(u < p_strong + p_weak, 1, 0)).astype(np.uint8)


def corner_patterns(size=34, seam=TILE):
    """(11 264, size, size): every 3 x 3 pattern over {0, 1} with each one of its set pixels as the strong one, and with
    none (2 816 maps), each alone in a frame, across the corner where four tiles meet, at each of the four ways the two seams
    cut it (one row or two above the seam x one column or two left of it)"""
    small = []
    for bits in range(512):
        pat = np.array([(bits >> k) & 1 for k in range(9)], np.uint8)
        small.append(pat)
        for k in np.flatnonzero(pat):
            seeded = pat.copy()
            seeded[k] = 2
            small.append(seeded)
    small = np.stack(small).reshape(-1, 3, 3)
    out = np.zeros((4, len(small), size, size), np.uint8)
    for k, (r0, c0) in enumerate((r0, c0) for r0 in (seam - 2, seam - 1) for c0 in (seam - 2, seam - 1)):
        out[k, :, r0:r0 + 3, c0:c0 + 3] = small
    return out.reshape(-1, size, size)


def all_3x3_class_maps():
    """(19 683, 3, 3): every map over {0, 1, 2}; entry k holds the base-3 digits of k, the lowest at (0, 0)"""
    k = np.arange(3 ** 9)
    return np.stack([(k // 3 ** d) % 3 for d in range(9)], axis=1).reshape(-1, 3, 3).astype(np.uint8)


def blocky(n, H, W, block=3, seed=0):
    """(n, H, W, 3) uint8: block x block squares, 0 or 255 per channel: the largest gradients an 8-bit image has"""
    by, bx = -(-H // block), -(-W // block)
    b = np.random.RandomState(seed).randint(0, 2, (n, by, bx, 3)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.repeat(np.repeat(b, block, axis=1), block, axis=2)[:, :H, :W])


def uniform(n, H, W, seed=0):
    """(n, H, W, 3) uint8 uniform noise (test_uniform_noise_would_not_do's recipe): useless around 50 / 100, but gradients
    up to +-885, and at 500 / 900 weak and strong pixels and every rule variant"""
    return np.random.RandomState(seed).randint(0, 256, (n, H, W, 3)).astype(np.uint8)


def step(H, W, direction, at, value=255):
    """a step to `value` at row / column `at`: "right" and "left" give dx = +-4 value with dy = 0, "down" and "up" dy"""
    img = np.zeros((H, W, 3), np.uint8)
    if direction == "right":
        img[:, at:] = value
    elif direction == "left":
        img[:, :at] = value
    elif direction == "down":
        img[at:] = value
    else:
        assert direction == "up", direction
        img[:at] = value
    return img


def gradients(img):
    """(dx, dy) of the channel rule 3 picks, (H, W) int32 each"""
    dx3, dy3 = sobel(np.asarray(img))
    ch = np.argmax(np.abs(dx3) + np.abs(dy3), axis=2)[:, :, None]
    return np.take_along_axis(dx3, ch, axis=2)[:, :, 0], np.take_along_axis(dy3, ch, axis=2)[:, :, 0]


def nms_branch(dx, dy):
    """which comparison rule 4 makes: 0 horizontal, 1 vertical, 2 diagonal"""
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    t22 = x * 13573
    return np.where(y < t22, 0, np.where(y > t22 + (x << 16), 1, 2))


def weak_fate(img, low, high):
    """(fraction of all pixels that are weak and end kept, weak and end dropped)"""
    c = classify(img, low, high)
    e = hysteresis(c)
    return float(((c == 1) & (e == 255)).mean()), float(((c == 1) & (e == 0)).mean())
