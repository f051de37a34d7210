"""Adversarial case sets for the reference's CUDA NMS backend (eval/src/nms_kernel.cu).  CPU only, deterministic.

Every set is built in float32 numpy with devIoU's own operation order (nms_kernel.cu:13-23: corners a[0] -+ a[2] / 2,
fmaxf / fminf, areas w * h, interS / (Sa + Sb - interS), every operation rounded once), and the property that makes it
adversarial is asserted while it is built.  `cases()` returns a list of dicts:

    family  threshold | contraction | blocks | chains | degenerate | nan | ties
    name    unique within the list
    dets    [n, 5] float32 (cx, cy, w, h, score), rows shuffled so that keep order != index order
    cats    [n] int64 classes for batched_nms (seeded, 1-3 classes)
    thr     float32 IoU threshold
    keep    the keep list of `nms_exact` (score-descending visiting order; for "ties" the stable-sort order)

The fused variant: hipcc's default contraction turns devIoU into (gfx950 assembly of the reference kernel)
    Sa = fl(a2 * a3);  S = fma(b2, b3, Sa);  den = fma(-width, height, S);  IoU = fl(fl(width * height) / den)
(the corner FMAs fma(-+0.5, w, c) equal the rounded a[0] -+ a[2] / 2 exactly).  `iou_fused` emulates that in float64, where
the product of two float32 values is exact; `_fma32` checks each float64 sum was exact too.
"""
from fractions import Fraction

import numpy as np

F32 = np.float32
THRESHOLDS = (0.3, 0.45, 0.5, 0.7)
BLOCK_NS = (1, 2, 63, 64, 65, 127, 128, 129, 400, 513, 1024, 4000, 9000)
STORED_MAX_N = 4000     # tests/golden/nms_cuda_ref.npz stores dets up to this n; larger sets are rebuilt from their seed


def _corners(d):
    two = F32(2)
    return d[..., 0] - d[..., 2] / two, d[..., 1] - d[..., 3] / two, d[..., 0] + d[..., 2] / two, d[..., 1] + d[..., 3] / two


def _inter(a, b):
    al, at, ar, ab = _corners(a)
    bl, bt, br, bb = _corners(b)
    left, right = np.fmax(al, bl), np.fmin(ar, br)
    top, bottom = np.fmax(at, bt), np.fmin(ab, bb)
    return np.fmax(right - left, F32(0)), np.fmax(bottom - top, F32(0))


def iou_exact(a, b):
    """devIoU(a, b), a = the row (earlier-visited) box, every operation rounded once."""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    with np.errstate(all="ignore"):
        w, h = _inter(a, b)
        inter = w * h
        return inter / (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter)


def iou_corner_area(a, b):
    """Mutant: areas from the corners, (x2 - x1) * (y2 - y1), as nms_cpu.cpp does."""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    with np.errstate(all="ignore"):
        w, h = _inter(a, b)
        inter = w * h
        al, at, ar, ab = _corners(a)
        bl, bt, br, bb = _corners(b)
        return inter / ((ar - al) * (ab - at) + (br - bl) * (bb - bt) - inter)


def iou_fused(a, b):
    """devIoU as hipcc contracts it by default (module docstring), emulated in float64."""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    with np.errstate(all="ignore"):
        w, h = _inter(a, b)
        inter = w * h
        sa = a[..., 2] * a[..., 3]
        s = (b[..., 2].astype(np.float64) * b[..., 3].astype(np.float64) + sa.astype(np.float64)).astype(F32)
        den = (s.astype(np.float64) - w.astype(np.float64) * h.astype(np.float64)).astype(F32)
        return inter / den


def _round32(v):
    """Correctly rounded float32 of a Fraction (nearest, ties to even)."""
    c = F32(float(v))
    best = None
    for x in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        if not np.isfinite(x):
            continue
        key = (abs(Fraction(float(x)) - v), int(np.asarray(x).view(np.int32)) & 1)
        if best is None or key < best[0]:
            best = (key, x)
    return best[1]


def _fma32(x, y, z):
    return _round32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))


def iou_fused_exact(a, b):
    """Scalar iou_fused with every fma evaluated in exact rational arithmetic (no double rounding)."""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    w, h = _inter(a, b)
    sa = a[2] * a[3]
    s = _fma32(b[2], b[3], sa)
    den = _fma32(-w, h, s)
    return (w * h) / den


def visiting_order(dets):
    """torch's sort restated as a stable descending sort: ties visited in ascending index order."""
    return np.argsort(-np.asarray(dets, F32)[:, 4], kind="stable")


def nms_exact(dets, thr, iou=iou_exact, ge=False, ascending=False, order=None):
    """nms_cuda (nms_kernel.cu:72-140) without the 64-wide tiling: greedy over the visiting order (default: visiting_order;
    `order` gives another, e.g. the one torch's GPU sort returned), a later box j is suppressed by a kept box i when
    iou(i, j) > thr.  ge / iou=iou_corner_area / ascending are the mutants the GPU tests must catch."""
    d = np.asarray(dets, F32)
    n = d.shape[0]
    if n == 0:
        return np.zeros(0, np.int64)
    order = visiting_order(d) if order is None else np.asarray(order, np.int64)
    s = d[order]
    thr = F32(thr)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if i + 1 < n:
            o = iou(s[i][None, :], s[i + 1:])
            removed[i + 1:] |= (o >= thr) if ge else (o > thr)
    k = order[np.asarray(keep, np.int64)]
    return np.sort(k) if ascending else k


# --------------------------------------------------------------------------------------------------------------------
# builders
# --------------------------------------------------------------------------------------------------------------------
def _ulp_shift(x, k):
    """x moved by k float32 ulps (same sign, finite)."""
    return (np.asarray(x, F32).view(np.int32) + np.asarray(k, np.int32)).view(F32)


def _ulp_dist(x, y):
    return np.abs(np.asarray(x, F32).view(np.int32).astype(np.int64) - np.asarray(y, F32).view(np.int32).astype(np.int64))


def _nearest(t):
    def accept(a, b):
        dist = _ulp_dist(_pair_sides(a, b, t, iou_exact), F32(t))
        return dist == dist.min()
    return accept


def _search_pair(rng, t, accept, scale, cx, cy, tries=64):
    """A box A at (cx, cy) and a box B that straddles IoU ~ t, searched over ulp perturbations of B until
    accept(a, b_candidates) -> bool mask holds for one.  Returns (a, b) rows without scores."""
    for _ in range(tries):
        w, h = (rng.uniform(0.1, 0.4, 2) * scale).astype(F32)
        a = np.array([cx, cy, w, h], F32)
        # same-size B shifted along x: IoU = (w - d) / (w + d)
        d = w * (1 - t) / (1 + t)
        m = 8192
        b = np.empty((m, 4), F32)
        b[:, 0] = _ulp_shift(F32(cx + d), rng.integers(-256, 257, m))
        b[:, 1] = _ulp_shift(F32(cy), rng.integers(-64, 65, m)) if cy != 0 else F32(cy)
        b[:, 2] = _ulp_shift(w, rng.integers(-256, 257, m))
        b[:, 3] = _ulp_shift(h, rng.integers(-64, 65, m))
        ok = np.flatnonzero(accept(np.broadcast_to(a, (m, 4)), b))
        if ok.size:
            return a, b[ok[0]]
    raise AssertionError("no pair found for t=%r" % t)


def _with_scores(rows, rng, pair_major=True):
    """Append distinct scores so that within each consecutive (A, B) pair A is visited first."""
    n = len(rows)
    sc = np.sort(rng.choice(np.arange(1, 100000), n, replace=False).astype(F32) / F32(100000))[::-1]
    # pairs keep A before B; pairs themselves interleave in a random order
    if pair_major:
        pair_rank = rng.permutation(n // 2)
        scores = np.empty(n, F32)
        for p in range(n // 2):
            scores[2 * p] = sc[2 * pair_rank[p]]
            scores[2 * p + 1] = sc[2 * pair_rank[p] + 1]
    else:
        scores = rng.permutation(sc)
    return np.concatenate([np.asarray(rows, F32), scores[:, None]], 1)


def _shuffle(d, rng):
    return d[rng.permutation(d.shape[0])]


def _finish(family, name, dets, thr, rng, ncls=3):
    dets = np.ascontiguousarray(dets, F32)
    cats = rng.integers(0, ncls, dets.shape[0]).astype(np.int64)
    return dict(family=family, name=name, dets=dets, cats=cats, thr=F32(thr), keep=nms_exact(dets, thr))


def _pair_sides(a, b, t, iou):
    return iou(np.concatenate([a, np.ones((len(a), 1), F32)], 1), np.concatenate([b, np.ones((len(b), 1), F32)], 1))


def threshold_family():
    """Pairs whose float32 IoU is exactly the threshold, one ulp above it and one ulp below it, at three coordinate scales.
    Where a search candidate exists, the pair at equality is one whose corner-area IoU lies above the threshold."""
    out = []
    for ti, t in enumerate(THRESHOLDS):
        t32 = F32(t)
        for si, scale in enumerate((1.0, 37.5, 600.0)):
            rng = np.random.Generator(np.random.PCG64(1000 + 10 * ti + si))
            rows, kinds = [], []
            targets = {"eq": t32, "above": np.nextafter(t32, F32(2)), "below": np.nextafter(t32, F32(-1))}
            k = 0
            for kind, target in targets.items():
                for rep in range(4):
                    cx, cy = F32((k % 6) * scale + 0.5 * scale), F32((k // 6) * scale + 0.5 * scale)
                    if kind == "eq" and rep < 2:
                        def accept(a, b, target=target):
                            return (_pair_sides(a, b, t, iou_exact) == target) & (_pair_sides(a, b, t, iou_corner_area) > t32)
                        try:
                            a, b = _search_pair(rng, t, accept, scale, cx, cy, tries=16)
                        except AssertionError:
                            a, b = _search_pair(rng, t, lambda a, b, target=target: _pair_sides(a, b, t, iou_exact) == target,
                                                scale, cx, cy)
                    else:
                        a, b = _search_pair(rng, t, lambda a, b, target=target: _pair_sides(a, b, t, iou_exact) == target,
                                            scale, cx, cy)
                    rows += [a, b]; kinds.append(kind); k += 1
            d = _with_scores(rows, rng)
            for p, kind in enumerate(kinds):
                o = iou_exact(d[2 * p], d[2 * p + 1])
                assert o == targets[kind], (t, scale, kind, o)
            out.append(_finish("threshold", "thr%g_s%g" % (t, scale), _shuffle(d, rng), t, rng))
            assert len(out[-1]["keep"]) == 24 - 4, (t, scale)      # only the four pairs above the threshold lose B
    return out


def contraction_family():
    """Pairs that land on opposite sides of the threshold with and without devIoU's FMAs (iou_fused), checked again in exact
    rational arithmetic."""
    out = []
    for ti, t in enumerate(THRESHOLDS):
        t32 = F32(t)
        for si, scale in enumerate((1.0, 96.0)):
            rng = np.random.Generator(np.random.PCG64(2000 + 10 * ti + si))
            rows = []
            for k in range(8):
                cx, cy = F32((k % 4) * scale + 0.5 * scale), F32((k // 4) * scale + 0.5 * scale)

                def accept(a, b):
                    return (_pair_sides(a, b, t, iou_exact) > t32) != (_pair_sides(a, b, t, iou_fused) > t32)
                a, b = _search_pair(rng, t, accept, scale, cx, cy)
                rows += [a, b]
            d = _with_scores(rows, rng)
            for p in range(8):
                a, b = d[2 * p], d[2 * p + 1]
                assert (iou_exact(a, b) > t32) != (iou_fused_exact(a, b) > t32), (t, scale, p)
                assert iou_fused_exact(a, b) == iou_fused(a, b)
            out.append(_finish("contraction", "contr%g_s%g" % (t, scale), _shuffle(d, rng), t, rng))
    return out


def random_boxes(n, seed, size=(0.02, 0.3)):
    rng = np.random.Generator(np.random.PCG64(seed))
    d = np.concatenate([rng.random((n, 2)), rng.random((n, 2)) * (size[1] - size[0]) + size[0], rng.random((n, 1))], 1)
    return d.astype(F32)


def blocks_family():
    """n across the 64-box block edges of nms_kernel's grid, up to 9000 (past the fused postprocess's LDS bit-matrix and
    om_nms_ex's single-workgroup sizes: the workspace path)."""
    out = []
    for i, n in enumerate(BLOCK_NS):
        rng = np.random.Generator(np.random.PCG64(3000 + n))
        size = (0.15, 0.5) if n <= 128 else (0.01, 0.6 * (128.0 / n) ** 0.5)
        d = random_boxes(n, 3000 + n, size)
        t = THRESHOLDS[i % len(THRESHOLDS)]
        c = _finish("blocks", "n%d" % n, d, t, rng)
        c["seed"] = 3000 + n
        if n >= 64:
            assert 0 < len(c["keep"]) < n, (n, len(c["keep"]))
        out.append(c)
    return out


def _chain_case(name, n, links, rng, thr=0.5):
    """Boxes at the given visiting positions form a chain along x: consecutive links overlap above thr, links two apart below
    it.  Fillers are tiny disjoint boxes.  Greedy NMS then keeps links 0, 2, 4, ... only."""
    w = F32(0.08)
    step = F32(0.02)                        # IoU(k, k+1) = 0.06 / 0.10 = 0.6, IoU(k, k+2) = 0.04 / 0.12 = 0.33
    rows = np.zeros((n, 5), F32)
    gx = np.arange(n) % 40; gy = np.arange(n) // 40
    rows[:, 0] = F32(2.0) + gx.astype(F32) * F32(0.05)
    rows[:, 1] = F32(2.0) + gy.astype(F32) * F32(0.05)
    rows[:, 2:4] = F32(0.01)
    scores = np.sort(rng.choice(np.arange(1, 1000000), n, replace=False).astype(F32) / F32(1e6))[::-1]
    for k, pos in enumerate(links):
        rows[pos, 0] = F32(0.3) + F32(k) * step
        rows[pos, 1] = F32(0.5)
        rows[pos, 2:4] = w
    rows[:, 4] = scores                     # row index == visiting position before the shuffle
    for k in range(len(links) - 1):
        assert iou_exact(rows[links[k]], rows[links[k + 1]]) > F32(thr)
        if k + 2 < len(links):
            assert iou_exact(rows[links[k]], rows[links[k + 2]]) <= F32(thr)
    perm = rng.permutation(n)
    d = rows[perm]
    c = _finish("chains", name, d, thr, rng)
    inv = np.argsort(perm)                  # visiting position -> shuffled row
    kept = set(c["keep"].tolist())
    for k, pos in enumerate(links):
        assert (inv[pos] in kept) == (k % 2 == 0), (name, k, pos)
    return c


def chains_family():
    rng = np.random.Generator(np.random.PCG64(4000))
    return [
        _chain_case("c62_63_64", 130, [62, 63, 64], rng),
        _chain_case("c63_64_65", 130, [63, 64, 65], rng),
        _chain_case("c63_64_127_128", 200, [63, 64, 127, 128], rng),
        _chain_case("c126_127_128", 200, [126, 127, 128], rng),
        _chain_case("c127_128_129", 260, [127, 128, 129], rng),
        _chain_case("c0_63_64_127_128_191", 256, [0, 63, 64, 127, 128, 191], rng),
    ]


def degenerate_family():
    out = []
    rng = np.random.Generator(np.random.PCG64(5000))
    inf = F32(np.inf)
    # duplicates with distinct scores, one pair straddling the 63/64 edge of the visiting order
    d = random_boxes(130, 5001, (0.01, 0.02))
    d[64, :4] = d[63, :4]; d[10, :4] = d[11, :4]; d[100, :4] = d[3, :4]
    d[:, 4] = np.linspace(1.0, 0.01, 130, dtype=F32)
    c = _finish("degenerate", "duplicates", _shuffle(d, rng), 0.5, rng)
    assert len(c["keep"]) <= 127
    out.append(c)
    # zero width / zero height; two identical zero-area boxes (0 / 0 = NaN: nothing suppressed)
    rows = [[0.5, 0.5, 0.0, 0.2], [0.5, 0.5, 0.2, 0.2], [0.5, 0.5, 0.2, 0.0], [0.52, 0.5, 0.2, 0.2],
            [2.0, 2.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0], [3.0, 3.0, 0.0, 0.1], [3.0, 3.0, 0.0, 0.1],
            [4.0, 4.0, 0.1, 0.0], [4.0, 4.0, 0.1, 0.0]]
    d = _with_scores(rows, rng, pair_major=False)
    assert np.isnan(iou_exact(d[4], d[5])) and np.isnan(iou_exact(d[6], d[7])) and np.isnan(iou_exact(d[8], d[9]))
    c = _finish("degenerate", "zero_area", _shuffle(d, rng), 0.3, rng)
    out.append(c)
    # infinite widths / heights (an overflowed exp in the decode)
    rows = [[0.5, 0.5, inf, 0.2], [0.5, 0.5, 0.2, 0.2], [0.5, 0.55, inf, 0.2], [0.6, 0.5, 0.3, inf],
            [0.6, 0.5, 0.3, 0.3], [5.0, 5.0, inf, 0.0], [5.0, 5.0, 0.1, 0.1], [9.0, 9.0, inf, inf], [9.0, 9.0, 0.5, 0.5]]
    d = _with_scores(rows, rng, pair_major=False)
    c = _finish("degenerate", "infinite", _shuffle(d, rng), 0.45, rng)
    out.append(c)
    # negative coordinates and large ones (batched_nms(normalized=False) shifts classes by ~1e4-1e6)
    for name, base, scale in (("negative", -50.0, 20.0), ("large1e4", 1.0e4, 300.0), ("large1e6", 1.0e6, 2000.0)):
        n = 200
        r = np.random.Generator(np.random.PCG64(5100 + int(abs(base)) % 997))
        d = np.concatenate([base + r.random((n, 2)) * scale, (r.random((n, 2)) * 0.25 + 0.02) * scale, r.random((n, 1))], 1)
        c = _finish("degenerate", name, d.astype(F32), THRESHOLDS[len(out) % 4], rng)
        assert 0 < len(c["keep"]) < n
        out.append(c)
    # corners that round: centres near 1e4 (ulp 2^-10), each pair the nearest to the threshold of 8192 candidates
    for ti, t in enumerate(THRESHOLDS):
        r = np.random.Generator(np.random.PCG64(5200 + ti))
        rows = []
        for k in range(6):
            a, b = _search_pair(r, t, _nearest(t), 40.0,
                                F32(1.0e4 + 100.0 * k), F32(2.0e4))
            rows += [a, b]
        d = _with_scores(rows, r)
        out.append(_finish("degenerate", "large_eq%g" % t, _shuffle(d, r), t, r))
    return out


def nan_family():
    """NaN in each coordinate, in the earlier-visited and in the later-visited box.  devIoU's max / min are fmaxf / fminf,
    which return the other operand when one is NaN; a ternary `a > b ? a : b` returns b."""
    out = []
    rng = np.random.Generator(np.random.PCG64(6000))
    nan = F32(np.nan)
    for col in range(4):
        rows = []
        for k, (pos, cx) in enumerate(((0, 0.5), (1, 2.5), (0, 4.5), (1, 6.5))):
            a = np.array([cx, 0.5, 0.4, 0.4], F32)
            b = np.array([cx + 0.05, 0.52, 0.38, 0.41], F32)
            if k >= 2:                                       # an overlapping box that is NaN-free on the other coordinate
                b = np.array([cx + 0.1, 0.5, 0.4, 0.4], F32)
            (a if pos == 0 else b)[col] = nan
            rows += [a, b]
        # a NaN box in front of a block of ordinary ones, and two NaN boxes with each other
        rows += [np.array([8.5, 0.5, 0.4, 0.4], F32), np.array([8.5, 0.5, 0.4, 0.4], F32)]
        rows[-2][col] = nan; rows[-1][col] = nan
        d = _with_scores(rows, rng)
        out.append(_finish("nan", "nan_col%d" % col, _shuffle(d, rng), 0.3 + 0.1 * col, rng))
    # scattered NaNs among 200 random boxes
    d = random_boxes(200, 6100, (0.02, 0.25))
    r = np.random.Generator(np.random.PCG64(6101))
    idx = r.choice(200, 24, replace=False)
    d[idx, r.integers(0, 4, 24)] = nan
    out.append(_finish("nan", "nan_scattered", d, 0.45, r))
    return out


def ties_family():
    """Score ties: groups of equal scores among overlapping boxes, at sizes where torch's GPU sort changes algorithm."""
    out = []
    for n in (8, 64, 200, 1000, 3000):
        rng = np.random.Generator(np.random.PCG64(7000 + n))
        d = random_boxes(n, 7000 + n, (0.02, max(0.03, 0.3 * (64.0 / n) ** 0.5)))
        levels = rng.integers(0, max(2, n // 8), n)
        d[:, 4] = (levels.astype(F32) + F32(1)) / F32(n)
        c = _finish("ties", "ties_n%d" % n, d, 0.45, rng)
        assert len(np.unique(d[:, 4])) < n
        out.append(c)
    return out


FAMILIES = ("threshold", "contraction", "blocks", "chains", "degenerate", "nan", "ties")
_CACHE = {}


def cases(families=FAMILIES):
    if "all" not in _CACHE:
        built = threshold_family() + contraction_family() + blocks_family() + chains_family() + degenerate_family() + \
            nan_family() + ties_family()
        names = [c["name"] for c in built]
        assert len(set(names)) == len(names)
        _CACHE["all"] = built
    return [c for c in _CACHE["all"] if c["family"] in families]
