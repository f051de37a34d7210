"""numpy model of the ALGORITHM of csrc/cocoeval.hip -- not of pycocotools' (that is tests/cocoeval_np.py): toggles XORed into a
column-major bit-packed bitmap, a word-wise prefix XOR with a carry, the OR-merge with its statistics, the popcount IoU over the
shared columns and the two-pass matching loop.  Not a test module.  It exists for the teeth test of
tests/test_cocoeval_kernels_cpu.py: with variant=None it equals the restatement on every case of tests/cocoeval_cases.py, and
each variant below is a mistake a kernel could make, which some named case must tell from the restatement.

Layout: with hw = ceil(h / 32), word x * hw + yb holds rows 32 yb .. 32 yb + 31 of column x, bit r = row 32 yb + r; the bits past
row h are zero."""
import numpy as np

INT_MAX = 2 ** 31 - 1

TOGGLE_VARIANTS = {
    "first_64_vertices": "only the first 64 vertices are read (the lane loop does not stride)",
    "prev_not_recomputed": "past the first 64 edges the previous point is not recomputed: the lane's own last point, of edge "
                           "j - 64, is compared instead",
    "nan_large": "(int)NaN of a zero-length edge is a large positive value",
    "yh_dropped": "a toggle at y == h is dropped instead of moved to the top of the next column",
    "no_cancel": "equal positions do not cancel (OR instead of XOR)",
}
SCAN_VARIANTS = {
    "carry_after_tail": "the carry out of a column's last word is taken after the tail mask",
    "no_tail_mask": "the tail mask is omitted",
}
IOU_VARIANTS = {
    "union_of_shared_columns": "the union's area terms are counted over the shared columns only",
}
MATCH_VARIANTS = {
    "first_tie_wins": "the first of equal IoUs wins",
    "crowd_once": "a crowd GT is matched once only",
    "ignored_pass_not_stopped": "the ignored pass is not stopped after a regular match",
    "area_exclusive": "the bounds of an area range are exclusive",
}
VARIANTS = dict(TOGGLE_VARIANTS, **SCAN_VARIANTS, **IOU_VARIANTS, **MATCH_VARIANTS)


def _cint(a, nan_v):
    """C's (int) of a double array: truncation toward zero; NaN -> nan_v (0 on the device)"""
    a = np.asarray(a, dtype=np.float64)
    nan = np.isnan(a)
    return np.where(nan, nan_v, np.trunc(np.where(nan, 0.0, a))).astype(np.int64)


def poly_points(xy, nan_v=0):
    """the flattened (j, d, u, v) of coco_poly_toggle_kernel's edge_point over all edges j and their points d"""
    xy = np.asarray(xy, dtype=np.float64)
    k = xy.size // 2
    x, y = _cint(5.0 * xy[0:2 * k:2] + .5, 0), _cint(5.0 * xy[1:2 * k:2] + .5, 0)
    xs, xe, ys, ye = x, np.roll(x, -1), y, np.roll(y, -1)
    dx, dy = np.abs(xe - xs), np.abs(ys - ye)
    horiz = dx >= dy
    flip = (horiz & (xs > xe)) | (~horiz & (ys > ye))
    xs, xe, ys, ye = np.where(flip, xe, xs), np.where(flip, xs, xe), np.where(flip, ye, ys), np.where(flip, ys, ye)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(horiz, (ye - ys).astype(np.float64) / dx, (xe - xs).astype(np.float64) / dy)
    n = np.maximum(dx, dy) + 1
    j = np.repeat(np.arange(k), n)
    d = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    t = np.where(flip[j], np.where(horiz, dx, dy)[j] - d, d)
    with np.errstate(invalid="ignore"):
        u = np.where(horiz[j], t + xs[j], _cint(xs[j] + s[j] * t + .5, nan_v))
        v = np.where(horiz[j], _cint(ys[j] + s[j] * t + .5, nan_v), t + ys[j])
    return j, d, u, v


def poly_toggles(xy, h, w, variant=None):
    """pixel positions x * h + y toggled by one polygon, duplicates kept, in the kernel's arithmetic"""
    xy = np.asarray(xy, dtype=np.float64)
    k = xy.size // 2
    if variant == "first_64_vertices":
        k = min(k, 64)
    xy = xy[:2 * k]
    if k == 0:
        return np.zeros(0, np.int64)
    j, d, u, v = poly_points(xy, INT_MAX if variant == "nan_large" else 0)
    prev = np.arange(len(u)) - 1
    use = np.ones(len(u), bool)
    use[0] = False                                           # j == 0, d == 0: no previous point
    if variant == "prev_not_recomputed":
        last = np.flatnonzero(np.append(j[1:] != j[:-1], True))          # last point of every edge
        start = (d == 0) & (j > 0)
        stale = start & (j >= 64)
        prev[stale] = last[j[stale] - 64]
        use[start & (j < 64)] = False                        # a lane's first edge: nothing to compare with yet
    pu, pv = u[prev], v[prev]
    use &= u != pu
    xd = (np.where(u < pu, u, u - 1).astype(np.float64) + .5) / 5.0 - .5
    use &= ~((np.floor(xd) != xd) | (xd < 0) | (xd > w - 1))
    yd = (np.where(v < pv, v, pv).astype(np.float64) + .5) / 5.0 - .5
    yd = np.ceil(np.where(yd < 0, 0.0, np.where(yd > h, float(h), yd)))
    if variant == "yh_dropped":
        use &= yd != h
    return (xd[use].astype(np.int64) * h + yd[use].astype(np.int64))


def counts_toggles(counts, h, w):
    """a toggle at every prefix sum; the pixels after the last run stay 0, so the end of a last run of zeros toggles nothing"""
    out, pos = [], 0
    for j, c in enumerate(counts):
        if pos >= h * w:
            break
        pos += int(c) & 0xffffffff
        if j + 1 < len(counts) or j & 1:
            out.append(pos)
    return np.array(out, dtype=np.int64)


def string_toggles(s, h, w):
    """coco_seq_toggle_kernel's decode of a compressed string, count by count, stopping at the end of the image or the input"""
    if isinstance(s, str):
        s = s.encode("ascii")
    out, pos, p, c1, c2, m = [], 0, 0, 0, 0, 0
    while p < len(s) and pos < h * w:
        x, kk, more = 0, 0, 1
        while more and p < len(s):
            c = s[p] - 48
            x |= (c & 0x1f) << 5 * kk
            more = c & 0x20
            p += 1
            kk += 1
            if not more and (c & 0x10):
                x |= -1 << 5 * kk
        if m > 2:
            x += c2
        cnt = x & 0xffffffff
        c2, c1, m = c1, cnt, m + 1
        pos += cnt
        if p < len(s) or not m & 1:
            out.append(pos)
    return np.array(out, dtype=np.int64)


def toggle_bitmap(pos, h, w, variant=None):
    """zeroed bitmap with the positions inside the image XORed in"""
    hw = (h + 31) // 32
    bm = np.zeros(w * hw, dtype=np.uint32)
    pos = np.asarray(pos, dtype=np.int64)
    pos = pos[(pos >= 0) & (pos < h * w)]
    x, y = pos // h, pos % h
    op = np.bitwise_or if variant == "no_cancel" else np.bitwise_xor
    op.at(bm, x * hw + (y >> 5), (np.uint32(1) << (y & 31).astype(np.uint32)).astype(np.uint32))
    return bm


def scan(bm, h, w, variant=None):
    """coco_scan_kernel: prefix XOR in pixel order, word by word; the carry into a word is bit 31 of the word before it"""
    hw = (h + 31) // 32
    tail = h & 31
    tail_mask = (1 << tail) - 1 if tail else 0xffffffff
    x = bm.astype(np.uint32).copy()
    for sh in (1, 2, 4, 8, 16):
        x ^= x << np.uint32(sh)
    out = np.zeros_like(x)
    carry = 0
    for i, word in enumerate(x.tolist()):
        if carry:
            word ^= 0xffffffff
        if variant != "carry_after_tail":
            carry = word >> 31
        if i % hw == hw - 1 and variant != "no_tail_mask":
            word &= tail_mask
        if variant == "carry_after_tail":
            carry = word >> 31
        out[i] = word
    return out


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)).sum())


def merge(sources, h, w):
    """coco_merge_kernel: OR of the source bitmaps, (area, first nonempty column, last nonempty column); empty: (0, w, -1)"""
    hw = (h + 31) // 32
    m = np.zeros(w * hw, dtype=np.uint32)
    for s in sources:
        m |= s
    cols = np.flatnonzero(m.reshape(w, hw).any(axis=1))
    return m, (popcount(m), int(cols[0]) if len(cols) else w, int(cols[-1]) if len(cols) else -1)


def sources_of(segm, h, w):
    """(mask h, mask w, [('poly' | 'counts' | 'string', data)]) of a json segmentation, the box quirk unfolded"""
    if isinstance(segm, list):
        if len(segm[0]) == 4:
            out = []
            for b in segm:
                xs, ys, bw, bh = (float(v) for v in b)
                out.append(("poly", [xs, ys, xs, ys + bh, xs + bw, ys + bh, xs + bw, ys]))
            return h, w, out
        return h, w, [("poly", p) for p in segm]
    rh, rw = segm["size"]
    return rh, rw, [("counts" if isinstance(segm["counts"], list) else "string", segm["counts"])]


def build_mask(segm, h, w, variant=None):
    """words and (area, col_lo, col_hi) of one annotation's mask"""
    h, w, srcs = sources_of(segm, h, w)
    maps = []
    for kind, data in srcs:
        if kind == "poly":
            pos = poly_toggles(data, h, w, variant)
        elif kind == "counts":
            pos = counts_toggles(data, h, w)
        else:
            pos = string_toggles(data, h, w)
        maps.append(scan(toggle_bitmap(pos, h, w, variant), h, w, variant))
    return merge(maps, h, w)


def pack(mask):
    """an [h, w] 0/1 array in the bitmap layout"""
    h, w = mask.shape
    hw = (h + 31) // 32
    bits = np.zeros((w, hw * 32), dtype=np.uint64)
    bits[:, :h] = np.asarray(mask, dtype=np.uint64).T
    return (bits.reshape(w, hw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32).ravel()


def unpack(words, h, w):
    """-> ([h, w] uint8 mask, True if any padding bit is set)"""
    hw = (h + 31) // 32
    bits = ((np.asarray(words, dtype=np.uint32).reshape(w, hw)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w, hw * 32)
    return bits[:, :h].T.astype(np.uint8), bool(bits[:, h:].any())


def stats_of(mask):
    """(area, first nonempty column, last nonempty column) of an [h, w] array, as coco_merge_kernel defines them"""
    cols = np.flatnonzero(np.asarray(mask).any(axis=0))
    return int(np.count_nonzero(mask)), int(cols[0]) if len(cols) else mask.shape[1], int(cols[-1]) if len(cols) else -1


def mask_iou(a, sa, b, sb, size_a, size_b, crowd, variant=None):
    """coco_mask_iou_kernel on a det (words a, stats sa) and a gt (b, sb)"""
    if tuple(size_a) != tuple(size_b):
        return -1.0
    hw = (size_a[0] + 31) // 32
    lo, hi = max(sa[1], sb[1]), min(sa[2], sb[2])
    inter = popcount(a[lo * hw:(hi + 1) * hw] & b[lo * hw:(hi + 1) * hw]) if lo <= hi else 0
    if inter == 0:
        return 0.0
    area_a, area_b = sa[0], sb[0]
    if variant == "union_of_shared_columns":
        area_a, area_b = popcount(a[lo * hw:(hi + 1) * hw]), popcount(b[lo * hw:(hi + 1) * hw])
    u = area_a if crowd else area_a + area_b - inter
    return float(np.float64(inter) / np.float64(u))


def match(gts, dts, ious, iou_thrs, area_rng, variant=None):
    """coco_match_kernel for one group: dt_match [40, D] (the gt's id, 0: none), dt_ignore [40, D], gt_matched [40, G]; lane
    t + 10 a"""
    D, G = len(dts), len(gts)
    T, A = len(iou_thrs), len(area_rng)
    ious = np.asarray(ious, dtype=np.float64).reshape(D, G)
    dt_match = np.zeros((T * A, D), dtype=np.int64)
    dt_ignore = np.zeros((T * A, D), dtype=np.uint8)
    gt_matched = np.zeros((T * A, G), dtype=np.uint8)
    crowd = [bool(g["iscrowd"]) for g in gts]
    for a, (lo, hi) in enumerate(area_rng):
        if variant == "area_exclusive":
            out = lambda ar: ar <= lo or ar >= hi
        else:
            out = lambda ar: ar < lo or ar > hi
        ig = [1 if (crowd[g] or out(gts[g]["area"])) else 0 for g in range(G)]
        for t in range(T):
            lane = t + T * a
            gtm = gt_matched[lane]
            thr = min(float(iou_thrs[t]), 1 - 1e-10)
            for d in range(D):
                best, m, m_ig = thr, -1, 0
                for p in (0, 1):
                    if p == 1 and m > -1 and m_ig == 0 and variant != "ignored_pass_not_stopped":
                        break
                    for g in range(G):
                        if ig[g] != p:
                            continue
                        if gtm[g] and (not crowd[g] or variant == "crowd_once"):
                            continue
                        v = ious[d, g]
                        if v < best or (variant == "first_tie_wins" and m > -1 and v == best):
                            continue
                        best, m, m_ig = v, g, p
                id_, dig = 0, 0
                if m > -1:
                    dig, id_ = m_ig, gts[m]["id"]
                    gtm[m] = 1
                if id_ == 0 and out(dts[d]["area"]):
                    dig = 1
                dt_match[lane, d] = id_
                dt_ignore[lane, d] = dig
    return dt_match, dt_ignore, gt_matched
