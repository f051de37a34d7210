"""Deterministic case tables for the kernels of csrc/cocoeval.hip, each case named for the edge it hits.  Not a test module and
no GPU: tests/test_cocoeval_kernels_cpu.py checks that every case really hits its edge and that the table catches a list of
kernel mistakes (tests/cocoeval_bitmap_np.py); tests/test_cocoeval_kernels.py runs the table through the C API.

    mask_cases()     [(name, h, w, segm)]: segm as a COCO json holds it -- a list of polygons (or of 4-number boxes), or a dict
                     with 'size' and uncompressed 'counts' or a compressed string.  Malformed counts and strings are part of
                     the table; tests/cocoeval_np.py reads them with ann_mask(..., strict=False)
    box_table()      (det boxes [D, 4], gt boxes [G, 4], gt crowd flags [G]); every det is paired with every gt
    match_groups()   [dict(name, gts, dts, ious)]: IoU matrices crafted directly as float64

Anything random comes from numpy generators seeded with SEED."""
import numpy as np

SEED = 20240611

# h covers 1, 31, 32, 33, 64, 65, 97 and w covers 1, 2, 9, 65, 129, 130, 256, 257.  In 32-row words: 32 x 256 is 256 words (one
# per scan thread), 32 x 257 is 257, 33 x 129 is 258 with two per column, 97 x 130 is 520 (three per thread), 97 x 257 is 1028.
# 97 x 257 has 24929 pixels: the only size whose counts need four characters in a compressed string.
SIZES = [(1, 9), (31, 1), (32, 256), (32, 257), (33, 129), (64, 2), (65, 65), (97, 130), (97, 257)]

STAR_VERTICES = [3, 63, 64, 65, 128, 129, 1000, 4096]        # around the 64 lanes of a wave, and the host limit
MAX_POLY_VERTICES = 4096


def star(n, h, w, inner=0.6, phase=0.1, fill=0.47):
    """n vertices alternating between an ellipse that nearly fills the image and `inner` times it, rounded to 2 decimals."""
    a = phase + 2 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, 1.0, inner)
    x = w / 2 + fill * w * r * np.cos(a)
    y = h / 2 + fill * h * r * np.sin(a)
    return np.round(np.stack([x, y], 1).ravel(), 2).tolist()


def doubled(p):
    """every vertex twice: a zero-length edge after each vertex"""
    v = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    return np.repeat(v, 2, axis=0).ravel().tolist()


def closed(p):
    """last vertex = first vertex, as many COCO json files write their polygons"""
    return list(p) + list(p[:2])


def triple_at(p, index):
    """a run of three identical vertices starting at `index`"""
    v = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([v[:index], np.repeat(v[index:index + 1], 3, axis=0), v[index + 1:]]).ravel().tolist()


def rect(x0, y0, x1, y1):
    return [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]


def _polygon_cases():
    out = []
    several = [(33, 129), (97, 130), (32, 257), (65, 65), (31, 1), (1, 9)]
    for n in STAR_VERTICES:
        if n <= 129:
            sizes = several
        elif n == 1000:
            sizes = [(33, 129), (97, 130), (32, 256)]
        else:
            sizes = [(97, 130), (33, 129), (64, 2)]          # the 4096-vertex cases are the slow ones: a handful
        for h, w in sizes:
            out.append(("star_%d_%dx%d" % (n, h, w), h, w, [star(n, h, w, inner=0.6 if n <= 129 else 0.85)]))
    for n in STAR_VERTICES[:-1]:                             # doubling 4096 vertices would pass the host limit
        for h, w in [(33, 129), (97, 130)]:
            out.append(("doubled_%d_%dx%d" % (n, h, w), h, w, [doubled(star(n, h, w, inner=0.6 if n <= 129 else 0.85))]))
    out.append(("doubled_2048_is_4096_32x257", 32, 257, [doubled(star(2048, 32, 257, inner=0.85))]))
    for n in (3, 64, 65, 129):
        for h, w in [(33, 129), (65, 65), (97, 130)]:
            out.append(("closed_%d_%dx%d" % (n, h, w), h, w, [closed(star(n, h, w))]))
    for h, w in [(33, 129), (97, 130), (32, 256)]:
        base = star(100, h, w)
        out.append(("triple_at_0_%dx%d" % (h, w), h, w, [triple_at(base, 0)]))
        out.append(("triple_at_64_%dx%d" % (h, w), h, w, [triple_at(base, 64)]))
        out.append(("triple_at_0_and_64_%dx%d" % (h, w), h, w, [triple_at(triple_at(base, 64), 0)]))
    # axis-aligned rectangles whose lower side lies on y = h or below it: the boundary points of that side have yd == h, a
    # toggle at the top of the next column -- or, in the last column, at h * w, which is no pixel
    for h, w in [(33, 129), (97, 130), (32, 257), (64, 2), (31, 1), (1, 9)]:
        xa, xb = (0, 1) if w < 4 else (w // 3, w // 3 + max(1, w // 4))
        top = h // 2
        out.append(("rect_to_h_inner_%dx%d" % (h, w), h, w, [rect(xa, top, xb, h)]))
        out.append(("rect_past_h_inner_%dx%d" % (h, w), h, w, [rect(xa, top, xb, h + 3)]))
        out.append(("rect_to_h_last_column_%dx%d" % (h, w), h, w, [rect(max(0, w - 2), top, w, h)]))
        out.append(("rect_past_h_last_column_%dx%d" % (h, w), h, w, [rect(max(0, w - 2), top, w + 2, h + 3)]))
        out.append(("rect_whole_image_and_more_%dx%d" % (h, w), h, w, [rect(-1, -1, w + 1, h + 1)]))
    # partly and wholly outside, on each side; coordinates within +-2 x the image side
    for h, w in [(33, 129), (65, 65), (97, 130)]:
        pent = np.array([[0.2, 0.1], [0.9, 0.25], [0.75, 0.9], [0.4, 0.7], [0.1, 0.8]])
        for side, (sx, sy) in (("left", (-1, 0)), ("right", (1, 0)), ("top", (0, -1)), ("bottom", (0, 1))):
            for how, shift in (("partly", 0.5), ("wholly", 1.0)):
                v = (pent + np.array([sx, sy]) * shift) * np.array([w, h])
                out.append(("outside_%s_%s_%dx%d" % (how, side, h, w), h, w, [np.round(v, 2).ravel().tolist()]))
        v = np.array([[-0.7, -0.5], [1.9, -0.2], [1.8, 1.9], [-0.4, 1.6]]) * np.array([w, h])     # around the whole image
        out.append(("outside_around_%dx%d" % (h, w), h, w, [np.round(v, 2).ravel().tolist()]))
        out.append(("negative_small_%dx%d" % (h, w), h, w, [[-0.87, -0.93, 6.3, -0.33, 7.1, 5.5, -0.17, 4.7]]))
    # coordinates on the .1 / .3 / .5 grids: these decide floor(xd) != xd
    rng = np.random.default_rng(SEED)
    for step in (0.1, 0.3, 0.5):
        for h, w in [(33, 129), (65, 65), (32, 256)]:
            n = 9
            ang = np.sort(rng.random(n) * 2 * np.pi)
            rr = 0.25 + 0.2 * rng.random(n)
            v = np.stack([w / 2 + w * rr * np.cos(ang), h / 2 + h * rr * np.sin(ang)], 1)
            v = np.round(np.round(v / step) * step, 1)
            out.append(("grid_%s_%dx%d" % (str(step).replace(".", "p"), h, w), h, w, [v.ravel().tolist()]))
    out.append(("grid_0p1_steps_33x129", 33, 129, [[10.1, 5.3, 20.3, 5.1, 20.5, 15.3, 15.1, 20.5, 10.3, 15.1]]))
    # the 4-number box quirk of frPyObjects: x, y, w, h -- one box, and two
    out.append(("box_quirk_33x129", 33, 129, [[10, 5, 20, 12]]))
    out.append(("box_quirk_fraction_65x65", 65, 65, [[3.5, 2.5, 10.2, 50.7]]))
    out.append(("box_quirk_two_97x130", 97, 130, [[5, 5, 30, 30], [20, 20, 100, 90]]))
    # an odd trailing number is ignored
    out.append(("odd_trailing_33x129", 33, 129, [star(5, 33, 129) + [77.0]]))
    out.append(("odd_trailing_97x130", 97, 130, [star(65, 97, 130) + [3.25]]))
    # 1, 2, 3 and 5 polygons in one annotation, disjoint and overlapping
    for h, w in [(33, 129), (97, 130)]:
        cell = lambda i, n, grow: rect(w * i / n - grow * w / n, h * 0.2, w * (i + 0.8) / n + grow * w / n, h * 0.9)
        for n in (1, 2, 3, 5):
            out.append(("polys_%d_disjoint_%dx%d" % (n, h, w), h, w, [cell(i, n, 0.0) for i in range(n)]))
            if n > 1:
                out.append(("polys_%d_overlapping_%dx%d" % (n, h, w), h, w, [cell(i, n, 0.4) for i in range(n)]))
        out.append(("polys_3_stars_%dx%d" % (h, w), h, w, [star(65, h, w), star(7, h, w, phase=0.7), star(129, h, w, inner=0.3)]))
    out.append(("polys_2_one_empty_33x129", 33, 129, [rect(-50, 5, -20, 20), rect(10, 5, 30, 20)]))
    out.append(("poly_empty_mask_33x129", 33, 129, [rect(-50, 5, -20, 20)]))
    return out


def counts_of(mask):
    """uncompressed RLE of an [h, w] mask: column-major runs, the first one counts zeros (and may be 0)"""
    flat = np.asarray(mask, dtype=np.uint8).T.ravel()
    edges = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    return ([0] if flat[0] else []) + [int(r) for r in runs]


def to_string(counts):
    """rleToString, written here so that the strings of this table do not come from the product"""
    out = []
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = x != -1 if ch & 0x10 else x != 0
            out.append(chr((ch | (0x20 if more else 0)) + 48))
    return "".join(out)


def base_masks(h, w):
    zero = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    first, last = zero.copy(), zero.copy()
    first[0, 0] = 1
    last[-1, -1] = 1
    straddle = zero.copy()                                   # runs that start in one column and end in the next
    straddle[h - (h + 1) // 2:, :] = 1
    straddle[:h // 3, 1:] = 1
    return [("zeros", zero), ("ones", zero + 1), ("checker", ((yy + xx) % 2).astype(np.uint8)), ("first_pixel", first),
            ("last_pixel", last), ("column_straddle", straddle)]


def _sequence_cases():
    out = []
    for h, w in SIZES:
        for name, m in base_masks(h, w):
            c = counts_of(m)
            out.append(("counts_%s_%dx%d" % (name, h, w), h, w, {"size": [h, w], "counts": c}))
            out.append(("string_%s_%dx%d" % (name, h, w), h, w, {"size": [h, w], "counts": to_string(c)}))
    for h, w in [(33, 129), (32, 256), (97, 130)]:
        n = h * w
        rle = lambda c: {"size": [h, w], "counts": c}
        tag = "_%dx%d" % (h, w)
        out += [
            ("counts_first_zero" + tag, h, w, rle([0, 5, n - 5])),
            ("counts_zero_run_cancels" + tag, h, w, rle([h - 2, 0, 4, 7, n - h - 9])),
            ("counts_two_zero_runs" + tag, h, w, rle([0, 0, 3, 0, 0, 6, n - 9])),
            ("counts_zero_run_at_column_end" + tag, h, w, rle([h, 0, h, n - 2 * h])),
            ("counts_overrun" + tag, h, w, rle([5, n])),
            ("counts_overrun_first" + tag, h, w, rle([n + 7, 3])),
            ("counts_overrun_after_ones" + tag, h, w, rle([0, n - 3, 2, 9, 4])),
            ("counts_stop_short" + tag, h, w, rle([3, 4])),
            ("counts_stop_short_in_zeros" + tag, h, w, rle([3, 4, h])),
            ("string_stop_short_in_zeros" + tag, h, w, rle(to_string([3, 4, h]))),
            ("string_first_zero" + tag, h, w, rle(to_string([0, 5, n - 5]))),
            ("string_zero_run_cancels" + tag, h, w, rle(to_string([h - 2, 0, 4, 7, n - h - 9]))),
            ("string_overrun_5_chars" + tag, h, w, rle(to_string([5, 3, 600000]))),
            ("string_negative_count_wraps" + tag, h, w, rle(to_string([4, 9, 2]) + to_string([-40]))),
        ]
    # 97 x 257: counts above 16383 take four characters, with positive and negative differences
    h, w = 97, 257
    n = h * w
    big = [1, 20000, 2, 1000, 3, n - 21006]
    out.append(("string_4_chars_negative_difference_97x257", h, w, {"size": [h, w], "counts": to_string(big)}))
    out.append(("counts_same_as_4_chars_97x257", h, w, {"size": [h, w], "counts": big}))
    # a string that ends in the middle of a count: the continuation bit of its last character is set
    s = to_string([n - 100, 100])
    out.append(("string_truncated_97x257", h, w, {"size": [h, w], "counts": s[:2]}))
    s = to_string([40, 700, 30, 1000, n - 1770])
    out.append(("string_truncated_in_difference_97x257", h, w, {"size": [h, w], "counts": s[:-2]}))
    return out


_MASK_CASES = None


def mask_cases():
    global _MASK_CASES
    if _MASK_CASES is None:
        _MASK_CASES = _polygon_cases() + _sequence_cases()
        names = [c[0] for c in _MASK_CASES]
        assert len(set(names)) == len(names)
    return _MASK_CASES


def mask_case(name):
    return next(c for c in mask_cases() if c[0] == name)


# masks for the IoU table: a mixed-size set whose pairs give -1 (sizes differ), 0.0 (disjoint columns, disjoint rows of the same
# columns, an empty mask) and proper ratios; iou_crowd() marks the ones that are paired as crowd GTs too
IOU_MASK_NAMES = [
    "star_65_33x129", "star_3_33x129", "closed_129_33x129", "rect_to_h_inner_33x129", "rect_to_h_last_column_33x129",
    "outside_partly_left_33x129", "outside_partly_right_33x129", "outside_wholly_top_33x129", "poly_empty_mask_33x129",
    "counts_checker_33x129", "string_column_straddle_33x129", "counts_last_pixel_33x129", "counts_ones_33x129",
    "iou_last_partial_word_a_33x129", "iou_last_partial_word_b_33x129", "iou_last_partial_word_c_33x129",
    "star_65_97x130", "polys_5_overlapping_97x130", "counts_checker_97x130", "string_ones_97x130",
    "star_65_65x65", "counts_checker_65x65",
]


def iou_mask_cases():
    """IOU_MASK_NAMES as mask cases.  The iou_last_partial_word masks of 33 x 129 live in row 32 alone, the single row of each
    column's second word: a and b share columns 40..59 there, c overlaps a only in rows 0..31."""
    h, w = 33, 129
    a, b, c = (np.zeros((h, w), np.uint8) for _ in range(3))
    a[32, 20:60] = 1
    a[5:9, 30:50] = 1
    b[32, 40:90] = 1
    c[0:32, 30:50] = 1
    extra = {"iou_last_partial_word_a_33x129": a, "iou_last_partial_word_b_33x129": b, "iou_last_partial_word_c_33x129": c}
    out = []
    for name in IOU_MASK_NAMES:
        if name in extra:
            out.append((name, h, w, {"size": [h, w], "counts": counts_of(extra[name])}))
        else:
            out.append(mask_case(name))
    return out


def iou_crowd():
    return [i % 3 == 1 for i in range(len(IOU_MASK_NAMES))]


def box_table():
    """x, y, w, h boxes.  Against the base box 10, 10, 20, 20: touching sides (intersection width or height exactly 0), zero-area
    boxes, the same box, containment, fractions, negative origins; every third gt is a crowd."""
    dets = [
        [10, 10, 20, 20],           # the base box
        [30, 10, 5, 20],            # touches its right side: w == 0
        [10, 30, 20, 5],            # touches its lower side: h == 0
        [30, 30, 5, 5],             # touches its corner
        [15, 15, 0, 10],            # zero width, inside
        [15, 15, 10, 0],            # zero height, inside
        [15, 15, 0, 0],             # a point
        [12, 12, 4, 4],             # inside
        [0, 0, 100, 100],           # contains
        [29.999, 10, 5, 20],        # overlaps by a sliver
        [10.25, 9.5, 20.125, 20.75],
        [-5, -5, 10, 10],           # negative origin, disjoint from the base box
        [-8, -2, 6, 6],
        [-20, -20, 35, 35],         # negative origin reaching the base box
        [0.1, 0.2, 0.3, 0.7],       # inexact fractions
        [1e6, 1e6, 1e3, 1e3],
    ]
    gts = [
        [10, 10, 20, 20], [10, 10, 20, 20], [30, 10, 5, 20], [-6, -6, 8, 8], [-6, -6, 8, 8], [15, 15, 0, 10], [15, 15, 0, 0],
        [0, 0, 31, 31], [0.1, 0.2, 0.3, 0.7], [0.2, 0.3, 0.3, 0.7], [-20, -20, 35, 35], [5, 20, 40, 0],
    ]
    crowd = [i % 3 == 1 for i in range(len(gts))]
    return np.array(dets, dtype=np.float64), np.array(gts, dtype=np.float64), np.array(crowd, dtype=np.uint8)


IOU_THRS = np.linspace(.5, 0.95, 10)


def _gt(id_, area, crowd=0):
    return {"id": int(id_), "area": float(area), "iscrowd": int(crowd)}


def _dts(areas):
    return [{"id": i + 1, "area": float(a), "score": 1.0 - i / 1024.0} for i, a in enumerate(areas)]


def match_groups():
    """Groups for coco_match_kernel.  Area ranges: all [0, 1e10], small [0, 1024], medium [1024, 9216], large [9216, 1e10], so
    a GT's area decides per lane whether it is ignored: 500 is regular for all / small, 5000 for all / medium."""
    G = []
    G.append(dict(name="tie_later_gt_wins", gts=[_gt(11, 500), _gt(12, 500), _gt(13, 500)], dts=_dts([500, 500, 500, 500]),
                  ious=[[0.7, 0.7, 0.7], [0.7, 0.7, 0.7], [0.6, 0.8, 0.8], [0.9, 0.9, 0.9]]))
    G.append(dict(name="tie_among_ignored_gts", gts=[_gt(21, 500, 1), _gt(22, 5000), _gt(23, 5000), _gt(24, 500, 1)],
                  dts=_dts([500, 5000, 500]), ious=[[0.8, 0.0, 0.0, 0.8], [0.6, 0.6, 0.6, 0.6], [0.75, 0.75, 0.75, 0.75]]))
    # IoUs exactly at the thresholds: linspace's own values, the decimal literals, and one ulp to either side
    thr_vals = list(IOU_THRS) + [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
    thr_vals += [np.nextafter(v, 0.0) for v in IOU_THRS] + [np.nextafter(v, 1.0) for v in IOU_THRS]
    n = len(thr_vals)
    G.append(dict(name="iou_at_thresholds", gts=[_gt(100 + i, 500) for i in range(n)], dts=_dts([500] * n),
                  ious=np.diag(np.array(thr_vals, dtype=np.float64))))
    one = 1 - 1e-10
    G.append(dict(name="iou_one_and_clamp", gts=[_gt(31, 500), _gt(32, 500), _gt(33, 500), _gt(34, 500)],
                  dts=_dts([500, 500, 500, 500]),
                  ious=[[1.0, one, 0.0, 0.0], [1.0, 1.0, np.nextafter(one, 0.0), 0.0], [1.0, 1.0, 1.0, 1.0], [one, 1.0, 1.0, 0.95]]))
    G.append(dict(name="dets_without_gts", gts=[], dts=_dts([500, 20000, 1024]), ious=np.zeros((3, 0))))
    G.append(dict(name="crowd_matched_by_several", gts=[_gt(41, 500), _gt(42, 800, 1), _gt(43, 5000)],
                  dts=_dts([500, 500, 500, 500, 5000]),
                  ious=[[0.0, 0.9, 0.0], [0.0, 0.9, 0.0], [0.6, 0.9, 0.0], [0.55, 0.7, 0.0], [0.0, 0.8, 0.85]]))
    G.append(dict(name="ignored_gt_not_taken_after_regular", gts=[_gt(51, 500, 1), _gt(52, 500), _gt(53, 5000), _gt(54, 20000)],
                  dts=_dts([500, 500, 5000]),
                  ious=[[0.95, 0.6, 0.9, 0.92], [0.95, 0.6, 0.9, 0.92], [0.0, 0.0, 0.55, 0.9]]))
    G.append(dict(name="gts_without_dets", gts=[_gt(61, 500), _gt(62, 5000, 1)], dts=[], ious=np.zeros((0, 2))))
    G.append(dict(name="gt_id_zero", gts=[_gt(0, 500), _gt(71, 500)], dts=_dts([500, 5000, 500]),
                  ious=[[0.9, 0.6], [0.9, 0.6], [0.9, 0.6]]))
    G.append(dict(name="areas_at_range_edges",
                  gts=[_gt(81, 1024), _gt(82, 9216), _gt(83, np.nextafter(1024.0, 0.0)), _gt(84, np.nextafter(9216.0, 1e9)),
                       _gt(85, 0), _gt(86, 1e10)],
                  dts=_dts([1024, 9216, 0, 1e10, np.nextafter(1024.0, 2000.0), 9215.999, 1024, 9216]),
                  ious=np.array([[0.9, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.9, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.9, 0.0, 0.0, 0.0],
                                 [0.0, 0.0, 0.0, 0.9, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.9, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.9],
                                 [0.1, 0.2, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.3, 0.3]])))
    # 100 detections against 90 GTs; IoUs on the 0.05 grid (linspace's values among them), so ties and thresholds abound
    rng = np.random.default_rng(SEED + 1)
    D, Gn = 100, 90
    grid = np.concatenate([[0.0, 0.25, 0.45], IOU_THRS, [1.0]])
    ious = grid[rng.integers(0, len(grid), size=(D, Gn))]
    ious[rng.random((D, Gn)) < 0.6] = 0.0
    areas = rng.choice([100.0, 1024.0, 3000.0, 9216.0, 20000.0], size=Gn)
    G.append(dict(name="hundred_dets_ninety_gts",
                  gts=[_gt(1000 + g, areas[g], rng.random() < 0.1) for g in range(Gn)],
                  dts=_dts(rng.choice([100.0, 1024.0, 3000.0, 9216.0, 20000.0], size=D)), ious=ious))
    for g in G:
        g["ious"] = np.asarray(g["ious"], dtype=np.float64).reshape(len(g["dts"]), len(g["gts"]))
    return G
