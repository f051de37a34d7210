"""Directed inputs for the loss kernels (csrc/loss.hip) on crowded images and piled-up cells; not a test module.

`build(name)` returns (cfg, heads, target) in the form tests/test_loss.py::_random_case uses: the loss's keyword arguments, the
heads as CPU tensors [(bbox, orien)] and the collate-format target as numpy arrays.  Every hand-written case asserts about itself,
in numpy, that it has the geometry it was written for (`match` below restates the match kernel's arithmetic).  `reference(name)`
holds what the restatements give for a case -- computed once, shared by every test that needs it, never written to -- and the case's
near-threshold counts, which must all be zero: a case that is not clean is a broken case.

Groups
  ladder_*   per-image counts 63, 64, 65, 128, 129, 256, 257, 1024 with unequal neighbours and empty images: the second and later
             ballot rounds of the orientation culls, the second and later trips of the box kernels' LDS fill, image offsets g0 that
             are no multiple of 64 or 256
  order      three instances of one (scale, anchor) at collate indices 10, 70, 130 whose ROIs share a block of pixels with the
             four mask patterns that tell the order of the walk apart
  pile*      cells holding exactly 3, 4, 5, 6 and 9 GTs of one anchor: the cls4 short path, the nmatch > 4 rescan, the winner
             beyond index 256
  seams      ROI edges on and next to the forward (16 x 64) and gradient (64 x 64 plus 2) tile seams, ROIs clamped to one column /
             one row
  tie        transposed anchors of two scales and square GTs (bit-equal anchor IoUs: the first maximum wins), a centre on a cell
             boundary and one at normalised 1.0
"""
import functools
import types

import numpy as np

from conftest import ANCHOR_MASK, ANCHORS_YOLOV4
import loss_grad_np
import loss_np

f32 = np.float32

LADDER_COUNTS = (63, 64, 65, 128, 129, 256, 257, 1024)
PILE_SIZES = (3, 4, 5, 6, 9)
# exclusive ROI ends and ROI starts against the gradient tile seam at 64 (these hold the forward seam's 64, 65 and 63, 64), the
# forward row seam at 16, and the border clamps
SEAM_X2, SEAM_X1 = (62, 63, 64, 65), (63, 64, 65, 66)
SEAM_Y2, SEAM_Y1 = (16, 17, 62, 63, 64, 65), (15, 16, 63, 64, 65, 66)
ANCHORS_TIE = [[12, 16], [19, 36], [32, 24], [24, 32], [76, 55], [72, 146], [142, 110], [192, 243], [459, 401]]


def make_cfg(size, anchors=ANCHORS_YOLOV4, **kw):
    """the anchor4 loss config at an image size (tests/test_loss.py::_cfg's values)"""
    h, w = size
    c = dict(grid_size=[[h // 32, w // 32], [h // 16, w // 16], [h // 8, w // 8]], image_size=[h, w], anchors=anchors,
             anchor_mask=ANCHOR_MASK, num_classes=80, center_region=0.6, valid_region=0.6, label_smooth=False,
             obj_ignore_threshold=0.7, weight=[1, 1, 1, 1, 1, 20, 20], scales_weight=[1, 1, 1])
    c.update(kw)
    return c


def match(cfg, gt_bbox, s, tie_last=False):
    """loss_match_kernel's arithmetic for every GT at scale s, as tests/loss_np.py writes it (float32, the reference's order):
    a (anchor within the scale, -1: matched elsewhere), cx, cy, key, the ROI [x1, x2) x [y1, y2), the centre and center_wh in
    pixels.  `tie_last` is the mutant that resolves equal anchor IoUs to the last maximum."""
    nH, nW = cfg["grid_size"][s]
    H, W = cfg["image_size"]
    mask = list(cfg["anchor_mask"][s])
    vr, cr = f32(cfg["valid_region"]), f32(cfg["center_region"])
    g = np.asarray(gt_bbox, f32).reshape(-1, 4) * np.asarray([nW, nH, nW, nH], f32)
    scale_wh = np.asarray([W, H], f32) / np.asarray([nW, nH], f32)
    ga = np.asarray(cfg["anchors"], f32) / scale_wh
    w, h = g[:, 2], g[:, 3]
    inter = np.minimum(w[:, None], ga[None, :, 0]) * np.minimum(h[:, None], ga[None, :, 1])
    ai = inter / (((w * h)[:, None] + (ga[:, 0] * ga[:, 1])[None]) - inter)
    best = ai.shape[1] - 1 - np.argmax(ai[:, ::-1], 1) if tie_last else np.argmax(ai, 1)
    a = np.asarray([mask.index(k) if k in mask else -1 for k in best], np.int64)
    cx = np.minimum(np.maximum(np.floor(g[:, 0]), f32(0)), f32(nW - 1)).astype(np.int64)
    cy = np.minimum(np.maximum(np.floor(g[:, 1]), f32(0)), f32(nH - 1)).astype(np.int64)
    x, y = g[:, 0] * scale_wh[0], g[:, 1] * scale_wh[1]
    vw = (w * vr + f32(0.5)) * scale_wh[0]
    vh = (h * vr + f32(0.5)) * scale_wh[1]
    clip = lambda v, hi: np.rint(np.minimum(np.maximum(v, f32(0)), f32(hi))).astype(np.int64)      # noqa: E731
    return types.SimpleNamespace(best=best, a=a, cx=cx, cy=cy, key=np.where(a < 0, -1, (a * nH + cy) * nW + cx), g=g,
                                 x1=clip(x - vw, W - 1), x2=clip(x + vw, W - 1) + 1, y1=clip(y - vh, H - 1),
                                 y2=clip(y + vh, H - 1) + 1, px=x, py=y, cw=vw / vr * cr, ch=vh / vr * cr)


def pile_sizes(cfg, target):
    """{(image, scale, key): [GT indices within the image]} of the cells that hold more than one GT"""
    out = {}
    gi = target[2]
    for s in range(len(cfg["grid_size"])):
        m = match(cfg, target[0], s)
        for b in range(len(gi) - 1):
            for j in range(int(gi[b]), int(gi[b + 1])):
                if m.key[j] >= 0:
                    out.setdefault((b, s, int(m.key[j])), []).append(j - int(gi[b]))
    return {k: v for k, v in out.items() if len(v) > 1}


def roi_edges(cfg, target):
    """the ROI edges of the matched GTs over all scales: sets of x1, x2, y1, y2"""
    e = dict(x1=set(), x2=set(), y1=set(), y2=set())
    for s in range(len(cfg["grid_size"])):
        m = match(cfg, target[0], s)
        for k in e:
            e[k] |= set(getattr(m, k)[m.a >= 0].tolist())
    return e


def _heads(seed, B, cfg):
    from orienmask_amd import synth
    heads = synth.synth_heads(900 + seed, B, cfg["grid_size"], num_classes=cfg["num_classes"], regime="sparse")
    return [(b.clone(), o.clone()) for b, o in heads]


def _ellipse(box, H, W, frac=0.48, n=16):
    from orienmask_amd import synth
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    cx, cy, w, h = box[0] * W, box[1] * H, box[2] * W, box[3] * H
    return synth._fill_polygon(cx + np.cos(t) * w * frac, cy + np.sin(t) * h * frac, H, W)


def _plant_pile(cfg, target, b, indices, s, anchor, cell, classes):
    """Overwrite the GTs `indices` of image b with a pile on cell (cy, cx) of scale s, all matched to `anchor` (an index into the
    anchor list): sizes and offsets differ from member to member, so the member that supplies the box targets is visible."""
    gb, gc, gi, gm = target
    H, W = cfg["image_size"]
    nH, nW = cfg["grid_size"][s]
    aw, ah = cfg["anchors"][anchor]
    for k, (j, c) in enumerate(zip(indices, classes)):
        n = int(gi[b]) + j
        box = [(cell[1] + 0.15 + 0.08 * k) / nW, (cell[0] + 0.85 - 0.07 * k) / nH, aw * (1 + 0.03 * k) / W, ah * (1 - 0.02 * k) / H]
        gb[n] = np.asarray(box, f32)
        gc[n] = c
        gm[n] = _ellipse(gb[n], H, W, frac=0.3 + 0.02 * k)


def _pile_key(cfg, s, anchor, cell):
    nH, nW = cfg["grid_size"][s]
    return (cfg["anchor_mask"][s].index(anchor) * nH + cell[0]) * nW + cell[1]


def _clear_pile_cells(cfg, target, b, piles):
    """Move every other GT of image b that sits on a pile's cell two cells along x (its mask with it), then assert that each
    pile's cell holds exactly the pile's members."""
    gb, gc, gi, gm = target
    g0, g1 = int(gi[b]), int(gi[b + 1])
    W = cfg["image_size"][1]
    for _ in range(8):
        moved = False
        for s, anchor, cell, indices, _c in piles:
            nW = cfg["grid_size"][s][1]
            own = np.flatnonzero(match(cfg, gb[g0:g1], s).key == _pile_key(cfg, s, anchor, cell))
            for j in set(own.tolist()) - set(indices):
                step = 2 if cell[1] + 2 < nW else -2
                gb[g0 + j, 0] += f32(step / nW)
                gm[g0 + j] = np.roll(gm[g0 + j], step * (W // nW), axis=1)
                moved = True
        if not moved:
            break
    for s, anchor, cell, indices, _c in piles:
        own = np.flatnonzero(match(cfg, gb[g0:g1], s).key == _pile_key(cfg, s, anchor, cell))
        assert own.tolist() == sorted(indices), ("a pile's cell does not hold exactly its members", s, cell, own)


def _ladder(size, counts, seed, **kw):
    from orienmask_amd import synth
    cfg = make_cfg(size, **kw)
    target = synth.synth_targets(seed, len(counts), size[0], size[1], list(counts))
    assert np.diff(target[2]).tolist() == list(counts)
    return cfg, _heads(seed, len(counts), cfg), target


def ladder_65_0_130_1():
    return _ladder((128, 128), [65, 0, 130, 1], 1)


def ladder_300_7_pile9():
    """nine GTs of image 0 on one S08 cell, their indices in five ballot rounds and the last one beyond 256"""
    cfg, heads, target = _ladder((128, 192), [300, 7], 1)
    p9 = (2, 1, (9, 14), [5, 40, 77, 120, 150, 200, 230, 260, 290], [5, 6, 7, 8, 5, 9, 10, 6, 11])
    _plant_pile(cfg, target, 0, p9[3], p9[0], p9[1], p9[2], p9[4])
    _clear_pile_cells(cfg, target, 0, [p9])
    return cfg, heads, target


def ladder_1024():
    return _ladder((64, 128), [1024], 1)


def ladder_1024_3():
    return _ladder((64, 128), [1024, 3], 4)


def ladder_257_63():
    return _ladder((96, 96), [257, 63], 3)


def ladder_64_0_129_256_128_0():
    return _ladder((64, 96), [64, 0, 129, 256, 128, 0], 5)


ORDER_INDICES = (10, 70, 130)


def order():
    """One image of 140 GTs.  GTs 10, 70 and 130 share S08's anchor 0 and overlap on a block; every seventh other GT shares the
    anchor too and lies in the same forward tiles but left of the block (so each round compacts more than one slot, and none of
    the three sits in slot 0 of its round); the rest match other anchors or scales.  In the block the masks of (10, 70, 130) are
    mask / non-mask / mask, non-mask / non-mask / mask, mask / non-mask / non-mask and non-mask throughout, by quadrant."""
    H, W, N = 64, 128, 140
    cfg = make_cfg((H, W))
    rng = np.random.default_rng(11)
    gb = np.zeros((N, 4), f32)
    gm = np.zeros((N, H, W), bool)
    main = dict(zip(ORDER_INDICES, [(56.0, 30.0, 12.0, 16.0), (60.0, 34.0, 13.0, 15.0), (58.0, 27.0, 11.5, 17.0)]))
    others = [a for a in ANCHORS_YOLOV4[1:7]]
    for j in range(N):
        if j in main:
            cx, cy, w, h = main[j]
        elif j % 7 == 3:                                   # the same anchor, left of the block
            cx, cy, w, h = 9.0 + (j % 5), 12.0 + (j * 5) % 40, 12.0 + 0.1 * (j % 4), 16.0 - 0.1 * (j % 3)
        else:
            aw, ah = others[j % len(others)]
            w, h = min(aw * rng.uniform(0.9, 1.1), 0.95 * W), min(ah * rng.uniform(0.9, 1.1), 0.95 * H)
            cx, cy = rng.uniform(w / 4, W - w / 4), rng.uniform(h / 4, H - h / 4)
        gb[j] = [cx / W, cy / H, w / W, h / H]
        gm[j] = _ellipse(gb[j], H, W)
    gc = (np.arange(N) * 7 % 80).astype(np.int64)
    m = match(cfg, gb, 2)
    i0, i1, i2 = ORDER_INDICES
    assert m.a[i0] == m.a[i1] == m.a[i2] == 0, m.a[list(ORDER_INDICES)]
    for s in (0, 1):
        assert np.all(match(cfg, gb, s).a[list(ORDER_INDICES)] == -1)
    same = np.flatnonzero(m.a == 0)
    assert set(same) == set(ORDER_INDICES) | {j for j in range(N) if j % 7 == 3 and j not in main}, same
    bx1, bx2 = int(m.x1[list(ORDER_INDICES)].max()), int(m.x2[list(ORDER_INDICES)].min())
    by1, by2 = int(m.y1[list(ORDER_INDICES)].max()), int(m.y2[list(ORDER_INDICES)].min())
    assert bx2 - bx1 >= 4 and by2 - by1 >= 4, (bx1, bx2, by1, by2)
    for j in same:                                          # nobody else of this anchor touches the block
        if j not in main:
            assert m.x2[j] <= bx1 or m.x1[j] >= bx2 or m.y2[j] <= by1 or m.y1[j] >= by2, j
    # every round holds culled-in instances of the anchor in front of its main instance, in the main instance's forward tile
    for j in ORDER_INDICES:
        before = [k for k in same if 64 * (j // 64) <= k < j and m.x1[k] < 64 and m.y1[k] < by2 and m.y2[k] > by1]
        assert before, j
    xm, ym = (bx1 + bx2) // 2, (by1 + by2) // 2
    quad = np.zeros((H, W), np.int8)                        # 1: m/n/m  2: n/n/m  3: m/n/n  4: n/n/n
    quad[by1:ym, bx1:xm], quad[by1:ym, xm:bx2], quad[ym:by2, bx1:xm], quad[ym:by2, xm:bx2] = 1, 2, 3, 4
    block = quad > 0
    gm[i0] = (gm[i0] & ~block) | (quad == 1) | (quad == 3)
    gm[i1] = gm[i1] & ~block
    gm[i2] = (gm[i2] & ~block) | (quad == 1) | (quad == 2)
    pattern = gm[i0].astype(int) * 4 + gm[i1] * 2 + gm[i2]
    for q, want in ((1, 5), (2, 1), (3, 4), (4, 0)):
        assert (quad == q).sum() > 0 and np.all(pattern[quad == q] == want), q
    target = (gb, gc, np.array([0, N], np.int64), gm)
    return cfg, _heads(12, 1, cfg), target


# (scale, anchor index in the list, cell (cy, cx), indices within the image, classes)
PILES = [(2, 0, (2, 3), [0, 64, 128], [3, 17, 40]),                                   # 3: lane 0 of three rounds, all different
         (2, 1, (5, 9), [63, 127, 191, 255], [1, 2, 3, 4]),                           # 4: the last lanes, all different
         (2, 2, (8, 4), [10, 11, 12, 13, 14], [7, 7, 9, 7, 9]),                       # 5: repeated classes
         (1, 3, (2, 5), [250, 251, 256, 257, 260, 269], [20, 21, 22, 23, 24, 25]),    # 6: all different, across index 256
         (2, 0, (9, 12), [3, 40, 66, 100, 129, 170, 200, 258, 265], [5, 6, 7, 8, 5, 9, 10, 6, 11])]   # 9: five rounds, past 256


def _pile(C=80, **kw):
    from orienmask_amd import synth
    H, W, N = 96, 128, 270
    cfg = make_cfg((H, W), num_classes=C, **kw)
    gb, gc, gi, gm = synth.synth_targets(21, 1, H, W, [N], num_classes=C)
    target = (gb, gc, gi, gm)
    for s, anchor, cell, indices, classes in PILES:
        _plant_pile(cfg, target, 0, indices, s, anchor, cell, [c % C for c in classes])
    _clear_pile_cells(cfg, target, 0, PILES)
    return cfg, _heads(22, 1, cfg), target


def pile():
    return _pile()


def pile_smooth():
    return _pile(label_smooth=True)


def pile_c1():
    return _pile(C=1)


def _find_box(cfg, s, anchor, along, edge, value, other_centre):
    """A box of `anchor`'s size (so that it matches it, at scale s) whose ROI edge `edge` ('1' or '2') along `along` ('x' or 'y')
    is `value`: the centre is searched in steps of 1/8 pixel over the restatement's own ROI formula."""
    H, W = cfg["image_size"]
    aw, ah = cfg["anchors"][anchor]
    L = W if along == "x" else H
    for c8 in range(-8 * 8, 8 * (L + 24) + 1):
        c = c8 / 8.0
        cx, cy = (c, other_centre) if along == "x" else (other_centre, c)
        box = np.asarray([cx / W, cy / H, aw / W, ah / H], f32)
        m = match(cfg, box, s)
        if int(getattr(m, along + edge)[0]) == value and m.a[0] >= 0:
            lo, hi = int(getattr(m, along + "1")[0]), int(getattr(m, along + "2")[0])
            if hi - lo > 1 or value in (L, L - 1):          # not a clamped sliver, unless that is what is asked for
                return box
    raise AssertionError(("no box", along, edge, value))


def seams():
    """One 128 x 128 image.  Each GT has S08 anchor 0's or anchor 1's size and one ROI edge on a chosen pixel next to a tile
    seam; two more are clamped to the last column and the last row.  The masks are small, so the ROI edges are non-mask pixels
    and a wrongly culled instance changes the count and the targets there."""
    H = W = 128
    cfg = make_cfg((H, W))
    boxes, want = [], []
    for i, v in enumerate(SEAM_X2):
        boxes.append(_find_box(cfg, 2, i % 2, "x", "2", v, 20.0 + 24 * i)); want.append(("x2", v))
    for i, v in enumerate(SEAM_X1):
        boxes.append(_find_box(cfg, 2, (i + 1) % 2, "x", "1", v, 24.0 + 24 * i)); want.append(("x1", v))
    for i, v in enumerate(SEAM_Y2):
        boxes.append(_find_box(cfg, 2, i % 2 if v > 17 else 0, "y", "2", v, 12.0 + 20 * i)); want.append(("y2", v))
    for i, v in enumerate(SEAM_Y1):
        boxes.append(_find_box(cfg, 2, (i + 1) % 2, "y", "1", v, 16.0 + 19 * i)); want.append(("y1", v))
    boxes.append(_find_box(cfg, 2, 0, "x", "1", W - 1, 40.0)); want.append(("x1", W - 1))      # one column at the right border
    boxes.append(_find_box(cfg, 2, 0, "y", "1", H - 1, 90.0)); want.append(("y1", H - 1))      # one row at the bottom
    gb = np.stack(boxes).astype(f32)
    m = match(cfg, gb, 2)
    for j, (k, v) in enumerate(want):
        assert m.a[j] >= 0 and int(getattr(m, k)[j]) == v, (j, k, v, int(getattr(m, k)[j]))
    assert (m.x1[-2], m.x2[-2]) == (W - 1, W) and (m.y1[-1], m.y2[-1]) == (H - 1, H)
    N = len(gb)
    gm = np.stack([_ellipse(b, H, W, frac=0.2) for b in gb])
    gc = (np.arange(N) * 3 % 80).astype(np.int64)
    return cfg, _heads(31, 1, cfg), (gb, gc, np.array([0, N], np.int64), gm)


def tie():
    """Anchors 2 (S08) and 3 (S16) are transposes, the image is square and the GTs are square with sizes exact in float32: the
    two anchor IoUs are bit-equal (the products commute) and the first maximum, anchor 2, must win -- positive at S08, key -1 at
    S16.  GT 1's centre lies on a cell boundary (tx = 0), GT 2's at normalised 1.0 (the cell clamps to nW - 1, tx = 1)."""
    H = W = 128
    cfg = make_cfg((H, W), anchors=ANCHORS_TIE)
    px = np.asarray([[52.5, 44.25, 28, 28], [40, 77.5, 27, 27], [128, 30.5, 28.5, 28.5], [90.5, 100.25, 28, 28],
                     [30.25, 20.5, 20, 34]], np.float64)
    gb = (px / [W, H, W, H]).astype(f32)
    N = len(gb)
    for s in range(3):
        g = match(cfg, gb, s).g
        ga = np.asarray(ANCHORS_TIE, f32) / f32(cfg["image_size"][0] // cfg["grid_size"][s][0])
        w, h = g[:4, 2:3], g[:4, 3:4]
        inter = np.minimum(w, ga[None, :, 0]) * np.minimum(h, ga[None, :, 1])
        ai = inter / ((w * h + (ga[:, 0] * ga[:, 1])[None]) - inter)
        assert np.all(ai[:, 2] == ai[:, 3]) and np.all(ai.max(1) == ai[:, 2]), (s, ai)
    m8, m16 = match(cfg, gb, 2), match(cfg, gb, 1)
    assert np.all(m8.a[:4] == 2) and np.all(m16.a[:4] == -1) and np.all(m16.key[:4] == -1)
    assert np.all(match(cfg, gb, 1, tie_last=True).a[:4] == 0)
    assert m8.g[1, 0] - m8.cx[1] == 0 and m8.cx[2] == 15 and m8.g[2, 0] - m8.cx[2] == 1
    gm = np.stack([_ellipse(b, H, W) for b in gb])
    gc = np.asarray([4, 9, 14, 19, 24], np.int64)
    return cfg, _heads(41, 1, cfg), (gb, gc, np.array([0, N], np.int64), gm)


CASES = dict(ladder_65_0_130_1=ladder_65_0_130_1, ladder_300_7_pile9=ladder_300_7_pile9, ladder_1024=ladder_1024,
             ladder_1024_3=ladder_1024_3, ladder_257_63=ladder_257_63, ladder_64_0_129_256_128_0=ladder_64_0_129_256_128_0,
             order=order, pile=pile, pile_smooth=pile_smooth, pile_c1=pile_c1, seams=seams, tie=tie)
NAMES = list(CASES)
# the cases tools/gen_golden_loss.py and tools/gen_golden_loss_grad.py run through the reference: fixture name, the seed of the
# heads (what _heads adds 900 to), full targets stored
FIXTURE_CASES = dict(ladder_65_0_130_1=("crowd_ladder_b4", 901, False), pile=("crowd_pile_b1", 922, True),
                     order=("crowd_order_b1", 912, True))
LIMIT = ("ladder_1024", "ladder_1024_3")


@functools.lru_cache(maxsize=None)
def build(name):
    """(cfg, heads, target) of a case; built once, shared, never written to"""
    cfg, heads, target = CASES[name]()
    for a in target:
        a.setflags(write=False)
    return cfg, heads, target


def heads_np(heads):
    return [(b.numpy(), o.numpy()) for b, o in heads]


class MemoNP(loss_grad_np.LossGradNP):
    """LossGradNP that builds each scale's targets once for the values and the gradient"""

    def __init__(self, **cfg):
        super().__init__(**cfg)
        self._built = {}

    def build_targets(self, s, *a):
        if s not in self._built:
            self._built[s] = super().build_targets(s, *a)
        return self._built[s]


def forward_near(ref, s, head, t):
    """tools/gen_golden_loss.py's four counts from the restatement's own values: IoUs within 4 ulp of obj_ignore_threshold, tiou
    of the positives within 4 ulp of 0.5 and of 0.75, |up-sampled head - torien| of the orientation pixels within 4 ulp of 0.5"""
    near = lambda a, thr: int(loss_grad_np.near_ulp(np.asarray(a, f32).ravel(), thr).sum())      # noqa: E731
    ious = np.concatenate([i.ravel() for i in t["ious"]]) if t["ious"] else np.zeros(0, f32)
    A = len(ref.mask[s])
    B = t["pos"].shape[0]
    po = loss_np.upsample4(np.asarray(head[1], f32)).reshape(B, A, 2, ref.H, ref.W).transpose(0, 1, 3, 4, 2)
    delta = np.abs(po - t["torien"])[t["opos"] | t["oneg"]]
    tiou = t["tiou"][t["pos"] > 0]
    return [near(ious, ref.thr), near(tiou, 0.5), near(tiou, 0.75), near(delta, 0.5)]


GOUT = 1.25


def run_restatement(ref, heads, target, gout=GOUT):
    """what a restatement object gives for a case: per scale the weighted terms, the metric pairs, the targets, both gradients
    and the seven near-threshold counts (four forward, three of the gradient)"""
    hn = heads_np(heads)
    values = ref(hn, target)
    grads = ref.grad(hn, target, gout)
    near = [forward_near(ref, s, hn[s], values[s][2]) + [int(v) for v in grads[s][2]] for s in range(len(hn))]
    return types.SimpleNamespace(values=values, grads=grads, near=near)


@functools.lru_cache(maxsize=None)
def reference(name):
    cfg, heads, target = build(name)
    return run_restatement(MemoNP(**cfg), heads, target)
