"""Directed cases for csrc/post.hip: heads and detections built value by value, and restatements of what the kernels must
return for them.  Plain numpy / torch on the CPU; tests/test_post_directed_cpu.py checks that every case has the property it
claims, tests/test_post_directed.py runs them on the GPU.

Select cases are (heads, cfg) pairs: every (candidate, class) pair of the heads is below conf_thresh except the planted ones,
whose objectness logit is +30 (sigmoid = 1.0f exactly in both of torch's paths), so a planted pair's confidence is
sigmoid(class logit) and the number of passing pairs, their scores and their positions are chosen one by one.

Mask cases are (geometry, anchor_mask, oriens, dets, fields, counts) tuples for om_postprocess_masks, the entry that takes the
detections from the caller.

Constants of csrc/post.hip restated here (statements of the code, not observations): DEC_TILE, SEL_LIST_MAX, SEL_LDS_MASK_N,
SEL_WAVES, MASK_PX and the launch form of launch_post_mask (mask_launch_unchunked)."""
import collections

import numpy as np
import torch

from conftest import ANCHORS_YOLOV4, ANCHOR_MASK
from oracle import orienmask_ref as R

C = 80
SIZE = (96, 128)             # 756 candidates, 60 480 pairs, 30 decode tiles: each of the 16 waves of the radix passes owns a tile
CONF_THRESH = 0.005
DEC_TILE = 2048              # pairs per decode workgroup = keys per tile
SEL_LIST_MAX = 4096          # passing pairs the compacted list holds; above: radix select
SEL_LDS_MASK_N = 512         # candidates up to which the suppression matrix stays in LDS
SEL_WAVES = 16               # waves of post_select_kernel; wave w owns tiles [ntiles * w / 16, ntiles * (w + 1) / 16)
MASK_PX = 16
VEC_CLASSES = (C // 32) * 32         # classes below this go through torch's vectorised sigmoid, the rest through the scalar one
F32 = np.float32


def grids_of(size):
    h, w = size
    return [[h // 32, w // 32], [h // 16, w // 16], [h // 8, w // 8]]


def make_oracle(size, anchor_mask=ANCHOR_MASK, **kw):
    args = dict(conf_thresh=CONF_THRESH, nms_pre=400, nms_post=100, orien_thresh=0.3)
    args.update(kw)
    return R.PostProcessOracle(grids_of(size), list(size), ANCHORS_YOLOV4, anchor_mask, C, **args)


def hip_kwargs(size, anchor_mask=ANCHOR_MASK, **kw):
    """Constructor arguments of orienmask_amd.eval.OrienMaskYOLOPostProcess for the same configuration as make_oracle."""
    args = dict(grid_size=grids_of(size), image_size=list(size), anchors=ANCHORS_YOLOV4, anchor_mask=anchor_mask, num_classes=C,
                conf_thresh=CONF_THRESH, nms_pre=400, nms_post=100, orien_thresh=0.3)
    args.update(kw)
    return args


# ------------------------------------------------------------------------------------------------------------------------
# heads
# ------------------------------------------------------------------------------------------------------------------------
class Heads:
    """bbox heads [1, A * (5 + C), nH, nW] per scale with every objectness and class logit at -30, tx = ty = 0 (box centre =
    cell centre), tw = th = -3 (boxes of 5 % of their anchor: far smaller than a cell), and a seeded orientation field."""

    def __init__(self, size=SIZE, seed=1):
        self.size = size
        self.grids = grids_of(size)
        self.bbox = []
        self.cand_off = [0]
        for gh, gw in self.grids:
            t = torch.full((1, 3, 5 + C, gh, gw), -30.0)
            t[:, :, 0:2] = 0.0
            t[:, :, 2:4] = -3.0
            self.bbox.append(t)
            self.cand_off.append(self.cand_off[-1] + 3 * gh * gw)
        self.ncand = self.cand_off[-1]
        rng = np.random.Generator(np.random.PCG64(seed))
        oh, ow = size[0] // 4, size[1] // 4
        self.oriens = [torch.from_numpy((rng.standard_normal((1, 6, oh, ow)) * 2).astype(F32)) for _ in self.grids]

    def locate(self, cand):
        s = sum(cand >= o for o in self.cand_off[1:3])
        gh, gw = self.grids[s]
        a, pix = divmod(cand - self.cand_off[s], gh * gw)
        return s, a, pix // gw, pix % gw

    def cand_index(self, s, a, y, x):
        gh, gw = self.grids[s]
        return self.cand_off[s] + a * gh * gw + y * gw + x

    def plant(self, pair, logit):
        s, a, y, x = self.locate(pair // C)
        self.bbox[s][0, a, 4, y, x] = 30.0
        self.bbox[s][0, a, 5 + pair % C, y, x] = float(logit)

    def set_box(self, cand, **kw):
        s, a, y, x = self.locate(cand)
        for k, v in kw.items():
            self.bbox[s][0, a, "xywh".index(k[1]), y, x] = float(v)

    def predict(self):
        return tuple((b.reshape(1, -1, b.shape[3], b.shape[4]).clone(), o.clone()) for b, o in zip(self.bbox, self.oriens))


def cat_batch(predicts):
    """Single-image predicts -> one batch."""
    return tuple((torch.cat([p[i][0] for p in predicts], 0), torch.cat([p[i][1] for p in predicts], 0)) for i in range(3))


def logits_for_keys(keys, cls):
    """Class logits whose float32 sigmoid, in the path torch takes for class `cls` of an 80-class row (vectorised below
    VEC_CLASSES, scalar above), has exactly the given bit patterns.  Search among the float neighbours of logit(key)."""
    out = []
    for key in keys:
        p = float(np.array([key], dtype=np.uint32).view(F32)[0])
        x0 = F32(np.log(p / (1.0 - p)))
        cand = [x0]
        lo = hi = x0
        for _ in range(256):
            lo = np.nextafter(lo, F32(-np.inf)); hi = np.nextafter(hi, F32(np.inf))
            cand += [lo, hi]
        got = sigmoid_as_decode(np.array(cand, dtype=F32), cls).view(np.uint32)
        hit = np.flatnonzero(got == key)
        assert hit.size, ("no float32 logit gives this sigmoid", hex(key))
        out.append(float(cand[hit[0]]))
    return out


def sigmoid_as_decode(x, cls):
    """torch's sigmoid of class logits as PostProcessOracle.decode_scale evaluates it: rows of 5 + C, column 5 + cls."""
    t = torch.full((len(x), 5 + C), -30.0)
    t[:, 5 + cls] = torch.from_numpy(np.asarray(x, dtype=F32))
    with R._single_thread():
        return t[:, 5:].sigmoid()[:, cls].numpy().copy()


SelectCase = collections.namedtuple("SelectCase", "id predict cfg claims stable")
# claims: dict of what the case plants (total, n, kept, tie group, ...), verified by tests/test_post_directed_cpu.py
# stable: True when an exact tie touches a cut (the expectation is expected_stable, not the oracle)


def _class_order():
    return [(k * 37 + 3) % C for k in range(C)]        # a permutation of the classes: both sigmoid paths from the first slots on


def free_slots(heads, taken=(), vector_only=False):
    """(candidate, class) pairs in a fixed order that walks every candidate of every scale before it changes class."""
    taken = set(taken)
    for cls in _class_order():
        if vector_only and cls >= VEC_CLASSES:
            continue
        for cand in range(heads.ncand):
            if cand * C + cls not in taken:
                yield cand * C + cls


def rank_logits(total, hi=3.0, step=1.0e-3):
    """Strictly decreasing logits by rank; their sigmoids are 5e-5 apart at the least, far more than the one ulp by which
    torch's two sigmoid paths can differ."""
    return [hi - r * step for r in range(total)]


def build_ranked(total, logits=None, fixed=None, partners=(), vector_ranks=(), seed=7, plant_upto=None, heads_seed=1, vector_only=False):
    """Heads with `total` passing pairs; rank r (0 = strongest) gets logits[r].
    fixed: {rank: pair} places chosen ranks on chosen pairs; every other rank gets a free slot by a seeded permutation, so index
    order and score order differ.  vector_ranks: ranks that must sit on a class of the vectorised sigmoid path.
    partners: (i, j) with i < j: rank j sits on rank i's cell and class under the next anchor, with tw / th set so that the two
    boxes coincide (IoU ~ 1: i suppresses j).
    plant_upto: plant only the ranks below it (the same layout with fewer passing pairs).  vector_only: every slot on a class of
    the vectorised sigmoid path."""
    heads = Heads(seed=heads_seed)
    logits = rank_logits(total) if logits is None else logits
    fixed = dict(fixed or {})
    partner_of = {j: i for i, j in partners}
    rng = np.random.Generator(np.random.PCG64(seed))
    n_free = total - len(fixed) - len(partner_of)
    slots = []
    gen = free_slots(heads, taken=fixed.values(), vector_only=vector_only)
    while len(slots) < n_free + 64:
        slots.append(next(gen))
    slots = [slots[i] for i in rng.permutation(len(slots))]
    vec = [p for p in slots if p % C < VEC_CLASSES]
    pair_of = dict(fixed)
    for r in vector_ranks:
        if r not in pair_of and r not in partner_of:
            pair_of[r] = vec.pop()
    used = set(pair_of.values())
    rest = [p for p in slots if p not in used]
    anchors = np.array(ANCHORS_YOLOV4, dtype=np.float64)
    for i, j in partners:                              # the suppressors and their partners first: both slots must be free
        while i not in pair_of:
            p = rest.pop()
            s, a, y, x = heads.locate(p // C)
            if heads.cand_index(s, (a + 1) % 3, y, x) * C + p % C not in used:
                pair_of[i] = p
                used.add(p)
        cand, cls = divmod(pair_of[i], C)
        s, a, y, x = heads.locate(cand)
        a2 = (a + 1) % 3
        cand2 = heads.cand_index(s, a2, y, x)
        assert cand2 * C + cls not in used
        pair_of[j] = cand2 * C + cls
        used.add(pair_of[j])
        wa, wb = anchors[ANCHOR_MASK[s][a]], anchors[ANCHOR_MASK[s][a2]]
        heads.set_box(cand2, tw=-3.0 + np.log(wa[0] / wb[0]), th=-3.0 + np.log(wa[1] / wb[1]))
    rest = [p for p in rest if p not in used]
    for r in range(total):
        if r not in pair_of:
            pair_of[r] = rest.pop()
    for r in range(total if plant_upto is None else plant_upto):
        heads.plant(pair_of[r], logits[r])
    return heads, pair_of


def wave_of_pair(pair, npairs):
    """The wave of post_select_kernel's radix passes that reads this pair's key."""
    ntiles = (npairs + DEC_TILE - 1) // DEC_TILE
    tile = pair // DEC_TILE
    for w in range(SEL_WAVES):
        if ntiles * w // SEL_WAVES <= tile < ntiles * (w + 1) // SEL_WAVES:
            return w
    raise AssertionError(pair)


def _tie_case(cid, total, nms_pre, g, r, where):
    """S5: ranks nms_pre - r .. nms_pre - r + g - 1 share one key; r of the g are inside the cut."""
    first = nms_pre - r
    logits = rank_logits(total)
    for k in range(first, first + g):
        logits[k] = logits[first]
    heads0 = Heads()
    npairs = heads0.ncand * C
    if where == "spread":        # one pair in each of g tiles that at least three waves own
        tiles = [1, 5, 9, 14, 18, 22, 27][:g]
        fixed = {first + k: (t * DEC_TILE + 300 + 7 * k) // C * C + [4, 9, 17, 23, 31, 40, 50][k] for k, t in enumerate(tiles)}
    else:                        # the whole group inside one 256-key row: classes 10 .. 10 + g - 1 of one candidate
        cand = 416                                            # pairs 33 280 .. 33 359 = row 130 exactly from its first key on
        assert (cand * C) % 256 == 0
        fixed = {first + k: cand * C + 10 + k for k in range(g)}
    heads, pair_of = build_ranked(total, logits, fixed=fixed)
    ties = sorted(pair_of[k] for k in range(first, first + g))
    claims = dict(total=total, n=nms_pre, tie_pairs=ties, r=r, g=g, waves=sorted({wave_of_pair(p, npairs) for p in ties}),
                  rows=sorted({p // 256 for p in ties}))
    return SelectCase(cid, heads.predict(), dict(nms_pre=nms_pre, nms_post=nms_pre), claims, True)


_SELECT = {}


def select_cases():
    """id -> SelectCase.  Built once per process."""
    if _SELECT:
        return _SELECT
    out = []
    # S1: total around nms_pre (case B <-> case A); nms_post = nms_pre, so that the output keeps the list's order in case B
    for nms_pre in (400, 1024):
        for total in (nms_pre - 1, nms_pre, nms_pre + 1):
            heads, _ = build_ranked(nms_pre + 1, plant_upto=total, seed=11)
            out.append(SelectCase("S1_pre%d_total%d" % (nms_pre, total), heads.predict(), dict(nms_pre=nms_pre, nms_post=nms_pre),
                                  dict(total=total, n=min(total, nms_pre), kept=min(total, nms_pre)), False))
    # S1t: one more pair exactly ON conf_thresh (the threshold is that pair's score): `>` leaves total at nms_pre
    heads, pair_of = build_ranked(401, seed=11)
    conf = decode_conf(make_oracle(SIZE), heads.predict(), 0)
    thr = float(conf.view(-1)[pair_of[400]])
    out.append(SelectCase("S1t_pair_on_conf_thresh", heads.predict(), dict(nms_pre=400, nms_post=400, conf_thresh=thr),
                          dict(total=400, n=400, kept=400, on_thresh=1), False))
    # S2, S5, S6, S7: nms_post = nms_pre, so that the whole selection -- the pairs at the cut included -- is in the output
    # S2: total around SEL_LIST_MAX, the same 4095 strongest pairs
    for total in (4095, 4096, 4097):
        heads, _ = build_ranked(4097, plant_upto=total, seed=12)
        out.append(SelectCase("S2_total%d" % total, heads.predict(), dict(nms_pre=400, nms_post=400), dict(total=total, n=400, kept=400), False))
    # S3: case B, kept around nms_post, six suppressed pairs, scores not monotone in index order
    for kept in (99, 100, 101):
        partners = [(3, 40), (10, 11), (50, 90), (60, 61), (70, 100), (80, 104)]
        heads, _ = build_ranked(kept + len(partners), partners=partners, seed=13)
        out.append(SelectCase("S3_kept%d" % kept, heads.predict(), dict(nms_pre=400),
                              dict(total=kept + len(partners), n=kept + len(partners), kept=kept), False))
    # S4: n around SEL_LDS_MASK_N; suppressing pairs on both sides of position 512 and of a 64-column word boundary
    for n in (512, 513):
        partners = [(10, 70), (60, 63), (62, 64), (100, 511), (447, 449), (450, 510)] + ([(300, 512)] if n == 513 else [])
        for backend in ("cpu", "cuda"):
            heads, _ = build_ranked(n, partners=partners, seed=14)
            out.append(SelectCase("S4_n%d_%s" % (n, backend), heads.predict(), dict(nms_pre=1024, nms_backend=backend),
                                  dict(total=n, n=n, kept=n - len(partners), partners=partners), False))
    # S5: exact ties across the nms_pre cut, list path and radix path, spread over waves and inside one row
    for path, total in (("list", 1000), ("radix", 4200)):
        out.append(_tie_case("S5_%s_spread" % path, total, 400, 7, 3, "spread"))
        out.append(_tie_case("S5_%s_one_row" % path, total, 400, 7, 3, "row"))
    # S6: every passing key identical, radix path
    heads, pair_of = build_ranked(4200, logits=[1.0] * 4200, vector_only=True, seed=16)
    out.append(SelectCase("S6_all_keys_equal", heads.predict(), dict(nms_pre=400, nms_post=400), dict(total=4200, n=400, all_equal=True), True))
    # S7: radix path, the keys around the cut share their top 13 bits (level 2 decides), then their top 24 (level 3 decides)
    logits = rank_logits(4200, hi=4.0)
    assert logits[367] > 0.13
    for k in range(368, 432):                      # 64 sigmoids inside [0.5, 0.53125): one level-1 bin, distinct level-2 bins
        logits[k] = 0.12 - (k - 368) * 1.5e-3
    for k in range(432, 4200):
        logits[k] = -0.01 - (k - 432) * 1.0e-3
    heads, _ = build_ranked(4200, logits=logits, seed=17)
    out.append(SelectCase("S7_shared_top13", heads.predict(), dict(nms_pre=400, nms_post=400),
                          dict(total=4200, n=400, kept=400, shared_bits=13, around=(368, 432)), False))
    key0 = 0x3F030540                               # sigmoid ~ 0.5118: 16 consecutive floats from here share bits 31..8
    cls7 = 5
    consecutive = logits_for_keys([key0 + 15 - k for k in range(16)], cls7)
    logits = list(logits)
    lo_x, hi_x = min(consecutive), max(consecutive)
    logits[368:432] = [hi_x + 0.07 - k * 1.5e-3 for k in range(24)] + consecutive + [lo_x - 1.0e-3 - k * 1.5e-3 for k in range(24)]
    fixed = {392 + k: ((1 + k * 27 // 15) * DEC_TILE + 11 * k + 160) // C * C + cls7 for k in range(16)}
    heads, _ = build_ranked(4200, logits=logits, fixed=fixed, seed=17)
    out.append(SelectCase("S7_shared_top24", heads.predict(), dict(nms_pre=400, nms_post=400),
                          dict(total=4200, n=400, kept=400, shared_bits=24, around=(392, 408), keys=[key0 + 15 - k for k in range(16)]), False))
    # S8: exact ties across the nms_post cut, case B (index-ordered list) and case A (sorted list)
    for name, total in (("caseB", 150), ("caseA", 500)):
        logits = rank_logits(total)
        for k in range(95, 105):
            logits[k] = logits[95]
        heads, pair_of = build_ranked(total, logits=logits, vector_ranks=range(95, 105), seed=18)
        out.append(SelectCase("S8_%s" % name, heads.predict(), dict(nms_pre=400),
                              dict(total=total, n=min(total, 400), kept=min(total, 400), post_ties=sorted(pair_of[k] for k in range(95, 105)),
                                   r=5, g=10), True))
    for c in out:
        assert c.id not in _SELECT
        _SELECT[c.id] = c
    return _SELECT


def all_pass_predict(batch):
    """Every logit 0: each of the 60 480 pairs of an image passes with confidence 0.25 (dirties the whole key workspace)."""
    h = Heads()
    return tuple((torch.zeros(batch, 255, gh, gw), o.repeat(batch, 1, 1, 1)) for (gh, gw), o in zip(h.grids, h.oriens))


def empty_predict():
    return Heads(seed=3).predict()


S9_MEMBERS = ("S2_total4097", "S1_pre400_total400", None)       # None: the empty image


# ------------------------------------------------------------------------------------------------------------------------
# the select pipeline restated with the tie rule of csrc/post.hip: ties go to the lowest pair index
# ------------------------------------------------------------------------------------------------------------------------
def decode_conf(oracle, predict, b):
    return torch.cat([oracle.decode_scale(predict[i][0][b], i)[1] for i in range(len(oracle.grids))], 0)


def _nms_stable(oracle, dets, cls):
    """batched_nms (function.py:77-103) with the visiting order made explicit: score descending, ties by list position."""
    if dets.shape[0] == 0:
        return torch.zeros(0, dtype=torch.long)
    if oracle.nms_backend == "cuda":
        return R.batched_nms(dets, cls, oracle.nms_thresh, oracle.nms_normalized, "cuda")[2]         # nms_cuda sorts stably itself
    max_coordinate = 1.5 if oracle.nms_normalized else dets[:, :2].max() + dets[:, 2:4].max() / 2
    shifted = dets.clone()
    shifted[:, :2] += cls.float().view(-1, 1) * (max_coordinate + 0.5)
    order = torch.sort(shifted[:, 4].contiguous(), stable=True, descending=True)[1].numpy()
    return torch.from_numpy(R.nms_numpy(shifted.numpy(), oracle.nms_thresh, order=order))


def expected_stable(oracle, predict, b, mutate=()):
    """PostProcessOracle's pipeline (decode_scale, orien_field, finish) with both topk calls replaced by a stable descending
    sort over the row-major (candidate, class) list.  mutate: names of deliberate errors (the teeth of the CPU test):
      "ge_thresh"      conf >= conf_thresh passes
      "highest_first"  ties at the nms_pre cut go to the highest pair index
      "caseB_sorted"   the output of case B sorted by score
    Returns the oracle's result dict plus total (passing pairs) and pairs (the pair index of every output row)."""
    with torch.no_grad():
        predict = [(p[0].detach().float().cpu(), p[1].detach().float().cpu()) for p in predict]
        coord = torch.cat([oracle.decode_scale(predict[i][0][b], i)[0] for i in range(len(oracle.grids))], 0)
        conf = decode_conf(oracle, predict, b)
        passing = (conf >= oracle.conf_thresh) if "ge_thresh" in mutate else (conf > oracle.conf_thresh)
        sel, cls = torch.nonzero(passing, as_tuple=True)
        score = conf[sel, cls]
        total = int(sel.numel())
        if total > oracle.nms_pre:
            if "highest_first" in mutate:
                top = torch.sort(score.flip(0), stable=True, descending=True)[1][:oracle.nms_pre]
                top = total - 1 - top
            else:
                top = torch.sort(score, stable=True, descending=True)[1][:oracle.nms_pre]
            sel, cls, score = sel[top], cls[top], score[top]
        dets = torch.cat([coord[sel], score.unsqueeze(-1)], 1)
        keep = _nms_stable(oracle, dets, cls)
        kept = int(keep.numel())
        if kept > oracle.nms_post or ("caseB_sorted" in mutate and kept):
            keep = keep[torch.sort(dets[keep, 4], stable=True, descending=True)[1][:oracle.nms_post]]
        field = oracle.orien_field(predict, b)
        masks = masks_of(oracle, field, dets[keep], oracle.flat_anchor_idx[sel][keep])
        return {"bbox": dets[keep], "cls": cls[keep], "keep": keep, "mask": masks, "total": total, "kept": kept,
                "pairs": (sel * oracle.num_classes + cls)[keep], "n_candidates": int(sel.numel())}


def masks_of(oracle, field, dets, a):
    """The predicate of PostProcessOracle.finish (postprocess.py:156-164) on given detections and anchors."""
    gsx = oracle.grid_sizes[a, 0]; gsy = oracle.grid_sizes[a, 1]
    xc = (gsx * dets[:, 0]).view(-1, 1, 1)
    yc = (gsy * dets[:, 1]).view(-1, 1, 1)
    dw = dets[:, 2].view(-1, 1, 1); dh = dets[:, 3].view(-1, 1, 1)
    return ((torch.abs(field[a, 0] - xc) < oracle.orien_thresh * dw * gsx.view(-1, 1, 1)) &
            (torch.abs(field[a, 1] - yc) < oracle.orien_thresh * dh * gsy.view(-1, 1, 1)))


# ------------------------------------------------------------------------------------------------------------------------
# mask cases
# ------------------------------------------------------------------------------------------------------------------------
MaskCase = collections.namedtuple("MaskCase", "id size anchor_mask oriens dets fields counts nms_post claims")
# oriens [B, 2 * fields, H/4, W/4] (the heads' orientation maps concatenated); dets [B, nms_post, 5]; fields [B, nms_post] int32;
# counts [B] int32.  Rows at or beyond counts[b] hold NaN boxes and field 0: they must not be read.

GEOMETRIES = [(32, 32), (32, 160), (96, 32), (64, 96), (160, 192)]
ANCHOR_MASKS = [ANCHOR_MASK, [[6, 7, 8], [3, 4, 5], [0, 1]], [[6], [3, 5], [0, 1, 2]]]


def field_table(anchor_mask):
    """field -> (scale, anchor id)."""
    return [(s, a) for s, m in enumerate(anchor_mask) for a in m]


def mask_launch_unchunked(size, batch, nfields):
    """launch_post_mask: one workgroup walks ALL detections of its field when ceil(items / 256) * B * fields >= 2048, where
    items = (H / 4 + 1) * (W / MASK_PX); otherwise the detections of a field are split into chunks of 8."""
    items = (size[0] // 4 + 1) * (size[1] // MASK_PX)
    return (items + 255) // 256 * batch * nfields >= 2048


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _field_normal(rng, batch, nfields, size):
    return (rng.standard_normal((batch, 2 * nfields, size[0] // 4, size[1] // 4)) * 3).astype(F32)


FEW_BIT = [0.8125, -0.4375, 1.25, -1.625, 0.3125, 2.5, -0.75, 0.1875, -2.25, 1.0625, 0.5625, -1.375, 3.0, -0.125, 0.875, -0.6875, 1.75, -3.5]


def _field_const(batch, nfields, size):
    v = np.array(FEW_BIT[:2 * nfields], dtype=F32)
    return np.broadcast_to(v[None, :, None, None], (batch, 2 * nfields, size[0] // 4, size[1] // 4)).copy()


def _blank(batch, nms_post):
    dets = np.full((batch, nms_post, 5), np.nan, dtype=F32)
    return dets, np.zeros((batch, nms_post), dtype=np.int32), np.zeros(batch, dtype=np.int32)


def _random_dets(rng, n, nfields):
    d = np.empty((n, 5), dtype=F32)
    d[:, 0:2] = rng.uniform(-0.1, 1.1, (n, 2))
    d[:, 2:4] = rng.uniform(0.05, 1.5, (n, 2))
    d[:, 4] = rng.uniform(0.01, 1.0, n)
    return d, rng.integers(0, nfields, n).astype(np.int32)


def _case(cid, size, anchor_mask, oriens, dets, fields, counts, nms_post, **claims):
    return MaskCase(cid, size, anchor_mask, torch.from_numpy(np.ascontiguousarray(oriens)), torch.from_numpy(dets),
                    torch.from_numpy(fields), torch.from_numpy(counts), nms_post, claims)


def _pixel_field(size, anchor_mask, oriens_b):
    """Pointed-to grid positions [anchor, 2, H, W] of one image (PostProcessOracle.orien_field)."""
    oracle = make_oracle(size, anchor_mask)
    return oracle, oracle.orien_field(split_oriens(torch.from_numpy(oriens_b[None]), anchor_mask), 0)


def split_oriens(oriens, anchor_mask):
    """[B, 2 * fields, oh, ow] -> the predict structure the oracle reads (bbox heads absent)."""
    out, at = [], 0
    for m in anchor_mask:
        out.append((None, oriens[:, at:at + 2 * len(m)]))
        at += 2 * len(m)
    return out


def _exact_sizes(d, scale, orien_thresh=F32(0.3)):
    """Box sizes bw whose threshold (0.3f * bw) * scale is exactly d, the float below d, the float above d (None where no float32
    box size gives it): tried among the float neighbours of d / (0.3 * scale)."""
    d = F32(d)
    want = [d, np.nextafter(d, F32(-np.inf)), np.nextafter(d, F32(np.inf))]
    b0 = F32(float(d) / (0.3 * float(scale)))
    cand = [b0]
    lo = hi = b0
    for _ in range(6):
        lo = np.nextafter(lo, F32(-np.inf)); hi = np.nextafter(hi, F32(np.inf))
        cand += [lo, hi]
    cand = np.array(cand, dtype=F32)
    t = (orien_thresh * cand) * F32(scale)
    out = []
    for w in want:
        hit = np.flatnonzero(t == w)
        out.append(cand[hit[0]] if hit.size else None)
    return out


def _d1_case(size, anchor_mask=ANCHOR_MASK, nms_post=100):
    """F2 planes (constant, few bits: they interpolate exactly, so P depends on the column -- or row -- alone) and, for chosen
    pixels, box sizes whose threshold equals |P - c| exactly in float32, plus the thresholds one float below and above."""
    nfields = len(field_table(anchor_mask))
    oriens = _field_const(1, nfields, size)
    oracle, P = _pixel_field(size, anchor_mask, oriens[0])
    dets, fields, counts = _blank(1, nms_post)
    k = 0
    kinds = []
    H, W = size
    for f in (nfields - 1, 0, nfields // 2):
        s, aid = field_table(anchor_mask)[f]
        nH, nW = oracle.grids[s]
        cxn, cyn = F32(0.4375), F32(0.5625)
        cx, cy = F32(nW) * cxn, F32(nH) * cyn
        for axis, n, npix in ((0, nW, W), (1, nH, H)):
            line = P[aid, axis, 0, :].numpy() if axis == 0 else P[aid, axis, :, 0].numpy()
            taken = 0
            for px in list(range(1, npix, 5)) + list(range(3, npix, 7)):
                dist = np.abs(line[px] - (cx if axis == 0 else cy))
                sizes = _exact_sizes(dist, n)
                if any(v is None for v in sizes) or dist == 0:
                    continue
                for kind, bw in zip(("eq", "lo", "hi"), sizes):
                    dets[0, k] = (cxn, cyn, bw, F32(8.0), 0.5) if axis == 0 else (cxn, cyn, F32(8.0), bw, 0.5)
                    fields[0, k] = f
                    kinds.append((k, "xy"[axis], kind, px))
                    k += 1
                taken += 1
                if taken == 5:
                    break
    counts[0] = k
    assert k <= nms_post
    return _case("D1_F2_%dx%d" % size, size, anchor_mask, oriens, dets, fields, counts, nms_post, kinds=kinds)


_SPECIAL_SIZES = [0.0, -0.0, -1.0, np.nan, np.inf, 1e-45, 3e-45, 3e38, -np.inf]
_SPECIAL_CENTRES = [np.inf, -np.inf, np.nan, 1.0e6, -5.0, 3e38]


def _d2_case(size, anchor_mask=ANCHOR_MASK, nms_post=100, seed=31):
    rng = _rng(seed)
    nfields = len(field_table(anchor_mask))
    oriens = _field_normal(rng, 1, nfields, size)
    dets, fields, counts = _blank(1, nms_post)
    k = 0
    special = []
    for f in (0, nfields - 1):
        for v in _SPECIAL_SIZES:
            for axis in (2, 3):
                dets[0, k] = (0.5, 0.5, 2.0, 2.0, 0.5)
                dets[0, k, axis] = v
                fields[0, k] = f
                special.append(k)
                k += 1
        for v in _SPECIAL_CENTRES:
            for axis in (0, 1):
                dets[0, k] = (0.5, 0.5, 2.0, 2.0, 0.5)
                dets[0, k, axis] = v
                fields[0, k] = f
                special.append(k)
                k += 1
    for f in range(nfields):                       # an ordinary detection on every field between them
        dets[0, k] = (0.5, 0.5, 0.7, 0.6, 0.5)
        fields[0, k] = f
        k += 1
    counts[0] = k
    assert k <= nms_post
    return _case("D2_special_%dx%d" % size, size, anchor_mask, oriens, dets, fields, counts, nms_post, special=special)


F3_SPOTS = ("row0", "row1", "last_row", "col0", "col1", "last_col", "interior")


def _f3_case(size, anchor_mask=ANCHOR_MASK, seed=41):
    """+inf, -inf and NaN planted one at a time (one image each) in source row 0, row 1, the last row, column 0, column 1, the
    last column and the interior, alternately in the x and the y plane of a field; one box that covers the image per field."""
    rng = _rng(seed)
    nfields = len(field_table(anchor_mask))
    oh, ow = size[0] // 4, size[1] // 4
    values = [np.inf, -np.inf, np.nan]
    batch = len(F3_SPOTS) * len(values)
    oriens = _field_normal(rng, batch, nfields, size) / F32(3)
    dets, fields, counts = _blank(batch, nfields)
    planted = []
    for i in range(batch):
        spot, v = F3_SPOTS[i // len(values)], values[i % len(values)]
        ch = (2 * i + i // nfields) % (2 * nfields)
        y, x = {"row0": (0, ow // 2), "row1": (1, ow // 2 - 1), "last_row": (oh - 1, 2), "col0": (oh // 2, 0), "col1": (oh // 2 - 1, 1),
                "last_col": (2, ow - 1), "interior": (oh // 2, ow // 2)}[spot]
        oriens[i, ch, y, x] = v
        planted.append((i, spot, ch, y, x))
        for f in range(nfields):
            dets[i, f] = (0.5, 0.5, 40.0, 40.0, 0.5)
            fields[i, f] = f
        counts[i] = nfields
    return _case("F3_nonfinite_%dx%d" % size, size, anchor_mask, oriens, dets, fields, counts, nfields, planted=planted)


def _f4_case(size, anchor_mask=ANCHOR_MASK, seed=51):
    rng = _rng(seed)
    nfields = len(field_table(anchor_mask))
    oriens = _field_normal(rng, 2, nfields, size)
    big = rng.random(oriens.shape) < 0.08
    oriens[big] = np.where(rng.random(int(big.sum())) < 0.5, F32(3e38), F32(-3e38))
    den = rng.random(oriens.shape) < 0.15
    oriens[den] = rng.choice(np.array([1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38], dtype=F32), int(den.sum()))
    oriens[1, :, :2] = F32(3e38)             # whole top rows and left columns at the largest magnitudes
    oriens[1, :, :, :2] = F32(-3e38)
    n = 2 * nfields
    dets, fields, counts = _blank(2, n)
    for b in range(2):
        for f in range(nfields):
            dets[b, 2 * f] = (0.5, 0.5, 40.0, 40.0, 0.5)
            dets[b, 2 * f + 1] = (0.45, 0.55, 0.6, 0.5, 0.5)
            fields[b, 2 * f] = fields[b, 2 * f + 1] = f
        counts[b] = n
    return _case("F4_huge_and_denormal_%dx%d" % size, size, anchor_mask, oriens, dets, fields, counts, n)


def _d3_cases(size=(64, 96)):
    out = []
    rng = _rng(61)
    nfields = 9
    oriens = _field_normal(rng, 1, nfields, size)
    dets, fields, counts = _blank(1, 100)
    dets[0], _ = _random_dets(rng, 100, nfields)
    fields[0] = 4
    counts[0] = 100
    out.append(_case("D3_100_on_one_field", size, ANCHOR_MASK, oriens, dets, fields, counts, 100, per_field={4: 100}))
    dets, fields, counts = _blank(1, 100)
    dets[0], _ = _random_dets(rng, 100, nfields)
    slots = rng.permutation(100)
    fields[0, slots[:65]] = 1             # scale 0
    fields[0, slots[65:]] = 8             # scale 2
    counts[0] = 100
    out.append(_case("D3_65_and_35_interleaved", size, ANCHOR_MASK, oriens, dets, fields, counts, 100, per_field={1: 65, 8: 35}))
    oriens = _field_normal(rng, 3, nfields, size)
    dets, fields, counts = _blank(3, 100)
    for b, n in enumerate((0, 100, 37)):
        dets[b, :n], fields[b, :n] = _random_dets(rng, n, nfields)
        counts[b] = n
    out.append(_case("D3_counts_0_100_37", size, ANCHOR_MASK, oriens, dets, fields, counts, 100, per_image=(0, 100, 37)))
    return out


UNCHUNKED = dict(size=(512, 512), batch=14, nms_post=4)


def unchunked_case():
    """The smallest launch that takes the unchunked form: fourteen 512 x 512 images (17 * 14 * 9 = 2142 >= 2048)."""
    size, batch, nms_post = UNCHUNKED["size"], UNCHUNKED["batch"], UNCHUNKED["nms_post"]
    rng = _rng(71)
    oriens = _field_normal(rng, batch, 9, size)
    dets, fields, counts = _blank(batch, nms_post)
    for b in range(batch):
        dets[b], fields[b] = _random_dets(rng, nms_post, 9)
        fields[b, 1] = fields[b, 0]             # two detections on one field
        counts[b] = nms_post if b != 5 else 2
    return _case("unchunked_14x512x512", size, ANCHOR_MASK, oriens, dets, fields, counts, nms_post)


_MASK = {}


def mask_cases():
    """id -> MaskCase (without the 14 x 512 x 512 launch: unchunked_case)."""
    if _MASK:
        return _MASK
    out = []
    rng = _rng(21)
    for size in GEOMETRIES:                                   # F1 x every geometry x every anchor mask, a dozen ordinary boxes
        for mi, am in enumerate(ANCHOR_MASKS):
            nfields = len(field_table(am))
            oriens = _field_normal(rng, 2, nfields, size)
            dets, fields, counts = _blank(2, 16)
            for b, n in enumerate((12, 16)):
                dets[b, :n], fields[b, :n] = _random_dets(rng, n, nfields)
                fields[b, :nfields] = np.arange(nfields)      # every field at least once
                counts[b] = n
            out.append(_case("F1_%dx%d_mask%d" % (size + (mi,)), size, am, oriens, dets, fields, counts, 16))
    out.append(_d1_case((64, 96)))
    out.append(_d1_case((32, 160), ANCHOR_MASKS[1]))
    out.append(_d1_case((96, 128)))
    out.append(_d2_case((64, 96)))
    out.append(_d2_case((32, 32), ANCHOR_MASKS[2]))
    out.append(_f3_case((32, 32)))
    out.append(_f3_case((64, 96), ANCHOR_MASKS[1]))
    out.append(_f4_case((32, 160)))
    out.append(_f4_case((96, 32), ANCHOR_MASKS[2]))
    out += _d3_cases()
    for c in out:
        assert c.id not in _MASK
        _MASK[c.id] = c
    return _MASK


def expected_masks(case, images=None):
    """Per image, bool [counts[b], H, W]: the oracle's own arithmetic (orien_field + the predicate of finish) on the case's
    detections, in float32."""
    oracle = make_oracle(case.size, case.anchor_mask, nms_post=case.nms_post)
    table = field_table(case.anchor_mask)
    predict = split_oriens(case.oriens, case.anchor_mask)
    out = []
    for b in (range(case.oriens.shape[0]) if images is None else images):
        n = int(case.counts[b])
        field = oracle.orien_field(predict, b)
        a = torch.tensor([table[int(f)][1] for f in case.fields[b, :n]], dtype=torch.long)
        out.append(masks_of(oracle, field, case.dets[b, :n], a).numpy() if n else np.zeros((0,) + tuple(case.size), dtype=bool))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the mask arithmetic restated in numpy, with deliberate errors for the teeth of the CPU test
# ------------------------------------------------------------------------------------------------------------------------
MASK_MUTATIONS = ("le", "left_unclamped", "top_unclamped", "neg_abs", "top_row0_twice")


def torch_small_output_form(size):
    """torch's CPU bilinear takes another loop when the OUTPUT's height + width is at most 128 (ATen UpSampleKernel.cpp:
    _use_vectorized_kernel_cond_2d; the orientation heads are NCHW with 2 .. 6 channels, so its other conditions never hold).  That
    loop multiplies the weights first and sums four products, which rounds differently from the two-step form."""
    return size[0] + size[1] <= 128


def fma_f32(a, b, c):
    """fmaf on float32 arrays: ONE rounding of a * b + c.  The product of two float32 is exact in float64; the float64 sum is
    rounded to odd (from its TwoSum error term) before the cast, so that an addend far below the product's last bit -- a
    denormal beside an ordinary value, an ordinary value beside 3e38 -- still breaks a rounding tie the way the hardware does
    (a plain float64 sum loses it and rounds the tie to even)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
        c = np.broadcast_to(np.asarray(c, dtype=np.float64), s.shape)
        r = s + c
        t = r - s
        e = (s - (r - t)) + (c - t)
        fix = np.isfinite(r) & np.isfinite(e) & (e != 0)
        bits = r.view(np.int64) if r.flags.writeable else r.copy().view(np.int64)
        sign = bits & np.int64(-0x8000000000000000)
        mag = bits & np.int64(0x7FFFFFFFFFFFFFFF)
        away = (e > 0) == (r > 0)                          # the exact sum is larger in magnitude than r
        odd = np.where(away, mag, mag - 1) | 1
        out = np.where(fix, (sign | odd).view(np.float64), r)
        return out.astype(F32)


def upsample_x4(plane, mutate=(), small=False):
    """torch's bilinear x4, align_corners=False, bit for bit, in both of its forms:
      small=False  oracle.bilinear_x4_restated: row(y) = fma(v[y][x0], wx0, v[y][x1] * wx1); out = fma(row(y0), wy0, row(y1) * wy1)
      small=True   (output height + width <= 128) w00 = wy0 * wx0, ...; out = fma(v11, w11, fma(v10, w10, fma(v00, w00, v01 * w01)))
    with optional errors:
      "left_unclamped" / "top_unclamped"  the first two columns / rows keep their phase weights 0.625 and 0.875 on the second tap
      "top_row0_twice"                    output rows 0 and 1 read source row 0 for both taps (weight 0 on the second)"""
    p = np.asarray(plane, dtype=F32)
    h, w = p.shape

    def taps(n, unclamped, first_twice):
        d = np.arange(n * 4, dtype=F32)
        raw = (d + F32(0.5)) * F32(0.25) - F32(0.5)
        src = np.maximum(raw, F32(0))
        i0 = np.floor(src).astype(np.int64)
        i1 = np.minimum(i0 + 1, n - 1)
        l1 = (src - i0.astype(F32)).astype(F32)
        if unclamped:
            l1[:2] = raw[:2] - np.floor(raw[:2])
        if first_twice:
            i1[:2] = 0
        return i0, i1, (F32(1) - l1).astype(F32), l1

    fma = fma_f32
    y0, y1, wy0, wy1 = taps(h, "top_unclamped" in mutate, "top_row0_twice" in mutate)
    x0, x1, wx0, wx1 = taps(w, "left_unclamped" in mutate, False)
    shape = (4 * h, 4 * w)
    wx0b = np.broadcast_to(wx0[None, :], shape); wx1b = np.broadcast_to(wx1[None, :], shape)
    wy0b = np.broadcast_to(wy0[:, None], shape); wy1b = np.broadcast_to(wy1[:, None], shape)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if small:
            out = (p[y0][:, x1] * (wy0b * wx1b).astype(F32)).astype(F32)
            out = fma(p[y0][:, x0], (wy0b * wx0b).astype(F32), out)
            out = fma(p[y1][:, x0], (wy1b * wx0b).astype(F32), out)
            return fma(p[y1][:, x1], (wy1b * wx1b).astype(F32), out)
        top = fma(p[y0][:, x0], wx0b, (p[y0][:, x1] * wx1b).astype(F32))
        bot = fma(p[y1][:, x0], wx0b, (p[y1][:, x1] * wx1b).astype(F32))
        return fma(top, wy0b, (bot * wy1b).astype(F32))


def restated_masks(case, mutate=(), images=None):
    """expected_masks in numpy float32 through upsample_x4; mutate also takes "le" (<= for <) and "neg_abs" (a negative
    threshold treated by its magnitude)."""
    oracle = make_oracle(case.size, case.anchor_mask, nms_post=case.nms_post)
    table = field_table(case.anchor_mask)
    ga = oracle.grid_anchors.numpy(); gs = oracle.grid_sizes.numpy(); base = oracle.base_xy.numpy()
    th = F32(oracle.orien_thresh)
    out = []
    for b in (range(case.oriens.shape[0]) if images is None else images):
        n = int(case.counts[b])
        masks = np.zeros((n,) + tuple(case.size), dtype=bool)
        cache = {}
        for k in range(n):
            f = int(case.fields[b, k]); aid = table[f][1]
            if f not in cache:
                with np.errstate(invalid="ignore", over="ignore"):
                    cache[f] = [(upsample_x4(case.oriens[b, 2 * f + c].numpy(), mutate, torch_small_output_form(case.size)) * ga[aid, c]) / F32(2) + base[aid, c] for c in (0, 1)]
            cx, cy, bw, bh = case.dets[b, k, :4].numpy()
            with np.errstate(invalid="ignore", over="ignore"):
                tx, ty = (th * bw) * gs[aid, 0], (th * bh) * gs[aid, 1]
                if "neg_abs" in mutate:
                    tx, ty = np.abs(tx), np.abs(ty)
                dx, dy = np.abs(cache[f][0] - gs[aid, 0] * cx), np.abs(cache[f][1] - gs[aid, 1] * cy)
                masks[k] = ((dx <= tx) & (dy <= ty)) if "le" in mutate else ((dx < tx) & (dy < ty))
        out.append(masks)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# D1 / D2 once more through heads: the fused om_postprocess computes the mask constants in the select kernel's tail
# ------------------------------------------------------------------------------------------------------------------------
FusedCase = collections.namedtuple("FusedCase", "id predict cfg claims")


def sigmoid_strided(x):
    """torch's sigmoid on a strided view (tx, ty and the objectness in decode_scale: the scalar loop)."""
    t = torch.from_numpy(np.asarray(x, dtype=F32))
    with R._single_thread():
        return torch.stack([t, t], 1)[:, 0].sigmoid().numpy().copy()


def _centre_logit(P_px, n, g, t):
    """A logit whose decoded centre c = n * ((sigmoid + g) / n) lies exactly t left of / above the position P_px:
    |P_px - c| == t in float32.  Returns the logits (on equality, of the nearest distance above t: outside, of the nearest below t: inside) or None."""
    sigma0 = float(P_px) - float(t) - g
    if not 0.05 < sigma0 < 0.95:
        return None
    x0 = F32(np.log(sigma0 / (1 - sigma0)))
    xs = (x0.view(np.int32) + np.arange(-2000, 2001, dtype=np.int32)).astype(np.int32).view(F32)        # consecutive floats
    xs = np.sort(xs)
    c = F32(n) * ((sigmoid_strided(xs) + F32(g)) / F32(n))
    d = np.abs(F32(P_px) - c)
    hit = np.flatnonzero(d == F32(t))
    if not hit.size:
        return None
    outside, inside = np.flatnonzero(d > F32(t)), np.flatnonzero(d < F32(t))
    if not outside.size or not inside.size:
        return None
    lo, hi = outside[np.argmin(d[outside])], inside[np.argmax(d[inside])]      # the nearest distances a logit can produce
    return float(xs[hit[0]]), float(xs[lo]), float(xs[hi])


def _const_heads():
    h = Heads()
    oh, ow = SIZE[0] // 4, SIZE[1] // 4
    h.oriens = [torch.from_numpy(np.broadcast_to(np.array(FEW_BIT[6 * s:6 * s + 6], dtype=F32)[None, :, None, None], (1, 6, oh, ow)).copy())
                for s in range(3)]
    return h


_FUSED = {}


def fused_cases():
    if _FUSED:
        return _FUSED
    # D1: tw = th = 0, so exp() = 1 exactly and the box is its anchor: the threshold is fixed and the CENTRE is moved onto it.
    # On the coarsest scale with a 32 x 24 anchor, so that positions, centres and thresholds are all below 0.5 grid cells and
    # the float grids of P - c and of the threshold meet.
    h = _const_heads()
    anchors = [list(a) for a in ANCHORS_YOLOV4]
    for aid in ANCHOR_MASK[0]:
        anchors[aid] = [32, 24]
    oracle = R.PostProcessOracle(grids_of(SIZE), list(SIZE), anchors, ANCHOR_MASK, C, conf_thresh=CONF_THRESH)
    P = oracle.orien_field(h.predict(), 0)
    s = 0
    nH, nW = oracle.grids[s]
    kinds, cls = [], 0
    for a, aid in enumerate(ANCHOR_MASK[s]):       # one x and one y triple per anchor slot: each detection needs a cell of its own
        tx = (F32(0.3) * oracle.norm_anchors[aid, 0].numpy()) * F32(nW)
        ty = (F32(0.3) * oracle.norm_anchors[aid, 1].numpy()) * F32(nH)
        for axis, n, t, line in ((0, nW, tx, P[aid, 0, 0, :].numpy()), (1, nH, ty, P[aid, 1, :, 0].numpy())):
            for px in range(len(line)):
                g = int(np.floor(float(line[px]) - float(t)))
                logits = _centre_logit(line[px], n, g, t) if g == 0 else None
                if logits is None:
                    continue
                for k, (kind, x) in enumerate(zip(("eq", "lo", "hi"), logits)):
                    y_, x_ = (k, 0) if axis == 0 else (0, 1 + k)          # column 0 for the x triple, row 0 for the y triple
                    cand = h.cand_index(s, a, y_, x_)
                    h.set_box(cand, tw=0.0, th=0.0, **{"tx" if axis == 0 else "ty": x})
                    h.plant(cand * C + cls, 2.0 - 0.01 * cls)
                    kinds.append((cand * C + cls, "xy"[axis], kind, px))
                    cls += 1
                break
    assert {k[1] for k in kinds} == {"x", "y"} and len(kinds) >= 9, kinds
    _FUSED["D1_fused"] = FusedCase("D1_fused", h.predict(), dict(nms_pre=400, anchors=anchors), dict(kinds=kinds))
    # D2: box sizes 0 (exp underflows), +inf (overflows), NaN, denormal and huge; a NaN centre
    h = Heads(seed=5)
    special = []
    logits = [("tw", -200.0), ("th", -200.0), ("tw", 100.0), ("th", 100.0), ("tw", np.nan), ("th", np.nan), ("tw", -103.0), ("th", -104.0),
              ("tw", 87.0), ("th", 87.5), ("tx", np.nan), ("ty", np.nan)]
    for k, (name, v) in enumerate(logits):
        sc = (0, 1, 2)[k % 3]
        gh, gw = h.grids[sc]
        cand = h.cand_index(sc, k % 3 if k % 2 else 2, (k * 5) % gh, (k * 3) % gw)
        h.set_box(cand, **{name: v})
        if name in ("tx", "ty"):
            h.set_box(cand, tw=0.0, th=0.0)
        h.plant(cand * C + 3 * k + 1, 2.0 - 0.01 * k)
        special.append((cand * C + 3 * k + 1, name, v))
    for k in range(6):                        # ordinary detections between them
        h.plant(h.cand_index(2, 1, 2 * k, 3 + 2 * k) * C + 40 + k, 1.0 - 0.01 * k)
        h.set_box(h.cand_index(2, 1, 2 * k, 3 + 2 * k), tw=1.0, th=0.5)
    _FUSED["D2_fused"] = FusedCase("D2_fused", h.predict(), dict(nms_pre=400), dict(special=special, total=len(logits) + 6))
    return _FUSED
