"""COCO bbox and segm AP without pycocotools.

Replaces what the reference's ``eval/coco_eval.py:80-105`` (``COCOMetrics.coco_eval``) takes from pycocotools: ``COCO``,
``COCO.loadRes`` and ``COCOeval`` with its default parameters (``useCats=1``, 10 IoU thresholds, 101 recall thresholds,
maxDets [1, 10, 100], area ranges all / small / medium / large), plus the reference's ``_get_per_cats_stats`` and
``Tester.display_coco_eval`` (``trainer/tester.py:64-96``).

Device part (``csrc/cocoeval.hip``): masks are built as column-major bit-packed bitmaps from GT polygons (pycocotools'
``rleFrPoly``), uncompressed RLE (crowd GT) and compressed RLE strings (results); IoUs are popcounts (segm) or ``bbIou``
in float64 (bbox); ``evaluateImg``'s greedy matching runs one wave per (image, category).  Host part (numpy):
``accumulate`` and ``summarize`` in pycocotools' own float64 arithmetic.  Images are evaluated in chunks whose bitmaps and
IoUs stay under ``max_bytes`` (1 GiB by default); the result does not depend on the chunk size.

Parity status: pycocotools is not available here, so nothing has been compared with its output.  The evaluator is pinned by
hand-computed known answers, an independent loop-form restatement of the published algorithms (``tests/cocoeval_np.py``),
a round trip against the pinned mask resize of ``coco_format`` and the reference's own display code
(``tests/golden/cocoeval_display.npz``).  The real pin is the first val2017 run with a checkpoint: the reference reports
bbox AP 0.385 and segm AP 0.345 (``assets/val2017_test_result.log``).

Kept pycocotools behaviours: a GT segmentation that is a list whose first entry has 4 numbers is a list of boxes
(``frPyObjects``); GT ``ignore`` is ``iscrowd`` whatever the json says; a det's area is ``w * h`` when the first result has
a ``bbox`` and the mask area otherwise (``loadRes``); "matched" means "GT id != 0", so a GT with id 0 counts as unmatched.
"""
import itertools
import json
import os

import numpy as np
import torch

from . import lib as _lib
from .segm import COUNTS as _COUNTS, MAX_POLY_VERTICES, POLY as _POLY, STRING as _STRING, sources as _sources  # noqa: F401

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
METRIC_KEYS = ["AP", "AP50", "AP75", "APS", "APM", "APL", "AR1", "AR10", "AR100", "ARS", "ARM", "ARL"]
DEFAULT_MAX_BYTES = 1 << 30


class COCOGroundTruth:
    """The parts of pycocotools' COCO that COCOeval reads: images (id, height, width), sorted image and category ids, and the
    annotations of each (image, category) in json order."""

    def __init__(self, dataset):
        self.dataset = dataset
        self.imgs = {int(im["id"]): im for im in dataset.get("images", [])}
        self.img_ids = sorted(self.imgs)
        self.cat_ids = sorted(int(c["id"]) for c in dataset.get("categories", []))
        self.anns = list(dataset.get("annotations", []))
        self.by_img_cat = {}
        for a in self.anns:
            self.by_img_cat.setdefault((int(a["image_id"]), int(a["category_id"])), []).append(a)

    @classmethod
    def from_file(cls, path):
        with open(path) as f:
            return cls(json.load(f))

    @classmethod
    def from_dict(cls, d):
        return cls(d)


def _load_results(gt, results):
    """COCO.loadRes: ids 1..N in list order; every image id must be a GT image; areas as loadRes sets them."""
    if isinstance(results, (str, os.PathLike)):
        with open(results) as f:
            results = json.load(f)
    if not isinstance(results, list):
        raise TypeError("results must be a list of result dicts or the path of a json file holding one")
    bad = {int(r["image_id"]) for r in results} - set(gt.imgs)
    if bad:
        raise ValueError("Results do not correspond to current coco set: image ids %s are not in the ground truth"
                         % sorted(bad)[:10])
    box_branch = bool(results) and "bbox" in results[0] and results[0]["bbox"] != []
    out = []
    for i, r in enumerate(results):
        d = dict(r)
        d["id"] = i + 1
        d["iscrowd"] = 0
        if box_branch:
            x, y, bw, bh = (float(v) for v in d["bbox"])
            d["area"] = bw * bh
            if "segmentation" not in d:
                d["segmentation"] = [[x, y, x, y + bh, x + bw, y + bh, x + bw, y]]
        elif "segmentation" not in d:
            raise ValueError("result %d has neither a bbox nor a segmentation" % i)
        out.append(d)
    return out, box_branch


class COCOEvaluator:
    """COCOeval(gt, loadRes(results), iou_type) with the default Params: evaluate(), accumulate(), summarize(), .stats and
    .eval ('precision' [T,R,K,A,M], 'recall' [T,K,A,M], 'scores' [T,R,K,A,M], -1 where undefined)."""

    def __init__(self, gt, results, iou_type="segm", device=None, max_bytes=DEFAULT_MAX_BYTES):
        if iou_type not in ("bbox", "segm"):
            raise ValueError("iou_type must be 'bbox' or 'segm', got %r" % (iou_type,))
        self.gt = gt if isinstance(gt, COCOGroundTruth) else (
            COCOGroundTruth.from_file(gt) if isinstance(gt, (str, os.PathLike)) else COCOGroundTruth.from_dict(gt))
        self.iou_type = iou_type
        self.dts, self._box_branch = _load_results(self.gt, results)
        if iou_type == "bbox" and not self._box_branch and self.dts:
            raise ValueError("bbox evaluation of results without boxes (maskUtils.toBbox) is not supported")
        self.device = torch.device(device) if device is not None else None        # None: the current device, at evaluate()
        self.max_bytes = int(max_bytes)
        self.iouThrs, self.recThrs, self.maxDets, self.areaRng = IOU_THRS, REC_THRS, list(MAX_DETS), AREA_RNG
        self.eval = {}
        self.stats = np.zeros((12,))
        self.ious = {}
        self.timings = {}
        self._src_cache = {}

    # ------------------------------------------------------------------------------------------------------------ evaluate
    def _groups(self):
        """(cat, img) groups in accumulate's order (category, then image id) with their GTs and score-ordered, cut dets."""
        gt = self.gt
        cat_set = set(gt.cat_ids)
        dts = {}
        for d in self.dts:
            c = int(d["category_id"])
            if c in cat_set:
                dts.setdefault((int(d["image_id"]), c), []).append(d)
        groups = []
        for c in gt.cat_ids:
            for i in gt.img_ids:
                g = gt.by_img_cat.get((i, c), [])
                d = dts.get((i, c), [])
                if not g and not d:
                    continue
                order = np.argsort([-float(x["score"]) for x in d], kind="mergesort")
                d = [d[j] for j in order[:self.maxDets[-1]]]
                groups.append((c, i, g, d))
        return groups

    def evaluate(self):
        L = _lib.load()
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        groups = self._groups()
        self._groups_list = groups
        n_dt = sum(len(g[3]) for g in groups)
        n_gt = sum(len(g[2]) for g in groups)
        T, A = len(self.iouThrs), len(self.areaRng)
        self._dt_match = np.zeros((A, T, n_dt), dtype=np.int64)
        self._dt_ignore = np.zeros((A, T, n_dt), dtype=bool)
        dt_first = np.zeros(len(groups) + 1, dtype=np.int64)
        gt_first = np.zeros(len(groups) + 1, dtype=np.int64)
        for k, g in enumerate(groups):
            dt_first[k + 1] = dt_first[k] + len(g[3])
            gt_first[k + 1] = gt_first[k] + len(g[2])
        self._dt_first, self._gt_first = dt_first, gt_first
        self._dt_area = np.zeros(n_dt, dtype=np.float64)
        # chunks of images; a group belongs to its image's chunk
        img_pos = {i: n for n, i in enumerate(self.gt.img_ids)}
        by_img = {}
        for k, g in enumerate(groups):
            by_img.setdefault(g[1], []).append(k)
        imgs = sorted(by_img, key=lambda i: img_pos[i])
        chunk, cost = [], 0
        for i in imgs:
            c = self._image_cost(L, [groups[k] for k in by_img[i]])
            if chunk and cost + c > self.max_bytes:
                self._evaluate_chunk(L, [k for j in chunk for k in by_img[j]])
                chunk, cost = [], 0
            chunk.append(i)
            cost += c
        if chunk:
            self._evaluate_chunk(L, [k for j in chunk for k in by_img[j]])

    def _image_cost(self, L, groups):
        pairs = sum(len(g[2]) * len(g[3]) for g in groups)
        cost = pairs * 17                                   # pair indices, crowd flag, IoU
        if self.iou_type == "segm":
            words, masks = 0, 0
            for _, i, g, d in groups:
                im = self.gt.imgs[i]
                for a in list(g) + list(d):
                    h, w, srcs = self._ann_sources(a, im)
                    n = 1 + (len(srcs) if len(srcs) > 1 else 0)
                    words += n * w * ((h + 31) // 32)
                    masks += 1
            cost += int(L.om_cocoeval_workspace_bytes(words, masks))
        return cost

    def _ann_sources(self, a, im):
        key = id(a)                             # the dicts are the caller's: cache beside them, never in them
        if key not in self._src_cache:
            self._src_cache[key] = _sources(a["segmentation"], int(im["height"]), int(im["width"]))
        return self._src_cache[key]

    def _evaluate_chunk(self, L, gidx):
        groups = self._groups_list
        dev = self.device
        st = _lib.current_stream_ptr(dev)
        T, A = len(self.iouThrs), len(self.areaRng)
        # local det / gt numbering of the chunk
        dts = [d for k in gidx for d in groups[k][3]]
        gts = [g for k in gidx for g in groups[k][2]]
        nd, ng = len(dts), len(gts)
        l_dt_first = np.zeros(len(gidx) + 1, dtype=np.int32)
        l_gt_first = np.zeros(len(gidx) + 1, dtype=np.int32)
        iou_off = np.zeros(len(gidx), dtype=np.int64)
        pairs, crowd = [], []
        n_pairs = 0
        for j, k in enumerate(gidx):
            D, G = len(groups[k][3]), len(groups[k][2])
            l_dt_first[j + 1] = l_dt_first[j] + D
            l_gt_first[j + 1] = l_gt_first[j] + G
            iou_off[j] = n_pairs
            if D and G:
                dd, gg = np.meshgrid(np.arange(D, dtype=np.int32) + l_dt_first[j], np.arange(G, dtype=np.int32) + l_gt_first[j],
                                     indexing="ij")
                pairs.append(np.stack([dd.ravel(), gg.ravel()], 1))
                cr = np.array([int(g.get("iscrowd", 0)) for g in groups[k][2]], dtype=np.uint8)
                crowd.append(np.tile(cr, D))
                n_pairs += D * G
        pairs = np.concatenate(pairs).astype(np.int32) if pairs else np.zeros((0, 2), np.int32)
        crowd = np.concatenate(crowd) if crowd else np.zeros(0, np.uint8)
        tt = lambda a, dtype=None: torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(dev)
        ptr = _or_null
        ious = torch.zeros(max(n_pairs, 1), dtype=torch.float64, device=dev)
        d_pairs, d_crowd = tt(pairs), tt(crowd)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        with _lib.on_device(dev):
            ev[0].record()
            if self.iou_type == "segm":
                mask_stats = self._build_masks(L, gts + dts, st)     # gts are masks [0, ng), dets [ng, ng + nd)
                ev[1].record()
                if n_pairs:
                    pr = pairs.copy()
                    pr[:, 0] += ng
                    pr_t = tt(pr)
                    _lib.launch("om_cocoeval_mask_iou", dev, n_pairs, ptr(pr_t), ptr(d_crowd), ng + nd, ptr(self._m_hw), ptr(self._m_off),
                                self._m_words, self._ws.data_ptr(), ptr(ious), stream=st)
                dt_area = mask_stats[ng:, 0].astype(np.float64) if not self._box_branch else \
                    np.array([float(d["area"]) for d in dts], dtype=np.float64)
            else:
                ev[1].record()
                dbox = tt(np.array([[float(v) for v in d["bbox"]] for d in dts], dtype=np.float64).reshape(-1, 4))
                gbox = tt(np.array([[float(v) for v in g["bbox"]] for g in gts], dtype=np.float64).reshape(-1, 4))
                if n_pairs:
                    _lib.launch("om_cocoeval_bbox_iou", dev, n_pairs, ptr(d_pairs), ptr(d_crowd), ptr(dbox), ptr(gbox), ptr(ious), stream=st)
                dt_area = np.array([float(d["area"]) for d in dts], dtype=np.float64)
            ev[2].record()
            lanes = T * A
            dtm = torch.zeros((lanes, max(nd, 1)), dtype=torch.int64, device=dev)
            dti = torch.zeros((lanes, max(nd, 1)), dtype=torch.uint8, device=dev)
            gtm = torch.zeros((lanes, max(ng, 1)), dtype=torch.uint8, device=dev)
            d_area = tt(dt_area)
            g_area = tt(np.array([float(g["area"]) for g in gts], dtype=np.float64))
            g_crowd = tt(np.array([int(g.get("iscrowd", 0)) for g in gts], dtype=np.uint8))
            g_id = tt(np.array([int(g["id"]) for g in gts], dtype=np.int64))
            rng = tt(np.array(self.areaRng, dtype=np.float64))
            thr = tt(np.asarray(self.iouThrs, dtype=np.float64))
            d_dtf, d_gtf, d_off = tt(l_dt_first), tt(l_gt_first), tt(iou_off)
            _lib.launch("om_cocoeval_match", dev, len(gidx), ptr(d_dtf), ptr(d_gtf), ptr(d_off), ptr(ious), ptr(d_area), ptr(g_area),
                        ptr(g_crowd), ptr(g_id), ptr(rng), ptr(thr), nd, ng, ptr(gtm), ptr(dtm), ptr(dti), stream=st)
            ev[3].record()
            h_dtm, h_dti = dtm.cpu().numpy(), dti.cpu().numpy().astype(bool)
            h_iou = ious.cpu().numpy()
        for a, b, name in ((0, 1, "masks"), (1, 2, "iou"), (2, 3, "match")):
            self.timings[name] = self.timings.get(name, 0.0) + ev[a].elapsed_time(ev[b])
        # scatter back into the global (category, image)-ordered arrays; lane = t + 10 a
        pos = np.concatenate([np.arange(self._dt_first[k], self._dt_first[k + 1]) for k in gidx]) if nd else np.zeros(0, np.int64)
        if nd:
            self._dt_match[:, :, pos] = h_dtm[:, :nd].reshape(A, T, nd)
            self._dt_ignore[:, :, pos] = h_dti[:, :nd].reshape(A, T, nd)
            self._dt_area[pos] = dt_area
        for j, k in enumerate(gidx):
            c, i = groups[k][0], groups[k][1]
            D, G = l_dt_first[j + 1] - l_dt_first[j], l_gt_first[j + 1] - l_gt_first[j]
            self.ious[(i, c)] = h_iou[iou_off[j]:iou_off[j] + D * G].reshape(D, G) if D and G else np.zeros((0, 0))

    def _build_masks(self, L, anns, st):
        """Bitmaps of the chunk's annotations (GT json segmentations / result RLEs) in one workspace; returns [n, 3] int32
        area, first and last nonempty column."""
        dev = self.device
        n = len(anns)
        hw = np.zeros((n, 2), dtype=np.int32)
        m_off = np.zeros(n, dtype=np.int64)
        src_first = np.zeros(n + 1, dtype=np.int32)
        polys, seqs = [], []                    # (mask, data, own bitmap offset)
        words = 0
        img_of = self.gt.imgs
        for m, a in enumerate(anns):
            h, w, srcs = self._ann_sources(a, img_of[int(a["image_id"])])
            if h <= 0 or w <= 0:
                raise ValueError("annotation %s: empty mask size %dx%d" % (a.get("id"), h, w))
            hw[m] = (h, w)
            nw = w * ((h + 31) // 32)
            m_off[m] = words
            words += nw
            for kind, data in srcs:
                off = m_off[m]
                if len(srcs) > 1:
                    off = words
                    words += nw
                (polys if kind == _POLY else seqs).append((m, kind, data, off))
            src_first[m + 1] = src_first[m] + len(srcs)
        srcs_all = polys + seqs                 # the kernel wants the polygons at [0, n_poly)
        order = sorted(range(len(srcs_all)), key=lambda s: srcs_all[s][0])     # stable: each mask's sources, in json order
        n_poly = len(polys)
        kind = np.array([s[1] for s in srcs_all], dtype=np.int32)
        smask = np.array([s[0] for s in srcs_all], dtype=np.int32)
        slen = np.zeros(len(srcs_all), dtype=np.int32)
        sdoff = np.zeros(len(srcs_all), dtype=np.int64)
        swoff = np.array([s[3] for s in srcs_all], dtype=np.int64)
        pdata, cdata, sdata = [], [], []
        np_off = nc_off = ns_off = 0
        for s, (m, k, data, _) in enumerate(srcs_all):
            if k == _POLY:
                slen[s], sdoff[s] = data.size, np_off
                pdata.append(data); np_off += data.size
            elif k == _COUNTS:
                slen[s], sdoff[s] = data.size, nc_off
                cdata.append(data); nc_off += data.size
            else:
                slen[s], sdoff[s] = len(data), ns_off
                sdata.append(data); ns_off += len(data)
        merge_woff = swoff[order]
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ptr = _or_null
        d_hw, d_moff, d_sf = tt(hw), tt(m_off), tt(src_first)
        d_kind, d_smask, d_slen, d_sdoff, d_swoff = tt(kind), tt(smask), tt(slen), tt(sdoff), tt(swoff)
        d_merge = tt(merge_woff)
        d_poly = tt(np.concatenate(pdata)) if pdata else None
        d_cnt = tt(np.concatenate(cdata)) if cdata else None
        d_str = tt(np.frombuffer(b"".join(sdata), dtype=np.uint8).copy()) if sdata else None
        need = int(L.om_cocoeval_workspace_bytes(words, n))
        ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = (ws.data_ptr() + 255) // 256 * 256
        _lib.launch("om_cocoeval_masks", dev, n, ptr(d_hw), ptr(d_moff), ptr(d_sf), ptr(d_merge), n_poly, len(srcs_all), ptr(d_kind),
                    ptr(d_smask), ptr(d_sdoff), ptr(d_slen), ptr(d_swoff), ptr(d_poly), ptr(d_cnt), ptr(d_str), words, base, need, stream=st)
        stats = torch.empty((n, 3), dtype=torch.int32, device=dev)
        _lib.launch("om_cocoeval_mask_stats", dev, n, words, base, ptr(stats), stream=st)
        self._ws_keep = ws
        self._ws = _Ptr(base)
        self._m_hw, self._m_off, self._m_words = d_hw, d_moff, words
        self._keep = (d_kind, d_smask, d_slen, d_sdoff, d_swoff, d_merge, d_poly, d_cnt, d_str, d_sf)
        return stats.cpu().numpy()

    # ---------------------------------------------------------------------------------------------------------- accumulate
    def accumulate(self):
        groups = self._groups_list
        K = len(self.gt.cat_ids)
        A = len(self.areaRng)
        cat_pos = {c: k for k, c in enumerate(self.gt.cat_ids)}
        grp_cat = np.array([cat_pos[g[0]] for g in groups], dtype=np.int64)
        n_dt = int(self._dt_first[-1])
        dt_grp = np.repeat(np.arange(len(groups)), np.diff(self._dt_first))
        dt_rank = np.arange(n_dt) - self._dt_first[dt_grp] if n_dt else np.zeros(0, np.int64)
        dt_score = np.array([float(d["score"]) for g in groups for d in g[3]], dtype=np.float64)
        gt_grp = np.repeat(np.arange(len(groups)), np.diff(self._gt_first))
        gts = [g for grp in groups for g in grp[2]]
        crowd = np.array([bool(g.get("iscrowd", 0)) for g in gts], dtype=bool)
        area = np.array([float(g["area"]) for g in gts], dtype=np.float64)
        gt_ignore = np.stack([crowd | (area < lo) | (area > hi) for lo, hi in self.areaRng]) if gts else np.zeros((A, 0), bool)
        self.eval = accumulate_records(K, grp_cat, grp_cat[dt_grp] if n_dt else np.zeros(0, np.int64), dt_rank, dt_score,
                                       self._dt_match != 0, self._dt_ignore, grp_cat[gt_grp] if gts else np.zeros(0, np.int64),
                                       gt_ignore, self.iouThrs, self.recThrs, self.maxDets)
        return self.eval

    def summarize(self, verbose=True):
        self.stats = summarize(self.eval, self.iouThrs, self.maxDets, verbose=verbose)
        return self.stats


class _Ptr:
    """A raw device address (the workspace is over-allocated and aligned to 256 bytes)."""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr

    def numel(self):
        return 1


def _or_null(t):
    """The launch argument of a table that may be absent or empty: the tensor, or None (a null pointer) when it has no elements."""
    return t if t is not None and t.numel() else None


def accumulate_records(K, grp_cat, dt_cat, dt_rank, dt_score, dt_matched, dt_ignore, gt_cat, gt_ignore, iou_thrs, rec_thrs,
                       max_dets):
    """COCOeval.accumulate on per-det / per-gt records in (category, image id, score rank) order.
    dt_matched, dt_ignore: [A, T, n_dt] bool; gt_ignore: [A, n_gt] bool; categories are indices 0..K-1; grp_cat lists the
    category of every evaluated (image, category) group (a category without any stays -1)."""
    T, R, A, M = len(iou_thrs), len(rec_thrs), gt_ignore.shape[0], len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    has = np.zeros(K, dtype=bool)
    has[np.asarray(grp_cat, dtype=np.int64)] = True
    dt_cat = np.asarray(dt_cat)
    gt_cat = np.asarray(gt_cat)
    for k in range(K):
        if not has[k]:
            continue
        dsel = np.nonzero(dt_cat == k)[0]
        gsel = np.nonzero(gt_cat == k)[0]
        for a in range(A):
            npig = np.count_nonzero(gt_ignore[a, gsel] == 0)
            if npig == 0:
                continue
            for m, maxDet in enumerate(max_dets):
                idx = dsel[dt_rank[dsel] < maxDet]
                sc = dt_score[idx]
                inds = np.argsort(-sc, kind="mergesort")
                sc_sorted = sc[inds]
                dtm = dt_matched[a][:, idx[inds]]
                dtIg = dt_ignore[a][:, idx[inds]]
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                nd = tp_sum.shape[1]
                rc = tp_sum / npig
                pr = tp_sum / (fp_sum + tp_sum + np.spacing(1))
                recall[:, k, a, m] = rc[:, -1] if nd else 0
                if nd:
                    pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                for t in range(T):
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    pi = np.searchsorted(rc[t], rec_thrs, side="left")
                    ok = pi < nd
                    q[ok] = pr[t, pi[ok]]
                    ss[ok] = sc_sorted[pi[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return {"counts": [T, R, K, A, M], "precision": precision, "recall": recall, "scores": scores}


def summarize(ev, iou_thrs=IOU_THRS, max_dets=MAX_DETS, verbose=True):
    """COCOeval.summarize (_summarizeDets): the 12 stats, each np.mean over the defined (> -1) entries; prints its lines."""
    def one(ap=1, iouThr=None, areaRng="all", maxDets=100):
        iStr = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
        titleStr = "Average Precision" if ap == 1 else "Average Recall"
        typeStr = "(AP)" if ap == 1 else "(AR)"
        iouStr = "{:0.2f}:{:0.2f}".format(iou_thrs[0], iou_thrs[-1]) if iouThr is None else "{:0.2f}".format(iouThr)
        aind = [i for i, aRng in enumerate(AREA_LBL) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(max_dets) if mDet == maxDets]
        if ap == 1:
            s = ev["precision"]
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = ev["recall"]
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        if verbose:
            print(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
        return mean_s

    stats = np.zeros((12,))
    stats[0] = one(1)
    stats[1] = one(1, iouThr=.5, maxDets=max_dets[2])
    stats[2] = one(1, iouThr=.75, maxDets=max_dets[2])
    stats[3] = one(1, areaRng="small", maxDets=max_dets[2])
    stats[4] = one(1, areaRng="medium", maxDets=max_dets[2])
    stats[5] = one(1, areaRng="large", maxDets=max_dets[2])
    stats[6] = one(0, maxDets=max_dets[0])
    stats[7] = one(0, maxDets=max_dets[1])
    stats[8] = one(0, maxDets=max_dets[2])
    stats[9] = one(0, areaRng="small", maxDets=max_dets[2])
    stats[10] = one(0, areaRng="medium", maxDets=max_dets[2])
    stats[11] = one(0, areaRng="large", maxDets=max_dets[2])
    return stats


def per_cats_stats(precisions, n_cats):
    """The reference's COCOMetrics._get_per_cats_stats (eval/coco_eval.py:207-217): AP x 100 per category at area 'all',
    maxDets 100; nan for a category without any defined precision."""
    assert n_cats == precisions.shape[2]
    out = []
    for idx in range(n_cats):
        precision = precisions[:, :, idx, 0, -1]
        precision = precision[precision > -1]
        ap = np.mean(precision) if precision.size else float("nan")
        out.append(float(ap * 100))
    return out


class COCOMetrics:
    """The reference's eval/coco_eval.py COCOMetrics with this package's evaluator and COCOFormatter: same methods,
    attributes, prediction files and coco_eval_log."""

    def __init__(self, gt_file, cat2label, with_mask, save_dir, device=None, max_bytes=DEFAULT_MAX_BYTES):
        self.gt_file = gt_file
        self.cat2label = torch.tensor(cat2label)
        self.with_mask = with_mask
        self.bbox_results = []
        self.segm_results = []
        self.bbox_eval_stats = []
        self.segm_eval_stats = []
        self.bbox_eval_per_cats_stats = []
        self.segm_eval_per_cats_stats = []
        self.bbox_pred_file = os.path.join(save_dir, "bbox_prediction.json")
        self.segm_pred_file = os.path.join(save_dir, "segm_prediction.json")
        self.metric_keys = list(METRIC_KEYS)
        self.device = device
        self.max_bytes = max_bytes
        self._formatter = None

    def reset(self):
        self.bbox_results = []
        self.segm_results = []
        self.bbox_eval_stats = []
        self.segm_eval_stats = []
        self.bbox_eval_per_cats_stats = []
        self.segm_eval_per_cats_stats = []

    def to_coco_format(self, image_info, detections):
        if self._formatter is None:
            from .coco_format import COCOFormatter
            self._formatter = COCOFormatter(self.cat2label.tolist(), with_mask=self.with_mask)
        return self._formatter.to_coco_format(image_info, detections)

    def update_results(self, coco_format):
        self.bbox_results += coco_format["bbox"]
        if self.with_mask:
            self.segm_results += coco_format["segm"]

    def save_as_json(self, filename):
        with open(filename, "w") as handle:
            json.dump({"bbox": self.bbox_results, "segm": self.segm_results}, handle)

    def update_from_json(self, filename):
        update = json.load(open(filename))
        self.bbox_results += update["bbox"]
        self.segm_results += update["segm"]

    def coco_eval(self, per_cats=False):
        coco_eval_log = {}
        gt = COCOGroundTruth.from_file(self.gt_file)
        for kind, results, path in (("bbox", self.bbox_results, self.bbox_pred_file),
                                    ("segm", self.segm_results, self.segm_pred_file)):
            if kind == "segm" and not self.with_mask:
                break
            with open(path, "w") as handle:
                json.dump(results, handle)
            ev = COCOEvaluator(gt, path, kind, device=self.device, max_bytes=self.max_bytes)
            ev.evaluate()
            ev.accumulate()
            ev.summarize(verbose=False)
            setattr(self, "%s_eval_stats" % kind, ev.stats)
            if per_cats:
                setattr(self, "%s_eval_per_cats_stats" % kind, self._get_per_cats_stats(ev))
            for key, value in zip(self.metric_keys, ev.stats.tolist()):
                coco_eval_log["{}_{}".format(kind, key)] = value
        return coco_eval_log

    def _get_per_cats_stats(self, coco_eval_obj):
        return per_cats_stats(coco_eval_obj.eval["precision"], self.cat2label.numel())


def display_coco_eval(metrics, eval_type="bbox", classes=None):
    """The reference's Tester.display_coco_eval (trainer/tester.py:64-96): the 12 stats and the per-category AP as two
    tabulate pipe tables.  classes defaults to the COCO class names."""
    from tabulate import tabulate
    if classes is None:
        from .visualizer import CLASSES
        classes = CLASSES["COCO"]
    if eval_type == "bbox":
        eval_stats = metrics.bbox_eval_stats
        eval_per_cats_stats = metrics.bbox_eval_per_cats_stats
    elif eval_type == "segm":
        eval_stats = metrics.segm_eval_stats
        eval_per_cats_stats = metrics.segm_eval_per_cats_stats
    else:
        raise KeyError
    table = tabulate(
        np.asarray(eval_stats).reshape(1, -1),
        tablefmt="pipe",
        floatfmt=".3f",
        headers=METRIC_KEYS,
        numalign="left",
    )
    print("\nCOCO eval {}: \n".format(eval_type) + table)
    eval_per_cats_stats = [(cat, stat) for cat, stat in zip(classes, eval_per_cats_stats)]
    N_COLS = min(6, len(eval_per_cats_stats) * 2)
    results_flatten = list(itertools.chain(*eval_per_cats_stats))
    results_2d = itertools.zip_longest(*[results_flatten[i::N_COLS] for i in range(N_COLS)])
    table = tabulate(
        results_2d,
        tablefmt="pipe",
        floatfmt=".3f",
        headers=["category", "AP"] * (N_COLS // 2),
        numalign="left",
    )
    print("\nPer-category {} AP: \n".format(eval_type) + table)
