"""Plain-Python restatement of the pycocotools pieces orienmask_amd/cocoeval.py replaces, written loop for loop from the
published sources (maskApi.c: rleFrPoly, rleFrBbox, bbIou, rleIou; cocoeval.py: evaluate, computeIoU, evaluateImg,
accumulate, summarize).  Shares no code with the product.  Not a test module (no test_ prefix): a helper for
tests/test_cocoeval.py.  Compressed RLE strings are decoded with the C restatement of rleFrString in oracle/rle_ref.c."""
import json
import math

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def _c_int(v):
    """C's (int) cast of a double: truncation toward zero.  NaN (a zero-length edge, where rleFrPoly divides 0 / 0) is
    undefined in C; x86 gives INT_MIN.  That point's v only enters the mask through min(v, v_prev) and the clamp of y at 0,
    so every value <= 0 gives the same mask."""
    if math.isnan(v):
        return -2 ** 31
    return int(math.trunc(v))


def rle_fr_poly(xy, h, w, trace=None):
    """maskApi.c rleFrPoly -> run lengths.  trace: a dict that receives the upsampled points u, v and the kept boundary points
    x, y (for tests that must know what a polygon exercised); it changes nothing."""
    k = len(xy) // 2
    scale = 5.0
    x = [_c_int(scale * xy[j * 2 + 0] + .5) for j in range(k)] + [0]
    y = [_c_int(scale * xy[j * 2 + 1] + .5) for j in range(k)] + [0]
    x[k] = x[0]
    y[k] = y[0]
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else float('nan')
        else:
            s = (xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(_c_int(ys + s * t + .5))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(_c_int(xs + s * t + .5))
    xs_, ys_ = [], []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / scale - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / scale - .5
            if yd < 0:
                yd = 0
            elif yd > h:
                yd = h
            yd = math.ceil(yd)
            xs_.append(int(xd))
            ys_.append(int(yd))
    if trace is not None:
        trace.update(u=u, v=v, x=xs_, y=ys_)
    a = [xs_[j] * h + ys_[j] for j in range(len(xs_))]
    a.append(h * w)
    a.sort()
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    b = [a[0]]
    j = 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return b


def counts_to_mask(counts, h, w):
    flat = np.zeros(h * w, dtype=np.uint8)
    p, val = 0, 0
    for c in counts:
        flat[p:p + c] = val
        p += c
        val = 1 - val
    return flat.reshape(w, h).T.copy()


def rle_fr_string(s):
    """maskApi.c rleFrString -> counts (uint32, as C keeps them), in plain Python.  Where the string ends in the middle of a
    count the C code reads past the terminator (undefined); here the count keeps the bits read so far, without a sign
    extension, which is the one defined reading of "the input ends"."""
    if isinstance(s, str):
        s = s.encode('ascii')
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, 1
        while more and p < len(s):
            c = s[p] - 48
            x |= (c & 0x1f) << 5 * k
            more = c & 0x20
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << 5 * k
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & 0xffffffff)
    return cnts


def ann_mask(segm, h, w, strict=True):
    """annToRLE + decode: polygons (or the 4-number box quirk) merged by OR, uncompressed and compressed RLE.
    strict=False decodes a string with rle_fr_string above and lets the counts stop short of or overrun h * w (the runs past
    the last pixel are dropped), for the malformed sources of tests/cocoeval_cases.py."""
    if isinstance(segm, list):
        m = np.zeros((h, w), dtype=np.uint8)
        for p in segm:
            if len(segm[0]) == 4:
                xs, ys = float(p[0]), float(p[1])
                xe, ye = xs + float(p[2]), ys + float(p[3])
                p = [xs, ys, xs, ye, xe, ye, xe, ys]
            m |= counts_to_mask(rle_fr_poly([float(v) for v in p], h, w), h, w)
        return m
    rh, rw = segm['size']
    if isinstance(segm['counts'], list):
        return counts_to_mask(segm['counts'], rh, rw)
    if not strict:
        return counts_to_mask(rle_fr_string(segm['counts']), rh, rw)
    from oracle.orienmask_ref import rle_string_decode
    return counts_to_mask(rle_string_decode(segm['counts'], rh * rw), rh, rw)


def bb_iou(dt, gt, iscrowd):
    o = np.zeros((len(dt), len(gt)))
    for g in range(len(gt)):
        G = gt[g]
        ga = G[2] * G[3]
        for d in range(len(dt)):
            D = dt[d]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            hh = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if hh <= 0:
                continue
            i = w * hh
            u = da if iscrowd[g] else da + ga - i
            o[d, g] = i / u
    return o


def mask_iou(dt, gt, iscrowd):
    o = np.zeros((len(dt), len(gt)))
    for d in range(len(dt)):
        for g in range(len(gt)):
            if dt[d].shape != gt[g].shape:
                o[d, g] = -1
                continue
            i = int(np.count_nonzero(dt[d] & gt[g]))
            u = int(np.count_nonzero(dt[d] | gt[g]))
            if i == 0:
                u = 1
            elif iscrowd[g]:
                u = int(np.count_nonzero(dt[d]))
            o[d, g] = i / u
    return o


class Eval:
    """COCOeval with default Params, useCats = 1."""

    def __init__(self, gt_dict, results, iou_type):
        if isinstance(results, str):
            results = json.load(open(results))
        self.gt = gt_dict
        self.iou_type = iou_type
        self.imgs = {im['id']: im for im in gt_dict['images']}
        self.img_ids = sorted(self.imgs)
        self.cat_ids = sorted(c['id'] for c in gt_dict['categories'])
        dts = [dict(r) for r in results]
        for i, d in enumerate(dts):
            assert d['image_id'] in self.imgs
            d['id'] = i + 1
            d['iscrowd'] = 0
        if dts and 'bbox' in dts[0] and dts[0]['bbox'] != []:
            for d in dts:
                bb = d['bbox']
                d['area'] = bb[2] * bb[3]
                if 'segmentation' not in d:
                    x1, x2, y1, y2 = [bb[0], bb[0] + bb[2], bb[1], bb[1] + bb[3]]
                    d['segmentation'] = [[x1, y1, x1, y2, x2, y2, x2, y1]]
        else:
            for d in dts:
                d['area'] = None
        self.dts = dts

    def _mask(self, ann):
        im = self.imgs[ann['image_id']]
        return ann_mask(ann['segmentation'], im['height'], im['width'])

    def evaluate(self):
        gts = [a for i in self.img_ids for a in self.gt['annotations'] if a['image_id'] == i and a['category_id'] in self.cat_ids]
        dts = [d for i in self.img_ids for d in self.dts if d['image_id'] == i and d['category_id'] in self.cat_ids]
        self._gts, self._dts = {}, {}
        for g in gts:
            g = dict(g)
            g['ignore'] = 'iscrowd' in g and g['iscrowd']
            self._gts.setdefault((g['image_id'], g['category_id']), []).append(g)
        for d in dts:
            if self.iou_type == 'segm':
                d['_mask'] = self._mask(d)
                if d['area'] is None:
                    d['area'] = int(d['_mask'].sum())
            self._dts.setdefault((d['image_id'], d['category_id']), []).append(d)
        if self.iou_type == 'segm':
            for lst in self._gts.values():
                for g in lst:
                    g['_mask'] = self._mask(g)
        self.ious = {(i, c): self.compute_iou(i, c) for i in self.img_ids for c in self.cat_ids}
        self.evalImgs = [self.evaluate_img(i, c, a, MAX_DETS[-1]) for c in self.cat_ids for a in AREA_RNG for i in self.img_ids]

    def compute_iou(self, i, c):
        gt = self._gts.get((i, c), [])
        dt = self._dts.get((i, c), [])
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[j] for j in inds][:MAX_DETS[-1]]
        if len(gt) == 0 or len(dt) == 0:
            return []
        iscrowd = [int(o.get('iscrowd', 0)) for o in gt]
        if self.iou_type == 'segm':
            return mask_iou([d['_mask'] for d in dt], [g['_mask'] for g in gt], iscrowd)
        return bb_iou([d['bbox'] for d in dt], [g['bbox'] for g in gt], iscrowd)

    def evaluate_img(self, i, c, aRng, maxDet):
        gt = self._gts.get((i, c), [])
        dt = self._dts.get((i, c), [])
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g['_ignore'] = 1 if (g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1])) else 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[j] for j in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[j] for j in dtind[0:maxDet]]
        iscrowd = [int(o.get('iscrowd', 0)) for o in gt]
        ious = self.ious[i, c][:, gtind] if len(self.ious[i, c]) > 0 else self.ious[i, c]
        T, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'dtMatches': dtm, 'gtMatches': gtm, 'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg}

    @classmethod
    def match_direct(cls, gts, dts, ious):
        """evaluate_img on one (image, category) group given directly: gts (dicts with id, area, iscrowd, in json order), dts
        (dicts with id, area, score, already in descending score order and cut to maxDets[-1]) and their [D, G] IoU matrix.
        Returns one evaluate_img record per area range, with gtMatches and gtIgnore put back into the json order of gts."""
        e = cls.__new__(cls)
        key = (0, 0)
        e._gts = {key: [dict(g, ignore=g.get('iscrowd', 0)) for g in gts]} if gts else {}
        e._dts = {key: [dict(d) for d in dts]} if dts else {}
        e.ious = {key: np.asarray(ious, dtype=np.float64).reshape(len(dts), len(gts)) if len(gts) and len(dts) else []}
        out = []
        for aRng in AREA_RNG:
            r = e.evaluate_img(0, 0, aRng, MAX_DETS[-1])
            if r is not None and len(gts):
                gtind = np.argsort([g['_ignore'] for g in e._gts[key]], kind='mergesort')
                inv = np.argsort(gtind, kind='mergesort')
                r = dict(r, gtMatches=r['gtMatches'][:, inv], gtIgnore=r['gtIgnore'][inv])
            out.append(r)
        return out

    @classmethod
    def match_lanes(cls, gts, dts, ious):
        """match_direct as three arrays of 40 rows, row t + 10 a for IoU threshold t and area range a: the matched gt's id per
        det (0: none), the det's ignore flag, and gtMatches > 0 per gt in json order."""
        D, G = len(dts), len(gts)
        recs = cls.match_direct(gts, dts, ious)
        n = len(IOU_THRS) * len(AREA_RNG)
        return (np.concatenate([r['dtMatches'] for r in recs]).astype(np.int64).reshape(n, D),
                np.concatenate([np.asarray(r['dtIgnore']) for r in recs]).astype(np.uint8).reshape(n, D),
                np.concatenate([r['gtMatches'] > 0 for r in recs]).astype(np.uint8).reshape(n, G))

    def accumulate(self):
        self.eval = accumulate(self.evalImgs, len(self.cat_ids), len(self.img_ids))

    def summarize(self):
        self.stats = summarize(self.eval)


def accumulate(evalImgs, K, I0):
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    A0 = A
    for k in range(K):
        Nk = k * A0 * I0
        for a in range(A):
            Na = a * I0
            for m, maxDet in enumerate(MAX_DETS):
                E = [evalImgs[Nk + Na + i] for i in range(I0)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind='mergesort')
                dtScoresSorted = dtScores[inds]
                dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e['gtIgnore'] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, REC_THRS, side='left')
                    try:
                        for ri, pi in enumerate(inds):
                            q[ri] = pr[pi]
                            ss[ri] = dtScoresSorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return {'precision': precision, 'recall': recall, 'scores': scores}


def summarize(ev):
    def _s(ap=1, iouThr=None, areaRng='all', maxDets=100):
        aind = [i for i, aRng in enumerate(AREA_LBL) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(MAX_DETS) if mDet == maxDets]
        if ap == 1:
            s = ev['precision']
            if iouThr is not None:
                s = s[np.where(iouThr == IOU_THRS)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = ev['recall']
            if iouThr is not None:
                s = s[np.where(iouThr == IOU_THRS)[0]]
            s = s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    return np.array([_s(1), _s(1, iouThr=.5), _s(1, iouThr=.75), _s(1, areaRng='small'), _s(1, areaRng='medium'),
                     _s(1, areaRng='large'), _s(0, maxDets=1), _s(0, maxDets=10), _s(0), _s(0, areaRng='small'),
                     _s(0, areaRng='medium'), _s(0, areaRng='large')], dtype=np.float64)
