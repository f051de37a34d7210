"""COCO bbox / segm evaluation without pycocotools (orienmask_amd/cocoeval.py, csrc/cocoeval.hip).

pycocotools is not installed, so nothing here compares with it directly: the evaluator is checked against hand-computed known
answers, against tests/cocoeval_np.py (a loop-for-loop restatement of the published algorithms sharing no code with the
product), against the pinned mask resize of coco_format, and against the reference's own display code
(tests/golden/cocoeval_display.npz, written by tools/gen_golden_cocoeval.py)."""
import contextlib
import inspect
import io
import json
import os

import numpy as np
import pytest
import torch

import cocoeval_np as ref
from orienmask_amd import lib as omlib
from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_module_surface_matches_reference():
    from orienmask_amd import cocoeval as CE
    assert list(inspect.signature(CE.COCOMetrics.__init__).parameters)[:5] == ["self", "gt_file", "cat2label", "with_mask",
                                                                               "save_dir"]
    for name in ("reset", "to_coco_format", "update_results", "save_as_json", "update_from_json", "coco_eval",
                 "_get_per_cats_stats"):
        assert callable(getattr(CE.COCOMetrics, name)), name
    assert list(inspect.signature(CE.COCOMetrics.coco_eval).parameters) == ["self", "per_cats"]
    assert inspect.signature(CE.COCOMetrics.coco_eval).parameters["per_cats"].default is False
    m = CE.COCOMetrics("gt.json", list(range(1, 4)), True, "/tmp")
    assert m.bbox_pred_file.endswith("bbox_prediction.json") and m.segm_pred_file.endswith("segm_prediction.json")
    assert m.metric_keys == ["AP", "AP50", "AP75", "APS", "APM", "APL", "AR1", "AR10", "AR100", "ARS", "ARM", "ARL"]
    for a in ("bbox_results", "segm_results", "bbox_eval_stats", "segm_eval_stats", "bbox_eval_per_cats_stats",
              "segm_eval_per_cats_stats"):
        assert getattr(m, a) == []
    for name in ("evaluate", "accumulate", "summarize"):
        assert callable(getattr(CE.COCOEvaluator, name))
    assert callable(CE.COCOGroundTruth.from_file) and callable(CE.COCOGroundTruth.from_dict)


def test_linspace_constants():
    from orienmask_amd import cocoeval as CE
    assert np.array_equal(CE.IOU_THRS, np.linspace(.5, .95, 10)) and CE.IOU_THRS.dtype == np.float64
    assert np.array_equal(CE.REC_THRS, np.linspace(0, 1, 101))
    assert (CE.IOU_THRS == .75).sum() == 1 and (CE.IOU_THRS == .5).sum() == 1
    assert CE.MAX_DETS == [1, 10, 100]
    assert CE.AREA_RNG == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def _random_records(seed, K=4, I0=6):
    """evalImgs-shaped records (per category, area range, image) and the same data as the product's flat arrays."""
    rng = np.random.default_rng(seed)
    T, A = 10, 4
    groups = []
    for k in range(K):
        for i in range(I0):
            if rng.random() < 0.2 or k == K - 1:            # the last category has no group at all: stays -1
                continue
            D, G = int(rng.integers(0, 130)), int(rng.integers(0, 6))
            if D == 0 and G == 0:
                continue
            sc = np.sort(np.round(rng.random(D), 2))[::-1].copy()          # ties on purpose
            dtm = rng.random((A, T, D)) < 0.4
            dti = rng.random((A, T, D)) < 0.1
            gti = rng.random((A, G)) < 0.3
            groups.append((k, i, sc, dtm, dti, gti))
    evalImgs = [None] * (K * A * I0)
    for k, i, sc, dtm, dti, gti in groups:
        for a in range(A):
            evalImgs[k * A * I0 + a * I0 + i] = {"dtScores": list(sc[:100]), "dtMatches": dtm[a][:, :100].astype(float) * 7,
                                                 "dtIgnore": dti[a][:, :100], "gtIgnore": gti[a].astype(int)}
    grp_cat = np.array([g[0] for g in groups])
    dt_cat = np.concatenate([[g[0]] * min(len(g[2]), 100) for g in groups]).astype(np.int64)
    dt_rank = np.concatenate([np.arange(min(len(g[2]), 100)) for g in groups]).astype(np.int64)
    dt_score = np.concatenate([g[2][:100] for g in groups])
    dtm = np.concatenate([g[3][:, :, :100] for g in groups], axis=2)
    dti = np.concatenate([g[4][:, :, :100] for g in groups], axis=2)
    gt_cat = np.concatenate([[g[0]] * g[5].shape[1] for g in groups]).astype(np.int64)
    gti = np.concatenate([g[5] for g in groups], axis=1)
    return evalImgs, (K, grp_cat, dt_cat, dt_rank, dt_score, dtm, dti, gt_cat, gti)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_accumulate_and_summarize_match_restatement(seed):
    from orienmask_amd import cocoeval as CE
    evalImgs, flat = _random_records(seed)
    want = ref.accumulate(evalImgs, flat[0], 6)
    got = CE.accumulate_records(*flat, CE.IOU_THRS, CE.REC_THRS, CE.MAX_DETS)
    for key in ("precision", "recall", "scores"):
        assert got[key].shape == want[key].shape
        assert np.array_equal(got[key], want[key]), key
    assert (got["precision"] == -1).any()
    with contextlib.redirect_stdout(io.StringIO()) as out:
        stats = CE.summarize(got)
    assert stats.tobytes() == ref.summarize(want).tobytes()
    lines = out.getvalue().splitlines()
    assert len(lines) == 12
    assert lines[0].startswith(" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ")
    assert lines[6].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = ")


def test_display_and_per_cats_match_reference_fixture():
    """tools/gen_golden_cocoeval.py ran the reference's _get_per_cats_stats and Tester.display_coco_eval on a seeded
    precision array; the product must print the same characters and compute the same floats."""
    from orienmask_amd import cocoeval as CE
    g = np.load(os.path.join(GOLDEN, "cocoeval_display.npz"), allow_pickle=False)
    for kind in ("bbox", "segm"):
        prec = g[kind + "_precision"]
        per = CE.per_cats_stats(prec, prec.shape[2])
        want = g[kind + "_per_cats"]
        assert np.array_equal(np.array(per), want, equal_nan=True)
    m = CE.COCOMetrics("gt.json", list(range(80)), True, "/tmp")
    m.bbox_eval_stats, m.segm_eval_stats = g["bbox_stats"], g["segm_stats"]
    m.bbox_eval_per_cats_stats = CE.per_cats_stats(g["bbox_precision"], 80)
    m.segm_eval_per_cats_stats = CE.per_cats_stats(g["segm_precision"], 80)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        CE.display_coco_eval(m, "bbox")
        CE.display_coco_eval(m, "segm")
    assert out.getvalue() == str(g["text"])


# ----------------------------------------------------------------------------------------------------------------- GPU
def _gt(images, anns, cats=(1, 2, 3)):
    return {"images": [dict(id=i, height=h, width=w) for i, h, w in images],
            "categories": [dict(id=c, name=str(c)) for c in cats],
            "annotations": [dict(a) for a in anns]}


def _ann(id_, img, cat, segm, area, bbox=None, crowd=0):
    return dict(id=id_, image_id=img, category_id=cat, segmentation=segm, area=float(area), iscrowd=crowd,
                bbox=bbox if bbox is not None else [0, 0, 1, 1])


def _run(gt, res, kind, **kw):
    from orienmask_amd.cocoeval import COCOEvaluator
    ev = COCOEvaluator(gt, res, kind, **kw)
    ev.evaluate()
    ev.accumulate()
    with contextlib.redirect_stdout(io.StringIO()):
        ev.summarize()
    return ev


def _string(mask):
    from oracle.orienmask_ref import rle_counts_c
    from orienmask_amd.coco_format import rle_to_string
    return {"size": list(mask.shape), "counts": rle_to_string(rle_counts_c(mask))}


def _masks_of(gt, anns, dev):
    """The product's bitmaps of GT annotations, decoded to [h, w] arrays (one evaluation with each as its own result)."""
    from orienmask_amd.cocoeval import COCOEvaluator, COCOGroundTruth
    G = COCOGroundTruth.from_dict(gt)
    ev = COCOEvaluator(G, [], "segm", device=dev)
    ev.device = dev
    out = []
    with torch.cuda.device(dev):
        stats = ev._build_masks(omlib.load(), anns, omlib.current_stream_ptr(dev))
        torch.cuda.synchronize()
        buf = ev._ws_keep
        off = ev._ws.data_ptr() - buf.data_ptr()
        bm = buf[off:off + 4 * ev._m_words].view(torch.int32).cpu().numpy().view(np.uint32)
    hw, moff = ev._m_hw.cpu().numpy(), ev._m_off.cpu().numpy()
    for m in range(len(anns)):
        h, w = hw[m]
        nh = (h + 31) // 32
        words_m = bm[moff[m]:moff[m] + w * nh].reshape(w, nh)
        bits = ((words_m[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w, nh * 32)
        assert not bits[:, h:].any()                         # padding bits stay zero
        out.append(bits[:, :h].T.astype(np.uint8))
        assert stats[m, 0] == out[-1].sum()
    return out


@pytest.mark.gpu
def test_polygon_rasterisation_known_answers(built):
    dev = torch.device("cuda:0")
    anns = [
        _ann(1, 1, 1, [[2, 2, 6, 2, 6, 5, 2, 5]], 12),                       # square: columns 2..5, rows 2..4
        _ann(2, 1, 1, [[0, 0, 4, 0, 0, 4]], 10),                              # right triangle
        _ann(3, 1, 1, [[1.5, 1.5, 3.5, 1.5, 3.5, 3.5, 1.5, 3.5]], 4),        # vertices at half-pixel positions
        _ann(4, 1, 1, [[-3, -3, 4, -3, 4, 3, -3, 3]], 16),                    # partly outside the image
        _ann(5, 1, 1, [[1, 1, 2, 2]], 4),                                     # the 4-number box quirk of frPyObjects
        _ann(6, 1, 1, [[0, 0, 2, 0, 2, 2, 0, 2], [4, 4, 6, 4, 6, 6, 4, 6]], 8),  # two polygons, ORed
    ]
    gt = _gt([(1, 8, 9)], anns)
    got = _masks_of(gt, gt["annotations"], dev)
    sq = np.zeros((8, 9), np.uint8); sq[2:5, 2:6] = 1
    assert np.array_equal(got[0], sq)
    # pixel x covers [x, x + 1), as the square shows (4 columns for a width of 4): the hypotenuse x + y = 4 leaves column x
    # the rows y < 3 - x (its value at the column's right side)
    tri = np.zeros((8, 9), np.uint8)
    for x in range(3):
        tri[0:3 - x, x] = 1
    assert np.array_equal(got[1], tri), got[1]
    half = np.zeros((8, 9), np.uint8); half[2:4, 2:4] = 1
    assert np.array_equal(got[2], half), got[2]
    out = np.zeros((8, 9), np.uint8); out[0:3, 0:4] = 1
    assert np.array_equal(got[3], out), got[3]
    box = np.zeros((8, 9), np.uint8); box[1:3, 1:3] = 1                     # x 1, y 1, w 2, h 2
    assert np.array_equal(got[4], box), got[4]
    two = np.zeros((8, 9), np.uint8); two[0:2, 0:2] = 1; two[4:6, 4:6] = 1
    assert np.array_equal(got[5], two), got[5]
    for a, m in zip(anns, got):                              # and the restatement agrees pixel for pixel
        assert np.array_equal(ref.ann_mask(a["segmentation"], 8, 9), m)


def _sq(x, y, s):
    return [[x, y, x + s, y, x + s, y + s, x, y + s]]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bbox", "segm"])
def test_one_perfect_detection(built, kind):
    gt = _gt([(1, 100, 100)], [_ann(1, 1, 1, _sq(10, 10, 50), 2500, bbox=[10, 10, 50, 50])])
    m = np.zeros((100, 100), np.uint8); m[10:60, 10:60] = 1
    res = [dict(image_id=1, category_id=1, score=0.9, **({"bbox": [10, 10, 50, 50]} if kind == "bbox" else
                                                          {"segmentation": _string(m)}))]
    ev = _run(gt, res, kind)
    # medium object: small and large have no GT -> -1.  A perfect precision is tp / (fp + tp + 2^-52) = 1 / (1 + 2^-52),
    # one ulp below 1, in pycocotools too; recall is tp / npig = 1 exactly
    p1 = 1.0 / (1.0 + np.spacing(1))
    ap, ap1 = np.mean(np.full(1010, p1)), np.mean(np.full(101, p1))       # summarize's np.mean over 10 x 101 / 101 samples
    want = [ap, ap1, ap1, -1, ap, -1, 1, 1, 1, -1, 1, -1]
    assert ev.stats.tolist() == want
    assert ev.eval["precision"].shape == (10, 101, 3, 4, 3) and ev.eval["recall"].shape == (10, 3, 4, 3)


@pytest.mark.gpu
def test_iou_062_detection():
    gt = _gt([(1, 200, 200)], [_ann(1, 1, 1, _sq(0, 0, 100), 10000, bbox=[0, 0, 100, 100])])
    # det [0, 0, 100, 62]: IoU = 6200 / 10000 = 0.62
    ev = _run(gt, [dict(image_id=1, category_id=1, bbox=[0, 0, 100, 62], score=0.5)], "bbox")
    assert ev.ious[(1, 1)][0, 0] == 0.62
    p1 = 1.0 / (1.0 + np.spacing(1))
    assert ev.stats[1] == np.mean(np.full(101, p1)) and ev.stats[2] == 0
    assert ev.stats[0] == np.mean([p1] * 303 + [0.0] * 707)  # thresholds .50 .55 .60 match: 3 of 10, 101 samples each


@pytest.mark.gpu
def test_crowd_gt_absorbs_detections():
    crowd = np.zeros((60, 60), np.uint8); crowd[0:60, 0:30] = 1
    from oracle.orienmask_ref import rle_counts_c
    gt = _gt([(1, 60, 60)], [_ann(1, 1, 1, _sq(40, 40, 10), 100, bbox=[40, 40, 10, 10]),
                             _ann(2, 1, 1, {"size": [60, 60], "counts": rle_counts_c(crowd)}, 1800, bbox=[0, 0, 30, 60], crowd=1)])
    res = []
    for k in range(3):                                       # three dets inside the crowd region
        m = np.zeros((60, 60), np.uint8); m[10 * k:10 * k + 10, 0:10] = 1
        res.append(dict(image_id=1, category_id=1, score=0.9 - 0.1 * k, segmentation=_string(m)))
    m = np.zeros((60, 60), np.uint8); m[40:50, 40:50] = 1
    res.append(dict(image_id=1, category_id=1, score=0.1, segmentation=_string(m)))
    ev = _run(gt, res, "segm")
    assert np.array_equal(ev.ious[(1, 1)][:3, 1], [1.0, 1.0, 1.0])   # crowd: union = det area
    assert ev.stats[0] == np.mean(np.full(1010, 1.0 / (1.0 + np.spacing(1))))     # crowd matches ignored, the GT found
    w = ref.Eval(gt, res, "segm"); w.evaluate(); w.accumulate(); w.summarize()
    assert ev.stats.tobytes() == w.stats.tobytes()


@pytest.mark.gpu
def test_ties_maxdet_absent_category_and_empty_images():
    anns = [_ann(1, 1, 1, _sq(0, 0, 32), 32 * 32, bbox=[0, 0, 32, 32]),          # area exactly 32^2: small AND medium
            _ann(2, 2, 1, _sq(0, 0, 20), 400, bbox=[0, 0, 20, 20]),
            _ann(3, 3, 2, _sq(0, 0, 20), 400, bbox=[0, 0, 20, 20])]                # image 3: GT, no dets
    gt = _gt([(1, 64, 64), (2, 64, 64), (3, 64, 64), (4, 64, 64)], anns)
    res = [dict(image_id=1, category_id=1, bbox=[0, 0, 32, 32], score=0.5),
           dict(image_id=2, category_id=1, bbox=[30, 30, 5, 5], score=0.5),         # equal scores across images
           dict(image_id=4, category_id=2, bbox=[1, 1, 5, 5], score=0.7),          # image 4: dets, no GT
           dict(image_id=1, category_id=7, bbox=[0, 0, 32, 32], score=0.99)]       # category absent from the GT
    res += [dict(image_id=2, category_id=1, bbox=[float(i % 40), 0, 20, 20], score=0.4 - i * 1e-3) for i in range(150)]
    ev = _run(gt, res, "bbox")
    w = ref.Eval(gt, res, "bbox"); w.evaluate(); w.accumulate(); w.summarize()
    for key in ("precision", "recall", "scores"):
        assert np.array_equal(ev.eval[key], w.eval[key]), key
    assert ev.stats.tobytes() == w.stats.tobytes()
    assert ev.eval["recall"][0, 0, 1, 2] == 1.0 and ev.eval["recall"][0, 0, 2, 2] >= 0     # 32^2 is in small and medium
    assert ev.ious[(2, 1)].shape == (100, 1)                 # the maxDet cut
    with pytest.raises(ValueError):
        _run(gt, [dict(image_id=99, category_id=1, bbox=[0, 0, 1, 1], score=0.5)], "bbox")


def _random_case(seed):
    rng = np.random.default_rng(seed)
    from oracle.orienmask_ref import rle_counts_c
    sizes = [(1, 1), (7, 5), (33, 65), (64, 31)] + [(int(rng.integers(40, 200)), int(rng.integers(40, 200))) for _ in range(4)]
    if seed == 0:
        sizes.append((480, 640))
    images = [(i + 1, h, w) for i, (h, w) in enumerate(sizes)]
    anns, res, aid = [], [], 1
    for i, h, w in images:
        for _ in range(int(rng.integers(0, 6))):
            c = int(rng.integers(1, 4))
            if rng.random() < 0.2:
                m = (rng.random((h, w)) < 0.5).astype(np.uint8)
                segm, crowd = {"size": [h, w], "counts": rle_counts_c(m)}, 1
                area = float(m.sum())
            else:
                polys = []
                for _ in range(int(rng.integers(1, 3))):
                    cx, cy, r = rng.random() * w, rng.random() * h, rng.random() * max(h, w) / 2 + 0.3
                    n = int(rng.integers(3, 12))
                    ang = np.sort(rng.random(n) * 2 * np.pi)
                    rr = r * (0.5 + rng.random(n))
                    polys.append(np.round(np.stack([cx + rr * np.cos(ang), cy + rr * np.sin(ang)], 1).ravel(), 2).tolist())
                segm, crowd = polys, 0
                area = float(ref.ann_mask(polys, h, w).sum()) if rng.random() < 0.5 else float(rng.random() * 2 * h * w)
            m = ref.ann_mask(segm, h, w)
            ys, xs = np.nonzero(m)
            bbox = [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)] \
                if len(xs) else [0.0, 0.0, 0.0, 0.0]
            anns.append(_ann(aid, i, c, segm, area, bbox=bbox, crowd=crowd))
            aid += 1
            for _ in range(int(rng.integers(0, 4))):         # perturbed copies as detections
                dm = m.copy()
                flip = rng.random((h, w)) < 0.1
                dm[flip] ^= 1
                res.append(dict(image_id=i, category_id=c if rng.random() < 0.8 else int(rng.integers(1, 4)),
                                score=float(np.round(rng.random(), 2)), segmentation=_string(dm),
                                bbox=[b + float(rng.normal()) for b in bbox[:2]] + [max(0.0, b + float(rng.normal())) for b in bbox[2:]]))
        for _ in range(int(rng.integers(0, 4))):             # false positives
            dm = (rng.random((h, w)) < 0.05).astype(np.uint8)
            res.append(dict(image_id=i, category_id=int(rng.integers(1, 4)), score=float(np.round(rng.random(), 2)),
                            segmentation=_string(dm), bbox=[float(rng.random() * w), float(rng.random() * h), 5.0, 5.0]))
    return _gt(images, anns), res


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind", ["bbox", "segm"])
def test_random_cases_match_restatement(built, seed, kind):
    gt, res = _random_case(seed)
    if kind == "bbox":
        res = [{k: v for k, v in r.items() if k != "segmentation"} for r in res]
    else:
        res = [{k: v for k, v in r.items() if k != "bbox"} for r in res]
    ev = _run(gt, res, kind)
    w = ref.Eval(gt, res, kind); w.evaluate(); w.accumulate(); w.summarize()
    for key, ious in w.ious.items():
        if len(ious):
            assert np.array_equal(ev.ious[key], ious), key
    for key in ("precision", "recall", "scores"):
        assert np.array_equal(ev.eval[key], w.eval[key]), key
    assert ev.stats.tobytes() == w.stats.tobytes()
    # chunking invariance: one image per chunk gives the same arrays
    ev2 = _run(gt, res, kind, max_bytes=1)
    for key in ("precision", "recall", "scores"):
        assert np.array_equal(ev.eval[key], ev2.eval[key]), key


@pytest.mark.gpu
def test_round_trip_with_coco_format_masks(built):
    """Strings from COCOFormatter decode to the masks recover_masks_rle(return_resized=True) produces (pinned against the
    reference), and an evaluation whose GT is those masks as uncompressed RLE scores AP = 1."""
    from oracle.orienmask_ref import rle_counts_c
    from orienmask_amd import coco_format as CF
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    K, H, W = 6, 96, 128
    raw = torch.from_numpy(rng.random((K, H, W)) < 0.3).to(dev)
    raw[:, 20:60, 30:90] = True
    info = dict(id=3, height=75, width=101, pad=[4, 6, 2, 0, H, W])
    rles, resized = CF.recover_masks_rle(raw, info, return_resized=True)
    fmt = CF.COCOFormatter(list(range(1, 81)))
    bbox = torch.tensor([[0.5, 0.5, 0.5, 0.5, 0.9 - 0.1 * k] for k in range(K)], dtype=torch.float32, device=dev)
    dets = [dict(bbox=bbox, cls=torch.zeros(K, dtype=torch.int64, device=dev), mask=raw)]
    out = fmt.to_coco_format([info], dets)
    masks = resized.cpu().numpy()
    gt = _gt([(3, 75, 101)], [_ann(k + 1, 3, 1, {"size": [75, 101], "counts": rle_counts_c(masks[k])}, float(masks[k].sum()))
                             for k in range(K)], cats=(1,))
    got = _masks_of(gt, [dict(image_id=3, segmentation=r["segmentation"]) for r in out["segm"]], dev)
    for k in range(K):
        assert np.array_equal(got[k], masks[k]), k
    ev = _run(gt, out["segm"], "segm")
    # six true positives: k / (k + 2^-52) rounds to exactly 1 for k >= 2, and the right-to-left maximum lifts the first one
    assert ev.stats[0] == 1.0 and ev.stats[8] == 1.0


@pytest.mark.gpu
def test_coco_metrics_end_to_end(built, tmp_path):
    """Tester over SyntheticLoader with COCOMetrics.to_coco_format / update_results as the batch hook, then coco_eval against a
    seeded polygon GT; the values equal the restatement on the very json files coco_eval wrote."""
    from orienmask_amd import synth
    from orienmask_amd.cocoeval import COCOMetrics, display_coco_eval
    from orienmask_amd.eval import OrienMaskYOLOPostProcess
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    from orienmask_amd.tester import SyntheticLoader, Tester
    from conftest import post_cfg
    dev = torch.device("cuda:0")
    net = OrienMaskYOLOFPNPlus(3, 80).eval()
    net.load_state_dict(synth.synth_state_dict(3, obj_bias=-16.0, head_gain=4.0), strict=True)
    net = net.to(dev)
    post = OrienMaskYOLOPostProcess(device=dev, **post_cfg((544, 544)))
    from orienmask_amd.visualizer import CAT2LABEL
    cat2label = list(CAT2LABEL["COCO"])
    rng = np.random.default_rng(11)
    anns, aid = [], 1
    for i in range(4):
        for _ in range(6):
            x, y, s = rng.random() * 400, rng.random() * 400, 20 + rng.random() * 140
            c = int(cat2label[int(rng.integers(0, 5))])
            anns.append(_ann(aid, i, c, _sq(x, y, s), s * s, bbox=[x, y, s, s]))
            aid += 1
    gt = {"images": [dict(id=i, height=544, width=544) for i in range(4)],
          "categories": [dict(id=int(c), name=str(c)) for c in cat2label], "annotations": anns}
    gt_file = tmp_path / "gt.json"
    gt_file.write_text(json.dumps(gt))
    metrics = COCOMetrics(str(gt_file), cat2label, True, str(tmp_path))
    Tester(net, post, SyntheticLoader(4, 2, seed=500), dev,
           on_batch=lambda info, dets: metrics.update_results(metrics.to_coco_format(info, dets))).test(verbose=False)
    assert metrics.bbox_results and metrics.segm_results
    log = metrics.coco_eval(per_cats=True)
    assert list(log) == ["bbox_" + k for k in metrics.metric_keys] + ["segm_" + k for k in metrics.metric_keys]
    assert os.path.exists(metrics.bbox_pred_file) and os.path.exists(metrics.segm_pred_file)
    for kind in ("bbox", "segm"):
        w = ref.Eval(gt, json.load(open(getattr(metrics, kind + "_pred_file"))), kind)
        w.evaluate(); w.accumulate(); w.summarize()
        assert getattr(metrics, kind + "_eval_stats").tobytes() == w.stats.tobytes(), kind
        assert [log[kind + "_" + k] for k in metrics.metric_keys] == w.stats.tolist()
        assert len(getattr(metrics, kind + "_eval_per_cats_stats")) == 80
    with contextlib.redirect_stdout(io.StringIO()) as out:
        display_coco_eval(metrics, "segm")
    assert "Per-category segm AP" in out.getvalue() and "| person" in out.getvalue()
