"""Time COCOEvaluator.evaluate + accumulate on a synthetic val2017-sized set (5000 images of 480 x 640, ~36k GTs, mostly
polygons and some crowd RLE, 100 segm results per image as RLE strings), for bbox and segm.  Per phase: HIP events around
mask building, IoU and matching (summed over chunks); accumulate and the whole call by wall time.  Median of three runs.
For contrast, tests/cocoeval_np.py (the loop-form restatement) on a 100-image subset, scaled to the full set.

    python tools/cocoeval_bench.py [--images 5000] [--runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def synth_set(n_images, seed=0):
    from orienmask_amd.coco_format import rle_to_string
    rng = np.random.default_rng(seed)
    H, W = 480, 640
    images, anns, res = [], [], []
    aid = 1
    # a pool of result strings, reused across images (building 500k strings would dominate the setup)
    pool = []
    for _ in range(64):
        m = np.zeros((H, W), np.uint8)
        x, y = rng.integers(0, W - 60), rng.integers(0, H - 60)
        m[y:y + rng.integers(10, 200), x:x + rng.integers(10, 300)] = 1
        flat = m.reshape(-1, order="F")
        edges = np.flatnonzero(np.diff(np.concatenate([[0], flat, [1 - flat[-1]]])))
        counts = np.diff(np.concatenate([[0], edges])).tolist()
        pool.append(rle_to_string(counts))
    for i in range(n_images):
        images.append(dict(id=i, height=H, width=W))
        for _ in range(int(rng.integers(3, 12))):
            c = int(rng.integers(1, 81))
            if rng.random() < 0.05:
                counts = [int(rng.integers(1000, 5000)) for _ in range(40)]
                counts.append(H * W - sum(counts))
                anns.append(dict(id=aid, image_id=i, category_id=c, iscrowd=1, area=float(sum(counts[1::2])),
                                 bbox=[0, 0, 100, 100], segmentation={"size": [H, W], "counts": counts}))
            else:
                cx, cy, r = rng.random() * W, rng.random() * H, 5 + rng.random() * 120
                ang = np.sort(rng.random(16) * 2 * np.pi)
                poly = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).ravel().round(2).tolist()
                anns.append(dict(id=aid, image_id=i, category_id=c, iscrowd=0, area=float(np.pi * r * r),
                                 bbox=[cx - r, cy - r, 2 * r, 2 * r], segmentation=[poly]))
            aid += 1
        for k in range(100):
            res.append(dict(image_id=i, category_id=int(rng.integers(1, 81)), score=float(rng.random()),
                            segmentation={"size": [H, W], "counts": pool[int(rng.integers(0, len(pool)))]},
                            bbox=[float(rng.random() * W), float(rng.random() * H), float(5 + rng.random() * 200),
                                  float(5 + rng.random() * 200)]))
    gt = {"images": images, "categories": [dict(id=c, name=str(c)) for c in range(1, 81)], "annotations": anns}
    return gt, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--np-images", type=int, default=100)
    args = ap.parse_args()
    import torch
    from orienmask_amd.cocoeval import COCOEvaluator, COCOGroundTruth
    gt, res = synth_set(args.images)
    G = COCOGroundTruth.from_dict(gt)
    out = {"images": args.images, "gts": len(gt["annotations"]), "results": len(res)}
    for kind in ("bbox", "segm"):
        r = [{k: v for k, v in d.items() if k != ("segmentation" if kind == "bbox" else "bbox")} for d in res]
        runs = []
        for _ in range(args.runs):
            ev = COCOEvaluator(G, r, kind)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ev.accumulate()
            t2 = time.perf_counter()
            runs.append(dict(evaluate_s=t1 - t0, accumulate_s=t2 - t1, total_s=t2 - t0,
                             **{k + "_gpu_ms": v for k, v in ev.timings.items()}))
        med = {k: float(np.median([x[k] for x in runs])) for k in runs[0]}
        out[kind] = med
        # the restatement on a subset
        import cocoeval_np as ref
        keep = set(range(args.np_images))
        gsub = dict(gt, images=[im for im in gt["images"] if im["id"] in keep],
                    annotations=[a for a in gt["annotations"] if a["image_id"] in keep])
        rsub = [d for d in r if d["image_id"] in keep]
        t0 = time.perf_counter()
        w = ref.Eval(gsub, rsub, kind)
        w.evaluate()
        w.accumulate()
        t1 = time.perf_counter()
        out[kind]["restatement_%d_images_s" % args.np_images] = t1 - t0
        out[kind]["restatement_scaled_s"] = (t1 - t0) * args.images / args.np_images
    print(json.dumps(out))


if __name__ == "__main__":
    main()
