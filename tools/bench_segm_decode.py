"""Measure the 'segm' data path against the 'mask' path of the same commit on the same box.

The batch is seeded and of COCO-like proportions (orienmask_amd.synth.synth_segm_batch: 32 sources of 480 x 640, about 7 GTs per
image, 1-3 polygons of 20-200 vertices each, one crowd RLE in every fourth image), planned by the shipped training pipeline at
544 x 544 with the same seeds in both forms.  The 'mask' form's arrays are the device decode's own output read back, so both forms
hold the same masks, and the two to_device results are compared with torch.equal before anything is timed.

  * to_device(planned, device) through 'mask' and through 'segm': HIP events around --calls calls, the two paths alternating
    within each of --rounds rounds; median and min-max of the per-call time over the rounds;
  * om_segm_decode alone (tables already on the device), the same way;
  * the H2D bytes of each path, from PlannedBatch.h2d_bytes();
  * worker-side host time per image of the 'mask' path's np.stack + np.packbits ALONE.  A real worker also pays pycocotools'
    frPyObjects / merge / decode in front of it; pycocotools is not available here, so that part is not measured and the number
    is a lower bound of what the 'segm' path takes off the worker;
  * planner time per sample (COCOTransform.__call__) in both forms.

    python tools/bench_segm_decode.py [--rounds 15] [--calls 10] [--out profiles/segm_decode_bench.json]
"""
import argparse
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from orienmask_amd import augment, synth, transform  # noqa: E402

MEAN = [123.675, 116.280, 103.530]
TRAIN = [dict(type="ColorJitter", brightness=0.2, contrast=0.5, saturation=0.5, hue=0.1),
         dict(type="RandomCrop", p=0.5, image_min_iou=0.64, bbox_min_iou=0.64),
         dict(type="Resize", size=(544, 544), pad_needed=True, warp_p=0.25, jitter=0.3, random_place=True, pad_p=0.75, pad_ratio=0.75,
              pad_value=MEAN),
         dict(type="RandomHorizontalFlip", p=0.5), dict(type="ToTensor"), dict(type="Normalize", mean=(0, 0, 0), std=(255, 255, 255))]


def plan(samples, seed):
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=TRAIN))
    random.seed(seed)
    torch.manual_seed(seed)
    ts, out = [], []
    for s in samples:
        t0 = time.perf_counter()
        out.append(tf(s))
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def spread(ts):
    return dict(median=round(float(np.median(ts)), 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "segm_decode_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    dev = torch.device("cuda:0")
    batch = synth.synth_segm_batch(a.seed)
    planned_s, plan_s = plan(batch, a.seed + 1)
    pb_s = transform.collate(planned_s).pin_memory()
    with torch.cuda.device(dev):
        packed = augment._segm_decode(pb_s, dev).cpu().numpy()
    as_mask, off = [], 0
    for s in batch:
        h, w = s["image"].shape[:2]
        n, wb = len(s["segm"]), (w + 7) // 8
        bits = packed[off:off + n * h * wb].reshape(n, h, wb)
        off += n * h * wb
        as_mask.append(dict({k: v for k, v in s.items() if k != "segm"}, mask=list(np.unpackbits(bits, axis=2)[:, :, :w])))
    planned_m, plan_m = plan(as_mask, a.seed + 1)
    pb_m = transform.collate(planned_m).pin_memory()
    host = []
    for s in as_mask:
        if not s["mask"]:
            continue
        t0 = time.perf_counter()
        np.packbits(np.stack(s["mask"]) > 0, axis=2)
        host.append((time.perf_counter() - t0) * 1e3)

    def flat(res):
        return [res[0]] + list(res[1])

    with torch.cuda.device(dev):
        for x, y in zip(flat(transform.to_device(pb_s, dev)), flat(transform.to_device(pb_m, dev))):
            assert torch.equal(x, y), "the two paths disagree"
        tables = pb_s.segm.to(dev)
        keep = pb_s.segm
        decode_only = type("P", (), dict(segm=tables, segm_layout=pb_s.segm_layout, segm_counts=pb_s.segm_counts, N=pb_s.N))()
        for _ in range(3):                                      # warm: code objects loaded, allocator blocks cached
            transform.to_device(pb_m, dev)
            transform.to_device(pb_s, dev)
            augment._segm_decode(decode_only, dev)
        torch.cuda.synchronize()
        t_mask, t_segm, t_dec = [], [], []
        for _ in range(a.rounds):
            t_mask.append(event_ms(lambda: transform.to_device(pb_m, dev), a.calls))
            t_segm.append(event_ms(lambda: transform.to_device(pb_s, dev), a.calls))
            t_dec.append(event_ms(lambda: augment._segm_decode(decode_only, dev), a.calls))
        assert pb_s.segm is keep
    c = pb_s.segm_counts
    res = dict(bench="segm_decode", batch=len(batch), src="480x640", out="544x544", N=pb_s.N, n_poly=c["n_poly"], n_srcs=c["n_srcs"],
               crowd_rles=c["n_srcs"] - c["n_poly"], bitmap_bytes=4 * c["bitmap_words"], rounds=a.rounds, calls_per_round=a.calls,
               to_device_ms=dict(mask=spread(t_mask), segm=spread(t_segm)),
               segm_over_mask=round(float(np.median(t_segm) / np.median(t_mask)), 3),
               segm_decode_alone_ms=spread(t_dec),
               h2d_bytes=dict(mask=dict(pb_m.h2d_bytes(), total=sum(pb_m.h2d_bytes().values())),
                              segm=dict(pb_s.h2d_bytes(), total=sum(pb_s.h2d_bytes().values()))),
               worker_stack_packbits_ms_per_image=dict(spread(host), note="np.stack + np.packbits only; the pycocotools "
                                                       "rasterisation a real worker pays in front of it is not measured"),
               planner_ms_per_sample=dict(mask=spread(plan_m), segm=spread(plan_s)), outputs_equal=True)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
