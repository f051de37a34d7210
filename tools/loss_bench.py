"""Time the validation loss at 544 x 544 for batch 8 / 16 / 32 with 7 and 50 GTs per image, beside the forward of the same batch.

  om_loss  the om_loss C call alone, its arguments bound beforehand (OrienMaskYOLOMultiScaleLoss.prepare): hipEvents around it,
           so the four kernels plus the call's own launch overhead
  call     the whole loss(predict, target, training=False) -- input checks, the call, the one device-to-host copy and the
           host aggregation -- wall clock after a synchronize
  forward  the model's forward of the same batch (split operands), hipEvents
Medians of --iters runs after --warmup.

    python tools/loss_bench.py [--iters 30] [--warmup 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from orienmask_amd import synth  # noqa: E402
from orienmask_amd.eval import OrienMaskYOLOMultiScaleLoss  # noqa: E402
from orienmask_amd.model import OrienMaskYOLOFPNPlus  # noqa: E402

ANCHORS_YOLOV4 = [[12, 16], [19, 36], [40, 28], [36, 75], [76, 55], [72, 146], [142, 110], [192, 243], [459, 401]]
ANCHOR_MASK = [[6, 7, 8], [3, 4, 5], [0, 1, 2]]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="8,16,32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 544
    loss = OrienMaskYOLOMultiScaleLoss([[17, 17], [34, 34], [68, 68]], [H, W], ANCHORS_YOLOV4, ANCHOR_MASK, 80, valid_region=0.6,
                                       obj_ignore_threshold=0.7, weight=[1, 1, 1, 1, 1, 20, 20], scales_weight=[1, 1, 1])
    net = OrienMaskYOLOFPNPlus(3, 80).eval()
    net.load_state_dict(synth.synth_state_dict(1, obj_bias=-6.0, head_gain=2.0), strict=True)
    net = net.to(dev).set_precision("f32_split")
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        x = synth.synth_image_batch(3, B, H, W).to(dev)
        with torch.no_grad():
            t_fwd = timed(lambda: net(x), args.iters, args.warmup)
            predict = list(net(x))
        for g in (7, 50):
            target = tuple(torch.from_numpy(a).to(dev) for a in synth.synth_targets(11 + B + g, B, H, W, g))
            run = loss.prepare(predict, target)            # checks, ctypes arguments and buffers outside the timed window
            t_loss = timed(run, args.iters, args.warmup)
            walls = []
            for _ in range(args.iters):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                loss(predict, target, training=False)
                walls.append((time.perf_counter() - t0) * 1e3)
            row = dict(batch=B, gts_per_image=g, loss_ms=round(t_loss, 4), call_ms=round(statistics.median(walls), 4),
                       forward_ms=round(t_fwd, 3))
            rows.append(row)
            print("bs %2d  %2d GTs/img  om_loss %8.3f ms   loss() call %8.3f ms   forward %8.3f ms"
                  % (B, g, t_loss, row["call_ms"], t_fwd), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
