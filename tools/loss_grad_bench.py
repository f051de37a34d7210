"""Time the loss's backward at 544 x 544 for batch 8 / 16 / 32 with 7 and 50 GTs per image, beside its forward.

  om_loss           the om_loss C call alone (OrienMaskYOLOMultiScaleLoss.prepare), hipEvents
  om_loss_backward  the om_loss_backward C call alone, its arguments and gradient tensors bound beforehand, hipEvents: the two
                    kernels plus the call's own launch overhead
  step              the whole loss(predict, target, training=True); loss_sum.backward() -- the forward's checks, call,
                    device-to-host copy and aggregation, the autograd node and the backward -- wall clock from a synchronize
                    to a synchronize
The backward's byte floor is the heads read once plus the gradients written once, at 6.3 TB/s; `floor_frac` is that time over
the measured om_loss_backward.  Medians of --iters runs after --warmup.

    python tools/loss_grad_bench.py [--iters 30] [--warmup 5] [--json out.json]
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
from orienmask_amd.model import OrienMaskYOLOFPNPlus  # noqa: E402
from orienmask_amd.train import OrienMaskYOLOMultiScaleLoss  # noqa: E402

ANCHORS_YOLOV4 = [[12, 16], [19, 36], [40, 28], [36, 75], [76, 55], [72, 146], [142, 110], [192, 243], [459, 401]]
ANCHOR_MASK = [[6, 7, 8], [3, 4, 5], [0, 1, 2]]
HBM_BYTES_PER_S = 6.3e12


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
            heads = [(b.clone(), o.clone()) for b, o in net(x)]
        nbytes = 2 * sum(t.numel() * 4 for p in heads for t in p)
        for g in (7, 50):
            target = tuple(torch.from_numpy(a).to(dev) for a in synth.synth_targets(11 + B + g, B, H, W, g))
            t_fwd = timed(loss.prepare(heads, target), args.iters, args.warmup)
            leaves = [(b.requires_grad_(), o.requires_grad_()) for b, o in heads]
            loss_sum = loss(leaves, target, training=True)[0]
            run, _, _ = loss_sum.grad_fn.call.bind(torch.ones((), device=dev))       # the autograd node is the Function's ctx
            t_bwd = timed(run, args.iters, args.warmup)
            del loss_sum
            walls = []
            for i in range(args.iters + args.warmup):
                for p in leaves:
                    for t in p:
                        t.grad = None
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                loss(leaves, target, training=True)[0].backward()
                torch.cuda.synchronize(dev)
                if i >= args.warmup:
                    walls.append((time.perf_counter() - t0) * 1e3)
            heads = [(b.detach(), o.detach()) for b, o in leaves]
            floor = nbytes / HBM_BYTES_PER_S * 1e3
            row = dict(batch=B, gts_per_image=g, loss_ms=round(t_fwd, 4), backward_ms=round(t_bwd, 4),
                       step_ms=round(statistics.median(walls), 4), bytes=nbytes, floor_ms=round(floor, 4),
                       floor_frac=round(floor / t_bwd, 3))
            rows.append(row)
            print("bs %2d  %2d GTs/img  om_loss %7.3f ms  om_loss_backward %7.3f ms (floor %.3f ms, %4.1f %%)  loss+backward %8.3f ms"
                  % (B, g, t_fwd, t_bwd, floor, 100 * floor / t_bwd, row["step_ms"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
