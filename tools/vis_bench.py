"""Device time of InferenceVisualizer.composite's kernels (om_visualize: per-mask pre-pass + composite), by hipEvents.

    python tools/vis_bench.py [--iters 50] [--warmup 5]

Cases: 480 x 640 with K = 20 kept masks; 1080 x 1920 with K = 100 masks covering the whole image ("full") and with K = 100
small masks ("sparse").  Masks are at the 544 x 544 network size.  The host part of a call (score filter, boxes, colours)
is prepared once; the timed loop is the launch pair alone.  Prints one JSON line per case: microseconds per call and the
effective bytes per output pixel -- the 12 bytes of float32 source and 3 bytes of uint8 output every pixel needs, plus the
case's mask bytes spread over its pixels -- and the rate that gives.
"""
import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from orienmask_amd import synth  # noqa: E402
from orienmask_amd.visualizer import InferenceVisualizer  # noqa: E402


def masks_for(kind, K, Hn, Wn, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "full":
        return torch.ones(K, Hn, Wn, dtype=torch.bool)
    yy, xx = np.mgrid[0:Hn, 0:Wn]
    out = np.zeros((K, Hn, Wn), dtype=bool)
    r_lo, r_hi = (0.03, 0.08) if kind == "sparse" else (0.05, 0.3)
    for k in range(K):
        ry, rx = rng.uniform(r_lo, r_hi) * Hn, rng.uniform(r_lo, r_hi) * Wn
        cy, cx = rng.uniform(ry, Hn - ry), rng.uniform(rx, Wn - rx)
        out[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return torch.from_numpy(out)


def bench_case(name, h, w, K, kind, dev, iters, warmup):
    Hn = Wn = 544
    g = torch.Generator().manual_seed(1)
    bbox = torch.cat([torch.rand(K, 4, generator=g) * 0.5 + 0.25, torch.rand(K, 1, generator=g) * 0.6 + 0.35], 1)
    dets = dict(bbox=bbox.to(dev), cls=(torch.arange(K) % 80).to(dev), mask=masks_for(kind, K, Hn, Wn, 2).to(dev))
    image = synth.synth_photo_batch(3, 1, h, w)[0].to(dev)
    v = InferenceVisualizer("COCO", dev, alpha=0.6, draw="device")
    random.seed(0)
    item = v._prepare(dets, image, [0, 0, 0, 0, Hn, Wn])
    out = torch.empty(image.shape, dtype=torch.uint8, device=dev)
    for _ in range(warmup):
        v._launch([item], [out], draw_boxes=False)
    torch.cuda.synchronize()
    times = []
    for _ in range(3):                       # three windows: the spread is reported
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            v._launch([item], [out], draw_boxes=False)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / iters)
    us = sorted(times)[1]
    pixels = h * w
    mask_bytes = K * Hn * Wn
    bpp = 15.0 + mask_bytes / pixels
    return dict(case=name, h=h, w=w, K=K, masks=kind, us_per_call=round(us, 1), us_windows=[round(t, 1) for t in times],
                effective_bytes_per_pixel=round(bpp, 2), effective_GBps=round(bpp * pixels / us * 1e-3, 1),
                Mpixel_per_s=round(pixels / us, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vis_bench.py needs an MI355X")
    dev = torch.device("cuda:0")
    for args in (("vga_k20", 480, 640, 20, "mixed"), ("1080p_k100_full", 1080, 1920, 100, "full"),
                 ("1080p_k100_sparse", 1080, 1920, 100, "sparse")):
        print(json.dumps(bench_case(*args, dev=dev, iters=a.iters, warmup=a.warmup)), flush=True)


if __name__ == "__main__":
    main()
