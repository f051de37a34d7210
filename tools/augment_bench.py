"""Measure the device data pipeline (orienmask_amd.augment: COCOTransform planner + collate + om_augment) on 640 x 480 sources.

Per configuration (bs 8 / 32, 7 / 50 GTs per image, the shipped train / val pipelines at 544 x 544):
  * host planner ms per sample (COCOTransform.__call__: draws, boxes, uint8 transport check, mask bit-packing) and collate ms;
  * H2D bytes and ms (hip events, pinned source): what crosses (uint8 images + packed masks + meta) against what the reference's
    loader ships (float32 [B,3,544,544] images + one byte per mask pixel), timed as copies of those sizes;
  * kernel ms (hip events, median of --reps): the whole launch set, and the image side (grey mean + image) and mask kernel apart
    (a launch set with the masks left out), each with the bytes it moves as a fraction of 6.3 TB/s.

    python tools/augment_bench.py [--reps 20] [--bs 8 32] [--gts 7 50]      # one JSON line per configuration
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from orienmask_amd import lib as omlib, synth, transform  # noqa: E402

HBM = 6.3e12
MEAN = [123.675, 116.280, 103.530]
TRAIN = [dict(type="ColorJitter", brightness=0.2, contrast=0.5, saturation=0.5, hue=0.1),
         dict(type="RandomCrop", p=0.5, image_min_iou=0.64, bbox_min_iou=0.64),
         dict(type="Resize", size=(544, 544), pad_needed=True, warp_p=0.25, jitter=0.3, random_place=True, pad_p=0.75, pad_ratio=0.75,
              pad_value=MEAN),
         dict(type="RandomHorizontalFlip", p=0.5), dict(type="ToTensor"), dict(type="Normalize", mean=(0, 0, 0), std=(255, 255, 255))]
VAL = [dict(type="Resize", size=(544, 544), pad_needed=False, warp_p=0., jitter=0., random_place=False, pad_p=0., pad_ratio=0.,
            pad_value=MEAN), dict(type="ToTensor"), dict(type="Normalize", mean=(0, 0, 0), std=(255, 255, 255))]


def timed(fn, reps, dev):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def launch(pb, dev_bufs, out_image, out_mask, ws, with_masks):
    meta, image, masks = dev_bufs
    L = omlib.load()
    N = pb.N if with_masks else 0
    rc = L.om_augment(ctypes.c_void_p(meta.data_ptr() + pb.layout["samples"][0]), pb.B, ctypes.c_void_p(image.data_ptr()),
                      int(pb.image.dtype == torch.uint8), (ctypes.c_float * 3)(*pb.mean), (ctypes.c_float * 3)(*pb.std),
                      pb.out_hw[0], pb.out_hw[1], ctypes.c_void_p(out_image.data_ptr()),
                      ctypes.c_void_p(masks.data_ptr() if N else None), ctypes.c_void_p(meta.data_ptr() + pb.layout["gt"][0]), N,
                      ctypes.c_void_p(out_mask.data_ptr() if N else None), int(pb.any_contrast),
                      ctypes.c_void_p(ws.data_ptr()), ws.numel(), omlib.current_stream_ptr(out_image.device))
    omlib.check(rc, "om_augment")


def run(name, pipeline, bs, gts, reps, dev):
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=pipeline))
    random.seed(bs * 100 + gts)
    torch.manual_seed(bs * 100 + gts)
    src = [synth.synth_coco_sample(s, 480, 640, gts) for s in range(bs)]
    t0 = time.perf_counter()
    planned = [tf(dict(s, mask=list(s["mask"]), info=dict(s["info"]))) for s in src]
    t1 = time.perf_counter()
    pb = transform.collate(planned)
    t2 = time.perf_counter()
    pb.pin_memory()
    H, W = pb.out_hw
    nb = pb.h2d_bytes()
    packed = sum(nb.values())
    unpacked = {"image": bs * 3 * H * W * 4, "mask": pb.N * H * W}
    with torch.cuda.device(dev):
        dev_bufs = [t.to(dev, non_blocking=True) for t in (pb.meta, pb.image, pb.mask)]
        h2d_packed = timed(lambda: [t.to(dev, non_blocking=True) for t in (pb.meta, pb.image, pb.mask)], reps, dev)
        host_unpacked = [torch.empty(v, dtype=torch.uint8).pin_memory() for v in unpacked.values()]
        h2d_unpacked = timed(lambda: [t.to(dev, non_blocking=True) for t in host_unpacked], reps, dev)
        out_image = torch.empty((bs, 3, H, W), dtype=torch.float32, device=dev)
        out_mask = torch.empty((pb.N, H, W), dtype=torch.bool, device=dev)
        ws = torch.empty(max(1, omlib.load().om_augment_workspace_bytes(bs)), dtype=torch.uint8, device=dev)
        for _ in range(3):
            launch(pb, dev_bufs, out_image, out_mask, ws, True)
        torch.cuda.synchronize()
        full = timed(lambda: launch(pb, dev_bufs, out_image, out_mask, ws, True), reps, dev)
        img = timed(lambda: launch(pb, dev_bufs, out_image, out_mask, ws, False), reps, dev)
    src_bytes = pb.image.numel() * pb.image.element_size()
    img_bytes = bs * 3 * H * W * 4 + src_bytes * (2 if pb.any_contrast else 1)       # output + source read (twice with contrast)
    mask_bytes = pb.N * H * W + pb.mask.numel()
    mask_ms = max(full - img, 1e-6)
    return dict(pipeline=name, bs=bs, gts_per_image=gts, src="640x480", out="%dx%d" % (H, W), N=pb.N,
                planner_ms_per_sample=round((t1 - t0) * 1e3 / bs, 3), collate_ms=round((t2 - t1) * 1e3, 3),
                h2d_bytes=dict(nb, total=packed), h2d_ms=round(h2d_packed, 4),
                h2d_unpacked_bytes=dict(unpacked, total=sum(unpacked.values())), h2d_unpacked_ms=round(h2d_unpacked, 4),
                kernel_ms=round(full, 4), image_side_ms=round(img, 4), image_side_bytes=img_bytes,
                image_side_hbm_frac=round(img_bytes / (img * 1e-3) / HBM, 3), mask_ms=round(mask_ms, 4), mask_bytes=mask_bytes,
                mask_hbm_frac=round(mask_bytes / (mask_ms * 1e-3) / HBM, 3) if pb.N else 0.0,
                kernels_over_own_upload=round(full / h2d_packed, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bs", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--gts", type=int, nargs="+", default=[7, 50])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    dev = torch.device("cuda:0")
    for bs in a.bs:
        for gts in a.gts:
            for name, pipe in (("train", TRAIN), ("val", VAL)):
                print(json.dumps(run(name, pipe, bs, gts, a.reps, dev)), flush=True)


if __name__ == "__main__":
    main()
