"""What the batched uint8 front door (FastCOCOTransform.batch, om_preprocess_batch) gains over the one-image float path.

    python tools/bench_preprocess.py [--repeats 20] [--warmup 3] [--loop-images 256] [--no-loop]
    python tools/bench_preprocess.py --kernels-only 50        # under a kernel tracer: the two kernels' own times

Workload: 32 uint8 BGR 480 x 640 host images (seeded synthetic photos, synth.synth_photo_batch) -> [32,3,544,544].
  (a) per image, what infer_loop does with such a decoded frame without `batch`: host conversion to float32 RGB, its own
      host-to-device copy (12 bytes per pixel), FastCOCOTransform.padded (om_preprocess, one launch)
  (b) FastCOCOTransform.batch(images, channel_order='bgr'): one packed copy of 3 bytes per pixel, two launches of 16 images
(a) and (b) alternate in one run after warm-up; each repeat is timed twice over, by device events around the work (the copies
and kernels as the stream saw them) and by a host clock that ends in a synchronise (what the caller waits); median and range
of the repeats are reported.  `resident` is the same alternation with the images already on the device ((a) as float32 RGB,
(b) as uint8 BGR), events only: the launches alone, kernel time plus whatever gaps the host leaves between 32 launches.  The
kernels' own times come from a tracer over --kernels-only (preprocess_kernel: 32 calls per repeat, preprocess_batch_kernel:
2 calls per repeat).

Then infer_loop over --loop-images such images (the 32, repeated) with synthetic weights: batch_size 1 (float32 RGB host
tensors, converted beforehand: the conversion is NOT in its figure) and batch_size 32 (the uint8 BGR arrays), images/s from the
loop's 'Main Loop' timer.  One JSON line per section."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from orienmask_amd import synth  # noqa: E402
from orienmask_amd.transform import FastCOCOTransform as T  # noqa: E402

N, H_SRC, W_SRC, SIZE = 32, 480, 640, 544
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def photos_bgr_u8(n=N):
    return [np.ascontiguousarray(synth.synth_photo_batch(7000 + i, 1, H_SRC, W_SRC)[0].numpy().astype(np.uint8)[:, :, ::-1])
            for i in range(n)]


def to_float_rgb(bgr):
    """The host conversion in front of the float path: cv2.cvtColor(BGR2RGB) + float32, in numpy."""
    return torch.from_numpy(np.ascontiguousarray(bgr[:, :, ::-1]).astype(np.float32))


def spread(values):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def timed(fn, dev):
    """(device ms by events, host ms ending in a synchronise) of one call of fn."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def alternate(fa, fb, dev, repeats, warmup):
    for _ in range(warmup):
        fa(); fb()
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(fa, dev))
        b.append(timed(fb, dev))
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-images", type=int, default=256)
    ap.add_argument("--no-loop", action="store_true", help="skip the infer_loop section (it builds the model)")
    ap.add_argument("--kernels-only", type=int, default=0, metavar="R",
                    help="R alternating repeats of the two resident forms and nothing else: the run to put under a kernel tracer")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess.py needs an MI355X")
    dev = torch.device("cuda:0")
    tf = T([T.Resize((SIZE, SIZE)), T.Normalize(MEAN, STD)])
    bgr = photos_bgr_u8()
    res_f32 = [to_float_rgb(im).to(dev) for im in bgr]
    res_u8 = [torch.from_numpy(im).to(dev) for im in bgr]

    def path_a():
        return [tf.padded(to_float_rgb(im).to(dev).unsqueeze(0), 32)[0] for im in bgr]

    def path_b():
        return tf.batch(bgr, 32, channel_order="bgr", device=dev)[0]

    def resident_a():
        return [tf.padded(im.unsqueeze(0), 32)[0] for im in res_f32]

    def resident_b():
        return tf.batch(res_u8, 32, channel_order="bgr")[0]

    same = torch.equal(torch.cat(path_a(), 0), path_b()) and torch.equal(torch.cat(resident_a(), 0), resident_b())
    if not same:
        raise SystemExit("bench_preprocess.py: the two paths disagree")
    if a.kernels_only:
        alternate(resident_a, resident_b, dev, a.kernels_only, a.warmup)
        print(json.dumps(dict(section="kernels_only", repeats=a.kernels_only, warmup=a.warmup, launches_per_repeat=dict(
            preprocess_kernel=N, preprocess_batch_kernel=2))), flush=True)
        return
    ta, tb = alternate(path_a, path_b, dev, a.repeats, a.warmup)
    out = dict(section="host_images", images=N, source="uint8 BGR %dx%d" % (H_SRC, W_SRC), output=[N, 3, SIZE, SIZE],
               repeats=a.repeats, identical=same,
               per_image_float_path=dict(device_ms=spread([t[0] for t in ta]), host_ms=spread([t[1] for t in ta]),
                                         h2d_bytes=N * H_SRC * W_SRC * 12, copies=N, launches=N),
               batch=dict(device_ms=spread([t[0] for t in tb]), host_ms=spread([t[1] for t in tb]),
                          h2d_bytes=N * H_SRC * W_SRC * 3, copies=1, launches=2))
    out["speedup_host_ms_median"] = round(out["per_image_float_path"]["host_ms"]["median"] / out["batch"]["host_ms"]["median"], 2)
    print(json.dumps(out), flush=True)
    ra, rb = alternate(resident_a, resident_b, dev, a.repeats, a.warmup)
    print(json.dumps(dict(section="resident", note="events around the launches alone: kernel time plus launch gaps",
                          float32_32_launches_ms=spread([t[0] for t in ra]), uint8_batch_2_launches_ms=spread([t[0] for t in rb]))),
          flush=True)
    if a.no_loop:
        return
    from orienmask_amd.eval import OrienMaskYOLOPostProcess
    from orienmask_amd.model import DEFAULT_PRECISION, OrienMaskYOLOFPNPlus
    from orienmask_amd.tester import infer_loop
    net = OrienMaskYOLOFPNPlus(3, 80).eval().set_precision(DEFAULT_PRECISION)
    net.load_state_dict(synth.synth_state_dict(3, obj_bias=-16.0, head_gain=4.0), strict=True)
    net = net.to(dev)
    anchors = [[12, 16], [19, 36], [40, 28], [36, 75], [76, 55], [72, 146], [142, 110], [192, 243], [459, 401]]
    post = OrienMaskYOLOPostProcess(device=dev, grid_size=[[SIZE // 32] * 2, [SIZE // 16] * 2, [SIZE // 8] * 2], image_size=[SIZE, SIZE],
                                    anchors=anchors, anchor_mask=[[6, 7, 8], [3, 4, 5], [0, 1, 2]], num_classes=80, conf_thresh=0.005,
                                    nms_pre=400, nms_post=100, orien_thresh=0.3)
    many_u8 = [bgr[i % N] for i in range(a.loop_images)]
    floats = [to_float_rgb(im) for im in bgr]
    many_f32 = [floats[i % N] for i in range(a.loop_images)]
    loops = {}
    for rep in range(3):                                   # alternating; the spread of the three is reported
        for name, images, kw in (("batch_size_1", many_f32, dict(batch_size=1)),
                                 ("batch_size_32", many_u8, dict(batch_size=32, channel_order="bgr"))):
            dets, _, log = infer_loop(net, tf, post, images, dev, warmup=10, **kw)
            assert len(dets) == a.loop_images
            loops.setdefault(name, []).append(dict(images_per_s=1000.0 * a.loop_images / log["Main Loop"],
                                                   load_ms=log["Load data"], forward_post_ms=log["Forward & Postprocess"]))
    print(json.dumps(dict(section="infer_loop", images=a.loop_images, precision=DEFAULT_PRECISION,
                          **{k: dict(images_per_s=spread([r["images_per_s"] for r in v]),
                                     load_data_ms_per_step=spread([r["load_ms"] for r in v]),
                                     forward_postprocess_ms_per_step=spread([r["forward_post_ms"] for r in v]))
                             for k, v in loops.items()})), flush=True)


if __name__ == "__main__":
    main()
