"""What decoding JPEG on the device (orienmask_amd.jpeg.JpegDecoder) gains over decoding on the host, from FILES to the network input.

    python tools/bench_jpeg.py [--repeats 15] [--warmup 3] [--threads 16] [--loop-images 256] [--no-loop]

Workload: 32 synthetic 480 x 640 photos (smooth seeded structure plus fine noise) written by PIL as 4:2:0 quality-90 JPEG files
-> [32,3,544,544].  Needs PIL to make the inputs (and as the path it is compared with).
  (new)    files -> JpegDecoder.decode (host entropy decoding on --threads threads, one staging copy, HIP IDCT + colour)
           -> FastCOCOTransform.batch of device-resident images
  (parent) files -> PIL Image.open(...).convert('RGB') on the same number of threads -> FastCOCOTransform.batch of host uint8
The two alternate in one run after warm-up; each repeat is a host clock that ends in a synchronise (what the caller waits);
median and range.  The results are compared first: they must be identical.
Then: host entropy decoding alone and PIL's full decode alone, ONE thread, MB of JPEG per second; the device kernels alone by
events (coefficients already on the device) and the bytes they move -- coefficients and tables read, planes written and read,
RGB written -- as a fraction of what a device-to-device copy of as many bytes reaches in the same run; infer_loop(batch_size=32)
from files both ways, images/s (the parent way: PIL decoding of each group on the threads, then the loop's own batch).
One JSON line per section."""
import argparse
import concurrent.futures
import ctypes
import io
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from orienmask_amd import jpeg as omjpeg, lib as omlib, synth  # noqa: E402
from orienmask_amd.transform import FastCOCOTransform as T  # noqa: E402

N, H_SRC, W_SRC, SIZE = 32, 480, 640, 544
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def photo(seed):
    """[480,640,3] uint8: low-frequency colour structure (a 15 x 20 seeded grid, bicubic) under fine noise -- a stream of the
    size a camera JPEG of this resolution has, not the incompressible one plain noise gives."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    coarse = Image.fromarray(rng.integers(0, 256, (15, 20, 3), dtype=np.uint8)).resize((W_SRC, H_SRC), Image.BICUBIC)
    fine = rng.normal(0.0, 6.0, (H_SRC, W_SRC, 3))
    return np.clip(np.asarray(coarse, dtype=np.float64) + fine, 0, 255).astype(np.uint8)


def spread(values, digits=3):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits))


def host_ms(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--loop-images", type=int, default=256)
    ap.add_argument("--no-loop", action="store_true", help="skip the infer_loop section (it builds the model)")
    a = ap.parse_args()
    from PIL import Image
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py needs an MI355X")
    dev = torch.device("cuda:0")
    threads = max(1, min(a.threads, omjpeg.MAX_THREADS))
    tmp = tempfile.TemporaryDirectory()
    paths = []
    for i in range(N):
        paths.append(os.path.join(tmp.name, "%02d.jpg" % i))
        Image.fromarray(photo(8000 + i)).save(paths[-1], "JPEG", quality=90, subsampling=2)
    sizes = [os.path.getsize(p) for p in paths]
    tf = T([T.Resize((SIZE, SIZE)), T.Normalize(MEAN, STD)])
    decoder = omjpeg.JpegDecoder(dev, threads=threads, on_unsupported="raise")
    pool = concurrent.futures.ThreadPoolExecutor(threads)

    def pil_read(path):
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)

    def path_new(group=paths):
        return tf.batch(decoder.decode(group), 32)[0]

    def path_parent(group=paths):
        return tf.batch(list(pool.map(pil_read, group)), 32, device=dev)[0]

    if not torch.equal(path_new(), path_parent()):
        raise SystemExit("bench_jpeg.py: the two paths disagree")
    for _ in range(a.warmup):
        path_new(); path_parent()
    tn, tp = [], []
    for _ in range(a.repeats):
        tn.append(host_ms(path_new, dev))
        tp.append(host_ms(path_parent, dev))
    out = dict(section="files_to_network_input", images=N, source="%dx%d 4:2:0 quality 90" % (H_SRC, W_SRC), threads=threads,
               jpeg_bytes=dict(total=sum(sizes), min=min(sizes), max=max(sizes)), output=[N, 3, SIZE, SIZE], repeats=a.repeats,
               identical=True, device_decode_ms=spread(tn), pil_decode_ms=spread(tp))
    out["speedup_median"] = round(out["pil_decode_ms"]["median"] / out["device_decode_ms"]["median"], 2)
    print(json.dumps(out), flush=True)

    # ---- one thread: the host's share of the new path beside PIL's full decode
    datas = [open(p, "rb").read() for p in paths]
    infos = [omjpeg.host_info(d) for d in datas]
    p = omjpeg.plan(infos)
    stage = np.zeros(p.stage_bytes, np.uint8)
    coef_all, quant_all = stage[:p.quant_stage_off].view(np.int16), stage[p.quant_stage_off:].view(np.uint16)

    def entropy_all():
        for k, d in enumerate(datas):
            end = p.coef_off[k + 1] if k + 1 < N else p.coef_elems
            omjpeg.host_entropy_decode(d, coef_all[p.coef_off[k]:end], quant_all[p.quant_off[k]:p.quant_off[k] + 192])

    def pil_all():
        for d in datas:
            with Image.open(io.BytesIO(d)) as im:
                np.asarray(im.convert("RGB"))

    te, tl = [], []
    for r in range(a.warmup + a.repeats):
        t0 = time.perf_counter(); entropy_all(); t1 = time.perf_counter(); pil_all(); t2 = time.perf_counter()
        if r >= a.warmup:
            te.append(t1 - t0); tl.append(t2 - t1)
    mb = sum(sizes) / 1e6
    print(json.dumps(dict(section="one_host_thread", jpeg_megabytes=round(mb, 3),
                          entropy_decode_mb_per_s=spread([mb / t for t in te], 1), entropy_decode_images_per_s=spread([N / t for t in te], 1),
                          pil_full_decode_mb_per_s=spread([mb / t for t in tl], 1), pil_full_decode_images_per_s=spread([N / t for t in tl], 1))),
          flush=True)

    # ---- the kernels alone, and a copy of as many bytes
    staged = torch.from_numpy(stage).to(dev)
    coef, quant = staged[:p.quant_stage_off], staged[p.quant_stage_off:]
    desc = p.desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    ws_bytes = omlib.workspace_bytes("om_jpeg_workspace_bytes", desc, N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rgb = torch.empty(p.out_bytes, dtype=torch.uint8, device=dev)
    moved = 2 * p.coef_elems + 2 * p.quant_elems + 2 * ws_bytes + N * H_SRC * W_SRC * 3      # read coef + tables, write + read planes, write RGB
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def kernels():
        omlib.launch("om_jpeg_decode_batch", dev, desc, N, coef, p.coef_elems, quant, p.quant_elems, ws, ws_bytes, rgb, p.out_bytes)

    tk, tc = [], []
    for r in range(a.warmup + a.repeats):
        k, c = events(kernels), events(lambda: dst.copy_(src))
        if r >= a.warmup:
            tk.append(k); tc.append(c)
    kern, copy = spread(tk, 4), spread(tc, 4)
    print(json.dumps(dict(section="device_kernels", note="events around the 4 launches of 32 images; the copy reads and writes `bytes_moved` in all",
                          launches=2 * ((N + omlib.OM_JPEG_BATCH - 1) // omlib.OM_JPEG_BATCH), bytes_moved=moved, kernels_ms=kern, copy_ms=copy,
                          kernels_gb_per_s=round(moved / kern["median"] / 1e6, 1), copy_gb_per_s=round(moved / copy["median"] / 1e6, 1),
                          fraction_of_copy_rate=round(copy["median"] / kern["median"], 3))), flush=True)
    if a.no_loop:
        return

    # ---- infer_loop from files
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
    many = [paths[i % N] for i in range(a.loop_images)]

    class PilDecoder:
        """The parent commit's way from files, in the place the loop decodes: PIL on the thread pool."""

        def decode(self, group):
            return list(pool.map(pil_read, group))

    loops = {}
    for rep in range(3):                                   # alternating; the spread of the three is reported
        for name, dec in (("device_decode", decoder), ("pil_decode", PilDecoder())):
            dets, _, log = infer_loop(net, tf, post, many, dev, warmup=10, batch_size=32, decoder=dec)
            assert len(dets) == a.loop_images
            loops.setdefault(name, []).append(dict(images_per_s=1000.0 * a.loop_images / log["Main Loop"], load_ms=log["Load data"],
                                                   forward_post_ms=log["Forward & Postprocess"]))
    print(json.dumps(dict(section="infer_loop_from_files", images=a.loop_images, batch_size=32, precision=DEFAULT_PRECISION, threads=threads,
                          **{k: dict(images_per_s=spread([r["images_per_s"] for r in v], 1),
                                     load_data_ms_per_step=spread([r["load_ms"] for r in v]),
                                     forward_postprocess_ms_per_step=spread([r["forward_post_ms"] for r in v]))
                             for k, v in loops.items()})), flush=True)
    pool.shutdown()
    tmp.cleanup()


if __name__ == "__main__":
    main()
