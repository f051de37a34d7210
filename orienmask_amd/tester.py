"""The reference's evaluation / inference loops on the HIP path.

``Tester.test`` mirrors /root/reference/trainer/tester.py:26-62 (what is timed, under which names, and how
fps is derived: 1000 * batch_size / mean batch ms); ``infer_loop`` mirrors the timed part of
/root/reference/infer.py:124-188 (10 warm-up iterations, 'Load data' / 'Forward & Postprocess' timers).
COCO metric computation (pycocotools) is outside the path; ``on_batch`` receives each batch's detections so
a caller can plug it in.  Batches come from any iterable yielding ``(image[B,3,H,W], ..., batch_info)``
tuples, e.g. ``SyntheticLoader``.
"""
import torch

from . import timer as _timer
from .dist import shard_range, world_info


class SyntheticLoader:
    """Deterministic stand-in for the COCO loader: n_images 544x544 images in batches (no dataset offline)."""

    def __init__(self, n_images, batch_size, size=(544, 544), seed=0, device="cuda"):
        from . import synth
        self.batch_size = batch_size
        rank, world = world_info()
        start, stop = shard_range(n_images, rank, world)            # each rank evaluates its own slice
        self._batches = []
        import torch
        for i, s in enumerate(range(start, stop, batch_size)):
            n = min(batch_size, stop - s)
            # one seed per IMAGE id: the images do not depend on the world size or on where a rank's batches begin, so the
            # shards of a sharded run are exactly the unsharded set (tests/test_dist_cpu.py compares every image)
            img = torch.cat([synth.synth_image_batch(seed + s + k, 1, size[0], size[1]) for k in range(n)], 0)
            info = [dict(id=s + k, height=size[0], width=size[1]) for k in range(n)]
            self._batches.append((img, None, info))
        self.device = device

    def __len__(self):
        return len(self._batches)

    def __iter__(self):
        return iter(self._batches)


class Tester:
    def __init__(self, model, postprocess, test_loader, device, on_batch=None):
        self.model = model
        self.postprocess = postprocess
        self.test_loader = test_loader
        self.device = device
        self.on_batch = on_batch

    def test(self, verbose=True, in_flight=1):
        """in_flight = 1: the reference's loop and timers.  in_flight > 1: the same batches through
        pipeline.InFlightPipeline (forward + postprocess of consecutive batches overlap on alternating HIP streams, so the two
        stages cannot be timed apart): one 'Forward & Postprocess' figure, wall time of the loop over its images; detections
        reach `on_batch` in the same order."""
        if in_flight > 1:
            return self._test_in_flight(verbose, in_flight)
        _timer.reset()
        _timer.cpu() if str(self.device) == "cpu" else _timer.cuda()
        self.model.eval()
        n_det = 0
        with torch.no_grad():
            for sample in self.test_loader:
                image = sample[0].to(self.device)
                batch_info = sample[2]
                with _timer.timer("Network Forward"):
                    predict = self.model(image)
                with _timer.timer("Postprocess"):
                    detections = self.postprocess(predict)
                n_det += sum(int(d["bbox"].shape[0]) for d in detections)
                if self.on_batch is not None:
                    with _timer.timer("Convert Format"):
                        self.on_batch(batch_info, detections)
        log = _timer.get_all_elapsed_time()
        bs = self.test_loader.batch_size
        stats = {k: dict(ms_per_image=v / bs, fps=1000.0 * bs / v) for k, v in log.items()}
        if verbose:
            print("Speed Statistics (batch size = {})".format(bs))
            for k, v in log.items():
                print("%s: %.3fms (%.3ffps)" % (k, v / bs, 1000 * bs / v))
        stats["detections"] = n_det
        return stats


    def test_and_gather(self, verbose=True, in_flight=1):
        """The multi-GPU form of `test`: every rank evaluates ITS slice of the loader (SyntheticLoader and
        tools/eval_val2017.py's Val2017Loader take contiguous slices by dist.shard_range) and whatever `on_batch` RETURNS per
        batch (a record or a list of records, any picklable objects) is merged in rank order on every rank -- rank-order
        concatenation of contiguous slices is dataset order.  This is /root/reference/trainer/trainer.py:175-181,201-205 (each
        rank writes _temp_coco_eval_<rank>.json, rank 0 concatenates them) without the files.  No collective in the step: one
        all_gather_object of host lists at the end.  Returns (this rank's stats, the merged records)."""
        from .dist import gather_detections
        records = []
        user = self.on_batch

        def collect(batch_info, detections):
            r = user(batch_info, detections) if user is not None else None
            if r is not None:
                records.extend(r if isinstance(r, list) else [r])

        self.on_batch = collect
        try:
            stats = self.test(verbose=verbose, in_flight=in_flight)
        finally:
            self.on_batch = user
        return stats, gather_detections(records)

    def _test_in_flight(self, verbose, depth):
        import time
        from .pipeline import InFlightPipeline
        self.model.eval()
        pipe = InFlightPipeline(self.model, self.postprocess, depth=depth)
        infos, n_det, n_img = [], 0, 0
        convert_ms = 0.0

        def batches():
            for sample in self.test_loader:
                infos.append(sample[2])
                yield sample[0].to(self.device)

        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for i, detections in enumerate(pipe.map(batches())):
            n_det += sum(int(d["bbox"].shape[0]) for d in detections)
            n_img += len(detections)
            if self.on_batch is not None:
                c0 = time.perf_counter()
                self.on_batch(infos[i], detections)
                convert_ms += (time.perf_counter() - c0) * 1e3
        torch.cuda.synchronize(self.device)
        total_ms = (time.perf_counter() - t0) * 1e3 - convert_ms
        stats = {"Forward & Postprocess": dict(ms_per_image=total_ms / max(n_img, 1), fps=1000.0 * n_img / total_ms)}
        if self.on_batch is not None:
            stats["Convert Format"] = dict(ms_per_image=convert_ms / max(n_img, 1), fps=1000.0 * n_img / max(convert_ms, 1e-9))
        if verbose:
            print("Speed Statistics (batch size = {}, {} batches in flight)".format(self.test_loader.batch_size, depth))
            for k, v in stats.items():
                print("%s: %.3fms (%.3ffps)" % (k, v["ms_per_image"], v["fps"]))
        stats["detections"] = n_det
        return stats


def infer_loop(model, transform, postprocess, images, device, warmup=10, size_divisor=32, use_graph=True, latency_mode=True,
               visualizer=None, batch_size=1, channel_order="rgb", decoder=None):
    """images: list of [h,w,3] float32 tensors (what cv2.imread + cvtColor give infer.py).
    Returns (list of per-image detections, list of pad_info, timer log in ms).

    batch_size > 1 (or channel_order='bgr'): consecutive groups of batch_size images go through transform.batch -- the images
    may then be uint8 or float32, of different sizes, numpy arrays or tensors on the host or the device, in RGB or (cv2.imread's)
    BGR order: one staging copy and one preprocess launch per group, timed as 'Load data' -- and then through the network and
    the postprocess as ONE batch ('Forward & Postprocess').  The last, shorter group is a second input shape (a second graph).
    Detections and pad_infos come back per image in input order; the visualizer gets each image as float32 RGB, derived on the
    device from the staged source.  The model's latency setting is left alone for batch_size > 1: it is a one-image device.

    decoder (a jpeg.JpegDecoder): `images` are then JPEG files -- paths or bytes -- and every group is decoded on the device
    (decoder.decode: host entropy decoding, HIP IDCT and colour) in front of transform.batch, all of it timed as 'Load data'; the
    loop goes through the batched path at any batch_size, in RGB order.  The detections are those of the same images decoded by
    PIL: the pixels are (tests/test_jpeg.py).

    visualizer (infer.py -v, :166-172): called as visualizer(detections, image on the device, pad_info) after each image's
    forward + postprocess and timed as 'Visualize'; the loop then returns a fourth element, the list of what it returned (for
    visualizer.InferenceVisualizer, uint8 [h,w,3] numpy images).

    use_graph (default): forward + postprocess of every network input SHAPE that occurs run as one captured hipGraph
    (graph.GraphedPipeline: ~95 kernel launches become one graph launch; bit-identical detections, tests/test_hip_parity.py::
    test_tester_and_infer_loops); a postprocess built for one image size only sees that size (infer.py resizes to 544 x 544
    first), other shapes fall back to eager launches.  Detections of a graphed call are views of graph-owned buffers that the
    next call overwrites, so they are cloned here (the reference returns fresh tensors).

    latency_mode (default): this is the reference's ONE-IMAGE loop (infer.py:143-172), so the model's latency mode is on while
    it runs (model.set_latency_mode: direct 3x3 convolutions instead of the fused Winograd kernel for a batch this small) and
    restored afterwards."""
    _timer.reset()
    _timer.cuda()
    model.eval()
    results, pads, shows = [], [], []
    graphs = {}
    restore = None
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("infer_loop: batch_size must be at least 1, got %d" % batch_size)
    if decoder is not None and channel_order != "rgb":
        raise ValueError("infer_loop: a decoder gives RGB images; channel_order must be 'rgb'")
    through_batch = batch_size > 1 or channel_order != "rgb" or decoder is not None
    if (latency_mode and batch_size == 1 and getattr(model, "precision", None) == "f32_split"
            and hasattr(model, "set_latency_mode")):
        restore = model.latency_cells
        model.set_latency_mode(True)
    # Only this package's postprocess with its own NMS can be captured: capture needs the kernel-only `launch` / `collect` split
    # and its workspace, and a foreign nms_func runs on the host in the middle of the step (a synchronisation, which stream
    # capture refuses).  Any other callable -- the reference's contract is just `postprocess(model(x))` -- runs eagerly.
    graphable = (use_graph and all(hasattr(postprocess, a) for a in ("launch", "collect", "_ws"))
                 and getattr(postprocess, "nms_thresh", None) is not None)

    def run(x):
        if not graphable:
            return postprocess(model(x))
        key = tuple(x.shape)
        if key not in graphs:
            from .graph import GraphedPipeline
            g = None
            if len(graphs) < 4:      # a handful of shapes at most
                try:
                    g = GraphedPipeline(model, postprocess, x)
                except RuntimeError as e:      # a capture that failed leaves nothing behind: this shape runs eagerly
                    import warnings
                    warnings.warn("infer_loop: hipGraph capture failed for input shape %s (%s); running it eagerly" % (key, e))
            graphs[key] = g
        g = graphs[key]
        if g is None:
            return postprocess(model(x))
        return [{k: v.clone() for k, v in d.items()} for d in g(x)]

    def batched():
        def load(group):
            if decoder is not None:
                group = decoder.decode(group)
            return transform._batch(group, size_divisor, 0, channel_order, device)

        if warmup and images:
            x = load(images[:batch_size])[0]
            for _ in range(warmup):
                run(x)
        with _timer.timer("Main Loop"):
            for s in range(0, len(images), batch_size):
                with _timer.timer("Load data"):
                    x, pad_infos, sources = load(images[s:s + batch_size])
                with _timer.timer("Forward & Postprocess"):
                    det = run(x)
                results.extend(det)
                pads.extend(pad_infos)
                if visualizer is not None:
                    for d, src, pad_info in zip(det, sources, pad_infos):
                        with _timer.timer("Visualize"):
                            # the visualiser's contract is a float32 RGB image on the device: derived there from the staged source
                            src = src.to(torch.float32)
                            shows.append(visualizer(d, src.flip(-1) if channel_order == "bgr" else src, pad_info))

    def single():
        if warmup and images:
            x, _ = transform.padded(images[0].to(device).unsqueeze(0), size_divisor)
            for _ in range(warmup):
                run(x)
        with _timer.timer("Main Loop"):
            for img in images:
                with _timer.timer("Load data"):
                    src = img.to(device)
                    x, pad_info = transform.padded(src.unsqueeze(0), size_divisor)
                with _timer.timer("Forward & Postprocess"):
                    det = run(x)
                results.append(det[0])
                pads.append(pad_info)
                if visualizer is not None:
                    with _timer.timer("Visualize"):
                        shows.append(visualizer(det[0], src, pad_info))

    try:
        with torch.no_grad():
            batched() if through_batch else single()
    finally:
        if restore is not None:
            model.set_latency_mode(restore > 0, restore or None)
    if visualizer is not None:
        return results, pads, _timer.get_all_elapsed_time(), shows
    return results, pads, _timer.get_all_elapsed_time()


class SyntheticLossLoader:
    """SyntheticLoader with targets: yields (image[B,3,H,W], (gt_bbox, gt_cls, gt_index, gt_mask), batch_info) as the reference's
    collate does (the reference's data/collate.py:13-30), with seeded boxes, classes and filled-polygon masks
    (synth.synth_targets).  Everything is made once, on `device`."""

    def __init__(self, n_images, batch_size, size=(544, 544), seed=0, gts_per_image=7, num_classes=80, device="cuda"):
        from . import synth
        self.batch_size = batch_size
        self._batches = []
        for s in range(0, n_images, batch_size):
            n = min(batch_size, n_images - s)
            img = torch.cat([synth.synth_image_batch(seed + s + k, 1, size[0], size[1]) for k in range(n)], 0)
            gb, gc, gi, gm = synth.synth_targets(seed + 7919 + s, n, size[0], size[1], gts_per_image, num_classes)
            target = tuple(torch.from_numpy(a).to(device) for a in (gb, gc, gi, gm))
            info = [dict(id=s + k, height=size[0], width=size[1]) for k in range(n)]
            self._batches.append((img.to(device), target, info))

    def __len__(self):
        return len(self._batches)

    def __iter__(self):
        return iter(self._batches)


def _model_device(model):
    for p in model.parameters():
        return p.device
    return torch.device("cuda", torch.cuda.current_device())


def validate(model, loss, postprocess, loader, coco_metrics=None, counter=None, group=None):
    """Trainer._val_epoch (the reference's trainer/trainer.py:135-209) for ONE rank: forward, loss(training=False), and -- when a
    cocoeval.COCOMetrics is given -- postprocess, to_coco_format / update_results and coco_eval.  The image and the targets
    are moved to the device of the model's parameters, as _val_epoch moves them to the trainer's.  Returns its val_log:
    val_loss, val_<loss_id>, val_<metric_id> (EvalCounter epoch averages) and val_<coco key>.  The tensorboard writes are left
    out.  Without coco_metrics the postprocess is not run (its output would go nowhere).

    Without `counter` the counters and COCO results of several ranks (the reference's _temp_counter_*.pth /
    _temp_coco_eval_*.json exchange) are not merged.  With `counter` (a loss.DeviceEvalCounter of `loss` on the model's device;
    it is reset) the loop is the deferred one -- ``loss.enqueue`` per batch, no device-to-host copy of the loss values, ONE read
    of the counter at the end -- and the ranks of `group` (None: the default process group, when there is one) merge: the
    counters by ``counter.gather`` (rank order), the COCO results in rank order as dist.gather_detections merges them; every
    rank returns the merged val_log."""
    from .loss import EvalCounter
    if counter is not None:
        return _validate_deferred(model, loss, postprocess, loader, coco_metrics, counter, group)
    if coco_metrics is not None:
        coco_metrics.reset()
    counter = EvalCounter()
    dev = _model_device(model)
    with torch.no_grad():
        for sample in loader:
            # trainer.py:152-154: the image and every label tensor to the model's device (collate yields CPU tensors)
            image = sample[0].to(dev)
            target = [anno.to(dev) for anno in sample[1]]
            batch_info = sample[2]
            predict = model(image)
            loss_v, loss_log, metric_log = loss(predict, target, training=False)
            if coco_metrics is not None:
                detections = postprocess(predict)
                coco_metrics.update_results(coco_metrics.to_coco_format(batch_info, detections))
            counter.update("loss", loss_v.item())
            for key, value in loss_log.items():
                counter.update(key, value)
            for key, value in metric_log.items():
                counter.update(key, value)
    val_log = {"val_loss": counter.average_epoch("loss")}
    for key in loss.loss_id:
        val_log["val_%s" % key] = counter.average_epoch(key)
    for key in loss.metric_id:
        val_log["val_%s" % key] = counter.average_epoch(key)
    if coco_metrics is not None:
        for key, value in coco_metrics.coco_eval().items():
            val_log["val_%s" % key] = value
    counter.reset_epoch()
    return val_log


def _validate_deferred(model, loss, postprocess, loader, coco_metrics, counter, group):
    import torch.distributed as dist
    from .dist import gather_detections
    if coco_metrics is not None:
        coco_metrics.reset()
    counter.reset_epoch()
    dev = _model_device(model)
    with torch.no_grad():
        for step, sample in enumerate(loader, 1):
            image = sample[0].to(dev)
            target = [anno.to(dev) for anno in sample[1]]
            predict = model(image)
            loss.enqueue(predict, target, counter, step, training=False)
            if coco_metrics is not None:
                coco_metrics.update_results(coco_metrics.to_coco_format(sample[2], postprocess(predict)))
    many = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    if many:
        counter.gather(group)
    means = counter.averages_epoch()
    val_log = {"val_loss": means["loss"]}
    for key in list(loss.loss_id) + list(loss.metric_id):
        val_log["val_%s" % key] = means[key]
    if coco_metrics is not None:
        if many:
            mine = [dict(bbox=coco_metrics.bbox_results, segm=coco_metrics.segm_results)]
            if group is None:
                parts = gather_detections(mine)
            else:
                parts = [None] * dist.get_world_size(group)
                dist.all_gather_object(parts, mine, group=group)
                parts = [d for part in parts for d in part]
            coco_metrics.bbox_results = [r for part in parts for r in part["bbox"]]
            coco_metrics.segm_results = [r for part in parts for r in part["segm"]]
        for key, value in coco_metrics.coco_eval().items():
            val_log["val_%s" % key] = value
    counter.reset_epoch()
    return val_log
