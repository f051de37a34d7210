"""Drop-in for the reference's GPU preprocessing and, from augment.py, its training / validation
data pipeline (COCOTransform, collate, to_device, device_batches: SURVEY.md row 14) and, from dataset.py, the datasets that feed it
(BaseDataset, COCODataset, VOCDataset; DataLoader is torch's): what trainer/builder.py:91-105 resolves against its data module.

  FastCOCOTransform(pipeline, use_cuda)   /root/reference/data/transform.py:444-510
  pad(image, size_divisor=32, pad_value=0) /root/reference/infer.py:21-32
  build_transform(config)                  /root/reference/trainer/builder.py:108-115

The reference's pipeline objects (Resize / ShortEdgeResize / Normalize) are kept as plain
parameter holders with the same constructor arguments; ``FastCOCOTransform.__call__`` runs the
whole pipeline as ONE HIP kernel (``om_preprocess``): HWC read once, resized + normalised NCHW
written once.  ``padded(image)`` additionally fuses ``pad`` into the same kernel and returns
``(image, pad_info)`` like ``infer.pad`` does.  ``batch(images)`` is the same for a LIST of images of their own
sizes, uint8 or float32, on the host or the device (``om_preprocess_batch``): one staging copy, one launch
per 16 images, every image centred in the common padded size.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from .augment import COCOTransform, collate, device_batches, to_device  # noqa: F401  (build_transform resolves names here)
from .dataset import BaseDataset, COCODataset, VOCDataset  # noqa: F401  (build(dataset_config, module) resolves names here)
from torch.utils.data import DataLoader  # noqa: F401  (as the reference's data/__init__.py exports it)


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


# ---- the batched form (om_preprocess_batch): images of their own sizes and element types ------------------------------------
STAGE_RING = 3          # pinned staging buffers per transform: a call fills one while the copies of the two before it may be pending
PlanRow = collections.namedtuple("PlanRow", "rh rw top left pad_info")


def _as_image(image, i):
    """Image i of a batch() call as it is packed: a numpy array or a tensor, [h,w,3] uint8 or float32 (nothing is copied)."""
    if not isinstance(image, (torch.Tensor, np.ndarray)):
        raise TypeError("image %d: a torch tensor or a numpy array is needed, got %s" % (i, type(image).__name__))
    kind = image.dtype if isinstance(image, torch.Tensor) else {np.dtype(np.uint8): torch.uint8,
                                                                np.dtype(np.float32): torch.float32}.get(image.dtype)
    if kind not in (torch.uint8, torch.float32):
        raise TypeError("image %d: uint8 or float32 is needed, got %s" % (i, image.dtype))
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("image %d: must be [h,w,3], got %s" % (i, tuple(image.shape)))
    return image


def _elem_size(image):
    return 1 if image.dtype == (torch.uint8 if isinstance(image, torch.Tensor) else np.uint8) else 4


def stage_layout(items):
    """Where the host images of one call lie in the staging buffer: items = (h, w, elem) per image, elem 1 (uint8) or 4
    (float32) bytes -> (offsets, total bytes).  Back to back in input order; a float32 image begins at the next multiple of 4
    (the kernel reads it with 4-byte loads), a uint8 image at the very next byte."""
    offsets, off = [], 0
    for h, w, elem in items:
        off = (off + elem - 1) // elem * elem
        offsets.append(off)
        off += int(h) * int(w) * 3 * elem
    return offsets, off


def fill_stage(buffer, images, offsets):
    """Copy host `images` (numpy arrays or host tensors, any strides) to their `offsets` of the uint8 host tensor `buffer`."""
    flat = buffer.numpy()
    for image, off in zip(images, offsets):
        h, w = image.shape[:2]
        nbytes = h * w * 3 * _elem_size(image)
        if isinstance(image, torch.Tensor):
            buffer[off:off + nbytes].view(image.dtype).view(h, w, 3).copy_(image)
        else:
            np.copyto(flat[off:off + nbytes].view(image.dtype).reshape(h, w, 3), image)


def geom_rows(shapes, is_u8, rows, channel_order):
    """The int32 [n,8] table of om_preprocess_batch (include/orienmask_hip.h): h, w, resize_h, resize_w, pad_top, pad_left,
    flags, 0 per image, from its (h, w), whether it is uint8, its PlanRow and the call's channel order."""
    geom = np.zeros((len(shapes), 8), dtype=np.int32)
    bgr = _lib.OM_PRE_BGR if channel_order == "bgr" else 0
    for g, (h, w), u8, r in zip(geom, shapes, is_u8, rows):
        g[:7] = (h, w, r.rh, r.rw, r.top, r.left, (_lib.OM_PRE_U8 if u8 else 0) | bgr)
    return geom


class FastCOCOTransform:
    class Resize:
        def __init__(self, size, interpolation="bilinear", align_corners=False):
            assert isinstance(size, int) or len(size) == 2
            if interpolation != "bilinear" or align_corners:
                raise NotImplementedError("the HIP preprocess implements bilinear, align_corners=False")
            self.size = _pair(size)

        def target(self, h, w):
            return self.size

    class ShortEdgeResize:
        def __init__(self, short_length, max_size, interpolation="bilinear", align_corners=False):
            if interpolation != "bilinear" or align_corners:
                raise NotImplementedError("the HIP preprocess implements bilinear, align_corners=False")
            self.short_length = short_length
            self.max_size = max_size

        def target(self, h, w):
            scale = min(self.short_length / min(h, w), self.max_size / max(h, w))
            return int(h * scale + 0.5), int(w * scale + 0.5)

    class Normalize:
        def __init__(self, mean, std):
            self.mean = [float(m) for m in mean]
            self.std = [float(s) for s in std]

    def __init__(self, pipeline, use_cuda=True):
        if not use_cuda:
            raise _lib.OrienMaskHipError("orienmask_amd.FastCOCOTransform runs on the GPU only (no CPU fallback)")
        self.pipeline = list(pipeline)
        self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        resizes = [t for t in self.pipeline if isinstance(t, (self.Resize, self.ShortEdgeResize))]
        norms = [t for t in self.pipeline if isinstance(t, self.Normalize)]
        if len(resizes) > 1 or len(norms) > 1 or len(resizes) + len(norms) != len(self.pipeline):
            raise NotImplementedError("pipeline must be [Resize|ShortEdgeResize]? + [Normalize]?")
        if resizes and norms and self.pipeline.index(resizes[0]) > self.pipeline.index(norms[0]):
            raise NotImplementedError("Normalize before Resize is not fused")
        self._resize = resizes[0] if resizes else None
        self._norm = norms[0] if norms else None

        self._ring = [None] * STAGE_RING          # [pinned uint8 buffer, event recorded behind its last copy] per slot
        self._ring_next = 0

    def _norm_arrays(self):
        mean = (ctypes.c_float * 3)(*(self._norm.mean if self._norm else [0.0] * 3))
        std = (ctypes.c_float * 3)(*(self._norm.std if self._norm else [1.0] * 3))
        return mean, std

    def _launch_batch(self, ptrs, geom, out_h, out_w, pad_value, device):
        """om_preprocess_batch over device pointers `ptrs` and the int32 [n,8] table `geom`: the [n,3,out_h,out_w] result."""
        n = len(ptrs)
        geom = np.ascontiguousarray(geom, dtype=np.int32)
        assert geom.shape == (n, 8)
        mean, std = self._norm_arrays()
        out = torch.empty((n, 3, out_h, out_w), dtype=torch.float32, device=device)
        _lib.launch("om_preprocess_batch", device, (ctypes.c_void_p * n)(*ptrs), geom.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                    n, mean, std, out_h, out_w, float(pad_value), out)
        return out

    def plan_batch(self, shapes, size_divisor=32):
        """Host only.  shapes: (h, w) per image -> (out_h, out_w, rows): every image's target is the pipeline's resize of its own
        size (its own size without one); the output is the largest target in each direction, rounded up to size_divisor (0: as
        it is); every image is centred in it as the reference's collate_plus / infer.pad do, the odd pixel going right and
        down.  rows[i] = PlanRow(rh, rw, top, left, pad_info) with pad_info = [left, right, top, down, out_h, out_w], the
        collate_pad form coco_format and the visualiser undo."""
        if not shapes:
            raise ValueError("plan_batch: no images")
        targets = [tuple(int(v) for v in (self._resize.target(int(h), int(w)) if self._resize else (h, w))) for h, w in shapes]
        oh, ow = max(t[0] for t in targets), max(t[1] for t in targets)
        if size_divisor:
            oh = int(math.ceil(oh / size_divisor) * size_divisor)
            ow = int(math.ceil(ow / size_divisor) * size_divisor)
        rows = []
        for rh, rw in targets:
            left, top = (ow - rw) // 2, (oh - rh) // 2
            rows.append(PlanRow(rh, rw, top, left, [left, ow - rw - left, top, oh - rh - top, oh, ow]))
        return oh, ow, rows

    def _stage_slot(self, nbytes):
        """The next pinned staging buffer of the ring, at least nbytes large and free: the copy that last read it has finished
        (its event).  Pinned memory is allocated only when a slot is first used or has to grow."""
        k = self._ring_next
        self._ring_next = (k + 1) % len(self._ring)
        slot = self._ring[k]
        if slot is not None:
            slot[1].synchronize()
        if slot is None or slot[0].numel() < nbytes:
            size = max(nbytes, 2 * slot[0].numel() if slot is not None else 0, 1 << 16)
            slot = self._ring[k] = [torch.empty(size, dtype=torch.uint8).pin_memory(), torch.cuda.Event()]
        return slot

    def _batch(self, images, size_divisor, pad_value, channel_order, device):
        """batch(), and the staged sources with it: (x, pad_infos, sources), sources[i] the [h,w,3] uint8 or float32 image on
        the device the kernel read (a view of the staged bytes, or the caller's own tensor)."""
        if channel_order not in ("rgb", "bgr"):
            raise ValueError("channel_order must be 'rgb' or 'bgr', got %r" % (channel_order,))
        srcs = [_as_image(im, i) for i, im in enumerate(images)]
        if not srcs:
            raise ValueError("batch: no images")
        resident = [s for s in srcs if isinstance(s, torch.Tensor) and s.is_cuda]
        if device is not None:
            device = torch.device(device)
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
        elif resident:
            device = resident[0].device
        else:
            device = self.device or torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda" or any(s.device != device for s in resident):
            raise _lib.OrienMaskHipError("batch: the images on a device must all be on %s, an MI355X device" % (device,))
        out_h, out_w, rows = self.plan_batch([s.shape[:2] for s in srcs], size_divisor)
        host = [i for i, s in enumerate(srcs) if not (isinstance(s, torch.Tensor) and s.is_cuda)]
        sources = list(srcs)
        with _lib.on_device(device):
            if host:
                offsets, total = stage_layout([tuple(srcs[i].shape[:2]) + (_elem_size(srcs[i]),) for i in host])
                pinned, event = self._stage_slot(total)
                fill_stage(pinned, [srcs[i] for i in host], offsets)
                staged = torch.empty(total, dtype=torch.uint8, device=device)
                staged.copy_(pinned[:total], non_blocking=True)                  # the one host-to-device copy of the call
                event.record(torch.cuda.current_stream(device))
                for i, off in zip(host, offsets):
                    h, w = srcs[i].shape[:2]
                    e = _elem_size(srcs[i])
                    sources[i] = staged[off:off + h * w * 3 * e].view(torch.uint8 if e == 1 else torch.float32).view(h, w, 3)
            sources = [s.contiguous() for s in sources]
            geom = geom_rows([s.shape[:2] for s in sources], [s.dtype == torch.uint8 for s in sources], rows, channel_order)
            x = self._launch_batch([s.data_ptr() for s in sources], geom, out_h, out_w, pad_value, device)
        return x, [r.pad_info for r in rows], sources

    def batch(self, images, size_divisor=32, pad_value=0, channel_order="rgb", device=None):
        """A list of [h,w,3] images of their own sizes, each uint8 or float32, each a numpy array or a tensor on the host or on
        the device -> (x [n,3,H,W], pad_infos): every image resized by the pipeline, normalised and centred in the common padded
        size of plan_batch, in ONE kernel launch per OM_PRE_BATCH images.  channel_order='bgr' (cv2.imread's) swaps the
        channels in the kernel.  The images on the host are packed back to back into one pinned staging buffer (a ring of
        STAGE_RING, each reused only after its copy has finished) and cross in ONE copy on the current stream; images on the
        device are read where they are.  Each plane set has the bits `padded` gives for that image alone as float32 RGB."""
        x, pad_infos, _ = self._batch(images, size_divisor, pad_value, channel_order, device)
        return x, pad_infos

    def _run(self, image, divisor, pad_value):
        if isinstance(image, torch.Tensor) and image.dtype == torch.uint8:
            return self._run_u8(image, divisor, pad_value)
        _lib.require_cuda_tensor(image, "image", torch.float32)
        if image.dim() != 4 or image.shape[3] != 3:
            raise ValueError("image must be [n,h,w,3] float32, got %s" % (tuple(image.shape),))
        image = image.contiguous()
        n, h, w, _ = image.shape
        rh, rw = self._resize.target(h, w) if self._resize else (h, w)
        if divisor:
            oh = int(math.ceil(rh / divisor) * divisor)
            ow = int(math.ceil(rw / divisor) * divisor)
        else:
            oh, ow = rh, rw
        left, top = (ow - rw) // 2, (oh - rh) // 2
        right, down = ow - rw - left, oh - rh - top
        mean, std = self._norm_arrays()
        out = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=image.device)
        _lib.launch("om_preprocess", image.device, image, n, h, w, rh, rw, mean, std, top, left, oh, ow, float(pad_value), out)
        return out, [left, right, top, down, oh, ow]

    def _run_u8(self, image, divisor, pad_value):
        """_run for a uint8 [n,h,w,3] device tensor (RGB): the same geometry, through om_preprocess_batch."""
        _lib.require_cuda_tensor(image, "image", torch.uint8)
        if image.dim() != 4 or image.shape[3] != 3:
            raise ValueError("image must be [n,h,w,3], got %s" % (tuple(image.shape),))
        image = image.contiguous()
        n, h, w, _ = image.shape
        oh, ow, rows = self.plan_batch([(h, w)], divisor)
        geom = geom_rows([(h, w)] * n, [True] * n, rows * n, "rgb")
        out = self._launch_batch([image.data_ptr() + i * h * w * 3 for i in range(n)], geom, oh, ow, pad_value, image.device)
        return out, list(rows[0].pad_info)

    def __call__(self, image):
        """[n,h,w,c] float32 or uint8 -> [n,c,H,W] (FastCOCOTransform.__call__)."""
        return self._run(image, 0, 0.0)[0]

    def padded(self, image, size_divisor=32, pad_value=0):
        """transform(image) followed by pad(): one kernel.  Returns (image, pad_info) like infer.pad."""
        return self._run(image, size_divisor, pad_value)


def pad(image, size_divisor=32, pad_value=0):
    """infer.pad: centred padding of an NCHW tensor to a multiple of size_divisor.
    Returns (image, [left, right, top, down, new_height, new_width])."""
    _lib.require_cuda_tensor(image, "image", torch.float32)
    height, width = image.shape[-2:]
    new_height = int(math.ceil(height / size_divisor) * size_divisor)
    new_width = int(math.ceil(width / size_divisor) * size_divisor)
    pad_left, pad_top = (new_width - width) // 2, (new_height - height) // 2
    pad_right, pad_down = new_width - width - pad_left, new_height - height - pad_top
    pad_info = [pad_left, pad_right, pad_top, pad_down, new_height, new_width]
    if new_height == height and new_width == width:
        return image, pad_info
    src = image.contiguous()
    planes = src.numel() // (height * width)
    out = torch.empty(tuple(src.shape[:-2]) + (new_height, new_width), dtype=torch.float32, device=src.device)
    _lib.launch("om_pad_nchw", src.device, src, planes, height, width, pad_top, pad_left, new_height, new_width, float(pad_value), out)
    return out, pad_info


def build_transform(config):
    """trainer/builder.py:108-115: config = dict(type='FastCOCOTransform', pipeline=[dict(type='Resize', ...), ...])."""
    import sys
    kwargs = dict(config)
    cls = getattr(sys.modules[__name__], kwargs.pop("type"))
    items = []
    for item in kwargs.pop("pipeline"):
        it = dict(item)
        items.append(getattr(cls, it.pop("type"))(**it))
    return cls(pipeline=items, **kwargs)
