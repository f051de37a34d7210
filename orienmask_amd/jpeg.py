"""JPEG files to device-resident RGB images: the host undoes the Huffman coding, the device does the arithmetic.

    decoder = JpegDecoder("cuda:0")
    images = decoder.decode(paths_or_bytes)            # list of [h,w,3] uint8 RGB tensors on the device, input order
    x, pad_infos = transform.batch(images)             # what FastCOCOTransform.batch and infer_loop(batch_size=B) take as they are

The pixels are libjpeg's (ISLOW IDCT, fancy up-sampling), bit for bit: PIL's ``Image.open(p).convert('RGB')``
(tests/golden/jpeg_cases.npz).  What the device path does not decode -- progressive streams, an Exif orientation, CMYK, ...:
include/orienmask_hip.h lists them -- goes to a host reader and is uploaded (``on_unsupported='fallback'``) or raises
(``'raise'``); ``stats()`` counts both ways and the reasons.  A BROKEN stream raises, naming the item, before anything of that
call is launched.

One call: the entropy decoders run in a pool of at most 16 threads (ctypes drops the GIL) and write their coefficients straight
into ONE pinned staging buffer, laid out by plan(); one copy crosses; ceil(n / OM_JPEG_BATCH) launch sets decode.
"""
import collections
import concurrent.futures
import ctypes
import io
import os

import numpy as np
import torch

from . import lib as _lib

MAX_THREADS = 16
STAGE_RING = 3          # pinned staging buffers per decoder, as transform.STAGE_RING
REASONS = {getattr(_lib, n): n[len("OM_JPEG_R_"):].lower() for n in dir(_lib) if n.startswith("OM_JPEG_R_")}

Plan = collections.namedtuple("Plan", "desc coef_off quant_off out_off coef_elems quant_elems out_bytes stage_bytes quant_stage_off")


class JpegError(_lib.OrienMaskHipError):
    """A stream the host decoder rejects, or an unsupported one under on_unsupported='raise'."""


def _read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    if isinstance(item, (str, os.PathLike)):
        with open(item, "rb") as f:
            return f.read()
    raise TypeError("a JPEG item is bytes or a path, got %s" % type(item).__name__)


def _name(i, item):
    return "item %d (%s)" % (i, item if isinstance(item, (str, os.PathLike)) else "%d bytes" % len(item))


def host_info(data):
    """om_jpeg_info of a byte string: the int32 record (host only; a loader worker may call it).  Raises JpegError."""
    rec = np.zeros(_lib.OM_JPEG_INFO_WORDS, np.int32)
    buf = np.frombuffer(data, np.uint8)
    rc = _lib.load().om_jpeg_info(buf.ctypes.data if buf.size else None, buf.size, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != 0:
        raise JpegError(_lib.load().om_last_error().decode())
    return rec


def host_entropy_decode(data, coef, quant):
    """om_jpeg_entropy_decode into the int16 array `coef` and the uint16 array `quant` (views of a staging buffer): the info
    record as the decoder left it.  Host only.  Raises JpegError for a stream it rejects."""
    rec = np.zeros(_lib.OM_JPEG_INFO_WORDS, np.int32)
    buf = np.frombuffer(data, np.uint8)
    L = _lib.load()
    rc = L.om_jpeg_entropy_decode(buf.ctypes.data, buf.size, coef.ctypes.data, coef.nbytes, quant.ctypes.data,
                                  rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != 0:
        raise JpegError(L.om_last_error().decode())          # the message is thread-local: read on the thread that failed
    return rec


def plan(infos):
    """Host only.  infos: the info records of the streams the DEVICE decodes, in order -> Plan: the int64 [n, OM_JPEG_DESC_WORDS]
    table of om_jpeg_decode_batch and where everything lies -- coefficients back to back (a multiple of 64 elements each), the
    tables of image i at 192 i, the outputs at multiples of 16 bytes.  The staging buffer holds the coefficients, then the
    tables: stage_bytes in all, the tables at quant_stage_off."""
    n = len(infos)
    desc = np.zeros((n, _lib.OM_JPEG_DESC_WORDS), np.int64)
    coef_off, quant_off, out_off = [], [], []
    c = o = 0
    for i, rec in enumerate(infos):
        w, h = int(rec[_lib.OM_JPEG_I_WIDTH]), int(rec[_lib.OM_JPEG_I_HEIGHT])
        coef_off.append(c)
        quant_off.append(192 * i)
        out_off.append(o)
        desc[i] = (w, h, rec[_lib.OM_JPEG_I_NCOMP], rec[_lib.OM_JPEG_I_HMAX], rec[_lib.OM_JPEG_I_VMAX], c, 192 * i, o)
        c += 64 * int(rec[_lib.OM_JPEG_I_BLOCKS])
        o += (h * w * 3 + 15) // 16 * 16
    quant_stage_off = 2 * c
    return Plan(desc, coef_off, quant_off, out_off, c, 192 * n, o, quant_stage_off + 2 * 192 * n, quant_stage_off)


def default_imread_bytes():
    """The host reader of unsupported streams, working from the bytes: dataset._default_imread's choice (cv2 as the reference
    reads when it can be imported, PIL otherwise) -> a callable bytes -> [h,w,3] uint8 RGB, or None when neither is there."""
    try:
        import cv2

        def imread(data):
            image = cv2.imdecode(np.frombuffer(data, np.uint8), cv2.IMREAD_COLOR)
            if image is None:
                raise JpegError("cv2 cannot decode the stream")
            return cv2.cvtColor(image, cv2.COLOR_BGR2RGB)
        return imread
    except ImportError:
        pass
    try:
        from PIL import Image
    except ImportError:
        return None

    def imread(data):
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert('RGB'), dtype=np.uint8)
    return imread


class JpegDecoder:
    """decode(items) -> device RGB images.  threads: entropy-decoder threads, at most MAX_THREADS (never sized from the machine's
    CPU count: a loader shares it).  on_unsupported: 'fallback' (the host reader `imread`, bytes -> [h,w,3] uint8 RGB; default
    default_imread_bytes()) or 'raise'."""

    def __init__(self, device=None, threads=8, on_unsupported="fallback", imread=None):
        if on_unsupported not in ("fallback", "raise"):
            raise ValueError("on_unsupported must be 'fallback' or 'raise', got %r" % (on_unsupported,))
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda":
            raise _lib.OrienMaskHipError("JpegDecoder decodes on an MI355X device, got %s (no CPU fallback)" % (device,))
        self.device = device
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.on_unsupported = on_unsupported
        self.imread = imread
        self._pool = None
        self._ring = [None] * STAGE_RING
        self._ring_next = 0
        self._stats = {"device": 0, "fallback": 0, "reasons": collections.Counter()}
        _lib.load()

    # ---- host side -------------------------------------------------------------------------------------------------------
    def stats(self):
        """{'device': streams decoded on the device, 'fallback': streams read by the host reader, 'reasons': {reason: count}}"""
        return {"device": self._stats["device"], "fallback": self._stats["fallback"], "reasons": dict(self._stats["reasons"])}

    def _map(self, fn, jobs):
        if self.threads == 1 or len(jobs) < 2:
            return [fn(j) for j in jobs]
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(self.threads, thread_name_prefix="om_jpeg")
        return list(self._pool.map(fn, jobs))

    def _stage_slot(self, nbytes):
        """The next pinned staging buffer of the ring, free (the copy that last read it has finished) and large enough."""
        k = self._ring_next
        self._ring_next = (k + 1) % len(self._ring)
        slot = self._ring[k]
        if slot is not None:
            slot[1].synchronize()
        if slot is None or slot[0].numel() < nbytes:
            size = max(nbytes, 2 * slot[0].numel() if slot is not None else 0, 1 << 16)
            slot = self._ring[k] = [self._alloc_stage(size), self._new_event()]
        return slot

    # the few places that touch the device, one method each (tests/test_jpeg_cpu.py runs the planner and the fallback logic on
    # a machine without one, with a stand-in for these)
    def _alloc_stage(self, size):
        return torch.empty(size, dtype=torch.uint8).pin_memory()

    def _new_event(self):
        return torch.cuda.Event()

    def _guard(self):
        return _lib.on_device(self.device)

    def _to_device(self, image):
        return torch.from_numpy(image).to(self.device)

    def _unsupported(self, i, item, data, rec):
        reason = REASONS.get(int(rec[_lib.OM_JPEG_I_REASON]), "reason %d" % rec[_lib.OM_JPEG_I_REASON])
        if self.on_unsupported == "raise":
            raise JpegError("%s: the device path does not decode this stream (%s)" % (_name(i, item), reason))
        if self.imread is None:
            self.imread = default_imread_bytes()
            if self.imread is None:
                raise JpegError("%s: unsupported stream (%s) and no host reader (cv2 or PIL) to fall back to" % (_name(i, item), reason))
        return reason

    # ---- device side -----------------------------------------------------------------------------------------------------
    def _launch(self, p, staged):
        """The staged bytes on the device -> the uint8 output buffer (om_jpeg_decode_batch)."""
        coef = staged[:p.quant_stage_off].view(torch.int16)
        quant = staged[p.quant_stage_off:p.stage_bytes].view(torch.int16)
        desc = p.desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        n = len(p.desc)
        ws_bytes = _lib.workspace_bytes("om_jpeg_workspace_bytes", desc, n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(p.out_bytes, dtype=torch.uint8, device=self.device)
        _lib.launch("om_jpeg_decode_batch", self.device, desc, n, coef, p.coef_elems, quant, p.quant_elems, ws, ws_bytes, out, p.out_bytes)
        return out

    def _upload(self, pinned, nbytes, event):
        staged = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        staged.copy_(pinned[:nbytes], non_blocking=True)                     # the one host-to-device copy of the call
        event.record(torch.cuda.current_stream(self.device))
        return staged

    def decode(self, items):
        """items: a list of bytes or paths -> the list of [h,w,3] uint8 RGB tensors on the device, in input order."""
        items = list(items)
        if not items:
            return []
        datas = self._map(_read, items)

        def probe(job):
            i, data = job
            try:
                return host_info(data)
            except JpegError as e:
                return e
        infos = self._map(probe, list(enumerate(datas)))
        for i, rec in enumerate(infos):
            if isinstance(rec, JpegError):
                raise JpegError("%s: %s" % (_name(i, items[i]), rec))
        dev_idx = [i for i, rec in enumerate(infos) if rec[_lib.OM_JPEG_I_SUPPORTED]]
        host_idx = {i: self._unsupported(i, items[i], datas[i], infos[i]) for i, rec in enumerate(infos) if not rec[_lib.OM_JPEG_I_SUPPORTED]}
        results = [None] * len(items)
        with self._guard():
            while dev_idx:
                p = plan([infos[i] for i in dev_idx])
                pinned, event = self._stage_slot(p.stage_bytes)
                flat = pinned.numpy()
                coef_all = flat[:p.quant_stage_off].view(np.int16)
                quant_all = flat[p.quant_stage_off:p.stage_bytes].view(np.uint16)

                def entropy(job):
                    k, i = job
                    end = p.coef_off[k + 1] if k + 1 < len(dev_idx) else p.coef_elems
                    try:
                        return host_entropy_decode(datas[i], coef_all[p.coef_off[k]:end], quant_all[p.quant_off[k]:p.quant_off[k] + 192])
                    except JpegError as e:
                        return e
                recs = self._map(entropy, list(enumerate(dev_idx)))
                for k, rec in enumerate(recs):                               # nothing has been launched yet
                    if isinstance(rec, JpegError):
                        raise JpegError("%s: %s" % (_name(dev_idx[k], items[dev_idx[k]]), rec))
                late = [k for k, rec in enumerate(recs) if not rec[_lib.OM_JPEG_I_SUPPORTED]]
                if late:                                                     # found unsupported only while decoding: plan again without them
                    for k in late:
                        i = dev_idx[k]
                        host_idx[i] = self._unsupported(i, items[i], datas[i], recs[k])
                    dev_idx = [i for k, i in enumerate(dev_idx) if k not in set(late)]
                    continue
                out = self._launch(p, self._upload(pinned, p.stage_bytes, event))
                for k, i in enumerate(dev_idx):
                    w, h = int(p.desc[k][0]), int(p.desc[k][1])
                    results[i] = out[p.out_off[k]:p.out_off[k] + h * w * 3].view(h, w, 3)
                self._stats["device"] += len(dev_idx)
                break
            for i, reason in sorted(host_idx.items()):
                image = np.array(self.imread(datas[i]), dtype=np.uint8, order='C')      # a copy: readers hand out read-only views
                if image.ndim != 3 or image.shape[2] != 3:
                    raise JpegError("%s: the host reader returned shape %s, not [h,w,3]" % (_name(i, items[i]), image.shape))
                results[i] = self._to_device(image)
                self._stats["fallback"] += 1
                self._stats["reasons"][reason] += 1
        return results
