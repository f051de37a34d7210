"""The reference's training / validation data pipeline on the device: COCOTransform + collate.

  COCOTransform(pipeline)    /root/reference/data/transform.py:65-441 (BaseTransform's ColorJitter and Normalize, COCOTransform's
                             RandomCrop, Resize, RandomHorizontalFlip, RandomVerticalFlip, ToTensor)
  collate(batch)             /root/reference/data/collate.py:13-30, host half: one contiguous buffer per kind + the parameter table
  to_device(planned, device) the device half: three H2D copies and one launch set (om_augment, csrc/augment.hip); returns what
                             the reference's collate returns -- (image, (bbox, cls, index, mask), info) -- on the device
                             (samples that carry 'segm': a fourth copy and om_segm_decode, csrc/segm_decode.hip, in front)
  device_batches(loader, device)

``COCOTransform.__call__`` runs in the DataLoader worker and touches no pixel.  It consumes the reference's random draws in the
reference's order, with the reference's expressions and numpy dtypes, computes bbox / cls / info exactly as the reference does, and
returns the SOURCE image (uint8 when that is exact: the dataset's float32 image is cv2's uint8 decode cast up), the source masks
bit-packed per row, and a small parameter record.  The kernels then do every pixel of ColorJitter -> RandomCrop -> Resize -> flips
-> ToTensor -> Normalize in one pass over the output.  A sample may carry its masks as 'segm' instead of 'mask': the annotation
json's own objects (polygons, boxes, RLE), one per GT.  Then the worker ships those few numbers, the device decodes them into the
same packed bits (om_segm_decode) and everything behind is unchanged.  Pipelines outside "the shipped order, any subset of it" raise
NotImplementedError, as ShortEdgeResize, Pad, collate_plus and the aspect-ratio-grouped loader do.
"""
import ctypes
import random

import numpy as np
import torch

from . import lib as _lib
from . import segm as _segm

# om_aug_sample (include/orienmask_hip.h)
AUG_SAMPLE_DTYPE = np.dtype([("image_off", "<i8"), ("mask_off", "<i8"), ("scale_x", "<f8"), ("scale_y", "<f8"),
                             ("src_h", "<i4"), ("src_w", "<i4"), ("crop_top", "<i4"), ("crop_left", "<i4"),
                             ("crop_h", "<i4"), ("crop_w", "<i4"), ("nh", "<i4"), ("nw", "<i4"),
                             ("pad_top", "<i4"), ("pad_left", "<i4"), ("hflip", "<i4"), ("vflip", "<i4"),
                             ("area2x", "<i4"), ("n_ops", "<i4"), ("op", "<i4", 4), ("fa", "<f4", 4), ("fb", "<f4", 4),
                             ("pad_value", "<f4", 3), ("gt_first", "<i4"), ("n_gt", "<i4"), ("reserved", "<i4")])
assert AUG_SAMPLE_DTYPE.itemsize == 160

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
_INTERP = ("nearest", "linear", "area", "cubic", "lanczos4")


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


class COCOTransform:
    """Host planner of the reference's COCOTransform: same nested classes, same constructor arguments."""

    class ColorJitter:
        def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
            self.brightness = self._check_input(brightness, 'brightness')
            self.contrast = self._check_input(contrast, 'contrast')
            self.saturation = self._check_input(saturation, 'saturation')
            self.hue = self._check_input(hue, 'hue', center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)

        @staticmethod
        def _check_input(value, name, center=1, bound=(0, float('inf')), clip_first_on_zero=True):
            if isinstance(value, (int, float)):
                if value < 0:
                    raise ValueError("If {} is a single number, it must be non negative.".format(name))
                value = [center - value, center + value]
                if clip_first_on_zero:
                    value[0] = max(value[0], 0)
            elif isinstance(value, (tuple, list)) and len(value) == 2:
                if not bound[0] <= value[0] <= value[1] <= bound[1]:
                    raise ValueError("{} values should be between {}".format(name, bound))
            else:
                raise TypeError("{} should be a single number or a list/tuple with lenght 2.".format(name))
            if value[0] == value[1] == center:
                value = None
            return value

        def __call__(self, st):
            # get_params: one uniform per active op in this order, then random.shuffle of the list of ops
            ops = []
            if self.brightness is not None:
                ops.append((BRIGHTNESS, random.uniform(self.brightness[0], self.brightness[1])))
            if self.contrast is not None:
                ops.append((CONTRAST, random.uniform(self.contrast[0], self.contrast[1])))
            if self.saturation is not None:
                ops.append((SATURATION, random.uniform(self.saturation[0], self.saturation[1])))
            if self.hue is not None:
                ops.append((HUE, random.uniform(self.hue[0], self.hue[1])))
            random.shuffle(ops)
            st.ops = ops

    class RandomCrop:
        def __init__(self, p=0.5, image_min_iou=0.64, bbox_min_iou=0.64):
            self.p = p
            self.image_min_iou = image_min_iou
            self.bbox_min_iou = bbox_min_iou
            self.image_max_ratio = image_min_iou ** 0.5
            self.bbox_max_ratio = bbox_min_iou ** 0.5

        def __call__(self, st):
            if random.random() < self.p:
                height, width = st.h, st.w
                if st.bbox.shape[0] == 0:
                    left = int(random.uniform(0, width * (1 - self.image_max_ratio)) + 0.5)
                    right = int(random.uniform(width * self.image_max_ratio, width) + 0.5)
                    top = int(random.uniform(0, height * (1 - self.image_max_ratio)) + 0.5)
                    down = int(random.uniform(height * self.image_max_ratio, height) + 0.5)
                else:
                    bx, by, bw, bh = np.split(st.bbox, 4, axis=1)
                    bx1 = (bx - bw / 2) * width
                    bx2 = (bx + bw / 2) * width
                    by1 = (by - bh / 2) * height
                    by2 = (by + bh / 2) * height

                    bbox_left = (bx1 * self.bbox_max_ratio + bx2 * (1 - self.bbox_max_ratio)).min()
                    bbox_right = (bx1 * (1 - self.bbox_max_ratio) + bx2 * self.bbox_max_ratio).max()
                    bbox_top = (by1 * self.bbox_max_ratio + by2 * (1 - self.bbox_max_ratio)).min()
                    bbox_down = (by1 * (1 - self.bbox_max_ratio) + by2 * self.bbox_max_ratio).max()

                    left = int(random.uniform(0, min(bbox_left, width * (1 - self.image_max_ratio))) + 0.5)
                    right = int(random.uniform(max(bbox_right, width * self.image_max_ratio), width) + 0.5)
                    top = int(random.uniform(0, min(bbox_top, height * (1 - self.image_max_ratio))) + 0.5)
                    down = int(random.uniform(max(bbox_down, height * self.image_max_ratio), height) + 0.5)

                    bx1_new = np.maximum(bx1 - left, 0)
                    bx2_new = np.minimum(bx2 - left, right - left + 1)
                    by1_new = np.maximum(by1 - top, 0)
                    by2_new = np.minimum(by2 - top, down - top + 1)

                    width_new = right - left + 1
                    height_new = down - top + 1
                    bx_new = (bx1_new + bx2_new) / 2 / width_new
                    by_new = (by1_new + by2_new) / 2 / height_new
                    bw_new = (bx2_new - bx1_new) / width_new
                    bh_new = (by2_new - by1_new) / height_new

                    st.bbox = np.hstack([bx_new, by_new, bw_new, bh_new])

                # image[top:down+1, left:right+1]: Python's slice clamps (right / down may equal the width / height)
                rows, cols = range(st.crop_top, st.crop_top + st.h)[top:down + 1], range(st.crop_left, st.crop_left + st.w)[left:right + 1]
                if len(rows) == 0 or len(cols) == 0:
                    raise ValueError("RandomCrop: empty window rows %d:%d cols %d:%d of %dx%d" % (top, down + 1, left, right + 1, height, width))
                st.crop_top, st.crop_left, st.h, st.w = rows.start, cols.start, len(rows), len(cols)
                if st.info is not None:
                    st.info['crop'] = (top, down + 1, left, right + 1) + (height, width)

    class Resize:
        def __init__(self, size, interpolation='linear', pad_needed=True, warp_p=0., jitter=0.,
                     random_place=False, pad_p=0., pad_ratio=0., pad_value=255 / 2):
            assert isinstance(size, int) or len(size) == 2
            self.size = _pair(size)
            self.aspect_ratio = self.size[1] / self.size[0]
            if interpolation not in _INTERP:
                raise KeyError(interpolation)
            if interpolation != 'linear':
                raise NotImplementedError("COCOTransform.Resize: the HIP kernels implement interpolation='linear' (cv2.INTER_LINEAR) "
                                          "for the image, got %r" % interpolation)
            self.pad_needed = pad_needed
            self.warp_p = warp_p
            self.jitter = jitter
            self.random_place = random_place
            self.pad_p = pad_p
            self.pad_ratio = pad_ratio
            if isinstance(pad_value, (list, tuple)) and len(pad_value) == 3:
                self.pad_value = [float(v) for v in pad_value]
            elif pad_needed:
                raise NotImplementedError("COCOTransform.Resize: pad_value must be a 3-list (per channel, as the configs' MEAN); "
                                          "how cv2's binding broadcasts a bare scalar onto 3 channels is not restated (got %r)"
                                          % (pad_value,))
            else:
                self.pad_value = [0.0, 0.0, 0.0]        # pad_needed=False never pads

        def __call__(self, st):
            h, w = self.size
            if self.pad_needed and random.random() > self.warp_p:
                oh, ow = st.h, st.w
                dh, dw = oh * self.jitter, ow * self.jitter
                new_aspect_ratio = (ow + random.uniform(-dw, dw)) / (oh + random.uniform(-dh, dh))
                if new_aspect_ratio < self.aspect_ratio:
                    nh = int(h * (1 - random.uniform(0, self.pad_ratio)) + 0.5) \
                        if random.random() < self.pad_p else h
                    nw = int(nh * new_aspect_ratio + 0.5)
                else:
                    nw = int(w * (1 - random.uniform(0, self.pad_ratio)) + 0.5) \
                        if random.random() < self.pad_p else w
                    nh = int(nw / new_aspect_ratio + 0.5)

                pad_left = int(random.uniform(0, w - nw) + 0.5) if self.random_place else int((w - nw) / 2 + 0.5)
                pad_top = int(random.uniform(0, h - nh) + 0.5) if self.random_place else int((h - nh) / 2 + 0.5)
                pad_right = w - nw - pad_left
                pad_down = h - nh - pad_top

                st.bbox[:, 0] = (st.bbox[:, 0] * nw + pad_left) / w
                st.bbox[:, 1] = (st.bbox[:, 1] * nh + pad_top) / h
                st.bbox[:, 2] = st.bbox[:, 2] * nw / w
                st.bbox[:, 3] = st.bbox[:, 3] * nh / h

                padding = (pad_top, pad_down, pad_left, pad_right)
                if nh <= 0 or nw <= 0 or min(padding) < 0:
                    raise ValueError("Resize: resized %dx%d with padding %s does not fit %dx%d" % (nh, nw, padding, h, w))
                st.resize = (nh, nw, pad_top, pad_left, h, w)
                st.padded = True
                st.pad_value = self.pad_value
                if st.info is not None:
                    st.info['pad'] = padding + (h, w)
            else:
                st.resize = (h, w, 0, 0, h, w)

    class RandomHorizontalFlip:
        def __init__(self, p=0.5):
            self.p = p

        def __call__(self, st):
            if random.random() < self.p:
                st.bbox[:, 0] = 1 - st.bbox[:, 0]
                st.hflip = not st.hflip
                if st.info is not None:
                    st.info['hflip'] = True

    class RandomVerticalFlip:
        def __init__(self, p=0.5):
            self.p = p

        def __call__(self, st):
            if random.random() < self.p:
                st.bbox[:, 1] = 1 - st.bbox[:, 1]
                st.vflip = not st.vflip
                if st.info is not None:
                    st.info['vflip'] = True

    class ToTensor:
        def __call__(self, st):
            shuffle = torch.randperm(st.bbox.shape[0])
            st.perm = shuffle
            st.bbox = torch.from_numpy(st.bbox).float()[shuffle]
            st.cls = torch.from_numpy(st.cls).long()[shuffle]

    class Normalize:
        def __init__(self, mean, std):
            self.mean = mean
            self.std = std

        def __call__(self, st):
            # torchvision F.normalize: as_tensor(mean / std, dtype=float32), sub_ then div_
            st.mean = torch.as_tensor(self.mean, dtype=torch.float32).reshape(-1).expand(3).tolist()
            st.std = torch.as_tensor(self.std, dtype=torch.float32).reshape(-1).expand(3).tolist()

    class ShortEdgeResize:
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("COCOTransform.ShortEdgeResize: variable-size batches (ShortEdgeResize, Pad, collate_plus) "
                                      "are not implemented on the device")

    class Pad:
        def __init__(self, *args, **kwargs):
            raise NotImplementedError("COCOTransform.Pad: variable-size batches (ShortEdgeResize, Pad, collate_plus) are not "
                                      "implemented on the device")

    _ORDER = {"ColorJitter": 0, "RandomCrop": 1, "Resize": 2, "RandomHorizontalFlip": 3, "RandomVerticalFlip": 3,
              "ToTensor": 5, "Normalize": 6}

    def __init__(self, pipeline, transport_uint8=True):
        self.pipeline = list(pipeline)
        self.transport_uint8 = transport_uint8
        names = [type(t).__name__ for t in self.pipeline]
        for t, n in zip(self.pipeline, names):
            if n not in self._ORDER or not isinstance(t, getattr(COCOTransform, n)):
                raise NotImplementedError("COCOTransform: %s is not part of the device pipeline (ColorJitter -> RandomCrop -> Resize "
                                          "-> flips -> ToTensor -> Normalize, any subset in that order)" % n)
        ranks = [self._ORDER[n] for n in names]
        if len(set(names)) != len(names) or ranks != sorted(ranks):
            raise NotImplementedError("COCOTransform: pipeline %s is not the shipped order (ColorJitter -> RandomCrop -> Resize -> "
                                      "flips -> ToTensor -> Normalize) or a subset of it" % names)
        if "ToTensor" not in names:
            raise NotImplementedError("COCOTransform: the device pipeline needs ToTensor (collate stacks tensors)")

    def __call__(self, sample):
        """sample: COCODataset._load_sample_data's dict (image [h,w,3] float32 or uint8 RGB, bbox, cls, optional mask list and
        info).  Returns the planned sample: bbox / cls tensors and info as the reference's pipeline leaves them, the source image,
        the packed masks and the parameter record 'aug'.  Instead of 'mask' the sample may carry 'segm': one entry per GT, each
        what the annotation json holds (a list of polygons or of 4-number boxes, or a dict with 'size' and list or string
        'counts'); the planned sample then carries the classified sources as flat arrays (segm.pack_sources), no pixel."""
        image = sample['image']
        if not isinstance(image, np.ndarray) or image.ndim != 3 or image.shape[2] != 3 or image.dtype not in (np.float32, np.uint8):
            raise ValueError("COCOTransform: image must be an [h,w,3] float32 or uint8 array, got %s"
                             % (getattr(image, 'shape', type(image)),))
        if 'mask' in sample and 'segm' in sample:
            raise ValueError("COCOTransform: a sample carries its masks as 'mask' or as 'segm', not both")
        st = _PlanState(sample)
        for t in self.pipeline:
            t(st)
        out = {'image': _transport_image(image, self.transport_uint8), 'bbox': st.bbox, 'cls': st.cls}
        if 'mask' in sample:
            masks = sample['mask']
            for m in masks:
                if m.shape != image.shape[:2]:
                    raise ValueError("COCOTransform: mask of shape %s for an image of %s" % (m.shape, image.shape[:2]))
            h, w = image.shape[:2]
            out['mask'] = np.packbits(np.stack(masks) > 0, axis=2) if len(masks) else np.zeros((0, h, (w + 7) // 8), np.uint8)
        if 'segm' in sample:
            segm = sample['segm']
            if len(segm) != len(sample['bbox']):
                raise ValueError("COCOTransform: %d segmentations for %d boxes" % (len(segm), len(sample['bbox'])))
            h, w = image.shape[:2]
            srcs = []
            for a in segm:
                mh, mw, lst = _segm.sources(a, h, w)
                if (mh, mw) != (h, w):
                    raise ValueError("COCOTransform: RLE of size %s for an image of %s" % ((mh, mw), (h, w)))
                srcs.append(lst)
            out['segm'] = _segm.pack_sources(srcs)
        if st.info is not None:
            out['info'] = st.info
        out['aug'] = st.record()
        return out


class _PlanState:
    """What the pipeline knows about a sample while planning: the crop window of the source, the resize / pad, the flips."""

    def __init__(self, sample):
        self.src_h, self.src_w = sample['image'].shape[:2]
        self.h, self.w = self.src_h, self.src_w
        self.crop_top = self.crop_left = 0
        self.bbox = np.array(sample['bbox'], copy=True)
        self.cls = sample['cls']
        self.info = sample.get('info')
        self.ops = []
        self.resize = None
        self.padded = False
        self.pad_value = [0.0, 0.0, 0.0]
        self.hflip = self.vflip = False
        self.perm = None
        self.mean, self.std = [0.0] * 3, [1.0] * 3

    def record(self):
        nh, nw, pad_top, pad_left, out_h, out_w = self.resize if self.resize else (self.h, self.w, 0, 0, self.h, self.w)
        return dict(src_h=self.src_h, src_w=self.src_w, crop=(self.crop_top, self.crop_left, self.h, self.w),
                    resize=(nh, nw, pad_top, pad_left), out=(out_h, out_w), padded=self.padded, pad_value=list(self.pad_value),
                    ops=list(self.ops), hflip=bool(self.hflip), vflip=bool(self.vflip),
                    perm=self.perm.numpy().astype(np.int64), mean=list(self.mean), std=list(self.std))


def _transport_image(image, transport_uint8):
    """The source image as it crosses to the device: uint8 when the float32 values are exactly uint8's (the dataset's image is
    cv2's uint8 decode cast up), else float32.  The kernels read either; the results are bit-identical."""
    if image.dtype == np.uint8 or not transport_uint8:
        return np.ascontiguousarray(image)
    u8 = image.astype(np.uint8)
    if np.array_equal(u8, image):
        return u8
    return np.ascontiguousarray(image)


def sample_row(aug, image_off, mask_off, gt_first, n_gt):
    """One om_aug_sample row from a planned sample's record."""
    row = np.zeros((), AUG_SAMPLE_DTYPE)
    top, left, ch, cw = aug['crop']
    nh, nw, pad_top, pad_left = aug['resize']
    row['image_off'], row['mask_off'] = image_off, mask_off
    row['scale_x'] = 1.0 / (float(nw) / cw)         # cv2: scale = 1 / inv_scale, inv_scale = (double)dsize / ssize
    row['scale_y'] = 1.0 / (float(nh) / ch)
    row['src_h'], row['src_w'] = aug['src_h'], aug['src_w']
    row['crop_top'], row['crop_left'], row['crop_h'], row['crop_w'] = top, left, ch, cw
    row['nh'], row['nw'], row['pad_top'], row['pad_left'] = nh, nw, pad_top, pad_left
    row['hflip'], row['vflip'] = int(aug['hflip']), int(aug['vflip'])
    row['area2x'] = int(ch == 2 * nh and cw == 2 * nw)       # cv2 resize: INTER_LINEAR at an exact 2x downscale -> INTER_AREA
    row['n_ops'] = len(aug['ops'])
    for k, (code, f) in enumerate(aug['ops']):
        row['op'][k] = code
        row['fa'][k] = np.float32(f)
        row['fb'][k] = np.float32(f * 360) if code == HUE else np.float32(1 - f)
    row['pad_value'] = np.float32(aug['pad_value'])
    row['gt_first'], row['n_gt'] = gt_first, n_gt
    return row


def _align(n, a=16):
    return (n + a - 1) // a * a


class PlannedBatch:
    """collate()'s result: host buffers (pinnable) and the layout of the meta buffer.  DataLoader(pin_memory=True) calls
    pin_memory().  A batch of 'segm' samples has an empty `mask` and, in `segm`, the arrays of om_segm_decode at the byte ranges
    of `segm_layout`; `segm_counts` holds n_poly, n_srcs, bitmap_words and mask_bytes, the size of the device scratch that the
    samples' mask_off point into."""

    def __init__(self, image, mask, meta, layout, B, N, out_hw, mean, std, any_contrast, has_mask, info, segm=None,
                 segm_layout=None, segm_counts=None):
        self.image, self.mask, self.meta, self.layout = image, mask, meta, layout
        self.B, self.N, self.out_hw, self.mean, self.std = B, N, out_hw, mean, std
        self.any_contrast, self.has_mask, self.info = any_contrast, has_mask, info
        self.segm, self.segm_layout, self.segm_counts = segm, segm_layout, segm_counts

    def pin_memory(self, device=None):
        self.image, self.mask, self.meta = (t if t.is_pinned() else t.pin_memory() for t in (self.image, self.mask, self.meta))
        if self.segm is not None and not self.segm.is_pinned():
            self.segm = self.segm.pin_memory()
        return self

    def h2d_bytes(self):
        return {"image": self.image.numel() * self.image.element_size(), "mask": self.mask.numel(), "meta": self.meta.numel(),
                "segm": self.segm.numel() if self.segm is not None else 0}


def collate(batch):
    """data/collate.py:collate, host half (picklable; runs in the DataLoader worker).  One contiguous buffer for the source
    images, one for the packed masks, one 'meta' buffer: the om_aug_sample table, the [N,2] int32 GT table (source GT, image) with
    ToTensor's permutation applied, bbox [N,4] f32, cls [N] i64 and index [B+1] i64 -- each at a 16-byte offset."""
    B = len(batch)
    if B == 0:
        raise ValueError("collate: empty batch")
    if any('aug' not in s for s in batch):
        raise ValueError("collate: samples must come from orienmask_amd.transform.COCOTransform")
    outs = {tuple(s['aug']['out']) for s in batch}
    if len(outs) != 1:
        raise NotImplementedError("collate: output sizes %s differ (variable-size batches are not implemented)" % sorted(outs))
    norms = {(tuple(s['aug']['mean']), tuple(s['aug']['std'])) for s in batch}
    if len(norms) != 1:
        raise ValueError("collate: samples of one batch were normalised differently")
    has_segm = any('segm' in s for s in batch)
    if has_segm and any('mask' in s for s in batch):
        raise ValueError("collate: a batch carries its masks as 'mask' or as 'segm', not a mixture")
    if has_segm and not all('segm' in s for s in batch):
        raise ValueError("collate: some samples have segmentations and some do not")
    has_mask = 'mask' in batch[0]
    if any(('mask' in s) != has_mask for s in batch):
        raise ValueError("collate: some samples have masks and some do not")
    u8 = all(s['image'].dtype == np.uint8 for s in batch)
    img_dtype = np.uint8 if u8 else np.float32
    n_gt = [int(s['bbox'].shape[0]) for s in batch]
    N = sum(n_gt)
    rows = np.zeros(B, AUG_SAMPLE_DTYPE)
    gt_table = np.zeros((N, 2), np.int32)
    image_off = mask_off = gt_first = 0
    segm_masks, segm_out_off = [], []
    for b, s in enumerate(batch):
        aug = s['aug']
        h, w = aug['src_h'], aug['src_w']
        if s['image'].shape != (h, w, 3):
            raise ValueError("collate: image %d is %s, planned for %dx%d" % (b, s['image'].shape, h, w))
        top, left, ch, cw = aug['crop']
        if not (0 <= top and top + ch <= h and 0 <= left and left + cw <= w and ch > 0 and cw > 0):
            raise ValueError("collate: crop window of image %d outside its source" % b)
        nh, nw, pt, pl = aug['resize']
        if not (nh > 0 and nw > 0 and pt >= 0 and pl >= 0 and pt + nh <= aug['out'][0] and pl + nw <= aug['out'][1]):
            raise ValueError("collate: resize of image %d does not fit the output" % b)
        perm = np.asarray(aug['perm'], np.int64)
        if sorted(perm.tolist()) != list(range(n_gt[b])):
            raise ValueError("collate: permutation of image %d is not a permutation of its %d GTs" % (b, n_gt[b]))
        if has_mask and s['mask'].shape != (n_gt[b], h, (w + 7) // 8):
            raise ValueError("collate: packed masks of image %d are %s, want %s" % (b, s['mask'].shape, (n_gt[b], h, (w + 7) // 8)))
        if has_segm:
            if int(s['segm']['n_gt']) != n_gt[b]:
                raise ValueError("collate: %d segmentations for the %d GTs of image %d" % (int(s['segm']['n_gt']), n_gt[b], b))
            for g, lst in enumerate(_segm.unpack_sources(s['segm'])):
                segm_masks.append((h, w, lst))
                segm_out_off.append(mask_off + g * h * ((w + 7) // 8))
        rows[b] = sample_row(aug, image_off, mask_off, gt_first, n_gt[b])
        gt_table[gt_first:gt_first + n_gt[b], 0] = gt_first + perm       # output GT gt_first + i holds source GT perm[i]
        gt_table[gt_first:gt_first + n_gt[b], 1] = b
        image_off += h * w * 3
        mask_off += n_gt[b] * h * ((w + 7) // 8)
        gt_first += n_gt[b]
    image = torch.from_numpy(np.concatenate([s['image'].astype(img_dtype, copy=False).reshape(-1) for s in batch]))
    mask = torch.from_numpy(np.concatenate([s['mask'].reshape(-1) for s in batch])) if has_mask and N else torch.zeros(0, dtype=torch.uint8)
    bbox = torch.cat([s['bbox'] for s in batch], dim=0).numpy().astype(np.float32, copy=False)
    cls = torch.cat([s['cls'] for s in batch], dim=0).numpy().astype(np.int64, copy=False)
    index = np.cumsum(np.array([0] + n_gt, np.int64))
    parts = [("samples", rows.view(np.uint8)), ("gt", gt_table.view(np.uint8).reshape(-1)),
             ("bbox", bbox.reshape(-1).view(np.uint8)), ("cls", cls.view(np.uint8)), ("index", index.view(np.uint8))]
    layout, off = {}, 0
    for name, arr in parts:
        layout[name] = (off, arr.size)
        off = _align(off + arr.size)
    meta = np.zeros(off, np.uint8)
    for name, arr in parts:
        meta[layout[name][0]:layout[name][0] + arr.size] = arr
    any_contrast = any(code == CONTRAST for s in batch for code, _ in s['aug']['ops'])
    mean, std = norms.pop()
    info = [s['info'] for s in batch] if 'info' in batch[0] else None
    segm = segm_layout = segm_counts = None
    if has_segm:
        tables, segm_counts = _segm.build_tables(segm_masks, segm_out_off)
        segm_counts["mask_bytes"] = mask_off
        segm_layout, off = {}, 0
        for name in _segm.TABLE_ORDER:
            nbytes = tables[name].size * tables[name].itemsize
            segm_layout[name] = (off, nbytes)
            off = _align(off + nbytes)
        buf = np.zeros(off, np.uint8)
        for name in _segm.TABLE_ORDER:
            buf[segm_layout[name][0]:segm_layout[name][0] + segm_layout[name][1]] = tables[name].view(np.uint8)
        segm = torch.from_numpy(buf)
    return PlannedBatch(image, mask, torch.from_numpy(meta), layout, B, N, outs.pop(), list(mean), list(std), any_contrast,
                        has_mask or has_segm, info, segm, segm_layout, segm_counts)


def _meta_view(meta, layout, name, dtype, shape):
    off, nbytes = layout[name]
    return meta[off:off + nbytes].view(dtype).view(shape)


def to_device(planned, device):
    """Device half of collate: three H2D copies (non-blocking, from pinned memory) and one launch set on the current stream; no
    D2H, no host synchronisation.  A batch of 'segm' samples takes one more copy (the source tables), and om_segm_decode fills a
    scratch with the packed masks that the 'mask' path would have copied; om_augment then reads that scratch.  Returns (image [B,3,H,W] f32, (bbox [N,4] f32, cls [N] i64, index [B+1] i64[, mask [N,H,W]
    bool])[, info]) -- the reference collate's tuple, every tensor on `device`."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.OrienMaskHipError("to_device: the augmentation kernels run on an MI355X device only (got %s)" % device)
    planned.pin_memory()
    B, N = planned.B, planned.N
    H, W = planned.out_hw
    with _lib.on_device(device):
        meta = planned.meta.to(device, non_blocking=True)
        image = planned.image.to(device, non_blocking=True)
        masks = planned.mask.to(device, non_blocking=True)
        if planned.segm is not None and N:
            masks = _segm_decode(planned, device)
        out_image = torch.empty((B, 3, H, W), dtype=torch.float32, device=device)
        out_mask = torch.empty((N, H, W), dtype=torch.bool, device=device)
        ws = None
        if planned.any_contrast:
            ws = torch.empty(_lib.load().om_augment_workspace_bytes(B), dtype=torch.uint8, device=device)
        samples = meta[planned.layout["samples"][0]:]
        gt = meta[planned.layout["gt"][0]:]
        mean = (ctypes.c_float * 3)(*planned.mean)
        std = (ctypes.c_float * 3)(*planned.std)
        _lib.launch("om_augment", device, samples, B, image, int(planned.image.dtype == torch.uint8), mean, std, H, W, out_image,
                    masks if N and planned.has_mask else None, gt, N if planned.has_mask else 0,
                    out_mask if N and planned.has_mask else None, int(planned.any_contrast), ws, ws.numel() if ws is not None else 0)
    bbox = _meta_view(meta, planned.layout, "bbox", torch.float32, (N, 4))
    cls = _meta_view(meta, planned.layout, "cls", torch.int64, (N,))
    index = _meta_view(meta, planned.layout, "index", torch.int64, (B + 1,))
    anno = (bbox, cls, index) + ((out_mask,) if planned.has_mask else ())
    if planned.info is not None:
        return out_image, anno, planned.info
    return out_image, anno


def _segm_decode(planned, device):
    """the packed masks of a 'segm' batch, decoded on the current stream into a fresh scratch"""
    c = planned.segm_counts
    tables = planned.segm.to(device, non_blocking=True)
    scratch = torch.empty(c["mask_bytes"], dtype=torch.uint8, device=device)
    ws_bytes = int(_lib.load().om_segm_decode_workspace_bytes(c["bitmap_words"], planned.N))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)

    def at(name):
        """the address of table `name` inside `tables`, null for an empty one"""
        off, nbytes = planned.segm_layout[name]
        return tables.data_ptr() + off if nbytes else None

    _lib.launch("om_segm_decode", device, planned.N, at("mask_hw"), at("mask_src_first"), at("mask_src_word_off"), at("mask_out_off"),
                c["n_poly"], c["n_srcs"], at("src_kind"), at("src_mask"), at("src_data_off"), at("src_len"), at("src_word_off"),
                at("poly"), at("counts"), at("strings"), c["bitmap_words"], ws if ws_bytes else None, ws_bytes, scratch)
    return scratch


def device_batches(loader, device):
    """Iterate a DataLoader whose collate is orienmask_amd.transform.collate, yielding the reference collate's tuples on `device`."""
    for planned in loader:
        yield to_device(planned, device)
