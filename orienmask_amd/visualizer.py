"""InferenceVisualizer on the HIP path: a drop-in for the reference's utils/visualizer.py (lines 33-127).

``InferenceVisualizer(dataset, device, ...)(detections, image, pad_info)`` returns the same uint8 ``[h,w,3]`` numpy image,
prints the same lines and makes the same ``random.randint`` call as the reference.  Its device part -- crop of the paddings,
bilinear resize of every kept mask to the original image, ascending sort by resized area, plot_all_mask's alpha composite and
round() -- is one pass of ``om_visualize`` (csrc/visualize.hip) over the output, without the reference's ``[K,h,w,3]`` float
intermediates (2.5 GB for 100 detections on a 1080 x 1920 photo).  The boxes and labels are then drawn with cv2 on the host
exactly as the reference draws them; without cv2 the kernel can draw the thickness-1 box outlines itself (``draw='device'``).

``composite`` does the device part for a list of images of different sizes in one launch pair and draws nothing.
"""
import importlib
import random
import warnings

import torch
import torch.nn.functional as F

from . import lib as _lib

# utils/visualizer.py:10-30
PALETTE = (
    (244, 67, 54),
    (233, 30, 99),
    (156, 39, 176),
    (103, 58, 183),
    (63, 81, 181),
    (33, 150, 243),
    (3, 169, 244),
    (0, 188, 212),
    (0, 150, 136),
    (76, 175, 80),
    (139, 195, 74),
    (205, 220, 57),
    (255, 235, 59),
    (255, 193, 7),
    (255, 152, 0),
    (255, 87, 34),
    (121, 85, 72),
    (158, 158, 158),
    (96, 125, 139),
)

# data/dataset.py: COCODataset.CLASSES / VOCDataset.CLASSES, the names the visualiser prints and draws
CLASSES = {
    "COCO": (
        'person', 'bicycle', 'car', 'motorbike', 'aeroplane', 'bus', 'train', 'truck',
        'boat', 'traffic-light', 'fire-hydrant', 'stop-sign', 'parking-meter', 'bench',
        'bird', 'cat', 'dog', 'horse', 'sheep', 'cow', 'elephant', 'bear', 'zebra',
        'giraffe', 'backpack', 'umbrella', 'handbag', 'tie', 'suitcase', 'frisbee', 'skis',
        'snowboard', 'sports-ball', 'kite', 'baseball-bat', 'baseball-glove', 'skateboard',
        'surfboard', 'tennis-racket', 'bottle', 'wine-glass', 'cup', 'fork', 'knife',
        'spoon', 'bowl', 'banana', 'apple', 'sandwich', 'orange', 'broccoli', 'carrot',
        'hot-dog', 'pizza', 'donut', 'cake', 'chair', 'sofa', 'potted-plant', 'bed',
        'dining-table', 'toilet', 'tv-monitor', 'laptop', 'mouse', 'remote', 'keyboard',
        'cell-phone', 'microwave', 'oven', 'toaster', 'sink', 'refrigerator', 'book',
        'clock', 'vase', 'scissors', 'teddy-bear', 'hair-drier', 'toothbrush'),
    "VOC": (
        'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair',
        'cow', 'dining-table', 'dog', 'horse', 'motorbike', 'person', 'potted-plant',
        'sheep', 'sofa', 'train', 'tv-monitor'),
}

# data/dataset.py: COCODataset.CAT2LABEL / VOCDataset.CAT2LABEL
CAT2LABEL = {
    "COCO": (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17,
             18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 31, 32, 33, 34, 35, 36,
             37, 38, 39, 40, 41, 42, 43, 44, 46, 47, 48, 49, 50, 51, 52, 53,
             54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 67, 70, 72, 73,
             74, 75, 76, 77, 78, 79, 80, 81, 82, 84, 85, 86, 87, 88, 89, 90),
    "VOC": tuple(range(1, 21)),
}

_DRAW_MODES = ("auto", "cv2", "device")


class InferenceVisualizer:
    """utils/visualizer.py:InferenceVisualizer, plus ``draw``: 'cv2' draws boxes and labels with cv2 as the reference does;
    'device' draws the thickness-1 box outlines in the kernel (no label text); 'auto' is cv2 when it can be imported, else
    device outlines and one warning."""

    def __init__(self, dataset, device, with_mask=True, conf_thresh=0.3, alpha=0.5, line_thickness=1, draw="auto"):
        if dataset not in CLASSES:
            raise ValueError("dataset must be one of %s, got %r" % (sorted(CLASSES), dataset))
        if draw not in _DRAW_MODES:
            raise ValueError("draw must be one of %s, got %r" % (_DRAW_MODES, draw))
        if draw == "device" and line_thickness != 1:
            raise ValueError("device outlines are drawn at thickness 1 only (line_thickness=%r)" % (line_thickness,))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.OrienMaskHipError("InferenceVisualizer needs an MI355X device (got %s); this path has no CPU fallback"
                                         % self.device)
        self.dataset = dataset
        self.classes = list(CLASSES[dataset])
        self.with_mask = with_mask
        self.conf_thresh = conf_thresh
        self.alpha = alpha
        self.line_thickness = line_thickness
        self.draw = draw
        self._tables = None
        self._warned = False

    # the reference's device tables, made on first use (building the visualiser touches no device)
    @property
    def palette(self):
        return self._device_tables()[0]

    @property
    def cat2label(self):
        return self._device_tables()[1]

    def _device_tables(self):
        if self._tables is None:
            self._tables = (torch.tensor(PALETTE, dtype=torch.float32, device=self.device),
                            torch.tensor(CAT2LABEL[self.dataset], dtype=torch.uint8, device=self.device))
        return self._tables

    # ---- the reference's __call__ ------------------------------------------------------------------------------------
    def __call__(self, detections, image, pad_info):
        cv2 = self._cv2()
        item = self._prepare(detections, image, pad_info)
        out = torch.empty(image.shape, dtype=torch.uint8, device=image.device)
        self._launch([item], [out], draw_boxes=cv2 is None)
        pred_show = out.cpu().numpy()
        if item["n"] > 0:
            xyxy = item["xyxy"].cpu()
            scores = item["scores"].cpu()
            colors = item["colors"].cpu()
            for xy, score, cls, color in zip(xyxy, scores, item["names"], colors):
                print(xy.tolist(), score.item(), cls)
                if cv2 is not None:
                    text = '%s %.2f' % (cls, score.item())
                    self._plot_one_box(cv2, xy, text, pred_show, color=color.tolist())
        return pred_show

    def composite(self, dets_list, images, pad_infos):
        """The device part of __call__ for several images at once (one launch pair): a list of uint8 [h,w,3] device
        tensors, no boxes drawn, nothing printed.  random.randint is called once per image with a kept detection, in order,
        as consecutive __call__s would."""
        if not (len(dets_list) == len(images) == len(pad_infos)):
            raise ValueError("composite: %d detections, %d images, %d pad_infos" % (len(dets_list), len(images), len(pad_infos)))
        items = [self._prepare(d, im, p) for d, im, p in zip(dets_list, images, pad_infos)]
        outs = [torch.empty(im.shape, dtype=torch.uint8, device=im.device) for im in images]
        self._launch(items, outs, draw_boxes=False)
        return outs

    def _composite_float(self, detections, image, pad_info, with_areas=False):
        """Test entry: (uint8 composite, float32 composite before round()) of one image, no boxes drawn; with_areas: also the
        kept masks' resized areas the composite sorted by (float64, kept order)."""
        item = self._prepare(detections, image, pad_info)
        out = torch.empty(image.shape, dtype=torch.uint8, device=image.device)
        out_f = torch.empty(image.shape, dtype=torch.float32, device=image.device)
        ws = self._launch([item], [out], draw_boxes=False, out_floats=[out_f])
        if not with_areas:
            return out, out_f
        n = item["n"] if item["mask"] is not None else 0
        return out, out_f, ws[:32 * n].view(torch.float64).view(n, 4)[:, 0]    # VisMaskStat: 32 bytes, the area first

    # ---- helpers ------------------------------------------------------------------------------------------------------
    def _cv2(self):
        """The cv2 module to draw with, or None for device outlines."""
        if self.draw == "device":
            return None
        try:
            return importlib.import_module("cv2")
        except ImportError:
            if self.draw == "cv2":
                raise
        if self.line_thickness != 1:
            raise ValueError("cv2 is not importable and device outlines are drawn at thickness 1 only (line_thickness=%r)"
                             % (self.line_thickness,))
        if not self._warned:
            warnings.warn("InferenceVisualizer: cv2 is not importable; drawing box outlines on the device, without labels")
            self._warned = True
        return None

    def _prepare(self, detections, image, pad_info):
        """Filter, boxes, colours (with the reference's random.randint call) and the keep list of one image."""
        _lib.require_cuda_tensor(image, "image", torch.float32)
        if image.dim() != 3 or image.shape[2] != 3:
            raise ValueError("image must be [h,w,3], got %s" % (tuple(image.shape),))
        bbox = detections["bbox"]
        _lib.require_cuda_tensor(bbox, "detections['bbox']", torch.float32)
        height, width = int(image.shape[0]), int(image.shape[1])
        keep = torch.nonzero(bbox[:, -1] > self.conf_thresh).reshape(-1)       # float32 comparison, as the reference
        n = int(keep.numel())
        item = dict(image=image, n=n, pad=[int(v) for v in pad_info], mask=None)
        if n == 0:
            return item
        if n > _lib.OM_VIS_MAX_KEPT:
            raise ValueError("InferenceVisualizer: %d detections above conf_thresh, at most %d supported" % (n, _lib.OM_VIS_MAX_KEPT))
        kept = bbox[keep]
        item["xyxy"] = self._recover_shape_bbox(kept[:, :4], width, height, pad_info)
        item["scores"] = kept[:, -1]
        item["names"] = [self.classes[c] for c in detections["cls"][keep].tolist()]
        colors_idx = torch.arange(n) * 5 + random.randint(1, self.palette.size(0))
        item["colors"] = self.palette[(colors_idx % self.palette.size(0)).to(self.palette.device)].contiguous()
        item["keep"] = keep.to(torch.int32)
        if self.with_mask:
            mask = detections["mask"]
            _lib.require_cuda_tensor(mask, "detections['mask']")
            if mask.dtype not in (torch.bool, torch.uint8):
                raise _lib.OrienMaskHipError("detections['mask'] must be bool or uint8, got %s" % mask.dtype)
            if mask.dim() != 3 or mask.shape[0] != bbox.shape[0]:
                raise ValueError("detections['mask'] must be [K,H,W] with K = %d, got %s" % (bbox.shape[0], tuple(mask.shape)))
            item["mask"] = mask.contiguous().view(torch.uint8)
        return item

    def _launch(self, items, outs, draw_boxes, out_floats=None):
        imgs = (_lib.VisImage * len(items))()
        alive = []                      # tensors whose pointers the descriptors hold, until the launch is enqueued
        dev = items[0]["image"].device
        for i, (it, out) in enumerate(zip(items, outs)):
            src = it["image"].contiguous()
            if src.data_ptr() % 16:
                src = src.clone()
            h, w = int(src.shape[0]), int(src.shape[1])
            d = imgs[i]
            d.image, d.out, d.h, d.w = src.data_ptr(), out.data_ptr(), h, w
            d.out_float = out_floats[i].data_ptr() if out_floats is not None else None
            d.n_keep = it["n"]
            d.alpha = float(self.alpha)
            d.with_mask = int(bool(self.with_mask))
            d.crop_left, d.crop_right, d.crop_top, d.crop_down = it["pad"][:4]
            alive.append(src)
            if it["n"] > 0:
                boxes = it["xyxy"].to(torch.int32).contiguous()
                d.keep, d.colors, d.boxes = it["keep"].data_ptr(), it["colors"].data_ptr(), boxes.data_ptr()
                d.draw_boxes = int(draw_boxes)
                alive.append(boxes)
                if it["mask"] is not None:
                    m = it["mask"]
                    d.mask, d.Hn, d.Wn = m.data_ptr(), int(m.shape[1]), int(m.shape[2])
        ws = torch.empty(int(_lib.load().om_visualize_workspace_bytes(imgs, len(items))), dtype=torch.uint8, device=dev)
        _lib.launch("om_visualize", dev, imgs, len(items), ws, ws.numel())
        del alive
        return ws

    def _plot_one_box(self, cv2, bbox, text, image, color):
        """utils/visualizer.py:84-93, call for call."""
        x1, y1, x2, y2 = bbox.cpu().tolist()
        cv2.rectangle(image, (x1, y1), (x2, y2), color, thickness=self.line_thickness)

        font_face = cv2.FONT_HERSHEY_DUPLEX
        text_pt = (x1, y1 - 3)
        text_color = [255, 255, 255]
        font_scale = 0.4
        font_thickness = 1
        text_w, text_h = cv2.getTextSize(text, font_face, font_scale, font_thickness)[0]
        cv2.rectangle(image, (x1, y1), (x1 + text_w, y1 - text_h - 4), color, -1)
        cv2.putText(image, text, text_pt, font_face, font_scale, text_color, font_thickness, cv2.LINE_AA)

    # ---- the reference's classmethods (utils/visualizer.py:102-126): plain tensor arithmetic, any device --------------
    @classmethod
    def _recover_shape_bbox(cls, bbox, width, height, pad_info):
        bx, by, bw, bh = bbox.split(1, dim=-1)

        left, right, top, down, h, w = pad_info
        nh = h - top - down
        nw = w - left - right
        bx = (bx * w - left) / nw
        by = (by * h - top) / nh
        bw = bw * w / nw
        bh = bh * h / nh

        bx1 = (bx - bw / 2) * width
        by1 = (by - bh / 2) * height
        bx2 = (bx + bw / 2) * width
        by2 = (by + bh / 2) * height
        xyxy = torch.cat([bx1, by1, bx2, by2], dim=-1)
        return xyxy.round().long()

    @classmethod
    def _recover_shape_segm(cls, mask, width, height, pad_info):
        left, right, top, down = pad_info[:4]
        mask = mask[:, top:-down if down else None, left:-right if right else None]
        mask = F.interpolate(mask.float().unsqueeze(0), size=(height, width), mode='bilinear', align_corners=False)
        return mask.squeeze(0)
