"""The reference's datasets (data/dataset.py: BaseDataset, COCODataset, VOCDataset) without pandas and without pycocotools.

Same constructor signatures, tables and method split as the reference, so ``build(config, module)`` resolves them from a
reference config unchanged and ``val_loader.dataset.CAT2LABEL`` / ``.with_mask`` read as they do there.  What differs:

  * the list file is read with the ``csv`` module (first column = the key, ``sample_path[0]`` in the reference);
  * with ``with_mask`` a sample carries ``'segm'``: the annotation json's own segmentation objects, one per GT, instead of
    ``'mask'`` (full-resolution arrays decoded by pycocotools).  ``orienmask_amd.transform.COCOTransform`` takes either; 'segm'
    is decoded on the device (``om_segm_decode``), so the loader worker touches no mask pixel;
  * the image is uint8 RGB, not float32: the augmentation kernels read either and the results are bit-identical
    (tests/test_augment.py::test_uint8_transport_bit_identical_to_float32).

``imread`` is a callable from a path to an [h,w,3] RGB uint8 array.  The default decodes with cv2 exactly as the reference does
(``cv2.imread`` + ``COLOR_BGR2RGB``) when cv2 can be imported and with PIL (``Image.open(p).convert('RGB')``) otherwise.  PIL's
JPEG decoder is NOT pinned to cv2's: the two may differ in the last bits of a pixel.  Lossless formats (PNG, BMP) decode
identically.  The project's own JPEG decoder (``orienmask_amd.jpeg``: host entropy decoding, HIP IDCT and colour) IS pinned: bit
for bit PIL's pixels.

A host-only reader of your own goes in as ``COCODataset(..., imread=my_reader)``: any callable path -> [h,w,3] uint8 RGB that
touches no GPU, since it runs in the loader's worker processes.  Of the JPEG decoder a worker may call the two HOST entries
(``jpeg.host_info`` / ``jpeg.host_entropy_decode``, i.e. ``om_jpeg_info`` and ``om_jpeg_entropy_decode``: they make no HIP
call), never ``om_jpeg_decode_batch`` or ``JpegDecoder.decode``: those launch kernels and belong to the process that owns the
device.  Carrying coefficients through ``collate`` into the training augmentation is not done yet.
"""
import csv
import json
import os

import numpy as np
from torch.utils.data import Dataset

from .visualizer import CAT2LABEL as _CAT2LABEL, CLASSES as _CLASSES


def _default_imread():
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        def imread(path):
            image = cv2.imread(path)
            if image is None:
                raise FileNotFoundError("cannot read image %s" % path)
            return cv2.cvtColor(image, cv2.COLOR_BGR2RGB)
        return imread
    from PIL import Image

    def imread(path):
        with Image.open(path) as im:
            return np.asarray(im.convert('RGB'), dtype=np.uint8)
    return imread


class BaseDataset(Dataset):
    """One sample per line of `list_file` (a csv without header; the first column is the image's path under `image_dir` and the
    key of its annotation).  __getitem__ = _transform(_load_sample_data(row))."""

    def __init__(self, list_file, image_dir, anno_file, transform):
        with open(list_file, newline='') as f:
            self.samples = [row for row in csv.reader(f) if row]
        self.image_dir = image_dir
        self.anno_file = anno_file
        self.transform = transform

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, idx):
        return self._transform(self._load_sample_data(list(self.samples[idx])))

    def _load_sample_data(self, sample_path):
        raise NotImplementedError

    def _transform(self, sample):
        return self.transform(sample)


class COCODataset(BaseDataset):
    """anno_file: {key: {'image_id': id, 'anno': {'bbox': [[cx, cy, w, h] normalised], 'cls': [label], 'mask': [segmentation]}}},
    the label json of the reference's tools.  imread: a host-only reader, path -> [h,w,3] uint8 RGB (the module docstring says
    what it may call); None: cv2 as the reference reads, else PIL."""
    CAT2LABEL = list(_CAT2LABEL["COCO"])
    CLASSES = list(_CLASSES["COCO"])

    def __init__(self, list_file, image_dir, anno_file, transform, with_mask=True, with_info=True, imread=None):
        super().__init__(list_file, image_dir, anno_file, transform)
        with open(self.anno_file) as f:
            self.annotations = json.load(f)
        self.with_mask = with_mask
        self.with_info = with_info
        self.imread = imread if imread is not None else _default_imread()

    def _load_sample_data(self, sample_path):
        key = sample_path[0]
        image = np.ascontiguousarray(self.imread(os.path.join(self.image_dir, key)), dtype=np.uint8)
        entry = self.annotations[key]
        anno = entry['anno']
        sample = {'image': image, 'bbox': np.array(anno['bbox']).astype(np.float32).reshape(-1, 4),
                  'cls': np.array(anno['cls']).astype(np.int64)}
        if self.with_mask:
            sample['segm'] = list(anno['mask'])         # the json objects themselves: decoded on the device
        if self.with_info:
            sample['info'] = {'id': entry['image_id'], 'height': image.shape[0], 'width': image.shape[1]}
        return sample


class VOCDataset(COCODataset):
    CAT2LABEL = list(_CAT2LABEL["VOC"])
    CLASSES = list(_CLASSES["VOC"])

    def __init__(self, list_file, image_dir, anno_file, transform, with_mask=False, with_info=True, imread=None):
        super().__init__(list_file, image_dir, anno_file, transform, with_mask, with_info, imread)
