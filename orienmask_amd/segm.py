"""COCO json segmentations as the device reads them: the sources of one annotation and the source tables of a set of masks.

Shared by ``cocoeval.py`` (``om_cocoeval_masks``: GT and result masks for the segm AP) and ``augment.py`` (``om_segm_decode``: the
GT masks of a training batch).  Host side only and numpy only: nothing here touches a pixel.

  sources(segm, h, w)        one annotation -> (mask h, mask w, [(kind, data)]) as pycocotools' annToRLE reads it
  pack_sources(srcs)         the [(kind, data)] of a sample's GTs as a few flat numpy arrays (picklable, no Python objects)
  unpack_sources(packed)     the inverse: [[(kind, data)] per GT]
  build_tables(masks)        [(h, w, [(kind, data)])] in mask order -> the arrays om_segm_decode takes, as one dict
"""
import numpy as np

POLY, COUNTS, STRING = 0, 1, 2
MAX_POLY_VERTICES = 4096        # csrc/cocoeval.hip: COCO_MAX_POLY
MAX_MASKS = 65535               # csrc/segm_decode.hip: one grid row per mask


def sources(segm, h, w):
    """One annotation's segmentation -> (mask h, mask w, [(kind, data)]) as pycocotools' annToRLE reads it."""
    if isinstance(segm, list):
        if len(segm) == 0:
            raise ValueError("empty segmentation list")
        if len(segm[0]) == 4:                       # frPyObjects: a list of boxes -> rleFrBbox
            out = []
            for b in segm:
                xs, ys, bw, bh = (float(v) for v in b)
                xe, ye = xs + bw, ys + bh
                out.append((POLY, np.array([xs, ys, xs, ye, xe, ye, xe, ys], dtype=np.float64)))
            return h, w, out
        if len(segm[0]) < 4:
            raise ValueError("segmentation polygon with fewer than 4 numbers")
        out = []
        for p in segm:
            a = np.asarray(p, dtype=np.float64)
            if a.size // 2 > MAX_POLY_VERTICES:
                raise ValueError("polygon with %d vertices (at most %d)" % (a.size // 2, MAX_POLY_VERTICES))
            out.append((POLY, a))
        return h, w, out
    rh, rw = int(segm["size"][0]), int(segm["size"][1])
    counts = segm["counts"]
    if isinstance(counts, list):
        return rh, rw, [(COUNTS, np.asarray(counts, dtype=np.uint32))]
    if isinstance(counts, bytes):
        counts = counts.decode("ascii")
    return rh, rw, [(STRING, counts.encode("ascii"))]


def _data_array(kind, data):
    if kind == POLY:
        return np.asarray(data, dtype=np.float64).reshape(-1)
    if kind == COUNTS:
        return np.asarray(data, dtype=np.uint32).reshape(-1)
    return np.frombuffer(bytes(data), dtype=np.uint8)


_DTYPES = {POLY: np.float64, COUNTS: np.uint32, STRING: np.uint8}
_NAMES = {POLY: "poly", COUNTS: "counts", STRING: "strings"}


def pack_sources(srcs):
    """[[(kind, data)] per GT] -> dict of flat arrays: per source its kind, GT and length, in GT order and json order within a
    GT; the data of each kind concatenated in that same order."""
    kind, gt, length = [], [], []
    data = {POLY: [], COUNTS: [], STRING: []}
    for g, lst in enumerate(srcs):
        for k, d in lst:
            a = _data_array(k, d)
            kind.append(k); gt.append(g); length.append(a.size)
            data[k].append(a)
    out = dict(n_gt=len(srcs), kind=np.array(kind, dtype=np.int32), gt=np.array(gt, dtype=np.int32),
               len=np.array(length, dtype=np.int32))
    for k, name in _NAMES.items():
        out[name] = np.concatenate(data[k]) if data[k] else np.zeros(0, _DTYPES[k])
    return out


def unpack_sources(packed):
    """pack_sources' inverse; a string comes back as bytes."""
    out = [[] for _ in range(int(packed["n_gt"]))]
    pos = {POLY: 0, COUNTS: 0, STRING: 0}
    for k, g, n in zip(packed["kind"].tolist(), packed["gt"].tolist(), packed["len"].tolist()):
        a = packed[_NAMES[k]][pos[k]:pos[k] + n]
        pos[k] += n
        out[g].append((k, a.tobytes() if k == STRING else a))
    return out


def build_tables(masks, out_off):
    """masks: [(h, w, [(kind, data)])] in mask order; out_off[m]: byte offset of mask m's packed rows.  Returns the arrays of
    om_segm_decode (include/orienmask_hip.h) by name, plus n_poly, n_srcs and bitmap_words.  Every source gets a bitmap of its own
    (w * ceil(h / 32) words); the kernel wants the polygons at sources [0, n_poly), so the source table is the polygons in mask
    order, then the sequences in mask order, and mask_src_word_off lists each mask's bitmaps in json order."""
    n = len(masks)
    if n > MAX_MASKS:
        raise ValueError("%d masks in one call (at most %d)" % (n, MAX_MASKS))
    mask_hw = np.zeros((n, 2), dtype=np.int32)
    src_first = np.zeros(n + 1, dtype=np.int32)
    polys, seqs, merge = [], [], []                 # (mask, kind, data array, word offset)
    words = 0
    for m, (h, w, srcs) in enumerate(masks):
        if h <= 0 or w <= 0:
            raise ValueError("mask %d: empty size %dx%d" % (m, h, w))
        mask_hw[m] = (h, w)
        for kind, data in srcs:
            a = _data_array(kind, data)
            if kind == POLY and a.size // 2 > MAX_POLY_VERTICES:
                raise ValueError("polygon with %d vertices (at most %d)" % (a.size // 2, MAX_POLY_VERTICES))
            (polys if kind == POLY else seqs).append((m, kind, a, words))
            merge.append(words)
            words += w * ((h + 31) // 32)
        src_first[m + 1] = src_first[m] + len(srcs)
    table = polys + seqs
    data = {POLY: [], COUNTS: [], STRING: []}
    pos = {POLY: 0, COUNTS: 0, STRING: 0}
    src_data_off = np.zeros(len(table), dtype=np.int64)
    for s, (_, k, a, _) in enumerate(table):
        src_data_off[s] = pos[k]
        pos[k] += a.size
        data[k].append(a)
    out = dict(mask_hw=mask_hw.reshape(-1), mask_src_first=src_first, mask_src_word_off=np.array(merge, dtype=np.int64),
               mask_out_off=np.asarray(out_off, dtype=np.int64).reshape(n),
               src_kind=np.array([t[1] for t in table], dtype=np.int32), src_mask=np.array([t[0] for t in table], dtype=np.int32),
               src_data_off=src_data_off, src_len=np.array([t[2].size for t in table], dtype=np.int32),
               src_word_off=np.array([t[3] for t in table], dtype=np.int64))
    for k, name in _NAMES.items():
        out[name] = np.concatenate(data[k]) if data[k] else np.zeros(0, _DTYPES[k])
    return out, dict(n_poly=len(polys), n_srcs=len(table), bitmap_words=int(words))


# order of the arrays in collate's segm buffer: 8-byte types first is not needed, every array starts at a 16-byte offset
TABLE_ORDER = ("mask_hw", "mask_src_first", "mask_src_word_off", "mask_out_off", "src_kind", "src_mask", "src_data_off", "src_len",
               "src_word_off", "poly", "counts", "strings")
TABLE_DTYPES = dict(mask_hw=np.int32, mask_src_first=np.int32, mask_src_word_off=np.int64, mask_out_off=np.int64,
                    src_kind=np.int32, src_mask=np.int32, src_data_off=np.int64, src_len=np.int32, src_word_off=np.int64,
                    poly=np.float64, counts=np.uint32, strings=np.uint8)
