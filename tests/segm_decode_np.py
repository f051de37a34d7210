"""numpy model of stage 2 of csrc/segm_decode.hip (segm_pack_kernel) and the cases its tests share.  Not a test module.

Stage 1 is cocoeval.hip's and has its own model, tests/cocoeval_bitmap_np.py: source_bitmaps() below is the inside of its
build_mask (toggles, XOR, scan) without the merge, because stage 2 merges while it packs.  pack_rows() then walks the kernel's
tiles of 32 rows x 64 columns: OR of the sources' words, one "ballot" per row, bytes MSB first, min(8, ceil(w/8) - x0/8) bytes
per row segment.  It writes into a buffer that continues behind the mask and counts the writes of every byte, so that a store
outside the mask or a byte stored twice or never shows.  With variant=None it equals np.packbits(mask > 0, axis=1) of the
restatement (tests/cocoeval_np.py: ann_mask) on every case; each variant is a mistake the kernel could make.

Truth for a decoded mask everywhere: truth(segm, h, w) = np.packbits(ann_mask(segm, h, w, strict=False) > 0, axis=1)."""
import numpy as np

import cocoeval_bitmap_np as B
import cocoeval_cases as C
import cocoeval_np as ref

SENTINEL = 0xA5
VARIANTS = {
    "lsb_first": "column x goes to bit x & 7 of its byte (LSB first)",
    "pad_not_cleared": "lanes at columns >= w are not zeroed (modelled as ones): the pad bits of a row's last byte are set",
    "columns_from_64_dropped": "only the first column group is stored",
    "rows_past_h_stored": "every one of a band's 32 rows is stored, also past row h",
    "sources_not_ored": "the last source's word replaces the others instead of being ORed in",
    "last_group_one_byte_short": "the last column group stores one byte too few",
    "last_group_one_byte_over": "the last column group stores one byte too many",
}

# the sizes around the 64-column x 32-row tile
EXTRA_W = (7, 8, 63, 64, 65, 72, 128, 640)
EXTRA_H = (1, 31, 32, 33, 480)
MEAN = [123.675, 116.280, 103.530]


def truth(segm, h, w):
    return np.packbits(ref.ann_mask(segm, h, w, strict=False) > 0, axis=1)


def source_bitmaps(segm, h, w):
    """(h, w, [words of each source's bitmap]) -- what stage 1 leaves in the workspace"""
    h, w, srcs = B.sources_of(segm, h, w)
    maps = []
    for kind, data in srcs:
        if kind == "poly":
            pos = B.poly_toggles(data, h, w)
        elif kind == "counts":
            pos = B.counts_toggles(data, h, w)
        else:
            pos = B.string_toggles(data, h, w)
        maps.append(B.scan(B.toggle_bitmap(pos, h, w), h, w))
    return h, w, maps


def tail_bytes(w):
    """bytes of the model's buffer behind the mask: the rows a band can reach past h, and a byte over"""
    return 32 * ((w + 7) // 8) + 8


def pack_rows(maps, h, w, variant=None):
    """-> (buffer [h * wb + tail_bytes(w)] uint8, initialised to SENTINEL, writes per byte)"""
    hw, wb = (h + 31) // 32, (w + 7) // 8
    n = h * wb + tail_bytes(w)
    buf = np.full(n, SENTINEL, dtype=np.uint8)
    writes = np.zeros(n, dtype=np.int32)
    shifts = np.arange(8) if variant == "lsb_first" else 7 - np.arange(8)
    n_groups = (w + 63) // 64
    for tx in range(1 if variant == "columns_from_64_dropped" else n_groups):
        x0 = 64 * tx
        xs = x0 + np.arange(64)
        inside = xs < w
        for yb in range(hw):
            v = np.zeros(64, dtype=np.uint32)
            for words in maps:
                got = np.where(inside, words[np.minimum(xs, w - 1) * hw + yb], 0).astype(np.uint32)
                v = got if variant == "sources_not_ored" else v | got
            if variant == "pad_not_cleared":
                v = np.where(inside, v, 0xffffffff).astype(np.uint32)
            n_bytes = min(8, wb - x0 // 8)
            if tx == n_groups - 1:
                n_bytes += {"last_group_one_byte_short": -1, "last_group_one_byte_over": 1}.get(variant, 0)
            for r in range(32):
                y = 32 * yb + r
                if y >= h and variant != "rows_past_h_stored":
                    continue
                ballot = ((v >> np.uint32(r)) & 1).astype(np.int64).reshape(8, 8)         # [byte][column of the byte]
                row = np.append((ballot << shifts).sum(axis=1), 0).astype(np.uint8)       # a ninth byte for the one stored over
                at = y * wb + x0 // 8
                buf[at:at + n_bytes] = row[:n_bytes]
                writes[at:at + n_bytes] += 1
    return buf, writes


def model(segm, h, w, variant=None):
    h, w, maps = source_bitmaps(segm, h, w)
    return pack_rows(maps, h, w, variant)


def expected(want_rows, w):
    """the model's buffer when all is right: the truth, then untouched sentinels"""
    return np.concatenate([np.asarray(want_rows, dtype=np.uint8).ravel(), np.full(tail_bytes(w), SENTINEL, dtype=np.uint8)])


def random_mask(rng, h, w):
    """dense noise at the small sizes; at the large ones blocks with sparse noise, so that the counts stay a few thousand"""
    if h * w <= 20000:
        return (rng.random((h, w)) < 0.5).astype(np.uint8)
    blocks = rng.random(((h + 15) // 16, (w + 15) // 16)) < 0.4
    m = np.kron(blocks, np.ones((16, 16), bool))[:h, :w]
    return (m ^ (rng.random((h, w)) < 0.01)).astype(np.uint8)


_EXTRA = None


def extra_cases():
    """[(name, h, w, segm)] over EXTRA_H x EXTRA_W: a seeded random mask as uncompressed counts (its last column and last row
    forced to ones, so that the pad bits and the last band matter) and a merge of two overlapping polygons"""
    global _EXTRA
    if _EXTRA is None:
        rng = np.random.default_rng(C.SEED + 23)
        out = []
        for h in EXTRA_H:
            for w in EXTRA_W:
                m = random_mask(rng, h, w)
                m[-1, :] = 1
                m[:, -1] = 1
                out.append(("random_counts_%dx%d" % (h, w), h, w, {"size": [h, w], "counts": C.counts_of(m)}))
                a = C.star(9, h, w, inner=0.5, phase=0.3)
                b = C.rect(w * 0.55, -1.0, w + 2.0, h * 0.6 + 1)
                out.append(("two_polygons_%dx%d" % (h, w), h, w, [a, b]))
        _EXTRA = out
    return _EXTRA


def train_pipeline(size):
    """config/base.py: transform_train_544 at another output size"""
    return [dict(type="ColorJitter", brightness=0.2, contrast=0.5, saturation=0.5, hue=0.1),
            dict(type="RandomCrop", p=0.5, image_min_iou=0.64, bbox_min_iou=0.64),
            dict(type="Resize", size=list(size), pad_needed=True, warp_p=0.25, jitter=0.3, random_place=True, pad_p=0.75,
                 pad_ratio=0.75, pad_value=MEAN),
            dict(type="RandomHorizontalFlip", p=0.5), dict(type="ToTensor"),
            dict(type="Normalize", mean=[0, 0, 0], std=[255, 255, 255])]


def as_mask_sample(sample):
    """a 'segm' sample with its masks decoded by the restatement: what the reference's dataset would have handed over"""
    h, w = sample["image"].shape[:2]
    out = {k: v for k, v in sample.items() if k != "segm"}
    out["mask"] = [ref.ann_mask(s, h, w, strict=False) for s in sample["segm"]]
    if "info" in out:
        out["info"] = dict(out["info"])
    return out


def end_to_end_samples():
    """four images of 97 x 130, 65 x 65, 120 x 160 and 33 x 129: three polygons per GT, no GT, a crowd RLE among polygons, mixed"""
    from orienmask_amd import synth
    rng = np.random.default_rng(C.SEED + 5)

    def base(seed, h, w, segm):
        n = len(segm)
        s = synth.synth_segm_sample(seed, h, w, 0, image_id=seed)
        s["segm"] = segm
        s["bbox"] = np.clip(rng.uniform(0.1, 0.5, (n, 4)).astype(np.float32) + np.array([0.2, 0.2, 0, 0], np.float32), 0.05, 0.9)
        s["cls"] = rng.integers(0, 80, n).astype(np.int64)
        return s

    three = lambda h, w, k: [C.star(7 + k, h, w, inner=0.4, phase=0.2 * k, fill=0.3), C.rect(w * 0.1 * k, h * 0.1, w * 0.1 * k + w * 0.3, h * 0.5),
                             C.star(64, h, w, inner=0.8, phase=0.5, fill=0.2 + 0.05 * k)]
    crowd = np.zeros((120, 160), np.uint8)
    crowd[10:70, 5:90] = 1
    crowd[40:119, 100:160] = 1
    return [base(1, 97, 130, [three(97, 130, k) for k in range(3)]),
            base(2, 65, 65, []),
            base(3, 120, 160, [[C.star(30, 120, 160)], {"size": [120, 160], "counts": C.counts_of(crowd)},
                               {"size": [120, 160], "counts": C.to_string(C.counts_of(crowd.T.copy().reshape(120, 160)))}]),
            base(4, 33, 129, [[[10, 5, 20, 12]], [C.star(129, 33, 129)]])]
