"""The resize kernels over image geometries: preprocess.hip, coco_format.hip (boxes, resized masks, run lengths, strings) and
visualize.hip, at every entry of tests/geometry_np.py's table (val2017-typical sizes, tiny and word-boundary sizes, extreme
aspect ratios and scales, the RLE kernel's LDS boundary, letterbox and collate crops, all four flip combinations).

CPU: the float64 restatement agrees with the torch-CPU oracle everywhere on the table (the tool), and every plausible wrong
variant of the float32 arithmetic disagrees with torch somewhere on it (its teeth).
GPU: each kernel equals the oracle bit for bit and satisfies the float64 bounds of geometry_np's docstring.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

import geometry_np as G
from oracle import orienmask_ref as R

TABLE = G.table()
BIG = 400_000                 # output pixels above which a geometry gets four mask families instead of all of them
_CACHE = {}                   # torch-CPU oracle results shared by the CPU and GPU tests of one session


def _families(geo):
    if geo.info["height"] * geo.info["width"] <= BIG:
        return G.MASK_FAMILIES
    i = [g.name for g in TABLE].index(geo.name) if geo in TABLE else 0
    return tuple(G.MASK_FAMILIES[(4 * i + j) % len(G.MASK_FAMILIES)] for j in range(4))


def _seed(geo):
    return sum(ord(c) for c in geo.name)


def _masks(geo):
    key = ("masks", geo.name, geo.H, geo.W)
    if key not in _CACHE:
        _CACHE[key] = G.mask_stack(geo.H, geo.W, _seed(geo), _families(geo))
    return _CACHE[key]


def _segm_oracle(geo):
    """R.recover_shape_segm of the geometry's masks: uint8 [K,oh,ow]."""
    key = ("segm", geo.name, geo.H, geo.W)
    if key not in _CACHE:
        _CACHE[key] = R.recover_shape_segm(torch.from_numpy(_masks(geo)), geo.info).numpy()
    return _CACHE[key]


def _chunks(n, geo):
    step = max(1, 4_000_000 // max(1, geo.info["height"] * geo.info["width"]))
    return [slice(i, min(n, i + step)) for i in range(0, n, step)]


def _check_mask_rule(got_u8, geo, tag):
    masks = _masks(geo)
    for sl in _chunks(len(masks), geo):
        v64, bound = G.resize64(G.crop_flip(masks[sl], geo.info).astype(np.float64), geo.info["height"], geo.info["width"],
                                with_bound=True)
        bad = G.mask_rule(got_u8[sl], v64, bound)
        assert bad.size == 0, "%s %s: %d pixels disagree with float64 away from 0.5 (first [k,y,x] = %s, v64 = %r)" % (
            tag, geo.name, len(bad), (bad[0] + [sl.start, 0, 0]).tolist(), float(v64[tuple(bad[0])]))


def _photo(n, h, w, seed, kind):
    """[n,h,w,3] float32 in [0, 255]: 'int' values, 'frac' non-integer values, 'edges' hard-edged blocks of 0 / 255 with
    fractional noise on top (where the fma placement shows: large tap differences)."""
    rng = np.random.default_rng(seed)
    if kind == "int":
        x = np.floor(rng.random((n, h, w, 3)) * 256)
    elif kind == "frac":
        x = rng.random((n, h, w, 3)) * 255
    else:
        by, bx = max(1, h // 7), max(1, w // 5)
        yy, xx = np.mgrid[0:h, 0:w]
        x = np.where((((yy // by) + (xx // bx)) % 2 == 0)[None, :, :, None], 255.0, 0.0) + rng.random((n, h, w, 3)) * 0.37
        x = np.minimum(x, 255.0)
    return torch.from_numpy(x.astype(np.float32))


MEAN_STD = {"255": ((0, 0, 0), (255, 255, 255)), "imagenet": ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375))}


def _targets(h, w):
    """The resizes of the sweep: Resize(544), Resize((odd, odd)), ShortEdgeResize(544, 1333), and two Resizes on either side of
    torch's small-output threshold (height + width = 128 and 129)."""
    return [("resize544", (544, 544)), ("resize_odd", ((h * 3) // 4 | 1, (w * 5) // 4 | 1)),
            ("short_edge", G.short_edge_target(h, w, 544, 1333)), ("small_128", (61, 67)), ("small_129", (61, 68))]


# ========================================================================================================================= CPU
@pytest.mark.parametrize("geo", TABLE, ids=[g.name for g in TABLE])
def test_restatement_agrees_with_oracle_masks(geo):
    """2(a), mask path: torch's rounded masks obey the MASK RULE against float64, the unrounded F.interpolate values are within
    the FLOAT BOUND, the float32 restatement equals torch bit for bit, and the bitmap run lengths equal R.rle_counts."""
    masks = _masks(geo)
    want = _segm_oracle(geo)
    oh, ow = geo.info["height"], geo.info["width"]
    assert want.shape == (len(masks), oh, ow)
    _check_mask_rule(want, geo, "torch")
    for sl in _chunks(len(masks), geo):
        crop = G.crop_flip(masks[sl], geo.info)
        v64, bound = G.resize64(crop.astype(np.float64), oh, ow, with_bound=True)
        vt = R.interpolate_bilinear(torch.from_numpy(crop.astype(np.float32))[None], (oh, ow))[0].numpy()
        err = np.abs(vt - v64) - bound
        assert err.max() <= 0, (geo.name, float(err.max()))
        assert np.array_equal(G.recover_segm32(masks[sl], geo.info), want[sl]), geo.name
    for k in range(len(masks)):
        assert G.rle_counts_bitmap(want[k]) == R.rle_counts(want[k]), (geo.name, k)


@pytest.mark.parametrize("geo", TABLE, ids=[g.name for g in TABLE])
def test_restatement_agrees_with_oracle_floats(geo):
    """2(a), float path: R.fast_coco_transform + R.pad_to_divisor against preprocess64 within the FLOAT BOUND, and the float32
    restatement of the resize equal to torch bit for bit, on the geometry's original size."""
    h, w = geo.info["height"], geo.info["width"]
    img = _photo(1, h, w, _seed(geo), ("edges", "frac", "int")[_seed(geo) % 3])
    for tname, size in _targets(h, w):
        mean, std = MEAN_STD["imagenet" if tname == "short_edge" else "255"]
        want, info = R.pad_to_divisor(R.fast_coco_transform(img, size, mean, std), 32, 0)
        v64, bound, info64 = G.preprocess64(img.numpy(), size, mean, std)
        assert info64 == info, (geo.name, tname)
        err = np.abs(want.numpy() - v64) - bound
        assert err.max() <= 0, (geo.name, tname, float(err.max()))
        plain = R.fast_coco_transform(img, size, (0, 0, 0), (1, 1, 1)).numpy()
        assert np.array_equal(G.resize32(img.numpy().transpose(0, 3, 1, 2), *size), plain), (geo.name, tname)


MASK_VARIANTS = ["round_half_up", "crop_top", "crop_down", "crop_left", "crop_right", "flip_before_crop", "i1_past",
                 "swap_scales", "generic_blend"]
FLOAT_VARIANTS = ["unfused", "scale_double", "i1_past", "swap_scales", "generic_blend", "small_lt", "small_129"]


def test_teeth_every_wrong_variant_is_caught():
    """2(b): each plausible bug of the float32 arithmetic disagrees with torch on at least one geometry of the table (printed
    with -s).  A variant nobody catches means the table lacks a case."""
    caught = {}
    for var in MASK_VARIANTS:
        for geo in TABLE:
            got = G.recover_segm32(_masks(geo), geo.info, var)
            if got is not None and not np.array_equal(got, _segm_oracle(geo)):
                caught["mask:" + var] = geo.name
                break
    for geo in TABLE:
        want = _segm_oracle(geo)
        if any(G.rle_counts_bitmap(want[k], "tail_bit") != R.rle_counts(want[k]) for k in range(len(want))):
            caught["counts:tail_bit"] = geo.name
            break
    for var in FLOAT_VARIANTS:
        for geo in TABLE:
            h, w = geo.info["height"], geo.info["width"]
            img = _photo(1, h, w, _seed(geo), "edges")
            for tname, size in _targets(h, w)[1:]:
                want = R.fast_coco_transform(img, size, (0, 0, 0), (1, 1, 1)).numpy()
                if not np.array_equal(G.resize32(img.numpy().transpose(0, 3, 1, 2), *size, variant=var), want):
                    caught["float:" + var] = "%s %s" % (geo.name, tname)
                    break
            if "float:" + var in caught:
                break
    for k, v in sorted(caught.items()):
        print("teeth: %-24s caught at %s" % (k, v))
    expected = ["mask:" + v for v in MASK_VARIANTS] + ["counts:tail_bit"] + ["float:" + v for v in FLOAT_VARIANTS]
    missed = [v for v in expected if v not in caught]
    assert not missed, "no table geometry catches %s" % missed


def test_table_holds_the_boundaries():
    names = [g.name for g in TABLE]
    (eh, ew), (ah, aw), (bh, bw) = G.lds_boundary()
    cap = G.rle_lds_max(G.MI355X_LDS_PER_BLOCK)
    assert cap == 153600 and G.rle_lds_bytes(eh, ew) == cap
    sizes = {(g.info["height"], g.info["width"]) for g in TABLE}
    assert {(eh, ew), (ah, aw), (bh, bw), (1080, 1920), (1, 1), (1, 7), (7, 1), (2, 3), (31, 33), (17, 17), (7, 7)} <= sizes
    assert {31, 32, 33, 63, 64, 65} <= {g.info["height"] for g in TABLE}
    assert {(bool(g.info["hflip"]), bool(g.info["vflip"])) for g in TABLE} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert any("collate_pad" in g.info and "pad" in g.info for g in TABLE) and "up_136_to_1920" in names
    outs = {g.info["height"] + g.info["width"] for g in TABLE}
    assert {G.SMALL_OUT, G.SMALL_OUT + 1} <= outs and "small_crop_37x34_to_33x31" in names


# ========================================================================================================================= GPU
@pytest.fixture(scope="module")
def dev(built):
    from orienmask_amd import lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib.load()
    return torch.device("cuda:0")


def _device_lds_per_block():
    """hipDeviceAttributeMaxSharedMemoryPerBlock of device 0, what coco_format.hip's rle_lds_max() reads."""
    hip = ctypes.CDLL("libamdhip64.so")
    v = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(v), 74, 0) == 0       # 74: hipDeviceAttributeMaxSharedMemoryPerBlock
    return v.value


def _bbox(geo, K):
    g = torch.Generator().manual_seed(_seed(geo))
    return torch.cat([torch.rand(K, 2, generator=g) * 1.2 - 0.1, torch.rand(K, 2, generator=g) * 0.9 + 0.01,
                      torch.rand(K, 1, generator=g)], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", TABLE, ids=[g.name for g in TABLE])
def test_coco_format_geometry(dev, geo):
    """recover_shape_bbox bit-exact and within 8 ulp (of the value plus the image side) of float64; recover_masks_rle's resized
    masks bit-exact and under the MASK RULE, its strings those of R.rle_to_string(R.rle_counts(.)) and decoding to them."""
    from orienmask_amd import coco_format as CF
    masks = _masks(geo)
    K = len(masks)
    bbox = _bbox(geo, K)
    got = CF.recover_shape_bbox(bbox.to(dev), geo.info).cpu().numpy()
    assert np.array_equal(got, R.recover_shape_bbox(bbox, geo.info).numpy()), geo.name
    b64 = G.recover_shape_bbox64(bbox.numpy(), geo.info)
    side = max(geo.info["height"], geo.info["width"])
    assert (np.abs(got - b64) <= 8 * G.EPS32 * (np.abs(b64) + side)).all(), geo.name
    rles, resized = CF.recover_masks_rle(torch.from_numpy(masks).to(dev), geo.info, return_resized=True)
    resized = resized.cpu().numpy()
    want = _segm_oracle(geo)
    assert np.array_equal(resized, want), (geo.name, np.argwhere(resized != want)[:4].tolist())
    _check_mask_rule(resized, geo, "kernel")
    oh, ow = geo.info["height"], geo.info["width"]
    for k, rle in enumerate(rles):
        counts = R.rle_counts(want[k])
        assert rle["size"] == [oh, ow]
        assert rle["counts"] == R.rle_to_string(counts), (geo.name, k, G.MASK_FAMILIES[k] if K == 14 else k)
        assert R.rle_string_decode(rle["counts"], oh * ow) == counts, (geo.name, k)


def _rle_launches(images, cap):
    """The launches om_recover_masks_rle_strings makes for [(K, oh, ow)]: (LDS batches, of which full RLE_BATCH ones,
    over-capacity images).  A MODEL of its host-side batching (coco_format.hip: K = 0 images skipped, an over-capacity image
    flushes the batch and goes alone through recover_rle_kernel, a batch flushes at RLE_BATCH = 24 images), not an observation
    of the launches: it shows what the call below exercises only as long as it and the host code agree."""
    batches, full, over, n = 0, 0, 0, 0
    for K, oh, ow in images:
        if K == 0:
            continue
        if G.rle_lds_bytes(oh, ow) > cap:
            batches += n > 0
            n = 0
            over += 1
        else:
            if n == 24:
                batches += 1
                full += 1
                n = 0
            n += 1
    return batches + (n > 0), full, over


@pytest.mark.gpu
def test_coco_formatter_batched_over_the_table(dev):
    """One to_coco_format call over the table twice (table order: LDS-path images, over-capacity images and K = 0 images
    interleaved across several RLE_BATCH flushes); ids, order, sizes, boxes and strings equal the per-image oracle.  Again with
    first-guess buffers so small that masks take the overflow path in the middle of the mixed batch."""
    from orienmask_amd.coco_format import COCOFormatter
    per_block = _device_lds_per_block()
    table = G.table(per_block)
    cap = G.rle_lds_max(per_block)
    print("device LDS per block %d B (torch reports %d), RLE LDS capacity %d B, exact-capacity geometry %s" % (
        per_block, torch.cuda.get_device_properties(0).shared_memory_per_block, cap, G.lds_boundary(per_block)[0]))
    infos, dets, want = [], [], []
    for i, geo in enumerate(table + table):
        masks = _masks(geo)
        K = 0 if i % 9 == 4 else min(len(masks), 1 + i % 3)
        sel = [(i + j) % len(masks) for j in range(K)]
        info = dict(geo.info, id=1000 + i)
        bbox = _bbox(geo, max(K, 1))[:K]
        infos.append(info)
        dets.append(dict(bbox=bbox.to(dev), cls=torch.arange(K, device=dev) % 80,
                         mask=torch.from_numpy(masks[sel].copy()).to(dev) if K else torch.zeros(0, geo.H, geo.W, dtype=torch.bool, device=dev)))
        seg = _segm_oracle(geo)
        xywh = R.recover_shape_bbox(bbox, info)
        want += [(info["id"], k % 80 + 1, xywh[k].tolist(), [info["height"], info["width"]], R.rle_to_string(R.rle_counts(seg[s])))
                 for k, s in enumerate(sel)]
    images = [(int(d["bbox"].shape[0]), i["height"], i["width"]) for i, d in zip(infos, dets)]
    batches, full, over = _rle_launches(images, cap)
    print("batched formatter: %d images, %d masks; the host batching rule gives %d LDS launches (%d full RLE_BATCH flushes) "
          "and %d over-capacity images" % (
        len(images), len(want), batches, full, over))
    assert len(images) >= 50 and batches >= 3 and full >= 2 and over >= 2
    for max_runs, bytes_per_mask in ((None, None), (64, 48)):
        fmt = COCOFormatter(list(range(1, 81)))
        if max_runs:
            fmt.MAX_RUNS, fmt.BYTES_PER_MASK = max_runs, bytes_per_mask
        res = fmt.to_coco_format(infos, dets)
        assert len(res["bbox"]) == len(res["segm"]) == len(want)
        for j, (b, s, w) in enumerate(zip(res["bbox"], res["segm"], want)):
            assert (b["image_id"], b["category_id"], b["bbox"]) == (w[0], w[1], w[2]), (j, max_runs)
            assert (s["image_id"], s["segmentation"]["size"]) == (w[0], w[3]), (j, max_runs)
            assert s["segmentation"]["counts"] == w[4], (j, w[0], max_runs)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", TABLE, ids=[g.name for g in TABLE])
def test_preprocess_geometry(dev, geo):
    """padded() against R.pad_to_divisor(R.fast_coco_transform(.)) bit for bit with the same pad info, and within the FLOAT
    BOUND of float64, for the three resizes; the mean/std, N and image kind cycle over the table."""
    from orienmask_amd.transform import FastCOCOTransform as T
    h, w = geo.info["height"], geo.info["width"]
    s = _seed(geo)
    for j, (tname, size) in enumerate(_targets(h, w)):
        norm = ("255", "imagenet")[(s + j) % 2]
        n = 3 if h * w * 3 <= 2_000_000 and (s + j) % 3 != 2 else 1
        kind = ("int", "frac", "edges")[(s + 2 * j) % 3]
        img = _photo(n, h, w, s + j, kind)
        mean, std = MEAN_STD[norm]
        resize = T.ShortEdgeResize(544, 1333) if tname == "short_edge" else T.Resize(size)
        assert resize.target(h, w) == size
        tf = T([resize, T.Normalize(mean, std)])
        got, info = tf.padded(img.to(dev))
        want, winfo = R.pad_to_divisor(R.fast_coco_transform(img, size, mean, std), 32, 0)
        tag = (geo.name, tname, norm, n, kind)
        assert info == winfo, tag
        assert torch.equal(got.cpu(), want), (tag, (got.cpu() - want).abs().max().item())
        v64, bound, _ = G.preprocess64(img.numpy(), size, mean, std)
        assert (np.abs(got.cpu().numpy() - v64) <= bound).all(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("geo", TABLE, ids=[g.name for g in TABLE])
def test_visualizer_geometry(dev, geo):
    """_composite_float at the geometry's original size (1 x N and N x 1 included: the reference adds the k >= 1 colour terms
    only to images taller than one row) against the float64 plot_all_mask: the float composite within the VISUALISER BOUND,
    the uint8 image equal away from a rounding boundary, and the kernel's area order that of float64 except between masks
    whose areas differ by less than 1e-6 relative (the float64 composite then follows the kernel's order: the corner, edge-row
    and edge-column families tie by symmetry)."""
    from orienmask_amd.visualizer import InferenceVisualizer
    h, w = geo.info["height"], geo.info["width"]
    top, down, left, right = G.crop_of(geo.info)
    pad_info = [left, right, top, down, geo.H, geo.W]
    masks = _masks(geo)[:4] if h * w > BIG else _masks(geo)
    K = len(masks)
    image = _photo(1, h, w, _seed(geo) + 1, "frac")[0]
    bbox = torch.cat([_bbox(geo, K)[:, :4], torch.full((K, 1), 0.9)], 1)
    dets = dict(bbox=bbox.to(dev), cls=torch.arange(K, device=dev) % 80, mask=torch.from_numpy(masks).to(dev))
    v = InferenceVisualizer("COCO", dev, alpha=0.6)
    random.seed(_seed(geo))
    out, out_f, areas = v._composite_float(dets, image.to(dev), pad_info, with_areas=True)
    random.seed(_seed(geo))
    colors = (torch.arange(K) * 5 + random.randint(1, len(v.palette))) % len(v.palette)
    colors = v.palette.cpu()[colors].double().numpy()
    plain = dict(geo.info, hflip=False, vflip=False)
    m64, b64 = [], []
    for k in range(K):
        a, b = G.resize64(G.crop_flip(masks[k:k + 1], plain).astype(np.float64), h, w, with_bound=True)
        m64.append(a[0]); b64.append(b[0])
    m64, b64 = np.stack(m64), np.stack(b64)
    area64 = m64.sum(axis=(1, 2))
    got_order = np.argsort(areas.cpu().numpy(), kind="stable")
    for r in range(K - 1):                  # ascending in float64 too, up to masks of (nearly) equal area
        a, b = area64[got_order[r]], area64[got_order[r + 1]]
        assert a <= b + 1e-6 * max(abs(a), abs(b)), (geo.name, r, got_order.tolist(), area64.tolist())
    want, bound, _, _ = G.plot_all_mask64(m64, b64, image.double().numpy(), colors, 0.6, order=got_order)
    f = out_f.cpu().double().numpy()
    err = np.abs(f - want) - bound
    assert err.max() <= 0, (geo.name, float(err.max()), np.unravel_index(np.argmax(err), err.shape))
    u8 = out.cpu().numpy().astype(np.int16)
    want_u8 = np.clip(np.rint(want), 0, 255).astype(np.int16)
    near = np.abs(want - np.floor(want) - 0.5) <= np.maximum(bound, 2e-3)
    diff = np.abs(u8 - want_u8)
    assert diff.max() <= 1 and not (diff[~near] > 0).any(), (geo.name, np.argwhere((diff > 0) & ~near)[:4].tolist())
