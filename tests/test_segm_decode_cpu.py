"""No-GPU tests of the 'segm' data path: the numpy model of segm_pack_kernel (tests/segm_decode_np.py) against the restatement
and against the mistakes it must tell apart, the host planner and collate (orienmask_amd/augment.py, orienmask_amd/segm.py) and
the datasets (orienmask_amd/dataset.py).  Every comparison is exact."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import cocoeval_cases as C
import segm_decode_np as S
from conftest import REPO
from orienmask_amd import augment, segm as segm_mod, synth, transform

# mutant -> a case that tells it from the truth, and why
TEETH = {
    "lsb_first": "counts_first_pixel_33x129",                   # one pixel at column 0: 0x80, not 0x01
    "pad_not_cleared": "counts_ones_65x65",                     # w = 65: seven pad bits behind column 64
    "columns_from_64_dropped": "counts_last_pixel_33x129",      # the only pixel is at column 128
    "rows_past_h_stored": "counts_ones_33x129",                 # h = 33: the second band has 31 rows past h
    "sources_not_ored": "polys_2_disjoint_33x129",
    "last_group_one_byte_short": "counts_ones_65x65",           # the last group is the single byte of column 64
    "last_group_one_byte_over": "counts_ones_65x65",
}


@pytest.fixture(scope="module")
def modelled():
    """(name, h, w, truth rows, source bitmaps) of every case of the table and of the extra sizes, each computed once"""
    out = []
    for name, h, w, segm in C.mask_cases() + S.extra_cases():
        want = S.truth(segm, h, w)
        want.setflags(write=False)
        mh, mw, maps = S.source_bitmaps(segm, h, w)
        out.append((name, mh, mw, want, maps))
    return out


def test_model_equals_the_truth_on_every_case(modelled):
    bad = []
    for name, h, w, want, maps in modelled:
        buf, writes = S.pack_rows(maps, h, w)
        n = h * ((w + 7) // 8)
        if want.shape != (h, (w + 7) // 8) or not np.array_equal(buf, S.expected(want, w)):
            bad.append((name, "bytes"))
        if not ((writes[:n] == 1).all() and (writes[n:] == 0).all()):
            bad.append((name, "a byte written twice, never, or outside the mask"))
    assert not bad, bad[:12]
    names = {m[0] for m in modelled}
    assert {"random_counts_%dx%d" % (h, w) for h in S.EXTRA_H for w in S.EXTRA_W} <= names
    assert {"two_polygons_%dx%d" % (h, w) for h in S.EXTRA_H for w in S.EXTRA_W} <= names


def test_sources_or_to_the_bitmap_models_mask(modelled):
    """source_bitmaps is build_mask without its merge"""
    import cocoeval_bitmap_np as B
    by_name = {c[0]: c for c in C.mask_cases()}
    for name in ("polys_3_stars_97x130", "box_quirk_two_97x130", "string_checker_33x129", "counts_ones_65x65"):
        _, h, w, segm = by_name[name]
        mh, mw, maps = S.source_bitmaps(segm, h, w)
        words, _ = B.build_mask(segm, h, w)
        assert np.array_equal(np.bitwise_or.reduce(np.stack(maps), axis=0), words), name


@pytest.mark.parametrize("variant", sorted(S.VARIANTS))
def test_teeth(modelled, variant):
    """each mistake is told from the truth by its named case, and the extra sizes tell it too"""
    assert set(TEETH) == set(S.VARIANTS)
    by_name = {m[0]: m for m in modelled}
    name, h, w, want, maps = by_name[TEETH[variant]]
    buf, _ = S.pack_rows(maps, h, w, variant)
    assert not np.array_equal(buf, S.expected(want, w)), (variant, name)
    told = [m[0] for m in modelled if m[0].startswith(("random_counts", "two_polygons"))
            and not np.array_equal(S.pack_rows(m[4], m[1], m[2], variant)[0], S.expected(m[3], m[2]))]
    assert told, variant


# ------------------------------------------------------------------------------------------------------------------ planner
def _plan(samples, size, seed):
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=S.train_pipeline(size)))
    random.seed(seed)
    torch.manual_seed(seed)
    planned = [tf(s) for s in samples]
    return planned, random.getstate(), torch.get_rng_state()


def _same_record(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.fixture(scope="module")
def e2e():
    samples = S.end_to_end_samples()
    return samples, [S.as_mask_sample(s) for s in samples]


def test_planner_draws_and_records_do_not_depend_on_the_mask_form(e2e):
    as_segm, as_mask = e2e
    for seed in (3, 11, 29):
        ps, rs, ts = _plan(as_segm, (96, 96), seed)
        pm, rm, tm = _plan(as_mask, (96, 96), seed)
        assert rs == rm and torch.equal(ts, tm)
        for a, b in zip(ps, pm):
            assert torch.equal(a['bbox'], b['bbox']) and a['bbox'].dtype == b['bbox'].dtype
            assert torch.equal(a['cls'], b['cls']) and a['info'] == b['info']
            _same_record(a['aug'], b['aug'])
            assert 'mask' not in a and 'segm' not in b
            assert np.array_equal(a['image'], b['image'])
            assert all(isinstance(v, (int, np.ndarray)) for v in a['segm'].values())       # flat arrays: picklable, no pixel
            assert sum(v.nbytes for v in a['segm'].values() if isinstance(v, np.ndarray)) < 64 * 1024


def test_planner_refuses(e2e):
    as_segm, as_mask = e2e
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=S.train_pipeline((96, 96))))
    s = dict(as_segm[2])
    with pytest.raises(ValueError):
        tf(dict(s, mask=as_mask[2]['mask']))                        # both forms
    with pytest.raises(ValueError):
        tf(dict(s, segm=s['segm'][:-1]))                            # a segmentation short
    with pytest.raises(ValueError):
        tf(dict(s, segm=[s['segm'][0], {"size": [160, 120], "counts": [160 * 120]}, s['segm'][2]]))     # an RLE of another size
    with pytest.raises(ValueError):
        tf(dict(s, segm=[[C.star(4097, 120, 160)], s['segm'][1], s['segm'][2]]))       # more vertices than the kernel holds


# ------------------------------------------------------------------------------------------------------------------ collate
def _table(pb, name):
    off, nbytes = pb.segm_layout[name]
    return pb.segm.numpy()[off:off + nbytes].view(segm_mod.TABLE_DTYPES[name])


def test_collate_tables_decode_back_to_the_sources(e2e):
    as_segm, as_mask = e2e
    ps, _, _ = _plan(as_segm, (96, 96), 7)
    pm, _, _ = _plan(as_mask, (96, 96), 7)
    bs, bm = transform.collate(ps), transform.collate(pm)
    assert bs.has_mask and bs.mask.numel() == 0 and bm.segm is None and bs.N == bm.N == 8
    rows_s = bs.meta.numpy()[bs.layout["samples"][0]:][:bs.B * 160].view(augment.AUG_SAMPLE_DTYPE)
    rows_m = bm.meta.numpy()[bm.layout["samples"][0]:][:bm.B * 160].view(augment.AUG_SAMPLE_DTYPE)
    assert np.array_equal(rows_s, rows_m)                           # mask_off among them
    assert torch.equal(bs.meta, bm.meta) and torch.equal(bs.image, bm.image)
    assert bs.segm_counts["mask_bytes"] == bm.mask.numel()
    t = {n: _table(bs, n) for n in segm_mod.TABLE_ORDER}
    c = bs.segm_counts
    assert all(off % 16 == 0 for off, _ in bs.segm_layout.values())
    assert len(t["src_kind"]) == c["n_srcs"] and (t["src_kind"][:c["n_poly"]] == 0).all() and (t["src_kind"][c["n_poly"]:] != 0).all()
    data = {0: t["poly"], 1: t["counts"], 2: t["strings"]}
    m, words = 0, 0
    for b, s in enumerate(as_segm):
        h, w = s['image'].shape[:2]
        for g, a in enumerate(s['segm']):
            assert tuple(t["mask_hw"][2 * m:2 * m + 2]) == (h, w)
            assert t["mask_out_off"][m] == rows_s[b]['mask_off'] + g * h * ((w + 7) // 8)
            _, _, want = segm_mod.sources(a, h, w)
            bitmaps = t["mask_src_word_off"][t["mask_src_first"][m]:t["mask_src_first"][m + 1]]
            assert len(bitmaps) == len(want)
            for word_off, (kind, d) in zip(bitmaps, want):
                assert word_off == words                            # a bitmap per source, back to back
                words += w * ((h + 31) // 32)
                k = int(np.flatnonzero(t["src_word_off"] == word_off)[0])
                assert t["src_kind"][k] == kind and t["src_mask"][k] == m
                got = data[kind][t["src_data_off"][k]:t["src_data_off"][k] + t["src_len"][k]]
                assert np.array_equal(got, np.frombuffer(d, np.uint8) if kind == 2 else d)
            m += 1
    assert m == bs.N and words == c["bitmap_words"] and t["mask_src_first"][m] == c["n_srcs"]
    assert bs.h2d_bytes() == {"image": bm.h2d_bytes()["image"], "mask": 0, "meta": bm.h2d_bytes()["meta"], "segm": bs.segm.numel()}
    assert bm.h2d_bytes()["segm"] == 0 and bm.h2d_bytes()["mask"] == bm.mask.numel() > 0


def test_collate_refuses_mixtures_and_wrong_counts(e2e):
    as_segm, as_mask = e2e
    ps, _, _ = _plan(as_segm, (96, 96), 7)
    pm, _, _ = _plan(as_mask, (96, 96), 7)
    with pytest.raises(ValueError):
        transform.collate([ps[0], pm[1]])
    with pytest.raises(ValueError):
        transform.collate([pm[0], ps[1]])
    with pytest.raises(ValueError):
        transform.collate([ps[0], {k: v for k, v in ps[1].items() if k != 'segm'}])
    with pytest.raises(ValueError):
        transform.collate([dict(ps[0], segm=ps[3]['segm'])])        # two segmentations for three GTs


def test_planned_batch_keeps_its_constructor():
    z = torch.zeros(0, dtype=torch.uint8)
    pb = augment.PlannedBatch(z, z, z, {}, 1, 0, (8, 8), [0.0] * 3, [1.0] * 3, False, False, None)
    assert pb.segm is None and pb.h2d_bytes()["segm"] == 0


def test_bench_batch_ships_fewer_bytes_as_segm():
    """at most 3 x 200 vertices x 16 bytes of polygon per GT against 480 x 80 bytes of bits; the masks' content does not enter a
    byte count, so the 'mask' form of the same batch carries zeros here"""
    batch = synth.synth_segm_batch()
    assert len(batch) == 32 and all(s['image'].shape == (480, 640, 3) for s in batch)
    n_gt = sum(len(s['segm']) for s in batch)
    assert 5 * 32 <= n_gt <= 9 * 32 and any(isinstance(a, dict) for s in batch for a in s['segm'])
    ps, _, _ = _plan(batch, (544, 544), 1)
    zero = np.zeros((480, 640), np.uint8)
    pm, _, _ = _plan([dict({k: v for k, v in s.items() if k != 'segm'}, mask=[zero] * len(s['segm'])) for s in batch], (544, 544), 1)
    hs, hm = transform.collate(ps).h2d_bytes(), transform.collate(pm).h2d_bytes()
    assert hm["mask"] == n_gt * 480 * 80 and hs["mask"] == 0
    assert hs["segm"] < hm["mask"] and hs["segm"] < hm["mask"] // 8
    assert hs["image"] == hm["image"] and hs["meta"] == hm["meta"]


# ----------------------------------------------------------------------------------------------------------------- datasets
def write_dataset(root):
    """two PNGs, a list file and a label json in the reference's format; returns (list_file, image_dir, anno_file, samples)"""
    from PIL import Image
    samples = S.end_to_end_samples()
    keys = ["a/first.png", "second.png"]
    os.makedirs(os.path.join(root, "images", "a"))
    labels = {}
    for key, s in zip(keys, (samples[0], samples[2])):
        Image.fromarray(s['image']).save(os.path.join(root, "images", key))
        labels[key] = {"image_id": int(s['info']['id']), "anno": {"bbox": s['bbox'].tolist(), "cls": s['cls'].tolist(), "mask": s['segm']}}
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("".join("%s,%d\n" % (k, i) for i, k in enumerate(keys)))        # a second column, as a list file may have
    with open(os.path.join(root, "labels.json"), "w") as f:
        json.dump(labels, f)
    return os.path.join(root, "list.txt"), os.path.join(root, "images"), os.path.join(root, "labels.json"), [samples[0], samples[2]]


def test_datasets(tmp_path):
    from orienmask_amd import dataset
    list_file, image_dir, anno_file, src = write_dataset(str(tmp_path))
    ident = lambda s: s
    coco = transform.COCODataset(list_file, image_dir, anno_file, ident)
    assert transform.COCODataset is dataset.COCODataset and issubclass(dataset.VOCDataset, dataset.COCODataset)
    assert issubclass(dataset.COCODataset, dataset.BaseDataset) and issubclass(dataset.BaseDataset, torch.utils.data.Dataset)
    assert len(coco) == 2 and coco.with_mask and coco.with_info
    for i, s in enumerate(src):
        got = coco[i]
        assert set(got) == {"image", "bbox", "cls", "segm", "info"}
        assert got['image'].dtype == np.uint8 and np.array_equal(got['image'], s['image'])       # PNG: lossless
        assert got['bbox'].dtype == np.float32 and np.array_equal(got['bbox'], s['bbox'])
        assert got['cls'].dtype == np.int64 and np.array_equal(got['cls'], s['cls'])
        assert got['segm'] == json.loads(json.dumps(s['segm']))
        assert got['info'] == {"id": s['info']['id'], "height": s['image'].shape[0], "width": s['image'].shape[1]}
    voc = transform.VOCDataset(list_file, image_dir, anno_file, ident)
    assert not voc.with_mask and len(voc) == 2 and set(voc[0]) == {"image", "bbox", "cls", "info"}
    assert set(transform.COCODataset(list_file, image_dir, anno_file, ident, with_mask=False, with_info=False)[1]) == {"image", "bbox", "cls"}
    assert len(coco.CAT2LABEL) == 80 == len(coco.CLASSES) and len(voc.CAT2LABEL) == 20 == len(voc.CLASSES)
    assert coco.CAT2LABEL[11] == 13 and coco.CAT2LABEL[-1] == 90 and coco.CLASSES[0] == "person" and voc.CLASSES[14] == "person"
    calls = []
    custom = transform.COCODataset(list_file, image_dir, anno_file, ident, imread=lambda p: calls.append(p) or src[0]['image'])
    assert np.array_equal(custom[1]['image'], src[0]['image']) and calls == [os.path.join(image_dir, "second.png")]
    # the registry resolves them from a reference config, through the transform and collate
    from orienmask_amd.builder import build
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=S.train_pipeline((96, 96))))
    ds = build(dict(type="COCODataset", list_file=list_file, image_dir=image_dir, anno_file=anno_file, transform=tf), transform)
    random.seed(1)
    torch.manual_seed(1)
    pb = transform.collate([ds[0], ds[1]])
    assert pb.N == 6 and pb.segm is not None and pb.info[1]['id'] == src[1]['info']['id']


def test_dataset_module_needs_no_pandas_pycocotools_or_cv2(tmp_path):
    list_file, image_dir, anno_file, _ = write_dataset(str(tmp_path))
    code = ("import importlib.util, sys\n"
            "sys.path.insert(0, %r)\n"
            "from orienmask_amd import dataset\n"
            "ds = dataset.COCODataset(%r, %r, %r, lambda s: s)\n"
            "assert ds[0]['image'].shape == (97, 130, 3) and len(ds[1]['segm']) == 3\n"
            "banned = ['pandas', 'pycocotools'] + ([] if importlib.util.find_spec('cv2') else ['cv2'])\n"
            "print([m for m in banned if m in sys.modules])\n" % (REPO, list_file, image_dir, anno_file))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "[]"
