"""GPU tests of om_segm_decode (csrc/segm_decode.hip) and of the 'segm' path of orienmask_amd.augment / orienmask_amd.dataset.

Truth for a decoded mask is np.packbits(ann_mask(segm, h, w, strict=False) > 0, axis=1) of the restatement (tests/cocoeval_np.py);
truth for a batch is the same batch given as 'mask' (masks = ann_mask) through the unchanged 'mask' path.  Every comparison is
exact; what each case hits, and that the cases catch a list of kernel mistakes, is proved without a GPU in
tests/test_segm_decode_cpu.py."""
import ctypes
import random

import numpy as np
import pytest
import torch

import cocoeval_cases as C
import segm_decode_np as S
from test_segm_decode_cpu import write_dataset
from orienmask_amd import lib as omlib, segm as segm_mod, transform

pytestmark = pytest.mark.gpu

CANARY = 64
CANARY_BYTE = 0xC3


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


def decode(cases, dev, stream=None):
    """the cases' masks through ONE om_segm_decode call, written back to back with CANARY bytes before, between and after them:
    (the whole buffer as numpy, [(offset, h, w)] per case)"""
    L = omlib.load()
    masks, offs, off = [], [], CANARY
    for _, h, w, segm in cases:
        mh, mw, srcs = segm_mod.sources(segm, h, w)
        masks.append((mh, mw, srcs))
        offs.append((off, mh, mw))
        off += mh * ((mw + 7) // 8) + CANARY
    tables, counts = segm_mod.build_tables(masks, [o[0] for o in offs])
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in tables.items()}
        ptr = lambda k: ctypes.c_void_p(d[k].data_ptr()) if d[k].numel() else None
        out = torch.full((max(off, CANARY),), CANARY_BYTE, dtype=torch.uint8, device=dev)
        ws_bytes = int(L.om_segm_decode_workspace_bytes(counts["bitmap_words"], len(cases)))
        ws = torch.full((max(ws_bytes, 4),), 0x5A, dtype=torch.uint8, device=dev)       # "contents undefined on entry"
        rc = L.om_segm_decode(len(cases), ptr("mask_hw"), ptr("mask_src_first"), ptr("mask_src_word_off"), ptr("mask_out_off"),
                              counts["n_poly"], counts["n_srcs"], ptr("src_kind"), ptr("src_mask"), ptr("src_data_off"),
                              ptr("src_len"), ptr("src_word_off"), ptr("poly"), ptr("counts"), ptr("strings"),
                              counts["bitmap_words"], ctypes.c_void_p(ws.data_ptr()), ws_bytes, ctypes.c_void_p(out.data_ptr()),
                              omlib.current_stream_ptr(dev))
        omlib.check(rc, "om_segm_decode")
        torch.cuda.current_stream(dev).synchronize()
        return out.cpu().numpy(), offs


def check(cases, buf, offs, want):
    bad, at = [], 0
    for (name, _, _, _), (off, h, w), rows in zip(cases, offs, want):
        n = h * ((w + 7) // 8)
        if rows.shape != (h, (w + 7) // 8):
            bad.append((name, "size"))
        elif not np.array_equal(buf[off:off + n].reshape(rows.shape), rows):
            bad.append((name, "%d bytes differ" % int((buf[off:off + n].reshape(rows.shape) != rows).sum())))
        if not (buf[at:off] == CANARY_BYTE).all():
            bad.append((name, "canary in front"))
        at = off + n
    if not (buf[at:] == CANARY_BYTE).all() or len(buf) - at != CANARY:
        bad.append(("end", "canary behind the last mask"))
    return bad


@pytest.fixture(scope="module")
def table_truth():
    want = [S.truth(c[3], c[1], c[2]) for c in C.mask_cases()]
    for m in want:
        m.setflags(write=False)
    return want


def test_whole_case_table_in_one_call(dev, table_truth):
    """mixed sizes, all three kinds, multi-polygon merges and the malformed sequences; pad bits and canaries included"""
    cases = C.mask_cases()
    buf, offs = decode(cases, dev)
    bad = check(cases, buf, offs, table_truth)
    assert not bad, "%d of %d: %s" % (len({b[0] for b in bad}), len(cases), bad[:12])
    kinds = {k for c in cases for k, _ in segm_mod.sources(c[3], c[1], c[2])[2]}
    assert kinds == {0, 1, 2} and any(len(segm_mod.sources(c[3], c[1], c[2])[2]) == 5 for c in cases)


def test_sizes_around_the_tile(dev):
    cases = S.extra_cases()
    assert {(c[1], c[2]) for c in cases} == {(h, w) for h in S.EXTRA_H for w in S.EXTRA_W} and len(cases) == 80
    buf, offs = decode(cases, dev)
    bad = check(cases, buf, offs, [S.truth(c[3], c[1], c[2]) for c in cases])
    assert not bad, bad[:12]


def test_repeatable_on_any_stream_and_empty_call(dev, table_truth):
    cases = [c for c in C.mask_cases() if c[0].startswith(("polys_", "star_65", "counts_checker", "string_column_straddle"))]
    a, offs = decode(cases, dev)
    b, _ = decode(cases, dev)
    c, _ = decode(cases, dev, stream=torch.cuda.Stream(dev))
    assert np.array_equal(a, b) and np.array_equal(a, c)
    idx = {c[0]: i for i, c in enumerate(C.mask_cases())}
    assert not check(cases, a, offs, [table_truth[idx[c[0]]] for c in cases])
    L = omlib.load()
    assert L.om_segm_decode(0, None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0, None, 0, None,
                            omlib.current_stream_ptr(dev)) == 0
    assert L.om_segm_decode(70000, None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0, None, 0, None,
                            omlib.current_stream_ptr(dev)) != 0
    assert L.om_segm_decode(1, None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0, None, 0, None,
                            omlib.current_stream_ptr(dev)) != 0           # null pointers: refused, nothing launched
    buf, offs = decode([], dev)
    assert (buf == CANARY_BYTE).all()


def _both_ways(samples, size, seed, dev):
    out = []
    for form in (samples, [S.as_mask_sample(s) for s in samples]):
        tf = transform.build_transform(dict(type="COCOTransform", pipeline=S.train_pipeline(size)))
        random.seed(seed)
        torch.manual_seed(seed)
        pb = transform.collate([tf(s) for s in form])
        image, anno, info = transform.to_device(pb, dev)
        out.append(([image.cpu()] + [a.cpu() for a in anno], info, pb))
    return out


def test_end_to_end_equals_the_mask_path(dev):
    samples = S.end_to_end_samples()
    assert [s['image'].shape[:2] for s in samples] == [(97, 130), (65, 65), (120, 160), (33, 129)]
    for seed in (2, 13):
        (got, info_s, pb_s), (want, info_m, pb_m) = _both_ways(samples, (96, 96), seed, dev)
        assert pb_s.segm is not None and pb_s.mask.numel() == 0 and pb_m.segm is None
        assert len(got) == len(want) == 5 and info_s == info_m
        for a, b, name in zip(got, want, ("image", "bbox", "cls", "index", "mask")):
            assert a.dtype == b.dtype and torch.equal(a, b), (seed, name)
        assert got[4].shape == (8, 96, 96) and got[4].any()
    # a batch without any GT
    empty = [samples[1], dict(samples[1], info=dict(samples[1]['info'], id=9))]
    (got, _, pb_s), (want, _, _) = _both_ways(empty, (96, 96), 4, dev)
    assert pb_s.N == 0 and pb_s.segm is not None and tuple(got[4].shape) == (0, 96, 96)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_to_device_does_not_synchronise(dev):
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=S.train_pipeline((96, 96))))
    random.seed(6)
    torch.manual_seed(6)
    pb = transform.collate([tf(s) for s in S.end_to_end_samples()]).pin_memory()
    assert pb.segm.is_pinned()
    transform.to_device(pb, dev)                # the library is loaded, the allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = transform.to_device(pb, dev)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out[1][3].shape == (8, 96, 96)


@pytest.mark.parametrize("workers", [0, 2])
def test_dataset_to_device(dev, tmp_path, workers):
    """COCODataset -> DataLoader(collate_fn=collate) -> device_batches yields the reference collate's tuple; the masks equal the
    restatement's pushed through the 'mask' path"""
    list_file, image_dir, anno_file, src = write_dataset(str(tmp_path))
    tf = transform.build_transform(dict(type="COCOTransform", pipeline=[
        dict(type="Resize", size=[96, 96], pad_needed=False, warp_p=0., jitter=0., random_place=False, pad_p=0., pad_ratio=0.,
             pad_value=S.MEAN), dict(type="ToTensor"), dict(type="Normalize", mean=[0, 0, 0], std=[255, 255, 255])]))
    ds = transform.COCODataset(list_file, image_dir, anno_file, tf)
    torch.manual_seed(8)            # ToTensor's randperm: drawn in this process (workers = 0) or from the workers' base seed
    loader = transform.DataLoader(ds, batch_size=2, shuffle=False, num_workers=workers, collate_fn=transform.collate, pin_memory=True)
    batches = list(loader)
    assert len(batches) == 1 and batches[0].segm is not None and batches[0].segm.is_pinned()
    (image, (bbox, cls, index, mask), info), = list(transform.device_batches(batches, dev))
    assert image.shape == (2, 3, 96, 96) and mask.shape == (6, 96, 96) and mask.dtype == torch.bool and index.tolist() == [0, 3, 6]
    assert [i['id'] for i in info] == [s['info']['id'] for s in src]
    # the same planned samples with the restatement's masks in place of the sources: the permutation is whatever was drawn
    pb = batches[0]
    gt = pb.meta.numpy()[pb.layout["gt"][0]:][:pb.N * 8].view(np.int32).reshape(-1, 2)
    planned = []
    for b, s in enumerate(src):
        m = S.as_mask_sample(s)
        random.seed(0)
        p = tf(m)
        perm = gt[gt[:, 1] == b, 0] - 3 * b
        p['aug']['perm'] = perm.astype(np.int64)
        p['bbox'], p['cls'] = torch.from_numpy(m['bbox'])[perm], torch.from_numpy(m['cls'])[perm]
        planned.append(p)
    want_image, (wb, wc, wi, wm), _ = transform.to_device(transform.collate(planned), dev)
    assert torch.equal(image, want_image) and torch.equal(bbox, wb) and torch.equal(cls, wc) and torch.equal(index, wi)
    assert torch.equal(mask, wm) and mask.any()
