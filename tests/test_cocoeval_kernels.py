"""Every kernel of csrc/cocoeval.hip on its own, against the restatement tests/cocoeval_np.py, over the case tables of
tests/cocoeval_cases.py (what each case hits, and that the tables catch a list of kernel mistakes, is proved without a GPU in
tests/test_cocoeval_kernels_cpu.py).

All comparisons are exact: pixels, padding bits, int32 statistics, float64 bit patterns, ids and flags.  Both sides divide the
same integers (mask IoU) or follow C's float64 order (bbIou; the file is built with -ffp-contract=off), so there is nothing to
tolerate.  No case is skipped or filtered: a size or a vertex count the device path refuses fails the test, except the 4097
vertices the host must refuse."""
import ctypes

import numpy as np
import pytest
import torch

import cocoeval_bitmap_np as B
import cocoeval_cases as C
import cocoeval_np as ref
from orienmask_amd import lib as omlib


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _evaluator(cases, dev):
    """an evaluator whose GT has one image per case, and the cases as annotations of their images"""
    from orienmask_amd.cocoeval import COCOEvaluator, COCOGroundTruth
    gt = {"images": [dict(id=i, height=c[1], width=c[2]) for i, c in enumerate(cases)], "categories": [dict(id=1, name="1")],
          "annotations": []}
    ev = COCOEvaluator(COCOGroundTruth.from_dict(gt), [], "segm", device=dev)
    ev.device = dev
    return ev, [dict(id=i + 1, image_id=i, segmentation=c[3]) for i, c in enumerate(cases)]


def _build(ev, anns, dev):
    """om_cocoeval_masks through _build_masks: (the words of each mask, [n, 3] statistics)"""
    with torch.cuda.device(dev):
        stats = ev._build_masks(omlib.load(), anns, omlib.current_stream_ptr(dev))
        torch.cuda.synchronize()
        off = ev._ws.data_ptr() - ev._ws_keep.data_ptr()
        bm = ev._ws_keep[off:off + 4 * ev._m_words].view(torch.int32).cpu().numpy().view(np.uint32)
    hw, moff = ev._m_hw.cpu().numpy(), ev._m_off.cpu().numpy()
    words = [bm[moff[m]:moff[m] + hw[m, 1] * ((hw[m, 0] + 31) // 32)].copy() for m in range(len(anns))]
    return words, stats, hw


@pytest.fixture(scope="module")
def table(dev):
    """the whole mask table built in ONE call, and the restatement's masks, each computed once"""
    cases = C.mask_cases()
    ev, anns = _evaluator(cases, dev)
    words, stats, hw = _build(ev, anns, dev)
    want = [ref.ann_mask(c[3], c[1], c[2], strict=False) for c in cases]
    for m in want:
        m.setflags(write=False)
    return dict(cases=cases, ev=ev, anns=anns, words=words, stats=stats, hw=hw, want=want)


@pytest.mark.gpu
def test_every_mask_case_equals_the_restatement(table):
    bad = []
    for i, (name, h, w, segm) in enumerate(table["cases"]):
        want = table["want"][i]
        if tuple(table["hw"][i]) != want.shape:
            bad.append((name, "size"))
            continue
        got, padding = B.unpack(table["words"][i], *want.shape)
        if not np.array_equal(got, want):
            bad.append((name, "pixels: %d differ" % int((got != want).sum())))
        if padding:
            bad.append((name, "padding bits set"))
        if tuple(int(v) for v in table["stats"][i]) != B.stats_of(want):
            bad.append((name, "stats %s, want %s" % (table["stats"][i].tolist(), B.stats_of(want))))
        if isinstance(segm, dict) and isinstance(segm["counts"], str) and sum(ref.rle_fr_string(segm["counts"])) == h * w:
            # a well-formed string: the C restatement of rleFrString (oracle/rle_ref.c) decodes it to the same mask
            if not np.array_equal(ref.ann_mask(segm, h, w), want):
                bad.append((name, "rle_fr_string and oracle/rle_ref.c disagree"))
    assert not bad, "%d of %d cases: %s" % (len({b[0] for b in bad}), len(table["cases"]), bad[:12])
    assert table["stats"].dtype == np.int32


@pytest.mark.gpu
def test_each_annotation_alone_gives_the_same_bitmap(table, dev):
    """the word offsets of the one-call table, and the single-source shortcut (a mask that IS its only source's bitmap)"""
    bad = []
    for i, a in enumerate(table["anns"]):
        words, stats, hw = _build(table["ev"], [a], dev)
        if not (np.array_equal(words[0], table["words"][i]) and np.array_equal(stats[0], table["stats"][i])
                and np.array_equal(hw[0], table["hw"][i])):
            bad.append(table["cases"][i][0])
    assert not bad, bad[:12]


@pytest.mark.gpu
def test_vertex_limit_4096_works_4097_raises(table, dev):
    i = next(k for k, c in enumerate(table["cases"]) if c[0] == "star_4096_97x130")
    assert len(table["cases"][i][3][0]) == 2 * 4096 and table["stats"][i][0] > 0          # built, and compared above
    ev, anns = _evaluator([("star_4097", 97, 130, [C.star(4097, 97, 130)])], dev)
    with pytest.raises(ValueError):
        _build(ev, anns, dev)


@pytest.mark.gpu
def test_mask_iou_over_all_pairs(dev):
    """om_cocoeval_mask_iou on every (det, gt) pair of a mixed-size mask set: -1 where the sizes differ, 0.0 for disjoint
    columns, disjoint rows and empty masks, the det's area as the union for a crowd GT"""
    L = omlib.load()
    cases = C.iou_mask_cases()
    crowd = C.iou_crowd()
    ev, anns = _evaluator(cases, dev)
    n = len(cases)
    words, stats, hw = _build(ev, anns + [dict(a) for a in anns], dev)        # masks [0, n) as GTs, [n, 2n) as dets
    masks = [ref.ann_mask(c[3], c[1], c[2], strict=False) for c in cases]
    for i in range(n):
        got, padding = B.unpack(words[n + i], *masks[i].shape)
        assert np.array_equal(got, masks[i]) and not padding, cases[i][0]
    want = ref.mask_iou(masks, masks, crowd)
    d, g = np.meshgrid(np.arange(n, dtype=np.int32) + n, np.arange(n, dtype=np.int32), indexing="ij")
    pairs = torch.from_numpy(np.ascontiguousarray(np.stack([d.ravel(), g.ravel()], 1))).to(dev)
    pair_crowd = torch.from_numpy(np.tile(np.array(crowd, dtype=np.uint8), n)).to(dev)
    iou = torch.full((n * n,), 7.0, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        omlib.check(L.om_cocoeval_mask_iou(n * n, _ptr(pairs), _ptr(pair_crowd), 2 * n, _ptr(ev._m_hw), _ptr(ev._m_off),
                                           ev._m_words, _ptr(ev._ws), _ptr(iou), omlib.current_stream_ptr(dev)),
                    "om_cocoeval_mask_iou")
        torch.cuda.synchronize()
    got = iou.cpu().numpy().reshape(n, n)
    diff = np.nonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(diff[0]) == 0, [(cases[a][0], cases[b][0], got[a, b], want[a, b]) for a, b in zip(*diff)][:8]
    assert (want == -1).any() and (want == 0).any() and (want == 1).any()


@pytest.mark.gpu
def test_bbox_iou_over_the_box_table(dev):
    L = omlib.load()
    dets, gts, crowd = C.box_table()
    D, G = len(dets), len(gts)
    want = ref.bb_iou(dets.tolist(), gts.tolist(), crowd.tolist())
    d, g = np.meshgrid(np.arange(D, dtype=np.int32), np.arange(G, dtype=np.int32), indexing="ij")
    pairs = torch.from_numpy(np.ascontiguousarray(np.stack([d.ravel(), g.ravel()], 1))).to(dev)
    pair_crowd = torch.from_numpy(np.tile(crowd, D)).to(dev)
    dbox, gbox = torch.from_numpy(dets).to(dev), torch.from_numpy(gts).to(dev)
    iou = torch.full((D * G,), 7.0, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        omlib.check(L.om_cocoeval_bbox_iou(D * G, _ptr(pairs), _ptr(pair_crowd), _ptr(dbox), _ptr(gbox), _ptr(iou),
                                           omlib.current_stream_ptr(dev)), "om_cocoeval_bbox_iou")
        torch.cuda.synchronize()
    got = iou.cpu().numpy().reshape(D, G)
    diff = np.nonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(diff[0]) == 0, [(dets[a].tolist(), gts[b].tolist(), got[a, b], want[a, b]) for a, b in zip(*diff)][:8]


def _match(groups, dev):
    """om_cocoeval_match on the groups in one launch, with the arrays the evaluator hands it: per group dt_match [40, D],
    dt_ignore [40, D], gt_matched [40, G]"""
    L = omlib.load()
    nd, ng = sum(len(g["dts"]) for g in groups), sum(len(g["gts"]) for g in groups)
    dt_first = np.cumsum([0] + [len(g["dts"]) for g in groups]).astype(np.int32)
    gt_first = np.cumsum([0] + [len(g["gts"]) for g in groups]).astype(np.int32)
    iou_off = np.cumsum([0] + [g["ious"].size for g in groups])[:-1].astype(np.int64)
    flat = np.concatenate([g["ious"].ravel() for g in groups] + [np.zeros(1)])
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ious = tt(flat)
    d_area = tt(np.array([d["area"] for g in groups for d in g["dts"]], dtype=np.float64))
    g_area = tt(np.array([x["area"] for g in groups for x in g["gts"]], dtype=np.float64))
    g_crowd = tt(np.array([x["iscrowd"] for g in groups for x in g["gts"]], dtype=np.uint8))
    g_id = tt(np.array([x["id"] for g in groups for x in g["gts"]], dtype=np.int64))
    rng, thr = tt(np.array(ref.AREA_RNG, dtype=np.float64)), tt(np.asarray(ref.IOU_THRS, dtype=np.float64))
    d_dtf, d_gtf, d_off = tt(dt_first), tt(gt_first), tt(iou_off)
    dtm = torch.zeros((40, max(nd, 1)), dtype=torch.int64, device=dev)
    dti = torch.zeros((40, max(nd, 1)), dtype=torch.uint8, device=dev)
    gtm = torch.zeros((40, max(ng, 1)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        omlib.check(L.om_cocoeval_match(len(groups), _ptr(d_dtf), _ptr(d_gtf), _ptr(d_off), _ptr(ious), _ptr(d_area), _ptr(g_area),
                                        _ptr(g_crowd), _ptr(g_id), _ptr(rng), _ptr(thr), nd, ng, _ptr(gtm), _ptr(dtm), _ptr(dti),
                                        omlib.current_stream_ptr(dev)), "om_cocoeval_match")
        torch.cuda.synchronize()
    dtm, dti, gtm = dtm.cpu().numpy(), dti.cpu().numpy(), gtm.cpu().numpy()
    return [(dtm[:, dt_first[k]:dt_first[k + 1]], dti[:, dt_first[k]:dt_first[k + 1]], (gtm[:, gt_first[k]:gt_first[k + 1]] != 0))
            for k in range(len(groups))]


@pytest.fixture(scope="module")
def match_want():
    return {g["name"]: ref.Eval.match_lanes(g["gts"], g["dts"], g["ious"]) for g in C.match_groups()}


@pytest.mark.gpu
def test_match_all_groups_in_one_launch(dev, match_want):
    groups = C.match_groups()
    got = _match(groups, dev)
    bad = []
    for g, (dtm, dti, gtm) in zip(groups, got):
        w_dtm, w_dti, w_gtm = match_want[g["name"]]
        for what, x, y in (("dt_match", dtm, w_dtm), ("dt_ignore", dti, w_dti), ("gt_matched", gtm, w_gtm != 0)):
            if x.shape != y.shape or not np.array_equal(x, y):
                lanes = sorted(set(np.nonzero(x != y)[0].tolist())) if x.shape == y.shape else "shape"
                bad.append((g["name"], what, lanes))
    assert not bad, bad


@pytest.mark.gpu
def test_match_one_launch_per_group_is_identical(dev, match_want):
    groups = C.match_groups()
    together = _match(groups, dev)
    for g, both in zip(groups, together):
        alone = _match([g], dev)[0]
        for x, y, z in zip(alone, both, match_want[g["name"]]):
            assert np.array_equal(x, y), g["name"]
            assert np.array_equal(x != 0, z != 0) and x.shape == z.shape, g["name"]
