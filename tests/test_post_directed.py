"""GPU: csrc/post.hip on the directed cases of tests/post_cases.py (what each plants is asserted by test_post_directed_cpu.py).

Select cases go through OrienMaskYOLOPostProcess: classes, last_keep, detection count and masks equal, centres and scores
bit-identical, box sizes within 2 ulps (MKL's exp of the reference cannot be restated).  Mask cases go through
om_postprocess_masks, called as eval.py's _launch_foreign calls it: torch.equal on every mask, and the rows of out_mask at or
beyond count[b] untouched.  No fallback and no skipped case anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import post_cases as K
from oracle import orienmask_ref as R
from orienmask_amd import lib as omlib

pytestmark = pytest.mark.gpu

_EXPECTED = {}


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


def _ulps(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _hip_post(dev, size=K.SIZE, anchor_mask=K.ANCHOR_MASK, **cfg):
    from orienmask_amd.eval import OrienMaskYOLOPostProcess
    return OrienMaskYOLOPostProcess(device=dev, **K.hip_kwargs(size, anchor_mask, **cfg))


def _to_device(predict, dev, layout):
    if layout == "plain":
        return tuple((b.to(dev), o.to(dev)) for b, o in predict)
    # the model's own layouts: NHWC boxes with a pixel stride of 256 floats, one orientation buffer
    B = predict[0][0].shape[0]
    oriens = torch.cat([p[1] for p in predict], 1).contiguous().to(dev)
    os_ = torch.split(oriens, [p[1].shape[1] for p in predict], dim=1)
    out = []
    for i, (b, _) in enumerate(predict):
        buf = torch.zeros(B, b.shape[2], b.shape[3], 256, device=dev)
        buf[..., :b.shape[1]] = b.permute(0, 2, 3, 1).to(dev)
        out.append((buf[..., :b.shape[1]].permute(0, 3, 1, 2), os_[i]))
    return tuple(out)


def _expected_select(cid):
    """Cases without a tie at a cut: the oracle itself.  With one: the oracle's pipeline under the tie rule (expected_stable)."""
    if cid not in _EXPECTED:
        c = K.select_cases()[cid]
        oracle = K.make_oracle(K.SIZE, **c.cfg)
        _EXPECTED[cid] = K.expected_stable(oracle, c.predict, 0) if c.stable else oracle(c.predict)[0]
    return _EXPECTED[cid]


def _check_exact(r, keep, want, tag):
    n = want["bbox"].shape[0]
    differing = -1 if r["mask"].shape != want["mask"].shape else int((r["mask"].cpu() != want["mask"]).sum())
    print("%s: %d detections (expected %d), %d differing mask pixels" % (tag, r["bbox"].shape[0], n, differing))
    assert r["bbox"].shape[0] == n, (tag, r["bbox"].shape[0], n)
    assert torch.equal(r["cls"].cpu(), want["cls"]), (tag, "cls")
    assert torch.equal(keep.cpu().long(), want["keep"]), (tag, "last_keep")
    got, wb = r["bbox"].cpu().numpy(), want["bbox"].numpy()
    if n:
        assert np.array_equal(got[:, [0, 1, 4]].view(np.uint32), wb[:, [0, 1, 4]].view(np.uint32)), (tag, "cx / cy / score not bit-identical")
        assert _ulps(got[:, 2:4], wb[:, 2:4]).max() <= 2, (tag, "w / h off by more than 2 ulps")
    assert r["mask"].dtype == torch.bool and torch.equal(r["mask"].cpu(), want["mask"]), (tag, "masks", differing)


SELECT_RUNS = [(cid, layout) for cid in K.select_cases() for layout in (("model", "plain") if cid[:2] in ("S2", "S5") else ("plain",))]


@pytest.mark.parametrize("cid,layout", SELECT_RUNS)
def test_select_case(dev, cid, layout):
    c = K.select_cases()[cid]
    post = _hip_post(dev, **c.cfg)
    res = post(_to_device(c.predict, dev, layout))
    assert len(res) == 1
    _check_exact(res[0], post.last_keep[0], _expected_select(cid), (cid, layout))


def test_s2_selection_does_not_depend_on_the_path(dev):
    """4095 and 4096 passing pairs are sorted from the compacted list, 4097 go through the radix select: same 400 pairs."""
    outs = []
    for total in (4095, 4096, 4097):
        c = K.select_cases()["S2_total%d" % total]
        post = _hip_post(dev, **c.cfg)
        r = post(_to_device(c.predict, dev, "model"))[0]
        outs.append((r["bbox"].clone(), r["cls"].clone(), r["mask"].clone(), post.last_keep[0].clone()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    assert outs[0][0].shape[0] == 400


def test_s9_batch_gives_each_image_its_own_result(dev):
    """The radix path, the list path at total == nms_pre and an empty image in one batch, after an all-pass run has filled
    the key workspace of every image: per image as when run alone."""
    members = [K.select_cases()[cid] if cid else None for cid in K.S9_MEMBERS]
    cfg = dict(nms_pre=400, nms_post=400)
    assert all(m is None or m.cfg == cfg for m in members)
    predict = K.cat_batch([m.predict if m else K.empty_predict() for m in members])
    post = _hip_post(dev, **cfg)
    dirty = post(_to_device(K.all_pass_predict(3), dev, "model"))
    assert all(r["bbox"].shape[0] > 0 for r in dirty)
    res = post(_to_device(predict, dev, "model"))
    assert len(res) == 3
    for b, (m, r) in enumerate(zip(members, res)):
        if m is None:
            assert r["bbox"].shape[0] == 0 and r["mask"].shape[0] == 0 and r["cls"].shape[0] == 0
        else:
            _check_exact(r, post.last_keep[b], _expected_select(m.id), ("S9", b, m.id))


# ------------------------------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------------------------------
def _run_masks(dev, case, images=None):
    """om_postprocess_masks on the case (or on a sub-batch of it), out_mask pre-filled with 0xAB."""
    L = omlib.load()
    sel = slice(None) if images is None else images
    oriens = case.oriens[sel].contiguous().to(dev)
    dets = case.dets[sel].contiguous().to(dev)
    fields = case.fields[sel].contiguous().to(dev)
    counts = case.counts[sel].contiguous().to(dev)
    B = oriens.shape[0]
    post = _hip_post(dev, case.size, case.anchor_mask, nms_pre=max(400, case.nms_post), nms_post=case.nms_post)
    cfg = post.cfg_struct(255)
    ws = post._workspace(cfg, B, dev, 255)
    out_mask = torch.full((B, case.nms_post, case.size[0], case.size[1]), 0xAB, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        omlib.check(L.om_postprocess_masks(ctypes.byref(cfg), p(oriens), B, p(dets), p(fields), p(counts), p(out_mask), p(ws), ws.numel(),
                                           omlib.current_stream_ptr(dev)), "om_postprocess_masks")
    torch.cuda.synchronize()
    return out_mask.cpu()


def _check_masks(out_mask, want, counts, tag):
    differing = 0
    for b, w in enumerate(want):
        n = int(counts[b])
        assert w.shape[0] == n
        got = out_mask[b, :n]
        differing += int((got != torch.from_numpy(w).to(torch.uint8)).sum())
    print("%s: %d differing mask pixels" % (tag, differing))
    for b, w in enumerate(want):
        n = int(counts[b])
        assert torch.equal(out_mask[b, :n], torch.from_numpy(w).to(torch.uint8)), (tag, b, differing)
        assert (out_mask[b, n:] == 0xAB).all(), (tag, b, "rows at or beyond count[b] were written")


@pytest.mark.parametrize("cid", list(K.mask_cases()))
def test_mask_case(dev, cid):
    case = K.mask_cases()[cid]
    _check_masks(_run_masks(dev, case), K.expected_masks(case), case.counts, cid)


def test_mask_unchunked_launch_equals_chunked(dev):
    """Fourteen 512 x 512 images take the form in which one workgroup walks all detections of its field; the first image run
    alone takes chunks of 8.  Same bits, and both equal the oracle."""
    case = K.unchunked_case()
    assert K.mask_launch_unchunked(case.size, case.oriens.shape[0], 9) and not K.mask_launch_unchunked(case.size, 1, 9)
    whole = _run_masks(dev, case)
    alone = _run_masks(dev, case, images=slice(0, 1))
    assert torch.equal(whole[0], alone[0])
    _check_masks(whole, K.expected_masks(case), case.counts, case.id)


@pytest.mark.parametrize("cid", list(K.fused_cases()))
def test_fused_postprocess_on_exact_and_special_boxes(dev, cid):
    """D1 and D2 through heads and the fused om_postprocess: the mask constants come from the select kernel's tail instead of
    post_detpar_kernel.  The detections equal the oracle's (sizes within 2 ulps, non-finite ones in the same places); the masks
    equal the oracle's arithmetic on the detections the kernel returned."""
    c = K.fused_cases()[cid]
    cfg = dict(c.cfg)
    anchors = cfg.pop("anchors", K.ANCHORS_YOLOV4)
    oracle = R.PostProcessOracle(K.grids_of(K.SIZE), list(K.SIZE), anchors, K.ANCHOR_MASK, K.C, conf_thresh=K.CONF_THRESH, **cfg)
    want = oracle(c.predict)[0]
    post = _hip_post(dev, anchors=anchors, **cfg)
    r = post(_to_device(c.predict, dev, "plain"))[0]
    n = want["bbox"].shape[0]
    assert r["bbox"].shape[0] == n > 0 and torch.equal(r["cls"].cpu(), want["cls"]) and torch.equal(post.last_keep[0].cpu().long(), want["keep"])
    got, wb = r["bbox"].cpu().numpy(), want["bbox"].numpy()
    assert np.array_equal(np.isnan(got), np.isnan(wb)) and np.array_equal(np.isinf(got), np.isinf(wb))
    fin = np.isfinite(wb)
    assert np.array_equal(got[:, [0, 1, 4]][fin[:, [0, 1, 4]]], wb[:, [0, 1, 4]][fin[:, [0, 1, 4]]])
    assert _ulps(got[:, 2:4][fin[:, 2:4]], wb[:, 2:4][fin[:, 2:4]]).max() <= 2
    if cid.startswith("D1"):                   # tw = th = 0: the sizes are the anchors themselves, bit for bit
        assert np.array_equal(got.view(np.uint32), wb.view(np.uint32))
    masks = K.masks_of(oracle, oracle.orien_field(c.predict, 0), torch.from_numpy(got), want["anchor"])
    differing = int((r["mask"].cpu() != masks).sum())
    print("%s: %d detections, %d differing mask pixels" % (cid, n, differing))
    assert torch.equal(r["mask"].cpu(), masks), (cid, differing)
    if np.array_equal(got.view(np.uint32), wb.view(np.uint32)):
        assert torch.equal(masks, want["mask"])
