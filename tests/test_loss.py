"""GPU tests of the validation loss (om_loss, csrc/loss.hip) against the reference's own values (tests/golden/loss_*.npz) and the
numpy restatement (tests/loss_np.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import ANCHOR_MASK, ANCHORS_YOLOV4, GOLDEN, golden_files
import loss_np
from test_loss_cpu import TIOU_ULP, _tiou_ulps

pytestmark = pytest.mark.gpu

FIXTURES = golden_files("loss_")
SIDS = ["S32", "S16", "S08"]
TERMS = ["loss_xy", "loss_wh", "loss_obj", "loss_noobj", "loss_cls", "loss_orien_pos", "loss_orien_neg"]
METRICS = ["cls_conf", "obj_pos", "obj_neg", "avg_iou", "recall50", "recall75", "orien_pos_acc", "orien_neg_acc"]
ANCHORS_YOLOV3 = [[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]]
REL = 1e-5


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _loss(cfg):
    from orienmask_amd.eval import OrienMaskYOLOMultiScaleLoss
    return OrienMaskYOLOMultiScaleLoss(**cfg)


def _to(dev, heads, target):
    return ([(b.to(dev), o.to(dev)) for b, o in heads],
            tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in target))


def _cfg(size, anchors, **kw):
    h, w = size
    c = dict(grid_size=[[h // 32, w // 32], [h // 16, w // 16], [h // 8, w // 8]], image_size=[h, w], anchors=anchors,
             anchor_mask=ANCHOR_MASK, num_classes=80, center_region=0.6, valid_region=0.6, label_smooth=False,
             obj_ignore_threshold=0.7, weight=[1, 1, 1, 1, 1, 20, 20], scales_weight=[1, 1, 1])
    c.update(kw)
    return c


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_values(dev, name):
    """Loss terms and float metrics within 1e-5 relative of the reference, integer counts exact, threshold counts exact up to the
    fixture's near-threshold allowance; the same keys in the same order with the same value types."""
    g, cfg, heads, target = loss_np.load_fixture(os.path.join(GOLDEN, name))
    predict, tgt = _to(dev, heads, target)
    loss = _loss(cfg)
    loss_sum, log, mlog = loss(predict, tgt, training=False)
    want = dict(zip([str(k) for k in g["loss_keys"]], g["loss_vals"]))
    wm = dict(zip([str(k) for k in g["metric_keys"]], g["metric_vals"]))
    assert list(log) == list(want) and list(mlog) == list(wm)
    assert loss_sum.device == dev and loss_sum.dim() == 0
    for k, v in want.items():
        assert isinstance(log[k], float)
        assert _rel(log[k], v) <= REL, (name, k, log[k], v)
    for s, sid in enumerate(SIDS):
        near = g["near_%d" % s]
        allow = dict(obj_neg=near[0], recall50=near[1], recall75=near[2], orien_pos_acc=near[3], orien_neg_acc=near[3])
        for k in METRICS:
            (num, cnt), (rn, rc) = mlog[sid + "_" + k], wm[sid + "_" + k]
            assert isinstance(cnt, float)
            if k in ("recall50", "recall75"):
                assert isinstance(num, int)
            if k in ("recall50", "recall75", "orien_pos_acc", "orien_neg_acc"):
                assert abs(num - rn) <= allow[k] and cnt == rc, (name, sid, k, num, rn, cnt, rc)
            elif k == "obj_neg":
                assert abs(cnt - rc) <= allow[k] and _rel(num, rn) <= REL + allow[k], (name, sid, k, num, rn, cnt, rc)
            else:
                assert cnt == rc and _rel(num, rn) <= REL, (name, sid, k, num, rn, cnt, rc)


@pytest.mark.parametrize("name", [f for f in FIXTURES if "544" not in f and "ladder" not in f])     # those with full targets
def test_fixture_targets(dev, name):
    """om_loss_targets against build_targets' outputs: orien_mask and torien bit-exact, txy / masks / bbox_pos_scale exact
    (bbox_neg up to the near-threshold allowance), twh within 1 ulp, tiou within TIOU_ULP, tcls' positive entries equal.
    loss_dup_overlap_border_b1 puts two GTs with different offsets, sizes and classes on one cell: the later GT's box targets
    and both classes."""
    g, cfg, heads, target = loss_np.load_fixture(os.path.join(GOLDEN, name))
    predict, tgt = _to(dev, heads, target)
    loss = _loss(cfg)
    for s in range(3):
        t = {k: v.cpu().numpy() for k, v in loss.targets([p[0] for p in predict], tgt, s).items()}
        n = lambda k: g["t%d_%s" % (s, k)]          # noqa: E731
        tag = (name, s)
        assert np.array_equal(t["orien_mask"], n("omask").astype(np.int32)), tag
        assert np.array_equal(t["torien"], n("torien")), tag
        assert np.array_equal(t["bbox_pos_mask"], n("pos")), tag
        assert np.abs(t["bbox_neg_mask"] - n("neg")).sum() <= g["near_%d" % s][0], tag
        assert np.array_equal(t["bbox_pos_scale"], n("pscale")), tag
        assert np.array_equal(t["txy"], n("txy")), tag
        ulp = np.abs(t["twh"].view(np.int32).astype(np.int64) - n("twh").view(np.int32).astype(np.int64))
        assert ulp.max(initial=0) <= 1, (tag, ulp.max())
        assert np.array_equal(np.argwhere(t["tcls"] > 0.5), n("tcls_on").astype(np.int64)), tag
        # within TIOU_ULP of the reference (exp of the predicted size: see tests/test_loss_cpu.py), zero off the positives
        assert _tiou_ulps(t["tiou"], n("tiou")) <= TIOU_ULP, tag
        on = t["tcls"] > 0.5
        assert np.all(t["tcls"][~on] == np.float32(loss.cfg_struct().label_smooth)), tag


def _random_case(seed):
    rng = np.random.default_rng(seed)
    from orienmask_amd import synth
    size = [(160, 128), (96, 160), (256, 192), (128, 128)][seed % 4]
    B = int(rng.integers(1, 9))
    counts = [int(rng.integers(0, 61)) if rng.random() < 0.8 else 0 for _ in range(B)]
    cfg = _cfg(size, ANCHORS_YOLOV4 if seed % 2 else ANCHORS_YOLOV3, label_smooth=bool(seed % 3 == 0),
               valid_region=[0.6, 0.7][seed % 2], obj_ignore_threshold=[0.5, 0.7][(seed // 2) % 2])
    heads = synth.synth_heads(1000 + seed, B, cfg["grid_size"], regime="sparse")
    target = synth.synth_targets(2000 + seed, B, size[0], size[1], counts)
    return cfg, heads, target


@pytest.mark.parametrize("seed", range(20))
def test_random_cases_match_restatement(dev, seed):
    """HIP against tests/loss_np.py on seeded random cases: B 1..8, 0..60 GTs per image, both anchor sets, label smoothing on and
    off.  The restatement uses correctly rounded elementary functions; so does the device except for its bit-exact sigmoids (one
    ulp apart on a few percent of inputs): terms within 1e-5 relative, counts exact (random data lands on no threshold).
    With at most 60 GTs per image these cases stay within one ballot round of the orientation culls and one trip of the box
    kernels' LDS fill, and rarely pile GTs on a cell; crowds of 63 .. 1024 GTs, piles of 3 .. 9, ROI edges on the tile seams
    and anchor ties are tests/test_loss_crowd.py's directed cases (tests/loss_cases.py)."""
    cfg, heads, target = _random_case(seed)
    predict, tgt = _to(dev, heads, target)
    _, log, mlog = _loss(cfg)(predict, tgt, training=False)
    got = loss_np.LossNP(**cfg)([(b.numpy(), o.numpy()) for b, o in heads], target)
    for s, (terms, metrics, _) in enumerate(got):
        for k, v in zip(TERMS, terms):
            assert _rel(log[SIDS[s] + "_" + k], float(v)) <= REL, (seed, s, k, log[SIDS[s] + "_" + k], float(v))
        for k, (num, cnt) in zip(METRICS, metrics):
            gn, gc = mlog[SIDS[s] + "_" + k]
            assert gc == cnt, (seed, s, k, gc, cnt)
            assert _rel(gn, num) <= REL, (seed, s, k, gn, num)


def test_repeat_and_side_stream_bit_identical(dev):
    cfg, heads, target = _random_case(5)
    predict, tgt = _to(dev, heads, target)
    loss = _loss(cfg)
    r0 = loss.launch(predict, tgt).cpu()
    for _ in range(3):
        assert torch.equal(loss.launch(predict, tgt).cpu(), r0)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        r1 = loss.launch(predict, tgt)
    side.synchronize()
    assert torch.equal(r1.cpu(), r0)


def test_model_heads_read_in_place(dev):
    """Heads straight from the HIP model (NHWC-backed bbox views, orientation views into one buffer) against the same heads as
    contiguous NCHW copies: bit-identical results."""
    from orienmask_amd import synth
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    H, W = 160, 128
    net = OrienMaskYOLOFPNPlus(3, 80).eval()
    net.load_state_dict(synth.synth_state_dict(4, obj_bias=-6.0, head_gain=2.0), strict=True)
    net = net.to(dev)
    x = synth.synth_image_batch(9, 2, H, W).to(dev)
    with torch.no_grad():
        out = net(x)
    assert not out[0][0].is_contiguous()
    target = synth.synth_targets(19, 2, H, W, 8)
    tgt = tuple(torch.from_numpy(a).to(dev) for a in target)
    loss = _loss(_cfg((H, W), ANCHORS_YOLOV4))
    r_view = loss.launch(list(out), tgt).cpu()
    r_copy = loss.launch([(b.contiguous(), o.contiguous()) for b, o in out], tgt).cpu()
    assert torch.equal(r_view, r_copy)


def test_training_mode_and_failures(dev):
    cfg, heads, target = _random_case(3)
    predict, tgt = _to(dev, heads, target)
    loss = _loss(cfg)
    s0, log0, m0 = loss(predict, tgt, training=False)
    s1, log1, m1 = loss(predict, tgt, training=True)
    assert log0 == log1 and torch.equal(s0, s1) and m1 == {} and m0
    # a non-finite pred_wh: the reference prints and exits; here FloatingPointError
    bad = [(b.clone(), o) for b, o in predict]
    bad[1][0][0, 2, 0, 0] = float("inf")
    with pytest.raises(FloatingPointError):
        loss(bad, tgt, training=False)
    # heads that require grad: the backward is out of scope
    with pytest.raises(NotImplementedError):
        loss([(b.clone().requires_grad_(), o) for b, o in predict], tgt)
    # more GTs in one image than the kernel holds
    from orienmask_amd import lib as omlib, synth
    n = omlib.OM_LOSS_MAX_GT + 1
    gb, gc, gi, gm = synth.synth_targets(5, 1, 96, 96, 3)
    big = (np.repeat(gb[:1], n, 0), np.repeat(gc[:1], n, 0), np.array([0, n], np.int64), np.repeat(gm[:1], n, 0))
    c2 = _cfg((96, 96), ANCHORS_YOLOV4)
    h2 = synth.synth_heads(1, 1, c2["grid_size"], regime="sparse")
    p2, t2 = _to(dev, h2, big)
    with pytest.raises(ValueError, match="GTs"):
        _loss(c2)(p2, t2, training=False)              # N > B * OM_LOSS_MAX_GT: refused on the host
    # N within B * OM_LOSS_MAX_GT but one image above the limit: the kernels clamp their reads, the flag word raises
    h3 = synth.synth_heads(1, 2, c2["grid_size"], regime="sparse")
    p3, t3 = _to(dev, h3, (big[0], big[1], np.array([0, n, n], np.int64), big[3]))
    with pytest.raises(ValueError, match="more than %d GTs" % omlib.OM_LOSS_MAX_GT):
        _loss(c2)(p3, t3, training=False)


def test_validate_returns_val_epoch_keys(dev, tmp_path):
    """tester.validate over SyntheticLossLoader with the native COCOMetrics: _val_epoch's val_log keys."""
    import json
    from orienmask_amd import synth
    from orienmask_amd.cocoeval import COCOMetrics
    from orienmask_amd.eval import OrienMaskYOLOPostProcess
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    from orienmask_amd.tester import SyntheticLossLoader, validate
    from orienmask_amd.visualizer import CAT2LABEL
    from conftest import post_cfg
    H = W = 96
    net = OrienMaskYOLOFPNPlus(3, 80).eval()
    net.load_state_dict(synth.synth_state_dict(3, obj_bias=-16.0, head_gain=4.0), strict=True)
    net = net.to(dev)
    post = OrienMaskYOLOPostProcess(device=dev, **post_cfg((H, W)))
    loss = _loss(_cfg((H, W), ANCHORS_YOLOV4))
    cat2label = list(CAT2LABEL["COCO"])
    gt = {"images": [dict(id=i, height=H, width=W) for i in range(4)],
          "categories": [dict(id=int(c), name=str(c)) for c in cat2label],
          "annotations": [dict(id=i + 1, image_id=i, category_id=int(cat2label[i]), segmentation=[[10, 10, 60, 10, 60, 60, 10, 60]],
                               area=2500.0, bbox=[10, 10, 50, 50], iscrowd=0) for i in range(4)]}
    gt_file = tmp_path / "gt.json"
    gt_file.write_text(json.dumps(gt))
    metrics = COCOMetrics(str(gt_file), cat2label, True, str(tmp_path))
    loader = SyntheticLossLoader(4, 2, size=(H, W), seed=7, gts_per_image=5, device=dev)
    val = validate(net, loss, post, loader, coco_metrics=metrics)
    want = ["val_loss"] + ["val_" + k for k in loss.loss_id] + ["val_" + k for k in loss.metric_id]
    assert list(val)[:len(want)] == want
    assert [k for k in val if k.startswith("val_bbox_") or k.startswith("val_segm_")] == \
        ["val_bbox_" + k for k in metrics.metric_keys] + ["val_segm_" + k for k in metrics.metric_keys]
    assert all(isinstance(v, float) or v == -1 for v in val.values())       # EvalCounter: -1 for a key with no items
    no_coco = validate(net, loss, post, loader)
    assert list(no_coco) == want and no_coco["val_loss"] == val["val_loss"]
    # what the reference's collate yields: CPU tensors, moved to the model's device by validate as _val_epoch does
    cpu_loader = SyntheticLossLoader(4, 2, size=(H, W), seed=7, gts_per_image=5, device="cpu")
    assert cpu_loader._batches[0][0].device.type == "cpu" and cpu_loader._batches[0][1][0].device.type == "cpu"
    assert validate(net, loss, post, cpu_loader) == no_coco


def test_peak_memory_bs32(dev):
    """At bs 32, 544 x 544 with 50 GTs per image the call allocates no more than its workspace and result vector."""
    from orienmask_amd import synth
    B, H = 32, 544
    cfg = _cfg((H, H), ANCHORS_YOLOV4)
    heads = synth.synth_heads(77, B, cfg["grid_size"], regime="sparse")
    target = synth.synth_targets(78, B, H, H, 50)
    predict, tgt = _to(dev, heads, target)
    loss = _loss(cfg)
    ws = loss.workspace_bytes(B, len(target[0]))
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    loss(predict, tgt, training=False)
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert peak <= ws + 2 * 1024 * 1024, (peak, ws)
