"""CPU tests of the validation loss (orienmask_amd/loss.py): the surface against the reference's, EvalCounter, the struct layout,
and the numpy restatement (tests/loss_np.py) against the reference's own values (tests/golden/loss_*.npz,
tools/gen_golden_loss.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden_files
import loss_np

FIXTURES = golden_files("loss_")


def _fixture(name):
    return loss_np.load_fixture(os.path.join(GOLDEN, name))


def test_fixtures_present():
    assert len(FIXTURES) >= 7, FIXTURES
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in FIXTURES) < 1.5e6


@pytest.mark.parametrize("name", ["loss_a4_544_b2.npz", "loss_base_544_b2.npz"])
def test_surface_and_key_order_match_reference(name):
    """builder.build(config['loss'], orienmask_amd.eval) from the reference's two configs: the attributes the Trainer reads and
    the key order of the reference's loss_log / metric_log (recorded in the fixture)."""
    from orienmask_amd import builder
    from orienmask_amd import eval as om_eval
    g, cfg, _, _ = _fixture(name)
    loss = builder.build(dict(cfg, type="OrienMaskYOLOMultiScaleLoss"), om_eval)
    assert type(loss).__name__ == "OrienMaskYOLOMultiScaleLoss"
    prefix, loss_suffix = ["S32", "S16", "S08"], ["loss_xy", "loss_wh", "loss_obj", "loss_noobj", "loss_cls", "loss_orien_pos",
                                                  "loss_orien_neg", "loss_sum"]
    metric_suffix = ["cls_conf", "obj_pos", "obj_neg", "avg_iou", "recall50", "recall75", "orien_pos_acc", "orien_neg_acc"]
    assert loss.scales_prefix == prefix and loss.loss_suffix == loss_suffix and loss.metric_suffix == metric_suffix
    want_loss = [str(k) for k in g["loss_keys"]]
    assert loss.loss_id + [loss.loss_sum_id] == [k for k in want_loss if k != "loss_sum"] + ["loss_sum"]
    assert loss.metric_id == [str(k) for k in g["metric_keys"]]
    assert loss.scales_loss_id[1] == ["S16_" + k for k in loss_suffix[:-1]]
    assert loss.scales_loss_sum_id == ["S32_loss_sum", "S16_loss_sum", "S08_loss_sum"]
    assert loss.scales_metric_id[2] == ["S08_" + k for k in metric_suffix]
    assert loss.cross_scale_loss_id == ["cross_scale_" + k for k in loss_suffix]
    assert loss.cross_scale_metric_id == ["cross_scale_" + k for k in metric_suffix]
    # the reference's constructor defaults (eval/orienmask_yolo_loss.py:259-267)
    d = om_eval.OrienMaskYOLOMultiScaleLoss(cfg["grid_size"], cfg["image_size"], cfg["anchors"], cfg["anchor_mask"], 80)
    assert (d.center_region, d.valid_region, d.label_smooth, d.obj_ignore_threshold) == (0.6, 0.7, False, 0.5)
    assert [float(w) for w in d.scale_item_weight[0]] == [1.0] * 7


def test_aggregate_matches_reference_on_its_own_values():
    """aggregate() rebuilds loss_log / metric_log, values and types, from a result vector holding the reference's per-scale
    items: the host-side arithmetic of eval/base.py."""
    import torch
    from orienmask_amd import lib as omlib
    from orienmask_amd.loss import OrienMaskYOLOMultiScaleLoss
    for name in FIXTURES:
        g, cfg, _, _ = _fixture(name)
        loss = OrienMaskYOLOMultiScaleLoss(**cfg)
        want = dict(zip([str(k) for k in g["loss_keys"]], g["loss_vals"]))
        wm = dict(zip([str(k) for k in g["metric_keys"]], g["metric_vals"]))
        host = torch.zeros(omlib.OM_LOSS_RESULT_FLOATS)
        for s in range(3):
            base = s * omlib.OM_LOSS_SCALE_FLOATS
            host[base:base + 7] = torch.tensor([want[k] for k in loss.scales_loss_id[s]])
            host[base + 7:base + 23] = torch.tensor([v for k in loss.scales_metric_id[s] for v in wm[k]])
        loss_sum, log, mlog = loss.aggregate(host, training=False)
        assert list(log) == list(want) and list(mlog) == list(wm)
        for k, v in want.items():
            assert log[k] == v, (name, k, log[k], v)
        for (k, v), is_int in zip(wm.items(), g["metric_int"]):
            assert mlog[k] == tuple(v), (name, k)
            assert isinstance(mlog[k][0], int) == bool(is_int), (name, k)
        assert np.float32(loss_sum.item()) == g["loss_sum"]
        _, _, m_train = loss.aggregate(host, training=True)
        assert m_train == {}


def test_eval_counter_known_answers():
    from orienmask_amd.eval import EvalCounter
    c = EvalCounter()
    c.update("loss", 2.0)
    c.update("loss", 4.0)
    c.update("acc", (3.0, 4.0))
    c.update("acc", (1, 4.0))
    c.update("none", (0.0, 0.0))
    assert c.keys == ["loss", "acc", "none"]
    assert c.average("loss") == 3.0 and c.average("acc") == 0.5 and c.average("none") == -1
    c.reset()
    assert c.items == {"loss": 0, "acc": 0, "none": 0} and c.counter["loss"] == 0.
    c.update("loss", 9.0)
    assert c.average("loss") == 9.0
    assert c.average_epoch("loss") == 5.0                   # (2 + 4 + 9) / 3, the stage folded in
    assert c.items["loss"] == 0 and c.items_epoch["loss"] == 3
    assert c.average_epoch("acc") == 0.5 and c.average_epoch("none") == -1
    other = {"items": {"loss": 1, "acc": 2.0, "none": 0}, "counter": {"loss": 3.0, "acc": 1.0, "none": 0.}}
    c.merge(other)
    assert c.average("loss") == 3.0 and c.average("acc") == 0.5
    c.merge_epoch({"items_epoch": {"loss": 1, "acc": 0, "none": 0}, "counter_epoch": {"loss": 1.0, "acc": 0., "none": 0.}})
    assert c.items_epoch["loss"] == 4 and c.counter_epoch["loss"] == 16.0
    c.reset_epoch()
    assert c.average("loss") == -1 and c.average_epoch("loss") == -1


def test_loss_cfg_layout_matches_header():
    """om_loss_cfg's ctypes mirror: field order and offsets as the header declares them (natural C alignment)."""
    from orienmask_amd import lib as omlib
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    body = re.search(r"typedef struct om_loss_cfg \{(.*?)\} om_loss_cfg;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[[^\]]+\])*\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert [f[0] for f in omlib.LossCfg._fields_] == names
    c = omlib.LossCfg
    assert c.anchor_w.offset == 4 * (1 + 3 + 3 + 2 + 3 + 9 + 1)
    assert c.weight.offset == c.anchor_w.offset + 4 * (18 + 1 + 5)
    assert c.bbox_stride.offset == 8 * ((c.weight.offset + 4 * 21 + 7) // 8)
    assert ctypes.sizeof(c) == c.orien_stride.offset + 8 * 9
    assert omlib.OM_LOSS_RESULT_FLOATS == 3 * (7 + 16) + 1


# tiou is the IoU of the predicted box, whose size goes through exp: the reference's (MKL vsExp) and the correctly rounded one
# differ by one ulp on ~1 % of inputs, which moved tiou by at most 2 ulp on the fixtures (measured); zero off the positives
TIOU_ULP = 4


def _tiou_ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.array_equal(a == 0, b == 0)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max(initial=0))


def _check_targets(t, g, s, tag):
    n = lambda k: g["t%d_%s" % (s, k)]          # noqa: E731
    assert np.array_equal(t["pos"], n("pos")), tag
    assert np.array_equal(t["neg"], n("neg")) or np.abs(t["neg"] - n("neg")).sum() <= g["near_%d" % s][0], tag
    assert np.array_equal(t["pscale"], n("pscale")), tag
    assert np.array_equal(t["txy"], n("txy")), tag
    ulp = np.abs(t["twh"].view(np.int32).astype(np.int64) - n("twh").view(np.int32).astype(np.int64))
    assert ulp.max(initial=0) <= 1, (tag, ulp.max())
    assert np.array_equal(np.argwhere(t["tcls"] > 0.5), n("tcls_on").astype(np.int64)), tag
    assert _tiou_ulps(t["tiou"], n("tiou")) <= TIOU_ULP, tag
    assert np.array_equal(t["omask"], n("omask").astype(np.int64)), tag
    assert np.array_equal(t["torien"], n("torien")), tag


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_reference(name):
    """tests/loss_np.py against the reference: the orientation targets and txy bit for bit, twh within 1 ulp, counts exact up to
    the fixture's near-threshold allowance, loss terms within 1e-6 relative (measured worst 1.9e-7: the one-ulp differences of exp / log / sigmoid, summed)."""
    g, cfg, heads, target = _fixture(name)
    got = loss_np.LossNP(**cfg)([(b.numpy(), o.numpy()) for b, o in heads], target)
    want = dict(zip([str(k) for k in g["loss_keys"]], g["loss_vals"]))
    wm = dict(zip([str(k) for k in g["metric_keys"]], g["metric_vals"]))
    worst = 0.0
    for s, (terms, metrics, t) in enumerate(got):
        if "t%d_pos" % s in g.files:
            _check_targets(t, g, s, (name, s))
        sid = ["S32", "S16", "S08"][s]
        for k, v in zip(["loss_xy", "loss_wh", "loss_obj", "loss_noobj", "loss_cls", "loss_orien_pos", "loss_orien_neg"], terms):
            ref = want[sid + "_" + k]
            err = abs(float(v) - ref) / max(abs(ref), 1e-30)
            worst = max(worst, err if ref else abs(float(v)))
            assert (err if ref else abs(float(v))) <= 1e-6, (name, sid, k, float(v), ref)
        near = g["near_%d" % s]
        allow = {"obj_neg": near[0], "recall50": near[1], "recall75": near[2], "orien_pos_acc": near[3], "orien_neg_acc": near[3]}
        for k, (num, cnt) in zip(["cls_conf", "obj_pos", "obj_neg", "avg_iou", "recall50", "recall75", "orien_pos_acc",
                                  "orien_neg_acc"], metrics):
            rn, rc = wm[sid + "_" + k]
            if k in ("recall50", "recall75", "orien_pos_acc", "orien_neg_acc"):
                assert abs(num - rn) <= allow[k] and cnt == rc, (name, sid, k, num, rn)
            elif k == "obj_neg":
                assert abs(cnt - rc) <= allow[k], (name, sid, k, cnt, rc)
                assert abs(num - rn) <= 1e-6 * abs(rn) + allow[k], (name, sid, k, num, rn)
            else:
                assert cnt == rc and abs(num - rn) <= 1e-6 * max(abs(rn), 1.0), (name, sid, k, num, rn)
