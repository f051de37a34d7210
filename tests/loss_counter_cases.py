"""Shared by tests/test_loss_counter_cpu.py and tests/test_loss_counter.py: the two minimal loss configurations, seeded result
vectors, the host path (``_finish`` + EvalCounter) and the comparison of a counter block against it.

The split of the comparison.  The raw keys -- every per-scale term and every per-scale metric pair -- are the result vector's own
floats and must be EQUAL, sums and items both.  Every other key is derived; the host derives it with torch-CPU sums whose order for
the seven-term scale sum is not left to right.  Both orders add seven non-negative float32 values, so each is within 6 roundings
of the exact sum: 12 roundings apart at most, 12 * 2^-24 < 2^-20 relative, which the identical operations applied afterwards
(products with scales_weight and sums of non-negative values) do not widen beyond the room left.  So every derived key is held to
|device - host| <= 2^-20 * host, items equal.
"""
import numpy as np
import torch

import loss_counter_np as cnp
from conftest import ANCHORS_YOLOV4, ANCHOR_MASK

DERIVED_BOUND = 2.0 ** -20
STEPS = 6
SCALES_WEIGHT = [1, 0.7, 1.3]
WEIGHT = [1.0, 2.0, 1.0, 0.5, 1.0, 3.0, 3.0]
IMAGE, NUM_CLASSES, BATCH, GTS_PER_IMAGE = 64, 3, 2, 3


def loss_kwargs(single=False):
    """image 64 x 64 (grids 2 / 4 / 8, orientation maps 16 x 16), 3 classes; `single`: one scale of one anchor."""
    if single:
        return dict(grid_size=[[IMAGE // 16, IMAGE // 16]], image_size=[IMAGE, IMAGE], anchors=ANCHORS_YOLOV4, anchor_mask=[[4]],
                    num_classes=NUM_CLASSES, scales_id=("S16",), weight=WEIGHT, scales_weight=[0.7])
    return dict(grid_size=[[IMAGE // 32] * 2, [IMAGE // 16] * 2, [IMAGE // 8] * 2], image_size=[IMAGE, IMAGE],
                anchors=ANCHORS_YOLOV4, anchor_mask=ANCHOR_MASK, num_classes=NUM_CLASSES, weight=WEIGHT,
                scales_weight=SCALES_WEIGHT)


def seeded_results(seed, steps=STEPS):
    """[steps, RESULT_FLOATS] float32: non-negative terms, metric pairs with whole counts, whole recall50 / recall75 numerators,
    flag word 0."""
    rng = np.random.RandomState(seed)
    out = np.zeros((steps, cnp.RESULT_FLOATS), np.float32)
    for r in out:
        for s in range(cnp.MAX_SCALES):
            v = r[s * cnp.SCALE_FLOATS:(s + 1) * cnp.SCALE_FLOATS]
            v[:cnp.TERMS] = rng.uniform(0, 4, cnp.TERMS) * rng.choice([1e-3, 1.0, 30.0], cnp.TERMS)
            pairs = v[cnp.TERMS:].reshape(cnp.METRICS, 2)
            pairs[:, 1] = rng.randint(1, 40, cnp.METRICS)
            pairs[:, 0] = rng.uniform(0, 1, cnp.METRICS) * pairs[:, 1]
            pairs[4:6, 0] = np.floor(pairs[4:6, 0])
    return out


def with_flag(result, bits):
    r = result.copy()
    r[cnp.FLAG_OFF:].view(np.int32)[0] = bits
    return r


def host_counter(loss, results, training):
    """The host path over the steps: ``_finish`` on each result vector (it accepts CPU tensors) and the existing EvalCounter fed as
    the reference's loops feed it.  Returns (counter, [loss_sum float32 per step])."""
    from orienmask_amd.loss import EvalCounter
    counter, sums = EvalCounter(), []
    for r in results:
        loss_sum, loss_log, metric_log = loss._finish(torch.from_numpy(np.ascontiguousarray(r)), training, None)
        counter.update("loss", loss_sum.item())
        for key, value in loss_log.items():
            counter.update(key, value)
        for key, value in metric_log.items():
            counter.update(key, value)
        sums.append(np.float32(loss_sum.item()))
    return counter, sums


def raw_keys(loss):
    return set(k for sl in loss.scales_loss_id for k in sl) | set(k for sm in loss.scales_metric_id for k in sm)


def compare_block(block, loss, host, with_metrics, report=None):
    """Assert a counter block (float64 array, stage pairs) against the host EvalCounter; `report` collects (key, device, host)."""
    keys = ["loss"] + list(loss.loss_id) + list(loss.metric_id)
    raw = raw_keys(loss)
    block = np.asarray(block, np.float64)
    n_loss = 1 + len(loss.loss_id)
    for i, key in enumerate(keys):
        dsum, ditems = float(block[cnp.STAGE_OFF + 2 * i]), float(block[cnp.STAGE_OFF + 2 * i + 1])
        if i >= n_loss and not with_metrics:
            assert (dsum, ditems) == (0.0, 0.0), "metric key %s counted with with_metrics=0: %r" % (key, (dsum, ditems))
            assert key not in host.counter
            continue
        hsum, hitems = float(host.counter[key]), float(host.items[key])
        if report is not None:
            report.append((key, dsum, hsum))
        assert ditems == hitems, "%s: items %r, host %r" % (key, ditems, hitems)
        if key in raw:
            assert dsum == hsum, "%s (raw): %r, host %r" % (key, dsum, hsum)
        else:
            assert abs(dsum - hsum) <= DERIVED_BOUND * abs(hsum), "%s (derived): %r, host %r, rel %g" % (
                key, dsum, hsum, abs(dsum - hsum) / max(abs(hsum), 1e-300))
    assert not block[2 * len(keys):cnp.EPOCH_OFF].any()               # nothing behind the loss's keys


def synthetic_batches(seed, n_batches, device, single=False):
    """[(heads, target)] at the minimal shapes: B = 2, 3 GTs per image, seeded heads of the three scales (`single`: of
    loss_kwargs(single=True)'s one scale of one anchor)."""
    from orienmask_amd import synth
    out = []
    for i in range(n_batches):
        g = torch.Generator().manual_seed(seed + i)
        heads = []
        for grid, na in (((IMAGE // 16, 1),) if single else ((IMAGE // 32, 3), (IMAGE // 16, 3), (IMAGE // 8, 3))):
            heads.append((torch.randn(BATCH, na * (5 + NUM_CLASSES), grid, grid, generator=g).to(device),
                          torch.randn(BATCH, 2 * na, IMAGE // 4, IMAGE // 4, generator=g).to(device)))
        gb, gc, gi, gm = synth.synth_targets(seed + 100 + i, BATCH, IMAGE, IMAGE, GTS_PER_IMAGE, NUM_CLASSES)
        out.append((heads, tuple(torch.from_numpy(a).to(device) for a in (gb, gc, gi, gm))))
    return out
