"""CPU: the arithmetic of om_loss_accumulate (tests/loss_counter_np.py restates it) against the host path it replaces, the
DeviceEvalCounter on a CPU block against the existing EvalCounter, its gather over two gloo ranks, and the C ABI's new surface.
The equal / 2^-20 split of the comparison is derived in tests/loss_counter_cases.py."""
import os
import re
import socket

import numpy as np
import pytest
import torch

import loss_counter_cases as cases
import loss_counter_np as cnp
from conftest import REPO


def _loss(single=False):
    from orienmask_amd.loss import OrienMaskYOLOMultiScaleLoss
    return OrienMaskYOLOMultiScaleLoss(**cases.loss_kwargs(single))


def _check_restatement(mutant=None, single=False):
    """Everything the restatement is held to; the mutants must fail it."""
    loss = _loss(single)
    w = [float(v) for v in loss.scales_weight]
    results = cases.seeded_results(11)
    for training in (True, False):
        host, host_sums = cases.host_counter(loss, results, training)
        block = cnp.new_block()
        sums = [cnp.accumulate(block, r, loss.num_scales, w, training is not True, step, mutant)
                for step, r in enumerate(results, 1)]
        cases.compare_block(block, loss, host, training is not True)
        for a, b in zip(sums, host_sums):
            assert abs(float(a) - float(b)) <= cases.DERIVED_BOUND * abs(float(b))
        assert cnp.status(block) == (0, 0)
    # the sticky status: bad steps 3 and 5 of 6; the first one stays latched, the bits accumulate
    block = cnp.new_block()
    for step, r in enumerate(results, 1):
        bits = {3: 1, 5: 4}.get(step, 0)
        cnp.accumulate(block, cases.with_flag(r, bits), loss.num_scales, w, False, step, mutant)
        assert cnp.status(block) == ((0, 0) if step < 3 else (1, 3) if step < 5 else (5, 3))
    # a non-finite loss_sum sets the counter's own bit
    block = cnp.new_block()
    r = results[0].copy()
    r[2] = np.inf
    cnp.accumulate(block, r, loss.num_scales, w, False, 7, mutant)
    assert cnp.status(block) == (cnp.FLAG_NONFINITE_LOSS, 7)


@pytest.mark.parametrize("single", [False, True], ids=["three_scales", "one_scale_one_anchor"])
def test_restatement_matches_the_host_path(built, single):
    _check_restatement(single=single)


@pytest.mark.parametrize("mutant", ["metrics_always", "weight_twice", "step_overwrite"])
def test_the_comparison_notices_each_mutant(built, mutant):
    with pytest.raises(AssertionError):
        _check_restatement(mutant)


@pytest.mark.parametrize("single", [False, True], ids=["three_scales", "one_scale_one_anchor"])
def test_torch_comparator_equals_the_restatement(built, single):
    """DeviceEvalCounter on a CPU block (the 'torch' comparator of the kernel): the block bit for bit, loss_sum bit for bit."""
    from orienmask_amd.loss import DeviceEvalCounter
    loss = _loss(single)
    w = [float(v) for v in loss.scales_weight]
    for with_metrics in (False, True):
        counter, block = DeviceEvalCounter(loss, "cpu"), cnp.new_block()
        for step, r in enumerate(cases.seeded_results(5), 1):
            r = cases.with_flag(r, 2) if step == 4 else r
            got = counter.accumulate(torch.from_numpy(r), step, with_metrics=with_metrics)
            want = cnp.accumulate(block, r, loss.num_scales, w, with_metrics, step)
            assert got.dtype == torch.float32 and got.numpy().tobytes() == np.float32(want).tobytes()
        assert counter.block.numpy().tobytes() == block.tobytes()
        with pytest.raises(ValueError, match="step 4"):
            counter.average("loss")


def test_device_counter_has_evalcounter_semantics(built):
    """average / average_epoch / reset / reset_epoch as the existing EvalCounter fed the same values, -1 for no items included."""
    from orienmask_amd.loss import DeviceEvalCounter, EvalCounter
    loss = _loss()
    results = cases.seeded_results(3)
    dev, host = DeviceEvalCounter(loss, "cpu"), EvalCounter()
    assert dev.keys == ["loss"] + loss.loss_id + loss.metric_id
    assert dev.average("loss") == -1 and dev.average_epoch("S32_cls_conf") == -1

    def feed(rs, first_step):
        for step, r in enumerate(rs, first_step):
            t = torch.from_numpy(r)
            loss_sum = dev.accumulate(t, step, with_metrics=True)
            # the host counter gets the device's own derived values: this test is about the counter, not the derivation
            _, values, mets = cnp.step_values(r, loss.num_scales, [float(v) for v in loss.scales_weight])
            assert np.float32(loss_sum.item()) == values[0]
            for key, v in zip(dev.keys, values):
                host.update(key, float(v))
            for key, (n, c) in zip(loss.metric_id, mets):
                host.update(key, (float(n), float(c)))

    feed(results[:2], 1)
    for key in dev.keys:
        assert dev.average(key) == host.average(key), key
    assert dev.averages() == {k: host.average(k) for k in dev.keys}
    dev.reset(), host.reset()
    for key in ("loss", "S08_avg_iou"):
        assert dev.average(key) == -1 == host.average(key)
    feed(results[2:5], 3)
    for key in dev.keys[::3]:                   # average_epoch folds the keys it answers for, as EvalCounter's does
        assert dev.average_epoch(key) == host.average_epoch(key), key
    for key in dev.keys:
        assert dev.average(key) == host.average(key), key
    feed(results[5:], 6)
    assert dev.averages_epoch() == {k: host.average_epoch(k) for k in dev.keys}
    dev.reset_epoch(), host.reset_epoch()
    assert not dev.block.any()
    for key in dev.keys:
        assert dev.average(key) == -1 == host.average(key) and dev.average_epoch(key) == -1 == host.average_epoch(key)


def test_check_raises_what_the_host_path_raises(built):
    from orienmask_amd import lib as omlib
    from orienmask_amd.loss import DeviceEvalCounter
    loss = _loss()
    r = cases.seeded_results(1)[0]
    nan = r.copy()
    nan[0] = np.nan
    for bad, exc, text in ((cases.with_flag(r, omlib.OM_LOSS_FLAG_NONFINITE_WH), FloatingPointError, "pred_wh not finite"),
                           (cases.with_flag(r, omlib.OM_LOSS_FLAG_TOO_MANY_GT), ValueError, "more than 1024 GTs"),
                           (cases.with_flag(r, omlib.OM_LOSS_FLAG_BAD_CLASS), ValueError, r"outside \[0, 3\)"),
                           (nan, FloatingPointError, "loss not finite")):
        counter = DeviceEvalCounter(loss, "cpu")
        counter.accumulate(torch.from_numpy(r), 1)
        counter.check()
        counter.accumulate(torch.from_numpy(bad), 2)
        counter.accumulate(torch.from_numpy(r), 3)
        for read in (counter.check, lambda: counter.average("loss"), lambda: counter.average_epoch("loss"), counter.averages):
            with pytest.raises(exc, match=text + r".*step 2"):
                read()
        assert counter.first_bad_step == 2 and counter.flags
        if not np.isnan(bad[0]):                # the same error as the host path's
            with pytest.raises(exc, match=text):
                loss._finish(torch.from_numpy(bad), True, None)


# ---- two gloo ranks (the idiom of tests/test_dist_cpu.py)
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_worker(rank, world, port, q):
    import torch.distributed as dist
    torch.set_num_threads(min(4, torch.get_num_threads()))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from orienmask_amd.loss import DeviceEvalCounter
    loss = _loss()
    counter = DeviceEvalCounter(loss, "cpu")
    results = cases.seeded_results(21 + rank, steps=3)
    for step, r in enumerate(results, 1):
        r = cases.with_flag(r, 4) if (rank, step) == (1, 2) else r
        counter.accumulate(torch.from_numpy(r), 10 * rank + step, with_metrics=True)
    counter.gather()
    q.put((rank, counter.block.numpy().tobytes()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gather_is_the_rank_order_merge(built):
    """gather() on both ranks equals ONE counter fed rank 0's values and then rank 1's; the flag of rank 1's second step and its
    step index arrive on both."""
    import torch.multiprocessing as mp
    from orienmask_amd.loss import DeviceEvalCounter
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted(q.get(timeout=120) for _ in range(2))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    loss = _loss()
    one = DeviceEvalCounter(loss, "cpu")
    for rank in range(2):
        for step, r in enumerate(cases.seeded_results(21 + rank, steps=3), 1):
            r = cases.with_flag(r, 4) if (rank, step) == (1, 2) else r
            one.accumulate(torch.from_numpy(r), 10 * rank + step, with_metrics=True)
    assert cnp.status(one.block.numpy()) == (4, 12)
    assert got[0][1] == got[1][1] == one.block.numpy().tobytes()


# ---- header, library, lib.py
def test_counter_symbol_and_layout_macros(built):
    from orienmask_amd import lib as omlib
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    assert re.search(r"\bint om_loss_accumulate\(const float\* result, int num_scales, const float\* scales_weight", header)
    assert "om_loss_accumulate" in omlib.SIGNATURES and hasattr(omlib.load(), "om_loss_accumulate")
    env = {"OM_MAX_SCALES": omlib.OM_MAX_SCALES, "OM_LOSS_METRICS": omlib.OM_LOSS_METRICS}
    for name in ("OM_COUNTER_MAX_KEYS", "OM_COUNTER_STAGE_OFF", "OM_COUNTER_EPOCH_OFF", "OM_COUNTER_FLAG_OFF", "OM_COUNTER_STEP_OFF",
                 "OM_COUNTER_BLOCK_DOUBLES", "OM_COUNTER_FLAG_NONFINITE_LOSS"):
        m = re.search(r"^#define %s (.+)$" % name, header, re.M)
        assert m, name
        env[name] = eval(m.group(1), {}, env)           # the macros are integer expressions of the ones before them
        assert env[name] == getattr(omlib, name), name
    assert (cnp.MAX_KEYS, cnp.STAGE_OFF, cnp.EPOCH_OFF, cnp.BLOCK_FLAG_OFF, cnp.STEP_OFF, cnp.BLOCK_DOUBLES, cnp.FLAG_NONFINITE_LOSS) == \
        tuple(env[n] for n in ("OM_COUNTER_MAX_KEYS", "OM_COUNTER_STAGE_OFF", "OM_COUNTER_EPOCH_OFF", "OM_COUNTER_FLAG_OFF",
                               "OM_COUNTER_STEP_OFF", "OM_COUNTER_BLOCK_DOUBLES", "OM_COUNTER_FLAG_NONFINITE_LOSS"))
    assert omlib.OM_COUNTER_FLAG_NONFINITE_LOSS & (omlib.OM_LOSS_FLAG_NONFINITE_WH | omlib.OM_LOSS_FLAG_TOO_MANY_GT
                                                   | omlib.OM_LOSS_FLAG_BAD_CLASS) == 0
    assert omlib.OM_COUNTER_MAX_KEYS == 1 + len(_loss().loss_id) + len(_loss().metric_id)


# ---- tester.validate(counter=, group=): the deferred validation loop and its merge over two gloo ranks
class _EnqueueLoss:
    """A loss with the real key lists whose enqueue feeds seeded result vectors: batch b of the loader is result vector b."""

    def __init__(self):
        self.real = _loss()
        self.loss_id, self.metric_id = self.real.loss_id, self.real.metric_id
        self.num_scales, self.scales_weight, self.num_classes = self.real.num_scales, self.real.scales_weight, self.real.num_classes
        self.results = cases.seeded_results(31, steps=5)

    def enqueue(self, predict, target, counter, step, training=True):
        return counter.accumulate(torch.from_numpy(self.results[int(predict)]), step, with_metrics=training is not True)


class _Coco:
    """The COCOMetrics surface validate touches."""
    with_mask = True

    def __init__(self):
        self.reset()

    def reset(self):
        self.bbox_results, self.segm_results = [], []

    def to_coco_format(self, info, detections):
        return dict(bbox=[dict(image_id=i["id"]) for i in info], segm=[dict(image_id=i["id"], m=1) for i in info])

    def update_results(self, fmt):
        self.bbox_results += fmt["bbox"]
        self.segm_results += fmt["segm"]

    def coco_eval(self):
        return dict(bbox_ids=[r["image_id"] for r in self.bbox_results], segm_n=len(self.segm_results))


def _batches(lo, hi):
    return [(torch.tensor(float(b)), (torch.zeros(1),), [dict(id=b)]) for b in range(lo, hi)]


def _validate(lo, hi):
    from orienmask_amd.loss import DeviceEvalCounter
    from orienmask_amd.tester import validate
    loss = _EnqueueLoss()
    model = torch.nn.Identity()
    model.register_parameter("p", torch.nn.Parameter(torch.zeros(1)))          # validate reads the model's device from it
    return validate(model, loss, lambda predict: None, _batches(lo, hi), _Coco(), counter=DeviceEvalCounter(loss, "cpu"))


def _validate_worker(rank, world, port, q):
    import torch.distributed as dist
    torch.set_num_threads(min(4, torch.get_num_threads()))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, _validate(*((0, 3) if rank == 0 else (3, 5)))))
    dist.barrier()
    dist.destroy_process_group()


def test_validate_with_a_counter_merges_two_ranks(built):
    """Rank 0 validates batches 0-2 and rank 1 batches 3-4; both return the val_log of one rank that validated all five (the
    counters added in rank order, the COCO records concatenated in rank order), and that log is the host path's."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_validate_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted(q.get(timeout=120) for _ in range(2))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    one = _validate(0, 5)
    assert got[0][1] == got[1][1] == one
    assert one["val_bbox_ids"] == [0, 1, 2, 3, 4] and one["val_segm_n"] == 5
    loss = _EnqueueLoss()
    host, _ = cases.host_counter(loss.real, loss.results, training=False)
    raw = cases.raw_keys(loss.real)
    assert set(one) == {"val_loss", "val_bbox_ids", "val_segm_n"} | {"val_" + k for k in loss.loss_id + loss.metric_id}
    for key in ["loss"] + loss.loss_id + loss.metric_id:
        want = host.average_epoch(key)
        if key in raw:
            assert one["val_" + key] == want, key
        else:
            assert abs(one["val_" + key] - want) <= cases.DERIVED_BOUND * abs(want), key
