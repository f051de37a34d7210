"""GPU: om_loss_accumulate (csrc/loss_counter.hip) behind DeviceEvalCounter and the losses' ``enqueue``, at the minimal shapes of
tests/loss_counter_cases.py (image 64 x 64, B = 2, 3 classes, 3 GTs per image; and one scale of one anchor): against the host
path with the equal / 2^-20 split derived there, against the numpy restatement bit for bit, the sticky status words, and the
gradients through ``enqueue(...).backward()``."""
import numpy as np
import pytest
import torch

import loss_counter_cases as cases
import loss_counter_np as cnp

pytestmark = pytest.mark.gpu

STEPS = 5


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.mark.parametrize("single", [False, True], ids=["three_scales", "one_scale_one_anchor"])
@pytest.mark.parametrize("training", [True, False], ids=["training", "validation"])
def test_five_steps_against_the_host_path_and_the_restatement(dev, single, training):
    """5 steps of om_loss + om_loss_accumulate.  The block against the host path (_finish + EvalCounter on the same result
    vectors): raw keys equal, derived keys within 2^-20; the block and every step's loss_sum against the restatement fed the
    same result vectors: bit for bit; with training=True the metric slots stay zero (compare_block asserts it)."""
    from orienmask_amd.loss import DeviceEvalCounter, OrienMaskYOLOMultiScaleLoss
    loss = OrienMaskYOLOMultiScaleLoss(**cases.loss_kwargs(single))
    counter = DeviceEvalCounter(loss, dev)
    w = [float(v) for v in loss.scales_weight]
    results, sums = [], []
    for step, (heads, target) in enumerate(cases.synthetic_batches(40, STEPS, dev, single), 1):
        result = loss.launch(heads, target)
        sums.append(counter.accumulate(result, step, with_metrics=training is not True))
        results.append(result)
    block = counter.block.cpu().numpy()
    results = [r.cpu().numpy() for r in results]
    host, _ = cases.host_counter(loss, results, training)
    report = []
    cases.compare_block(block, loss, host, training is not True, report)
    print("derived keys that differ from the host path:", [(k, d, h) for k, d, h in report if d != h])
    want = cnp.new_block()
    for step, (r, got) in enumerate(zip(results, sums), 1):
        ls = cnp.accumulate(want, r, loss.num_scales, w, training is not True, step)
        assert got.cpu().numpy().tobytes() == np.float32(ls).tobytes(), (step, got.item(), ls)
    assert block.tobytes() == want.tobytes()
    assert cnp.status(block) == (0, 0)
    assert counter.average("loss") == host.average("loss") or \
        abs(counter.average("loss") - host.average("loss")) <= cases.DERIVED_BOUND * host.average("loss")
    # the same steps through enqueue: the same block
    again = DeviceEvalCounter(loss, dev)
    for step, (heads, target) in enumerate(cases.synthetic_batches(40, STEPS, dev, single), 1):
        out = loss.enqueue(heads, target, again, step, training=training)
        assert out.device == dev and out.dim() == 0
    assert again.block.cpu().numpy().tobytes() == block.tobytes()


def test_nan_pred_wh_is_latched_not_raised(dev):
    """A NaN pred_wh logit at step 3 of 5 (a NaN input, not a fault): enqueue does not raise, the flag and first_bad_step == 3 are
    latched and steps 4 and 5 leave them alone; the read raises FloatingPointError naming step 3."""
    from orienmask_amd import lib as omlib
    from orienmask_amd.train import DeviceEvalCounter, OrienMaskYOLOMultiScaleLoss
    loss = OrienMaskYOLOMultiScaleLoss(**cases.loss_kwargs())
    counter = DeviceEvalCounter(loss, dev)
    seen = []
    for step, (heads, target) in enumerate(cases.synthetic_batches(60, STEPS, dev), 1):
        if step == 3:
            heads[1][0][1, 2, 0, 1] = float("nan")            # anchor 0's w logit of one cell of the middle scale
        loss.enqueue(heads, target, counter, step)
        seen.append(cnp.status(counter.block.cpu().numpy()))
    assert seen[:2] == [(0, 0), (0, 0)]
    assert seen[2][0] & omlib.OM_LOSS_FLAG_NONFINITE_WH and seen[2][1] == 3
    assert seen[3] == seen[2] and seen[4] == seen[2]
    for read in (lambda: counter.average("loss"), lambda: counter.average_epoch("loss")):
        with pytest.raises(FloatingPointError, match="step 3"):
            read()
    assert counter.first_bad_step == 3


def test_gradients_through_enqueue_are_those_through_forward(dev):
    """``enqueue(...).backward()`` against the existing ``loss(...)[0].backward()``: the heads' gradients bit for bit."""
    from orienmask_amd.train import DeviceEvalCounter, OrienMaskYOLOMultiScaleLoss
    loss = OrienMaskYOLOMultiScaleLoss(**cases.loss_kwargs())
    counter = DeviceEvalCounter(loss, dev)
    heads, target = cases.synthetic_batches(80, 1, dev)[0]
    grads = []
    for deferred in (False, True):
        leaves = [(b.clone().requires_grad_(), o.clone().requires_grad_()) for b, o in heads]
        out = loss.enqueue(leaves, target, counter, 1) if deferred else loss(leaves, target, training=True)[0]
        assert out.grad_fn is not None
        out.backward()
        grads.append([t.grad for pair in leaves for t in pair])
    for a, b in zip(*grads):
        assert a is not None and b is not None and torch.equal(a, b)
    # a scale without a positive has an all-zero orientation gradient; the bbox heads always have the no-object term's
    assert all(g.abs().max().item() > 0 for g in grads[0][0::2])
    assert counter.average("loss") > 0
