"""GPU tests of the loss kernels (csrc/loss.hip) on crowded images and piled-up cells: the directed cases of tests/loss_cases.py
against the restatements (tests/loss_np.py, tests/loss_grad_np.py), under the checkers of tests/loss_crowd_checks.py.

What these inputs run for the first time with a checked result: the second and later ballot rounds of both orientation culls
(counts 65 .. 1024, image offsets that are no multiple of 64), the second and later trips of the box kernels' LDS fill (counts
above 256), the cls4 short path with 3 and 4 GTs on a cell and the nmatch > 4 rescan (5, 6 and 9), a winner beyond index 256,
ROI edges on the forward and gradient tile seams, bit-equal anchor IoUs, and OM_LOSS_MAX_GT GTs in one image.

Every case must be clean: before the device is touched each test asserts that the restatement's near-threshold counts of its
case are all zero, so every count and zero pattern is compared exactly."""
import pytest
import torch

import loss_cases
import loss_crowd_checks as checks
from test_loss import METRICS, SIDS, TERMS, _loss, _to
from test_loss_grad import _hip_grads

pytestmark = pytest.mark.gpu

CROWD = "ladder_300_7_pile9"
_ON_DEVICE = {}


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _case(name):
    """(cfg, heads, target, restatement record) of a clean case; nothing here touches the device"""
    cfg, heads, target = loss_cases.build(name)
    ref = loss_cases.reference(name)
    checks.check_near_zero(ref.near, name)
    return cfg, heads, target, ref


def _uploaded(dev, name, heads, target):
    if name not in _ON_DEVICE:
        _ON_DEVICE[name] = _to(dev, heads, target)
    return _ON_DEVICE[name]


@pytest.mark.parametrize("name", loss_cases.NAMES)
def test_values(dev, name):
    """Loss terms and float metrics within 1e-5 relative of LossNP, every count exact, the flag word clear."""
    from orienmask_amd import lib as omlib
    cfg, heads, target, ref = _case(name)
    predict, tgt = _uploaded(dev, name, heads, target)
    loss = _loss(cfg)
    result = loss.launch(predict, tgt)
    assert int(result.cpu()[omlib.OM_LOSS_FLAG_OFF:].view(torch.int32)[0]) == 0
    _, log, mlog = loss._finish(result, False, dev)
    got = [([log[sid + "_" + k] for k in TERMS], [mlog[sid + "_" + k] for k in METRICS]) for sid in SIDS]
    worst = checks.check_values(got, checks.restatement_values(ref), name)
    print("crowd values %s: worst relative term error %.3g" % (name, worst))


@pytest.mark.parametrize("name", loss_cases.NAMES)
def test_targets(dev, name):
    """om_loss_targets against LossNP.build_targets under tests/test_loss.py::test_fixture_targets' rules, at every scale (the
    two 1024-GT cases at S08, where their positives are): the tight pin on the culls and on the winner rule."""
    cfg, heads, target, ref = _case(name)
    predict, tgt = _uploaded(dev, name, heads, target)
    loss = _loss(cfg)
    for s in ([2] if name in loss_cases.LIMIT else range(3)):
        t = {k: v.cpu().numpy() for k, v in loss.targets([p[0] for p in predict], tgt, s).items()}
        checks.check_targets(t, ref.values[s][2], loss.cfg_struct().label_smooth, (name, s))


@pytest.mark.parametrize("name", loss_cases.NAMES)
def test_gradients(dev, name):
    """Both heads' gradients at every scale against LossGradNP: loss_grad_np.mismatches with its default bounds is 0; the
    channels-last bbox head gives the same bits; the values-only path gives the loss values bit for bit."""
    from orienmask_amd.loss import OrienMaskYOLOMultiScaleLoss as ValuesLoss
    cfg, heads, target, ref = _case(name)
    loss_sum, log, grads = _hip_grads(dev, cfg, heads, target, loss_cases.GOUT)
    worst = checks.check_grads([(gb.cpu().numpy(), go.cpu().numpy()) for gb, go in grads], ref.grads, name)
    print("crowd gradients %s: worst error %.3g of the bound" % (name, worst))
    cl = [(b.contiguous(memory_format=torch.channels_last), o) for b, o in heads]
    _, _, g_cl = _hip_grads(dev, cfg, cl, target, loss_cases.GOUT)
    for (a, ao), (b, bo) in zip(grads, g_cl):
        assert b.stride() == b.contiguous(memory_format=torch.channels_last).stride()
        assert torch.equal(a, b.contiguous()) and torch.equal(ao, bo)
    predict, tgt = _uploaded(dev, name, heads, target)
    v_sum, v_log, _ = ValuesLoss(**cfg)(predict, tgt, training=True)
    assert log == v_log and torch.equal(loss_sum.detach(), v_sum)


def test_crowd_repeat_and_side_stream_bit_identical(dev):
    """A crowded batch ([300, 7] GTs, more partial counts for the reduce kernel than any earlier input) twice and once on a side
    stream: the result vectors and both heads' gradients bit-identical."""
    cfg, heads, target, _ = _case(CROWD)
    predict, tgt = _uploaded(dev, CROWD, heads, target)
    loss = _loss(cfg)
    r0 = loss.launch(predict, tgt).cpu()
    assert torch.equal(loss.launch(predict, tgt).cpu(), r0)
    _, _, g0 = _hip_grads(dev, cfg, heads, target, loss_cases.GOUT)
    _, _, g1 = _hip_grads(dev, cfg, heads, target, loss_cases.GOUT)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        r1 = loss.launch(predict, tgt)
        _, _, g2 = _hip_grads(dev, cfg, heads, target, loss_cases.GOUT)
    side.synchronize()
    assert torch.equal(r1.cpu(), r0)
    for (a, ao), (b, bo), (c, co) in zip(g0, g1, g2):
        assert torch.equal(a, b) and torch.equal(ao, bo) and torch.equal(a, c) and torch.equal(ao, co)
