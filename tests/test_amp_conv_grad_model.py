"""GPU tests of the training models with amp='bf16', conv_forward='hip' and conv_grad='hip': every convolution node of a step, forward
and backward, is this package's (csrc/conv_fwd_bf16.hip, csrc/conv_grad_bf16.hip, csrc/conv_dw.hip).

tests/test_amp_conv_model.py's setting: FPN-Plus and the non-Plus model at 2 x 3 x 96 x 96, truth = the same model in float64 on the
CPU (backend 'torch', no amp).  The comparator is conv_grad='torch' (torch's bf16 gradients behind the same forward) on the same GPU,
same weights, same input; the project's bound: the maximum error over a tensor's scale may be at most TWICE the comparator's, with a
floor at the bf16 unit 2^-8.  Measured ratios are recorded in DESIGN.md 3.29."""
import numpy as np
import pytest
import torch

import bn_act_np as N
import train_step as T
from orienmask_amd import lib as omlib, model as infer_model, train
from test_amp_conv_model import GRADS, MODELS, UNIT, _build, _step, _weights, fixture  # noqa: F401  (fixture: a pytest fixture)

pytestmark = pytest.mark.gpu

HIPGRAD = dict(amp="bf16", conv_forward="hip", conv_grad="hip")
GRAD_ENTRIES = ("om_conv2d_bf16_grad_input", "om_conv2d_bf16_grad_weight")


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(MODELS))
def test_gradients_against_float64_and_the_torch_gradients(dev, fixture, name):
    sd0, x, cot = fixture
    sd = _weights(name, sd0)
    ref, _ = _step(name, sd, x, cot, "cpu", torch.float64, backend="torch")
    want = {n: p.grad.numpy() for n, p in ref.named_parameters() if n in GRADS}
    err, heads = {}, {}
    for cg in ("hip", "torch"):
        net, heads[cg] = _step(name, sd, x, cot, dev, amp="bf16", conv_forward="hip", conv_grad=cg)
        assert all(p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all() for p in net.parameters()), cg
        assert list(net.state_dict()) == list(sd)
        params = dict(net.named_parameters())
        err[cg] = {n: N.rel_max(params[n].grad.cpu().numpy(), want[n]) for n in GRADS}
    # the forward is the same
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(heads["hip"], heads["torch"]))
    failed = []
    for k in GRADS:
        bound = max(2 * err["torch"][k], UNIT)
        print("%-14s %-40s conv_grad hip %.3g  torch %.3g  ratio %.2f  bound %.3g"
              % (name, k, err["hip"][k], err["torch"][k], err["hip"][k] / max(err["torch"][k], 1e-30), bound))
        if not err["hip"][k] <= bound:
            failed.append((k, err["hip"][k], err["torch"][k]))
    assert not failed, failed


def _census(dev, fixture, monkeypatch, frozen_stages):
    sd, x, cot = fixture
    net = _build("OrienMaskYOLOFPNPlus", sd, dev, frozen_stages=frozen_stages, **HIPGRAD).train()
    calls, backends = [], []
    launch, backward = omlib.launch, train.conv2d_bf16_backward
    monkeypatch.setattr(omlib, "launch", lambda name, *a, **k: (calls.append(name), launch(name, *a, **k))[1])
    monkeypatch.setattr(train, "conv2d_bf16_backward", lambda *a, **k: (backends.append(k.get("backend")), backward(*a, **k))[1])
    T.step(net, x.to(dev), [c.to(dev) for c in cot])
    torch.cuda.synchronize(dev)
    return net, calls, backends


def test_every_gradient_of_a_step_is_a_launch_of_this_package(dev, fixture, monkeypatch):
    net, calls, backends = _census(dev, fixture, monkeypatch, 0)
    assert calls.count("om_conv2d_bf16_forward") == 90
    assert calls.count("om_conv2d_bf16_grad_weight") == 90
    assert calls.count("om_conv2d_bf16_grad_input") == 89              # none for the image
    assert backends == ["hip"] * 90
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


def test_a_frozen_backbone_launches_no_gradient(dev, fixture, monkeypatch):
    net, calls, backends = _census(dev, fixture, monkeypatch, 6)
    assert calls.count("om_conv2d_bf16_frozen_forward") == 52
    assert calls.count("om_conv2d_bf16_grad_weight") == 90 - 52 and backends == ["hip"] * (90 - 52)
    # the layers that read a backbone feature still owe no gradient to it: one input gradient fewer per such layer
    assert 0 < calls.count("om_conv2d_bf16_grad_input") <= 90 - 52
    for n, p in net.named_parameters():
        assert (p.grad is None) == n.startswith("backbone."), n


def test_two_trainer_steps_repeat_bit_for_bit_without_the_deterministic_flag(dev):
    """The point of conv_grad='hip': every node of an amp step is this package's, so the loss and every parameter after each of two
    trainer steps are identical between two runs from scratch, with cudnn.deterministic off."""
    assert not torch.backends.cudnn.deterministic
    cfg = dict(amp="bf16", conv_forward="hip", conv_grad="hip", route_backend="hip")
    la, pa, net = T.trainer_steps(dev, cfg, 2)
    assert net.conv_grad == "hip"
    lb, pb, _ = T.trainer_steps(dev, cfg, 2)
    assert not torch.backends.cudnn.deterministic
    for s in range(2):
        assert np.array_equal(la[s], lb[s]), s
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(pa[s], pb[s])), s


def test_the_checkpoint_moves(dev):
    _, _, net = T.trainer_steps(dev, HIPGRAD, 1)
    sd = net.state_dict()
    plain = train.OrienMaskYOLOFPNPlus(3, 80)
    plain.load_state_dict(sd, strict=True)
    assert all(a.dtype == b.dtype and torch.equal(a, b.cpu()) for a, b in zip(plain.state_dict().values(), sd.values()))
    infer_model.OrienMaskYOLOFPNPlus(3, 80).load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
