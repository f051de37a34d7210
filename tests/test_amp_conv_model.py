"""GPU tests of the training models with amp='bf16' and conv_forward='hip': every forward convolution is this package's bf16 kernel
(csrc/conv_fwd_bf16.hip) -- conv2d_bf16 in the blocks and heads, one fused kernel per frozen block -- with torch's bf16 gradients.

tests/test_amp_model.py's setting: FPN-Plus and the non-Plus model at 2 x 3 x 96 x 96, truth = the same model in float64 on the CPU
(backend 'torch', no amp).  The comparator is amp='bf16' with torch's convolutions on the same GPU, same weights, same input; the
project's bound: the maximum error over a tensor's scale may be at most TWICE the comparator's, with a floor at the bf16 unit 2^-8.
Measured ratios are recorded in DESIGN.md 3.28."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, fixture_weights_and_input
import bn_act_np as N
import train_step as T
from orienmask_amd import builder, lib as omlib, model as infer_model, synth, train
from orienmask_amd import optim as O

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -8
GRADS = ("backbone.conv1.conv_block.0.weight", "neck4.4.conv_block.0.weight")
HIPCONV = dict(amp="bf16", conv_forward="hip")
MODELS = {"OrienMaskYOLOFPNPlus": train.OrienMaskYOLOFPNPlus, "OrienMaskYOLO": train.OrienMaskYOLO}


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(GOLDEN, "train_step_f96_b2.npz"))
    sd, x = fixture_weights_and_input(g)
    cot = [torch.from_numpy(c) for c in N.cotangents(int(g["gseed"]), [g[k].shape for k in N.HEAD_KEYS])]
    return sd, x, cot


def _weights(name, sd):
    """The fixture's FPN-Plus weights; for the non-Plus model the tensors of the same name and shape over a seeded initialisation."""
    if name == "OrienMaskYOLOFPNPlus":
        return sd
    torch.manual_seed(11)
    own = MODELS[name](3, 80, backend="torch").state_dict()
    own.update({k: v for k, v in sd.items() if k in own and tuple(v.shape) == tuple(own[k].shape)})
    return own


def _build(name, sd, device, **kw):
    net = MODELS[name](3, 80, **kw)
    net.load_state_dict(sd, strict=True)
    return net.to(device)


def _step(name, sd, x, cot, device, dtype=None, **kw):
    net = _build(name, sd, device, **kw).train()
    if dtype is not None:
        net, x, cot = net.to(dtype), x.to(dtype), [c.to(dtype) for c in cot]
    heads = [t.detach() for t in T.step(net, x.to(device), [c.to(device) for c in cot])]
    return net, heads


@pytest.mark.parametrize("name", list(MODELS))
def test_heads_and_gradients_against_float64_and_the_torch_convolutions(dev, fixture, name):
    sd0, x, cot = fixture
    sd = _weights(name, sd0)
    ref, want_heads = _step(name, sd, x, cot, "cpu", torch.float64, backend="torch")
    want_grads = {n: p.grad.numpy() for n, p in ref.named_parameters() if n in GRADS}
    err = {}
    for cf in ("hip", "torch"):
        net, heads = _step(name, sd, x, cot, dev, amp="bf16", conv_forward=cf)
        assert all(h.dtype == torch.float32 and torch.isfinite(h).all() for h in heads), cf
        assert all(p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all() for p in net.parameters()), cf
        assert list(net.state_dict()) == list(sd)
        assert all(v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, v in net.state_dict().items())
        params = dict(net.named_parameters())
        err[cf] = {k: N.rel_max(h.cpu().numpy(), w.numpy()) for k, h, w in zip(N.HEAD_KEYS, heads, want_heads)}
        err[cf].update({n: N.rel_max(params[n].grad.cpu().numpy(), want_grads[n]) for n in GRADS})
    failed = []
    for k in err["hip"]:
        bound = max(2 * err["torch"][k], UNIT)
        print("%-14s %-40s conv_forward hip %.3g  torch %.3g  ratio %.2f  bound %.3g"
              % (name, k, err["hip"][k], err["torch"][k], err["hip"][k] / max(err["torch"][k], 1e-30), bound))
        if not err["hip"][k] <= bound:
            failed.append((k, err["hip"][k], err["torch"][k]))
    assert not failed, failed


def test_frozen_backbone_is_52_fused_launches(dev, fixture, monkeypatch):
    """frozen_stages=6: the 52 backbone layers are om_conv2d_bf16_frozen_forward launches, every other convolution
    om_conv2d_bf16_forward; the frozen buffers and weights are untouched by a step; the heads are float32."""
    sd, x, cot = fixture
    net = _build("OrienMaskYOLOFPNPlus", sd, dev, frozen_stages=6, **HIPCONV).train()
    calls = []
    launch = omlib.launch
    monkeypatch.setattr(omlib, "launch", lambda name, *a, **k: (calls.append(name), launch(name, *a, **k))[1])
    heads = T.step(net, x.to(dev), [c.to(dev) for c in cot])
    torch.cuda.synchronize(dev)
    assert calls.count("om_conv2d_bf16_frozen_forward") == 52
    assert calls.count("om_conv2d_bf16_forward") == 90 - 52
    assert all(h.dtype == torch.float32 and torch.isfinite(h).all() for h in heads)
    frozen = [k for k in sd if k.startswith("backbone.")]
    assert len(frozen) == 52 * 6 and all(torch.equal(net.state_dict()[k].cpu(), sd[k]) for k in frozen)
    for n, p in net.named_parameters():
        assert (p.grad is None) == n.startswith("backbone."), n


@pytest.mark.parametrize("name", list(MODELS))
def test_forwards_repeat_their_bits_without_the_deterministic_flag(dev, fixture, name):
    """Two eval-mode forwards, and two training-mode forwards from the same state: bit-identical heads with cudnn.deterministic
    off (every kernel of the forward is this package's).  Not asserted of the gradients, which are torch's."""
    sd0, x, _ = fixture
    sd = _weights(name, sd0)
    assert not torch.backends.cudnn.deterministic
    xd = x.to(dev)
    net = _build(name, sd, dev, route_backend="hip", **HIPCONV).eval()
    with torch.no_grad():
        a = [t for pair in net(xd) for t in pair]
        b = [t for pair in net(xd) for t in pair]
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in a)
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
    runs = []
    for _ in range(2):
        net = _build(name, sd, dev, route_backend="hip", **HIPCONV).train()
        runs.append([t.detach() for pair in net(xd) for t in pair])
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(*runs))


def test_one_trainer_step_and_the_checkpoint_moves(dev):
    """tests/train_step.py's step (build_train_model -> the HIP loss -> backward -> the HIP SGD step) with amp='bf16',
    conv_forward='hip', frozen_stages=2: finite loss, every trainable parameter moves, the frozen ones do not.  The checkpoint then
    loads strictly into an amp=None model and into orienmask_amd.model."""
    h = w = 96
    target = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.synth_targets(51, 2, h, w, 6))
    x = synth.synth_image_batch(8, 2, h, w).to(dev)
    torch.manual_seed(3)
    with torch.cuda.device(dev):
        net = builder.build_train_model(dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None,
                                             freeze_backbone=False, backbone_batchnorm_eval=False, frozen_stages=2, **HIPCONV))
    assert net.amp == "bf16" and net.conv_forward == "hip" and net.conv_backend == "torch"
    loss_fn = builder.build(T.loss_cfg(h, w), train)
    optimizer = builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), 1, net)
    assert type(optimizer) is O.SGD
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    out = net(x)
    assert all(t.dtype == torch.float32 for pair in out for t in pair)
    loss, _, _ = loss_fn(out, target, training=True)
    assert torch.isfinite(loss)
    loss.backward()
    optimizer.step()
    torch.cuda.synchronize(dev)
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all() and not torch.equal(p.detach(), before[n]), n
        else:
            assert p.grad is None and torch.equal(p.detach(), before[n]), n
    sd = net.state_dict()
    plain = train.OrienMaskYOLOFPNPlus(3, 80)
    plain.load_state_dict(sd, strict=True)
    assert all(a.dtype == b.dtype and torch.equal(a, b.cpu()) for a, b in zip(plain.state_dict().values(), sd.values()))
    infer_model.OrienMaskYOLOFPNPlus(3, 80).load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
