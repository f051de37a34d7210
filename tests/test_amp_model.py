"""GPU tests of the training model under amp='bf16' (orienmask_amd.train.OrienMaskYOLOFPNPlus at 2 x 3 x 96 x 96).

Truth is the same model with the same weights in float64 on the CPU (backend 'torch', no amp).  The yardstick is the project's
(tests/test_bn_act.py): the comparator is the amp model with backend 'torch' on the same GPU -- the same torch bf16 convolutions,
torch's own bf16 batch_norm + leaky_relu between them -- and the 'hip' model's maximum error over a tensor's scale may be at most
TWICE the comparator's, with a floor at the bf16 unit 2^-8.  Judged: the six heads, and the gradients of backbone.conv1's and of
the last neck block's convolution weight after one backward of a loss that is linear in the heads (the seeded cotangents of the
train_step fixtures, so that the float64 CPU model can take the same backward).  'hip' rounds once per block where torch rounds
after batch_norm, after leaky_relu and after the residual add, so it is expected below the comparator."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, fixture_weights_and_input
import bn_act_np as N
import train_step as T
from orienmask_amd import optim as O
from orienmask_amd import lib as omlib, train

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -8
GRADS = ("backbone.conv1.conv_block.0.weight", "neck4.4.conv_block.0.weight")


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


def _step(sd, x, cot, device, dtype=None, **kw):
    net = train.OrienMaskYOLOFPNPlus(3, 80, **kw)
    net.load_state_dict(sd, strict=True)
    net = net.to(device).train()
    if dtype is not None:
        net, x, cot = net.to(dtype), x.to(dtype), [c.to(dtype) for c in cot]
    heads = [t.detach() for t in T.step(net, x.to(device), [c.to(device) for c in cot])]
    return net, heads


@pytest.fixture(scope="module")
def truth(fixture):
    """The float64 CPU model's heads and gradients: computed once, never modified."""
    sd, x, cot = fixture
    net, heads = _step(sd, x, cot, "cpu", torch.float64, backend="torch")
    grads = {n: p.grad.numpy() for n, p in net.named_parameters() if n in GRADS}
    return [h.numpy() for h in heads], grads


def test_amp_model_against_float64_and_the_torch_comparator(dev, fixture, truth):
    sd, x, cot = fixture
    want_heads, want_grads = truth
    err, nets = {}, {}
    for backend in ("hip", "torch"):
        net, heads = _step(sd, x, cot, dev, backend=backend, amp="bf16")
        nets[backend] = net
        assert all(h.dtype == torch.float32 and torch.isfinite(h).all() for h in heads), backend
        assert all(p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all() for p in net.parameters()), backend
        assert all(v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32)
                   for k, v in net.state_dict().items()), backend
        assert all(int(v) == int(sd[k]) + 1 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")), backend
        params = dict(net.named_parameters())
        err[backend] = {k: N.rel_max(h.cpu().numpy(), w) for k, h, w in zip(N.HEAD_KEYS, heads, want_heads)}
        err[backend].update({n: N.rel_max(params[n].grad.cpu().numpy(), want_grads[n]) for n in GRADS})
    failed = []
    for k in err["hip"]:
        bound = max(2 * err["torch"][k], UNIT)
        print("%-40s hip %.3g  torch %.3g  ratio %.2f  bound %.3g" % (k, err["hip"][k], err["torch"][k],
                                                                     err["hip"][k] / max(err["torch"][k], 1e-30), bound))
        if not err["hip"][k] <= bound:
            failed.append((k, err["hip"][k], err["torch"][k]))
    assert not failed, failed
    # the running statistics stay float32 values of the float64 model's, at bf16 activations' accuracy
    for key in ("backbone.conv1.conv_block.1.running_mean", "neck4.4.conv_block.1.running_var"):
        a, b = nets["hip"].state_dict()[key], nets["torch"].state_dict()[key]
        assert a.dtype == torch.float32 and torch.isfinite(a).all() and not torch.equal(a, sd[key].to(dev)) and b.dtype == torch.float32


def test_two_eval_forwards_give_the_same_bits(dev, fixture):
    """The model's own kernels repeat their bits unconditionally (tests/test_bn_act_bf16.py, tests/test_route_bf16.py); torch's
    convolutions are asked for theirs the way the project's other bit-repeat tests ask, with cudnn.flags(deterministic=True).  A
    difference is reported with the first block whose output differed on an identical input."""
    sd, x, _ = fixture
    net = train.OrienMaskYOLOFPNPlus(3, 80, amp="bf16")
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    seen = {}
    for name, m in net.named_modules():
        if isinstance(m, train.ConvBNLeaky):
            m.register_forward_hook(lambda mod, inp, out, name=name: seen.setdefault(name, []).append((inp[0], out)))
    with torch.no_grad(), torch.backends.cudnn.flags(deterministic=True):
        a = [t for pair in net(x.to(dev)) for t in pair]
        b = [t for pair in net(x.to(dev)) for t in pair]
    assert all(t.dtype == torch.float32 for t in a)
    cause = [n for n, ((x0, y0), (x1, y1)) in seen.items() if torch.equal(x0, x1) and not torch.equal(y0, y1)]
    assert all(torch.equal(p.contiguous().view(torch.int32), q.contiguous().view(torch.int32)) for p, q in zip(a, b)), cause[:3]
    assert not cause, cause[:3]
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in net.state_dict().items())          # eval mode changes no buffer


def test_block_saves_bf16_and_refuses_a_residual_of_the_other_type(dev):
    torch.manual_seed(4)
    blk = train.ConvBNLeaky(8, 16, 3, padding=1, amp="bf16").to(dev).train()
    x = torch.randn(2, 8, 12, 12, device=dev, requires_grad=True)
    y = blk(x)
    assert y.dtype == torch.bfloat16 and y.grad_fn is not None
    saved = [t for t in y.grad_fn.saved_tensors if t.dim() == 4]
    assert saved and all(t.dtype == torch.bfloat16 for t in saved)             # the saved convolution output is bf16
    res = torch.randn_like(y)
    assert blk(x, residual=res).dtype == torch.bfloat16
    with pytest.raises(omlib.OrienMaskHipError, match="residual"):
        blk(x, residual=res.float())
    plain = train.ConvBNLeaky(8, 16, 3, padding=1).to(dev).train()
    with pytest.raises(omlib.OrienMaskHipError, match="residual"):
        plain(x, residual=res)
    y.float().sum().backward()
    assert x.grad.dtype == torch.float32 and all(p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all() for p in blk.parameters())


def test_one_trainer_step_with_hip_routes_and_hip_sgd(dev):
    """build_train_model(amp, route_backend 'hip') -> the HIP loss -> backward -> the HIP SGD step: finite, every parameter moves."""
    seen = []
    _, _, net = T.trainer_steps(dev, dict(amp="bf16", route_backend="hip"), 1,
                                on_output=lambda out: seen.extend(t.dtype for pair in out for t in pair))
    assert net.amp == "bf16" and net.route_backend == "hip" and seen == [torch.float32] * 6
    assert all(p.dtype == torch.float32 for p in net.parameters())


def test_one_step_with_frozen_stages(dev, fixture):
    sd, x, cot = fixture
    net = train.OrienMaskYOLOFPNPlus(3, 80, amp="bf16", frozen_stages=2)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    opt = O.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=5e-4)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    heads = T.step(net, x.to(dev), [c.to(dev) for c in cot])
    opt.step()
    torch.cuda.synchronize(dev)
    assert all(h.dtype == torch.float32 and torch.isfinite(h).all() for h in heads)
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), n
            assert not torch.equal(p.detach(), before[n]), n
        else:
            assert p.grad is None and torch.equal(p.detach(), before[n]), n
    frozen = [k for k in sd if k.startswith(("backbone.conv1.", "backbone.conv2."))]
    assert frozen and all(torch.equal(net.state_dict()[k].cpu(), sd[k]) for k in frozen)   # buffers and counters included


def test_checkpoints_move_between_amp_and_float32(dev, fixture):
    sd, x, cot = fixture
    amp, _ = _step(sd, x, cot, dev, amp="bf16")
    plain = train.OrienMaskYOLOFPNPlus(3, 80).to(dev)
    plain.load_state_dict(amp.state_dict(), strict=True)
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(plain.state_dict().values(), amp.state_dict().values()))
    back = train.OrienMaskYOLOFPNPlus(3, 80, amp="bf16").to(dev)
    back.load_state_dict(plain.state_dict(), strict=True)
    assert list(back.state_dict()) == list(sd)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), amp.state_dict().values()))
