"""The conv_backend argument of the training models (orienmask_amd/train.py), without a GPU: it is accepted and checked, changes
nothing about the module tree, has no CPU fallback, and with 'torch' (the default) leaves the model's arithmetic as it was."""
import re

import pytest
import torch

import train_step as T
from orienmask_amd import lib as omlib, train


def test_conv_backend_is_accepted_and_defaults_to_torch():
    assert train.ConvBNLeaky(4, 8, 3, padding=1).conv_backend == "torch"
    assert train.ConvBNLeaky(4, 8, 3, padding=1, conv_backend="hip").conv_backend == "hip"
    for net in T.models():
        assert net.conv_backend == "torch"
        assert all(m.conv_backend == "torch" for m in net.modules() if isinstance(m, train.ConvBNLeaky))
    for net in T.models(conv_backend="hip"):
        assert net.conv_backend == "hip" and net.backend == "hip"
        blocks = [m for m in net.modules() if isinstance(m, train.ConvBNLeaky)]
        assert len(blocks) in (83, 86) and all(m.conv_backend == "hip" for m in blocks)


def test_unknown_conv_backend_is_refused():
    with pytest.raises(ValueError, match="conv_backend"):
        train.ConvBNLeaky(4, 8, 1, conv_backend="bogus")
    for cls in (train.OrienMaskYOLOFPNPlus, train.OrienMaskYOLO):
        with pytest.raises(ValueError, match="conv_backend"):
            cls(3, 80, conv_backend="bogus")


def test_hip_conv_backend_leaves_the_module_tree_alone():
    for a, b in zip(T.models(conv_backend="hip"), T.models()):
        assert list(a.state_dict().keys()) == list(b.state_dict().keys())
        assert [(n, tuple(p.shape)) for n, p in a.named_parameters()] == [(n, tuple(p.shape)) for n, p in b.named_parameters()]
        assert [(n, type(m)) for n, m in a.named_modules()] == [(n, type(m)) for n, m in b.named_modules()]
        heads = [m for n, m in a.named_modules() if re.fullmatch(r"bbox_head\d+\.1|orien_head\.5", n)]
        assert len(heads) == 4 and all(type(m) is torch.nn.Conv2d for m in heads)


def test_hip_conv_backend_has_no_cpu_fallback():
    x = torch.zeros(2, 3, 32, 32)
    for net in T.models(conv_backend="hip") + T.models(conv_backend="hip", backend="torch"):
        with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
            net(x)
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.ConvBNLeaky(3, 8, 3, padding=1, backend="torch", conv_backend="hip")(x)
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.conv2d(x, torch.zeros(8, 3, 3, 3), None, 1, 1)


def test_torch_conv_backend_is_the_model_without_the_argument():
    """The same seed, the same CPU input: forward and every gradient bit for bit."""
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    runs = []
    for kw in (dict(), dict(conv_backend="torch")):
        torch.manual_seed(11)
        net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch", **kw).train()
        heads = [t for pair in net(x) for t in pair]
        torch.autograd.backward(heads, [torch.ones_like(t) for t in heads])
        runs.append(([t.detach() for t in heads], [p.grad for p in net.parameters()]))
    (ha, ga), (hb, gb) = runs
    assert all(torch.equal(a, b) for a, b in zip(ha, hb))
    assert all(a is not None and torch.equal(a, b) for a, b in zip(ga, gb))
