"""The conv_forward argument of the training models and the forward argument of train.conv2d (orienmask_amd/train.py), without a
GPU: accepted and checked, tied to conv_backend 'hip', no change to the module tree, no CPU fallback, and with 'torch' (the
default) the model's arithmetic as it was."""
import os
import re

import pytest
import torch

import train_step as T
from orienmask_amd import builder, lib as omlib, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_forward_is_accepted_and_defaults_to_torch():
    assert train.CONV_FORWARDS == ("torch", "hip")
    assert train.ConvBNLeaky(4, 8, 3, padding=1).conv_forward == "torch"
    assert train.ConvBNLeaky(4, 8, 3, padding=1, conv_backend="hip").conv_forward == "torch"
    assert train.ConvBNLeaky(4, 8, 3, padding=1, conv_backend="hip", conv_forward="hip").conv_forward == "hip"
    for net in T.models() + T.models(conv_backend="hip"):
        assert net.conv_forward == "torch"
        assert all(m.conv_forward == "torch" for m in net.modules() if isinstance(m, train.ConvBNLeaky))
    for net in T.models(conv_backend="hip", conv_forward="hip"):
        assert net.conv_forward == "hip" and net.conv_backend == "hip"
        blocks = [m for m in net.modules() if isinstance(m, train.ConvBNLeaky)]
        assert len(blocks) in (83, 86) and all(m.conv_forward == "hip" and m.conv_backend == "hip" for m in blocks)


def test_unknown_conv_forward_is_refused():
    with pytest.raises(ValueError, match="conv_forward"):
        train.ConvBNLeaky(4, 8, 1, conv_backend="hip", conv_forward="bogus")
    for cls in (train.OrienMaskYOLOFPNPlus, train.OrienMaskYOLO):
        with pytest.raises(ValueError, match="conv_forward"):
            cls(3, 80, conv_backend="hip", conv_forward="bogus")
    with pytest.raises(ValueError, match="forward"):
        train.conv2d(torch.zeros(1, 3, 4, 4), torch.zeros(8, 3, 3, 3), None, 1, 1, forward="bogus")


def test_hip_forward_needs_hip_gradients():
    """torch's gradient node under the HIP forward is not built: the error names both arguments."""
    for make in (lambda **kw: train.ConvBNLeaky(4, 8, 1, **kw), lambda **kw: train.OrienMaskYOLOFPNPlus(3, 80, **kw),
                 lambda **kw: train.OrienMaskYOLO(3, 80, **kw)):
        for kw in (dict(conv_forward="hip"), dict(conv_backend="torch", conv_forward="hip")):
            with pytest.raises(ValueError, match="conv_forward.*conv_backend"):
                make(**kw)


def test_hip_conv_forward_leaves_the_module_tree_alone():
    for a, b in zip(T.models(conv_backend="hip", conv_forward="hip"), T.models()):
        assert list(a.state_dict().keys()) == list(b.state_dict().keys())
        assert [(n, tuple(p.shape)) for n, p in a.named_parameters()] == [(n, tuple(p.shape)) for n, p in b.named_parameters()]
        assert [(n, type(m)) for n, m in a.named_modules()] == [(n, type(m)) for n, m in b.named_modules()]
        heads = [m for n, m in a.named_modules() if re.fullmatch(r"bbox_head\d+\.1|orien_head\.5", n)]
        assert len(heads) == 4 and all(type(m) is torch.nn.Conv2d for m in heads)


def test_hip_conv_forward_has_no_cpu_fallback():
    x = torch.zeros(2, 3, 32, 32)
    for net in T.models(conv_backend="hip", conv_forward="hip") + T.models(conv_backend="hip", conv_forward="hip", backend="torch"):
        with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
            net(x)
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.ConvBNLeaky(3, 8, 3, padding=1, backend="torch", conv_backend="hip", conv_forward="hip")(x)
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.conv2d(x, torch.zeros(8, 3, 3, 3), None, 1, 1, forward="hip")


def test_convert_sync_batchnorm_keeps_the_attribute():
    net = train.convert_sync_batchnorm(train.OrienMaskYOLO(3, 80, conv_backend="hip", conv_forward="hip"))
    assert net.conv_forward == "hip"
    assert all(m.conv_forward == "hip" and m.sync for m in net.modules() if isinstance(m, train.ConvBNLeaky))


def test_build_train_model_passes_conv_forward_through(monkeypatch):
    """The builder hands the config's keys to the model class (the move to the current device is taken out: no GPU here)."""
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    cfg = dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False,
               backbone_batchnorm_eval=False, conv_backend="hip", conv_forward="hip")
    net = builder.build_train_model(cfg)
    assert net.conv_forward == "hip" and net.conv_backend == "hip"
    assert all(m.conv_forward == "hip" for m in net.modules() if isinstance(m, train.ConvBNLeaky))
    assert cfg["conv_forward"] == "hip" and cfg["type"] == "OrienMaskYOLOFPNPlus"       # the caller's dict is not mutated
    del cfg["conv_forward"]
    assert builder.build_train_model(cfg).conv_forward == "torch"
    with pytest.raises(ValueError, match="conv_forward"):
        builder.build_train_model(dict(cfg, conv_backend="torch", conv_forward="hip"))


def test_torch_conv_forward_is_the_model_without_the_argument():
    """The same seed, the same CPU input: forward and every gradient bit for bit."""
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    runs = []
    for kw in (dict(), dict(conv_forward="torch")):
        torch.manual_seed(11)
        net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch", **kw).train()
        heads = [t for pair in net(x) for t in pair]
        torch.autograd.backward(heads, [torch.ones_like(t) for t in heads])
        runs.append(([t.detach() for t in heads], [p.grad for p in net.parameters()]))
    (ha, ga), (hb, gb) = runs
    assert all(torch.equal(a, b) for a, b in zip(ha, hb))
    assert all(a is not None and torch.equal(a, b) for a, b in zip(ga, gb))


def test_the_header_declares_what_lib_binds():
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    assert re.search(r"int om_conv2d_forward\(const float\* x, const float\* w, const float\* bias, int B, int cin, int H, int W, "
                     r"int cout, int ksize, int stride,\s+float\* y, om_stream stream\);", header)
    assert len(omlib.SIGNATURES["om_conv2d_forward"][1]) == 12
