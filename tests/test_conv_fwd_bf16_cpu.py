"""Without a GPU: the C-ABI surface of the bf16 forward convolution (om_conv2d_bf16_forward, om_conv2d_bf16_frozen_forward,
csrc/conv_fwd_bf16.hip), the option combination amp='bf16' + conv_forward='hip' on the block and both models, conv2d_bf16's
refusal of CPU tensors, its backward function against autocast's own gradients on CPU tensors, and the plumbing through
builder.build_train_model and tools/train.py.  No GPU compute."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO
from orienmask_amd import builder, lib as omlib, train

OM_EINVAL = -1


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entries_are_declared_bound_exported_and_refuse_by_name(built):
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    L = omlib.load()
    for name in ("om_conv2d_bf16_forward", "om_conv2d_bf16_frozen_forward"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in omlib.SIGNATURES and hasattr(L, name) and not name.endswith("_bf16")
    assert len(omlib.SIGNATURES["om_conv2d_bf16_forward"][1]) == 13 and len(omlib.SIGNATURES["om_conv2d_bf16_frozen_forward"][1]) == 18
    p = 4096            # never dereferenced: every call below is refused on the host
    shape = (2, 4, 6, 6, 8)
    assert L.om_conv2d_bf16_forward(None, p, None, *shape, 3, 1, p, 0, None) == OM_EINVAL
    assert b"om_conv2d_bf16_forward" in L.om_last_error() and b"null" in L.om_last_error()
    assert L.om_conv2d_bf16_forward(p, None, None, *shape, 3, 1, p, 1, None) == OM_EINVAL
    assert L.om_conv2d_bf16_forward(p, p, None, *shape, 3, 1, None, 1, None) == OM_EINVAL
    assert L.om_conv2d_bf16_forward(p, p, None, *shape, 5, 1, p + 8192, 0, None) == OM_EINVAL
    assert b"om_conv2d_bf16_forward" in L.om_last_error() and b"ksize 5" in L.om_last_error()
    stats = (p, p, p, p)
    assert L.om_conv2d_bf16_frozen_forward(None, p, *shape, 3, 1, *stats, 1e-5, 0.1, None, p, None) == OM_EINVAL
    assert b"om_conv2d_bf16_frozen_forward" in L.om_last_error() and b"null" in L.om_last_error()
    assert L.om_conv2d_bf16_frozen_forward(p, p, *shape, 3, 1, p, p, p, None, 1e-5, 0.1, None, 2 * p, None) == OM_EINVAL
    assert L.om_conv2d_bf16_frozen_forward(p, p, *shape, 5, 1, *stats, 1e-5, 0.1, None, 2 * p, None) == OM_EINVAL
    assert b"om_conv2d_bf16_frozen_forward" in L.om_last_error() and b"ksize 5" in L.om_last_error()
    assert L.om_conv2d_bf16_frozen_forward(p, p, *shape, 3, 1, *stats, 0.0, 0.1, None, 2 * p, None) == OM_EINVAL
    assert b"om_conv2d_bf16_frozen_forward" in L.om_last_error() and b"eps" in L.om_last_error()
    for alias in (dict(x=2 * p), dict(w=2 * p), dict(res=2 * p)):
        a = dict(x=p, w=3 * p, res=None, **{})
        a.update(alias)
        assert L.om_conv2d_bf16_frozen_forward(a["x"], a["w"], *shape, 3, 1, *stats, 1e-5, 0.1, a["res"], 2 * p, None) == OM_EINVAL
        assert b"om_conv2d_bf16_frozen_forward" in L.om_last_error() and b"alias" in L.om_last_error()


# ---------------------------------------------------------------------------------------------------------------- the option
def test_block_and_models_construct_with_amp_and_the_hip_forward():
    """amp='bf16' with conv_forward='hip' and conv_backend='torch' is a legal combination; the module tree and the state-dict keys
    are the reference's."""
    blk = train.ConvBNLeaky(4, 8, 1, amp="bf16", conv_forward="hip")
    assert blk.amp == "bf16" and blk.conv_forward == "hip" and blk.conv_backend == "torch"
    assert [n for n, _ in blk.named_parameters()] == ["conv_block.0.weight", "conv_block.1.weight", "conv_block.1.bias"]
    keys = np.load(os.path.join(GOLDEN, "model_keys.npz"))
    for cls in (train.OrienMaskYOLOFPNPlus, train.OrienMaskYOLO):
        net = cls(3, 80, amp="bf16", conv_forward="hip", frozen_stages=2)
        assert net.amp == "bf16" and net.conv_forward == "hip" and net.conv_backend == "torch"
        blocks = [m for m in net.modules() if isinstance(m, train.ConvBNLeaky)]
        assert all(m.amp == "bf16" and m.conv_forward == "hip" for m in blocks)
        sd = net.state_dict()
        assert list(sd) == [str(k) for k in keys[cls.__name__ + "_state_dict"]]
        assert all(v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())


def test_what_stays_refused():
    for kw in (dict(conv_backend="hip"), dict(conv_backend="hip", conv_forward="hip")):
        with pytest.raises(ValueError, match="amp"):
            train.ConvBNLeaky(4, 8, 1, amp="bf16", **kw)
        with pytest.raises(ValueError, match="amp"):
            train.OrienMaskYOLO(3, 80, amp="bf16", **kw)
    with pytest.raises(ValueError, match="conv_forward 'torch'.*conv_forward 'hip'"):     # the message names what is available
        train.ConvBNLeaky(4, 8, 1, amp="bf16", conv_backend="hip")
    with pytest.raises(ValueError, match="conv_backend"):                                 # without amp: as before
        train.ConvBNLeaky(4, 8, 1, conv_forward="hip")
    with pytest.raises(ValueError, match="conv_backend"):
        train.OrienMaskYOLOFPNPlus(3, 80, conv_forward="hip")


def test_cpu_tensors_are_refused(built):
    x = torch.randn(2, 4, 5, 5).to(torch.bfloat16)
    w = torch.randn(8, 4, 3, 3)
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.conv2d_bf16(x, w, None, 1, 1)
    with pytest.raises(omlib.OrienMaskHipError, match="CPU|MI355X"):
        train.ConvBNLeaky(4, 8, 3, padding=1, amp="bf16", conv_forward="hip")(x.float())
    with pytest.raises(omlib.OrienMaskHipError, match="CPU|MI355X"):
        train.ConvBNLeaky(4, 8, 3, padding=1, amp="bf16", conv_forward="hip", frozen=True)(x.float())
    assert "conv2d_bf16" in train.__all__


# ---------------------------------------------------------------------------------------------------------------- the backward
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("ks,stride", [(1, 1), (3, 1), (3, 2)], ids=["1x1", "3x3", "3x3s2"])
def test_backward_function_equals_autocast_gradients(ks, stride, bias):
    """conv2d_bf16_backward on CPU tensors: bit-equal to what F.conv2d under torch.autocast('cpu', bfloat16) leaves in .grad for a
    bf16 x, a float32 master weight and bias; gradients that were not asked for are None."""
    torch.manual_seed(ks * 10 + stride)
    x = torch.randn(2, 5, 7, 6).to(torch.bfloat16).requires_grad_(True)
    w = torch.randn(4, 5, ks, ks, requires_grad=True)
    b = torch.randn(4, requires_grad=True) if bias else None
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y = F.conv2d(x, w, b, stride, ks // 2)
    assert y.dtype == torch.bfloat16
    dy = torch.randn(y.shape).to(torch.bfloat16)
    y.backward(dy)
    dx, dw, db = train.conv2d_bf16_backward(dy, x.detach(), w.detach(), stride, ks // 2, bias, (True, True, True))
    assert dx.dtype == torch.bfloat16 and torch.equal(dx, x.grad)
    assert dw.dtype == torch.float32 and torch.equal(dw, w.grad)
    if bias:
        assert db.dtype == torch.float32 and torch.equal(db, b.grad)
    else:
        assert db is None
    for needs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, False, False)):
        got = train.conv2d_bf16_backward(dy, x.detach(), w.detach(), stride, ks // 2, bias, needs)
        want = (x.grad, w.grad, b.grad if bias else None)
        for g, t, need in zip(got, want, (needs[0], needs[1], needs[2] and bias)):
            assert (g is None) == (not need), (needs, bias)
            if need:
                assert torch.equal(g, t), needs


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_build_train_model_passes_conv_forward_through(monkeypatch):
    """The builder hands the config's keys to the model class (the move to the current device is taken out: no GPU here)."""
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    cfg = dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False,
               backbone_batchnorm_eval=False, amp="bf16", conv_forward="hip")
    net = builder.build_train_model(cfg)
    assert net.amp == "bf16" and net.conv_forward == "hip" and net.conv_backend == "torch" and cfg["conv_forward"] == "hip"
    assert builder.build_train_model(dict(cfg, conv_forward="torch")).conv_forward == "torch"
    with pytest.raises(ValueError, match="amp"):
        builder.build_train_model(dict(cfg, conv_backend="hip"))
    del cfg["amp"]
    with pytest.raises(ValueError, match="conv_backend"):
        builder.build_train_model(cfg)


def test_train_tool_carries_conv_forward_into_the_model_config():
    spec = importlib.util.spec_from_file_location("om_tools_train", os.path.join(REPO, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    config = dict(model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80), seed=1)
    args = tool.parse_args(["--config", "c.json", "--amp", "bf16", "--conv-forward", "hip", "--frozen-stages", "6"])
    out = tool.apply_overrides(config, args)
    assert out["model"] == dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, amp="bf16", conv_forward="hip",
                                frozen_stages=6)
    assert "conv_forward" not in config["model"]                           # the caller's dict is not mutated
    assert tool.apply_overrides(config, tool.parse_args(["--config", "c.json"])) is config
    assert tool.apply_overrides(config, tool.parse_args(["--config", "c.json", "--conv-forward", "torch"]))["model"]["conv_forward"] == "torch"
    with pytest.raises(SystemExit):
        tool.parse_args(["--config", "c.json", "--conv-forward", "miopen"])
