"""Without a GPU: the C-ABI surface of the bf16 convolution gradients (om_conv2d_bf16_grad_workspace_bytes, om_conv2d_bf16_grad_input,
om_conv2d_bf16_grad_weight; csrc/conv_grad_bf16.hip, csrc/conv_dw.hip), the option conv_grad='hip' on the block, both models, the builder and
tools/train.py, conv2d_bf16_backward's 'torch' backend against its default, and the test helper's truth against torch.autograd in
float64.  No GPU compute."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_bf16_np as C
from conftest import GOLDEN, REPO
from orienmask_amd import builder, lib as omlib, train

OM_EINVAL = -1
ENTRIES = ("om_conv2d_bf16_grad_workspace_bytes", "om_conv2d_bf16_grad_input", "om_conv2d_bf16_grad_weight")
HIPGRAD = dict(amp="bf16", conv_forward="hip", conv_grad="hip")


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entries_are_declared_bound_and_exported(built):
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    L = omlib.load()
    for name in ENTRIES:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert name in omlib.SIGNATURES and hasattr(L, name) and not name.endswith("_bf16")
    assert [len(omlib.SIGNATURES[n][1]) for n in ENTRIES] == [7, 14, 14]


def test_entries_refuse_by_name(built):
    L = omlib.load()
    p = 4096            # never dereferenced: every call below is refused on the host
    shape = (2, 4, 6, 6, 8)
    for args in ((None, p, *shape, 3, 1, 2 * p), (p, None, *shape, 3, 1, 2 * p), (p, p, *shape, 3, 1, None)):
        assert L.om_conv2d_bf16_grad_input(*args, 0, None, 0, None) == OM_EINVAL
        assert b"om_conv2d_bf16_grad_input" in L.om_last_error() and b"null" in L.om_last_error()
    assert L.om_conv2d_bf16_grad_input(p, 3 * p, *shape, 5, 1, 2 * p, 1, None, 0, None) == OM_EINVAL
    assert b"om_conv2d_bf16_grad_input" in L.om_last_error() and b"ksize 5" in L.om_last_error()
    assert L.om_conv2d_bf16_grad_input(p, 3 * p, *shape, 3, 1, p, 0, None, 0, None) == OM_EINVAL      # dx aliasing dy
    assert b"om_conv2d_bf16_grad_input" in L.om_last_error() and b"alias" in L.om_last_error()
    for args in ((None, p, *shape, 3, 1, p, None), (p, None, *shape, 3, 1, p, None), (p, p, *shape, 3, 1, None, None)):
        assert L.om_conv2d_bf16_grad_weight(*args, None, 0, None) == OM_EINVAL
        assert b"om_conv2d_bf16_grad_weight" in L.om_last_error() and b"null" in L.om_last_error()
    assert L.om_conv2d_bf16_grad_weight(p, p, *shape, 5, 1, p, None, None, 0, None) == OM_EINVAL
    assert b"om_conv2d_bf16_grad_weight" in L.om_last_error() and b"ksize 5" in L.om_last_error()
    assert L.om_conv2d_bf16_grad_workspace_bytes(*shape, 5, 1) == 0


# ---------------------------------------------------------------------------------------------------------------- the option
def test_block_and_models_construct_with_the_hip_gradients(monkeypatch):
    blk = train.ConvBNLeaky(4, 8, 1, **HIPGRAD)
    assert blk.conv_grad == "hip" and blk.conv_backend == "torch"
    assert train.ConvBNLeaky(4, 8, 1).conv_grad == "torch"
    assert [n for n, _ in blk.named_parameters()] == ["conv_block.0.weight", "conv_block.1.weight", "conv_block.1.bias"]
    keys = np.load(os.path.join(GOLDEN, "model_keys.npz"))
    for cls in (train.OrienMaskYOLOFPNPlus, train.OrienMaskYOLO):
        net = cls(3, 80, frozen_stages=2, **HIPGRAD)
        assert net.conv_grad == "hip" and net.amp == "bf16" and net.conv_forward == "hip" and net.conv_backend == "torch"
        assert all(m.conv_grad == "hip" for m in net.modules() if isinstance(m, train.ConvBNLeaky))
        sd = net.state_dict()
        assert list(sd) == [str(k) for k in keys[cls.__name__ + "_state_dict"]]
        assert all(v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
        assert cls(3, 80).conv_grad == "torch"
    # and through the builder (the move to the current device is taken out: no GPU here)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    cfg = dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False,
               backbone_batchnorm_eval=False, **HIPGRAD)
    net = builder.build_train_model(cfg)
    assert net.conv_grad == "hip" and cfg["conv_grad"] == "hip"
    assert list(net.state_dict()) == [str(k) for k in keys["OrienMaskYOLOFPNPlus_state_dict"]]
    with pytest.raises(ValueError, match="conv_grad"):
        builder.build_train_model(dict(cfg, amp=None, conv_forward="torch"))


def test_what_conv_grad_refuses():
    for make in (lambda **kw: train.ConvBNLeaky(4, 8, 1, **kw), lambda **kw: train.OrienMaskYOLO(3, 80, **kw),
                 lambda **kw: train.OrienMaskYOLOFPNPlus(3, 80, **kw)):
        with pytest.raises(ValueError, match="conv_grad 'hip'.*amp 'bf16'.*conv_forward 'hip'.*conv_backend 'torch'"):
            make(conv_grad="hip")                                                  # without amp
        with pytest.raises(ValueError, match="conv_grad 'hip'"):
            make(conv_grad="hip", conv_backend="hip", conv_forward="hip")          # the float32 kernels
        with pytest.raises(ValueError, match="conv_grad 'hip'"):
            make(conv_grad="hip", amp="bf16", conv_forward="torch")
        with pytest.raises(ValueError):
            make(conv_grad="hip", amp="bf16", conv_forward="hip", conv_backend="hip")
        with pytest.raises(ValueError, match="conv_grad must be one of"):
            make(conv_grad="miopen", amp="bf16", conv_forward="hip")
    with pytest.raises(ValueError, match="conv_forward 'torch'.*conv_forward 'hip'"):      # amp with conv_backend 'hip': as before
        train.ConvBNLeaky(4, 8, 1, amp="bf16", conv_backend="hip")


def test_train_tool_carries_conv_grad_into_the_model_config():
    spec = importlib.util.spec_from_file_location("om_tools_train", os.path.join(REPO, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    config = dict(model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80), seed=1)
    args = tool.parse_args(["--config", "c.json", "--amp", "bf16", "--conv-forward", "hip", "--conv-grad", "hip"])
    assert tool.apply_overrides(config, args)["model"] == dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, **HIPGRAD)
    assert "conv_grad" not in config["model"]
    assert tool.apply_overrides(config, tool.parse_args(["--config", "c.json"])) is config
    with pytest.raises(SystemExit):
        tool.parse_args(["--config", "c.json", "--conv-grad", "miopen"])


# ---------------------------------------------------------------------------------------------------------------- the backward
@pytest.mark.parametrize("ks,stride", [(1, 1), (3, 1), (3, 2)], ids=["1x1", "3x3", "3x3s2"])
def test_torch_backend_is_the_default_call(ks, stride):
    torch.manual_seed(ks * 10 + stride)
    x = torch.randn(2, 5, 7, 6).to(torch.bfloat16)
    w = torch.randn(4, 5, ks, ks)
    dy = torch.randn(2, 4, *C.G.out_hw(7, 6, ks, stride)).to(torch.bfloat16)
    a = train.conv2d_bf16_backward(dy, x, w, stride, ks // 2, True, (True, True, True))
    b = train.conv2d_bf16_backward(dy, x, w, stride, ks // 2, True, (True, True, True), backend="torch")
    assert [t.dtype for t in b] == [torch.bfloat16, torch.float32, torch.float32]
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    with pytest.raises(ValueError, match="backend"):
        train.conv2d_bf16_backward(dy, x, w, stride, ks // 2, True, (True, True, True), backend="miopen")
    with pytest.raises(omlib.OrienMaskHipError):           # 'hip' takes no CPU tensors: there is no fallback
        train.conv2d_bf16_backward(dy, x, w, stride, ks // 2, True, (True, True, True), backend="hip")
    with pytest.raises(ValueError, match="backward"):
        train.conv2d_bf16(x, w, None, stride, ks // 2, backward="miopen")


# ---------------------------------------------------------------------------------------------------------------- the helper
@pytest.mark.parametrize("ks,stride", [(1, 1), (3, 1), (3, 2)], ids=["1x1", "3x3", "3x3s2"])
def test_helper_truth_is_autograd_of_conv2d_in_float64(ks, stride):
    d = C.inputs(2, 5, 7, ks, stride, 9, 8, seed=ks + stride)
    assert np.array_equal(C.Q.quantise(d["x"]), d["x"]) and np.array_equal(C.Q.quantise(d["dy"]), d["dy"])
    o = C.operands(d)
    assert not np.array_equal(o["w"], d["w"]) and np.array_equal(C.Q.quantise(o["w"]), o["w"])
    x = torch.from_numpy(o["x"]).double().requires_grad_(True)
    w = torch.from_numpy(o["w"]).double().requires_grad_(True)
    b = torch.zeros(7, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, stride, ks // 2)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), torch.from_numpy(o["dy"]).double())
    t, S = C.truth(d), C.scale(d)
    for got, want in ((t["dx"], gx), (t["dw"], gw), (t["db"], gb)):
        assert got.dtype == np.float64 and np.allclose(got, want.numpy(), rtol=1e-12, atol=1e-12)
    assert all((S[k] >= np.abs(t[k]) * (1 - 1e-12)).all() for k in t)
    assert C.k_of(d, "dx") == 7 * ks * ks and C.k_of(d, "dw") == 2 * d["dy"].shape[2] * d["dy"].shape[3]
    i = C.integer_inputs(2, 5, 7, ks, stride, 9, 8, seed=3)
    assert all(np.abs(i[k]).max() <= 4 and np.array_equal(np.round(i[k]), i[k]) for k in ("x", "dy", "w"))
