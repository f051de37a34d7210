"""CPU tests of the training model (orienmask_amd.train: ConvBNLeaky, OrienMaskYOLOFPNPlus, OrienMaskYOLO; builder.build_train_model)
and of the C-ABI surface of csrc/bn_act.hip.  No GPU compute: the 'torch' backend on CPU tensors is held to what the REFERENCE model
produced in training mode (tests/golden/train_step_*.npz, model_keys.npz; tools/gen_golden.py train), and the float64 restatement
the GPU tests use as truth (tests/bn_act_np.py) is held to torch-CPU float64 autograd."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO, fixture_weights_and_input
import bn_act_np as N
from orienmask_amd import builder, lib as omlib, model as infer_model, train

MODELS = ("OrienMaskYOLOFPNPlus", "OrienMaskYOLO")
ENTRIES = ("om_bn_act_workspace_bytes", "om_bn_act_forward", "om_bn_act_backward")


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entries_are_declared_bound_and_exported(built):
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    L = omlib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in omlib.SIGNATURES and hasattr(L, name)
    mk = open(os.path.join(REPO, "orienmask_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*build/bn_act\.o", mk, re.M)          # the ISA audit runs over every object of OBJS
    assert re.search(r"^EXTRA_bn_act = -ffp-contract=off", mk, re.M)  # z is the same expression in forward and backward


def test_null_pointers_and_bad_shapes_are_refused_by_name(built):
    L = omlib.load()
    rc = L.om_bn_act_forward(None, 2, 4, 3, 3, None, None, None, None, None, 1, 0.1, 1e-5, 0.1, None, None, None, None, None, 0, None)
    assert rc != 0 and b"om_bn_act_forward" in L.om_last_error()
    rc = L.om_bn_act_backward(None, None, 2, 4, 3, 3, None, None, None, None, 1, 0.1, None, None, None, None, 0, None)
    assert rc != 0 and b"om_bn_act_backward" in L.om_last_error()
    with pytest.raises(omlib.OrienMaskHipError, match="om_bn_act_forward"):
        omlib.check(L.om_bn_act_forward(None, 2, 4, 3, 3, None, None, None, None, None, 1, 0.1, 1e-5, 0.1, None, None, None, None, None,
                                        0, None), "om_bn_act_forward")
    # one value per channel in training mode: refused before anything is launched (the pointers are never dereferenced on the host)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 128)
    rc = L.om_bn_act_forward(p, 1, 8, 1, 1, p, p, p, p, None, 1, 0.1, 1e-5, 0.1, None, q, p, p, None, 0, None)
    assert rc != 0 and b"more than 1 value per channel" in L.om_last_error()
    rc = L.om_bn_act_forward(p, 2, 8, 1, 1, p, p, p, p, None, 1, 0.1, 1e-5, 0.1, None, p, p, p, None, 0, None)
    assert rc != 0 and b"alias" in L.om_last_error()


def test_workspace_query(built):
    L = omlib.load()
    assert L.om_bn_act_workspace_bytes(0, 8, 4, 4) == 0 and L.om_bn_act_workspace_bytes(2, 0, 4, 4) == 0
    small = L.om_bn_act_workspace_bytes(2, 1024, 3, 3)
    big = L.om_bn_act_workspace_bytes(16, 32, 544, 544)
    assert small == 1024 * 16                       # one (sum, sum) pair of doubles per channel
    assert big % 16 == 0 and 32 * 16 < big <= 2048 * 16      # at most 2048 workgroups write a pair each


# ---------------------------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("name", MODELS)
def test_keys_and_parameter_order_are_the_references(name):
    g = np.load(os.path.join(GOLDEN, "model_keys.npz"))
    net = getattr(train, name)(3, 80, backend="torch")
    inf = getattr(infer_model, name)(3, 80)
    keys = [str(k) for k in g[name + "_state_dict"]]
    params = [str(k) for k in g[name + "_parameters"]]
    assert list(net.state_dict()) == keys == list(inf.state_dict())
    assert [n for n, _ in net.named_parameters()] == params == [n for n, _ in inf.named_parameters()]
    assert all(p.requires_grad for p in net.parameters())
    assert [tuple(p.shape) for p in net.parameters()] == [tuple(p.shape) for p in inf.parameters()]


@pytest.mark.parametrize("name", MODELS)
def test_state_dict_moves_both_ways(name):
    net = getattr(train, name)(3, 80, backend="torch")
    inf = getattr(infer_model, name)(3, 80)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.25)
    inf.load_state_dict(net.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(inf.state_dict().values(), net.state_dict().values()))
    back = getattr(train, name)(3, 80, backend="torch")
    back.load_state_dict(inf.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), net.state_dict().values()))


def test_init_and_train_flags():
    net = train.OrienMaskYOLOFPNPlus(3, 80, backbone_batchnorm_eval=True, backend="torch")
    for n, m in net.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d) and "backbone" not in n:
            assert torch.all(m.weight == 1) and torch.all(m.bias == 0)
    net.train()
    flags = {n: m.training for n, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert not any(v for n, v in flags.items() if n.startswith("backbone.")) and all(v for n, v in flags.items() if not n.startswith("backbone."))
    net.eval()
    assert not any(m.training for m in net.modules())
    plain = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch").train()
    assert all(m.training for m in plain.modules())


def test_pretrained_loads_backbone_relative_keys(tmp_path):
    src = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch")
    sd = {k: v + 0.5 if v.is_floating_point() else v for k, v in src.backbone.state_dict().items()}
    path = str(tmp_path / "darknet.pth")
    torch.save(sd, path)
    net = train.OrienMaskYOLOFPNPlus(3, 80, pretrained=path, backend="torch")
    assert all(torch.equal(net.backbone.state_dict()[k], v) for k, v in sd.items())
    inf = infer_model.OrienMaskYOLOFPNPlus(3, 80, pretrained=path)
    assert all(torch.equal(inf.state_dict()["backbone." + k], v) for k, v in sd.items())


# ---------------------------------------------------------------------------------------------------------------- the reference's step
def _check(got, want, what, tol=1e-4):
    err = N.rel_l2(got, want)
    print("%-60s rel L2 %.3g" % (what, err))
    assert err <= tol, (what, err)


@pytest.mark.parametrize("fixture", ["train_step_f96_b2", "train_step_bneval_f96_b2"])
def test_torch_backend_reproduces_the_reference_training_step(fixture):
    """Heads, running statistics and gradients of the reference model in train() mode, within 1e-4 (relative L2 per tensor; a wiring
    mistake is an O(1) error), num_batches_tracked exactly."""
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    sd, x = fixture_weights_and_input(g)
    net = train.OrienMaskYOLOFPNPlus(3, 80, backbone_batchnorm_eval=bool(int(g["bneval"])), backend="torch")
    net.load_state_dict(sd, strict=True)
    net.train()
    out = net(x)
    heads = [t for pair in out for t in pair]
    for k, t in zip(N.HEAD_KEYS, heads):
        assert N.rel_max(t.detach().numpy(), g[k]) <= 1e-4, k
    cot = N.cotangents(int(g["gseed"]), [t.shape for t in heads])
    torch.autograd.backward(heads, [torch.from_numpy(c) for c in cot])
    after = net.state_dict()
    layers = [str(k) for k in g["bn_layers"]]
    assert layers == [k[:-len(".running_mean")] for k in after if k.endswith("running_mean")]
    _check(np.concatenate([after[k + ".running_mean"].numpy() for k in layers]), g["running_mean"], "running_mean")
    _check(np.concatenate([after[k + ".running_var"].numpy() for k in layers]), g["running_var"], "running_var")
    assert [int(after[k + ".num_batches_tracked"]) for k in layers] == g["num_batches_tracked"].tolist()
    params = dict(net.named_parameters())
    assert list(params) == [str(k) for k in g["param_names"]]
    for i, n in enumerate(N.GRAD_NAMES):
        _check(params[n].grad.numpy(), g["grad_%d" % i], "grad " + n)
    for i, (n, p) in enumerate(params.items()):
        gr = p.grad.double()
        l2, s = float(g["grad_l2"][i]), float(g["grad_sum"][i])
        assert abs(gr.norm().item() - l2) <= 1e-4 * l2, n
        # |sum of an error vector| <= its L2 norm * sqrt(numel)
        assert abs(gr.sum().item() - s) <= 1e-4 * l2 * np.sqrt(gr.numel()), n


def test_eval_forward_reproduces_the_inference_fixture():
    g = np.load(os.path.join(GOLDEN, "fwd_f96_b2.npz"))
    sd, x = fixture_weights_and_input(g)
    net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch")
    net.load_state_dict(sd, strict=True)
    net.eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        out = net(x)
    got = dict(bbox32=out[0][0], bbox16=out[1][0], bbox8=out[2][0], oriens=torch.cat([out[0][1], out[1][1], out[2][1]], 1))
    for k, t in got.items():
        assert N.rel_max(t.numpy(), g[k]) <= 1e-4, k
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())       # eval mode changes no buffer


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_loud_errors(built):
    blk = train.ConvBNLeaky(4, 8, 1)
    assert blk.backend == "hip"
    with pytest.raises(omlib.OrienMaskHipError, match="CPU|MI355X"):
        blk(torch.rand(2, 4, 5, 5))                               # 'hip' on a CPU tensor: no fallback
    for backend in train.BACKENDS:
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            train.ConvBNLeaky(4, 8, 1, backend=backend).train()(torch.rand(1, 4, 1, 1))
    with pytest.raises(ValueError):                               # torch raises too
        F.batch_norm(torch.rand(1, 8, 1, 1), None, None, training=True)
    none = train.ConvBNLeaky(4, 8, 1, backend="torch")
    none.conv_block[1].momentum = None
    with pytest.raises(ValueError, match="momentum"):
        none(torch.rand(2, 4, 5, 5))
    with pytest.raises(ValueError, match="backend"):
        train.ConvBNLeaky(4, 8, 1, backend="triton")
    with pytest.raises(ValueError, match="backend"):
        train.OrienMaskYOLO(3, 80, backend="eager")
    for freeze in (True, 3):
        with pytest.raises(NotImplementedError):
            train.OrienMaskYOLOFPNPlus(3, 80, freeze_backbone=freeze)
    with pytest.raises(NotImplementedError, match="SyncBatchNorm"):
        builder.build_train_model(dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80), is_distributed=True)
    # the registry swap of trainer/builder.py:84
    cfg = dict(type="OrienMaskYOLO", num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False,
               backbone_batchnorm_eval=False, backend="torch")
    net = builder.build(cfg, train)
    assert type(net) is train.OrienMaskYOLO and cfg["type"] == "OrienMaskYOLO"
    eval_blk = train.ConvBNLeaky(4, 8, 3, padding=1, backend="torch").eval()
    assert eval_blk(torch.rand(1, 4, 1, 1)).shape == (1, 8, 1, 1)          # one value per channel is fine in eval mode


# ---------------------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 3, 3), (1, 3, 1, 2), (3, 7, 17, 17)])
def test_restatement_equals_torch_float64_autograd(shape, residual, training):
    rng = np.random.default_rng(sum(shape) + 2 * residual + training)
    C = shape[1]
    x = rng.standard_normal(shape) * 2 + 0.5
    gamma, beta = rng.standard_normal(C) + 1.5, rng.standard_normal(C)
    rm, rv = rng.standard_normal(C), rng.random(C) + 0.5
    res = rng.standard_normal(shape) if residual else None
    dy = rng.standard_normal(shape)
    want = N.forward(x, gamma, beta, rm, rv, training, res)
    tx, tg, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, gamma, beta))
    trm, trv = torch.tensor(rm), torch.tensor(rv)
    ty = F.leaky_relu(F.batch_norm(tx, trm, trv, tg, tb, training, N.MOMENTUM, N.EPS), N.SLOPE)
    if residual:
        ty = ty + torch.tensor(res)
    ty.backward(torch.tensor(dy))
    assert N.rel_max(ty.detach().numpy(), want["y"]) < 1e-13
    assert N.rel_max(trm.numpy(), want["running_mean"]) < 1e-13 and N.rel_max(trv.numpy(), want["running_var"]) < 1e-13
    dx, dgamma, dbeta = N.backward(x, dy, gamma, want["mean"], want["invstd"], want["z"] > 0, training)
    # dx is a difference of terms of the size of gamma * invstd * dy (with two values per channel nearly all of it cancels)
    terms = np.abs(gamma * want["invstd"]).max() * np.abs(dy).max()
    assert np.abs(tx.grad.numpy() - dx).max() < 1e-12 * max(terms, np.abs(dx).max())
    assert N.rel_max(tg.grad.numpy(), dgamma) < 1e-12 and N.rel_max(tb.grad.numpy(), dbeta) < 1e-12


def test_naive_float32_variance_is_what_the_ill_conditioned_case_catches():
    """Channel mean 1000, std 1: E[x^2] - E[x]^2 in float32 is off by tens of percent, the two-pass float64 value is the truth."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 16, 48, 48)) + 1000.0).astype(np.float32)
    _, var, _ = N.batch_stats(x)
    n = np.float32(x.shape[0] * x.shape[2] * x.shape[3])
    naive = (x * x).sum(axis=(0, 2, 3), dtype=np.float32) / n - (x.sum(axis=(0, 2, 3), dtype=np.float32) / n) ** 2
    assert np.abs(var - 1).max() < 0.05 and np.abs(naive - var).max() > 0.05
