"""CPU tests of the synchronised BatchNorm + LeakyReLU block: the float64 restatement the GPU tests use as truth (tests/bn_sync_np.py)
is held to the full-batch statistics of tests/bn_act_np.py and to torch-CPU float64 autograd on the whole batch, and the surface of
train.convert_sync_batchnorm / the four om_bn_sync_* entry points is checked.  No GPU compute."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
import bn_act_np as N
import bn_sync_np as S
from orienmask_amd import arch, lib as omlib, train

ENTRIES = ("om_bn_sync_stats", "om_bn_sync_forward", "om_bn_sync_backward_sums", "om_bn_sync_backward_dx")
CUTS = [[8], [4, 4], [3, 5], [1, 2, 5], [3, 3, 2], [1] * 8]


def _batch(seed, shape=(8, 5, 7, 3)):
    rng = np.random.default_rng(seed)
    C = shape[1]
    return dict(x=rng.standard_normal(shape) * 2 + 0.5 + 3 * np.arange(C).reshape(1, C, 1, 1), gamma=rng.standard_normal(C) + 1.5,
                beta=rng.standard_normal(C), dy=rng.standard_normal(shape))


@pytest.mark.parametrize("cuts", CUTS, ids=lambda c: "-".join(map(str, c)))
def test_merged_records_equal_the_full_batch_statistics(cuts):
    d = _batch(len(cuts))
    records = np.stack([S.record(p) for p in S.split(d["x"], cuts)])
    n, mean, var, unbiased, invstd = S.statistics(records, N.EPS)
    want_mean, want_var, want_unbiased = N.batch_stats(d["x"])
    assert np.all(n == d["x"].size // d["x"].shape[1])
    assert N.rel_max(mean, want_mean) <= 1e-12 and N.rel_max(var, want_var) <= 1e-12 and N.rel_max(unbiased, want_unbiased) <= 1e-12
    assert N.rel_max(invstd, 1.0 / np.sqrt(want_var + N.EPS)) <= 1e-12


@pytest.mark.parametrize("cuts", CUTS, ids=lambda c: "-".join(map(str, c)))
def test_synchronised_dx_equals_torch_float64_autograd_on_the_whole_batch(cuts):
    d = _batch(10 + len(cuts))
    tx, tg, tb = (torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("x", "gamma", "beta"))
    ty = F.leaky_relu(F.batch_norm(tx, None, None, tg, tb, True, N.MOMENTUM, N.EPS), N.SLOPE)
    ty.backward(torch.tensor(d["dy"]))
    positive = ty.detach().numpy() > 0
    xs, dys, pos = S.split(d["x"], cuts), S.split(d["dy"], cuts), S.split(positive, cuts)
    n, mean, _, _, invstd = S.statistics(np.stack([S.record(p) for p in xs]), N.EPS)
    sums_all = np.stack([S.backward_sums(x, dy, mean, invstd, p, N.SLOPE) for x, dy, p in zip(xs, dys, pos)])
    want = S.split(tx.grad.numpy(), cuts)
    terms = np.abs(d["gamma"] * invstd).max() * np.abs(d["dy"]).max()
    for x, dy, p, w in zip(xs, dys, pos, want):
        dx = S.backward_dx(x, dy, d["gamma"], mean, invstd, p, sums_all, n, N.SLOPE)
        assert np.abs(dx - w).max() <= 1e-12 * max(terms, np.abs(w).max())
    # the local sums add up to the full batch's dgamma / dbeta
    assert N.rel_max(sums_all.sum(axis=0)[1], tg.grad.numpy()) <= 1e-12 and N.rel_max(sums_all.sum(axis=0)[0], tb.grad.numpy()) <= 1e-12


def test_convert_marks_every_block_and_keeps_keys_and_order():
    """Every Conv -> BatchNorm -> LeakyReLU block of the model is marked: 86 of its 90 convolutions (the four head convolutions
    have no BatchNorm)."""
    net = train.OrienMaskYOLOFPNPlus(3, 80)
    keys, params = list(net.state_dict()), [n for n, _ in net.named_parameters()]
    modules = [n for n, _ in net.named_modules()]
    blocks = [m for m in net.modules() if isinstance(m, train.ConvBNLeaky)]
    assert len(blocks) == sum(spec.bn for spec in arch.fpnplus_convs()) == 86 and not any(m.sync for m in blocks)
    group = object()
    assert train.convert_sync_batchnorm(net, process_group=group) is net
    assert all(m.sync and m.process_group is group for m in blocks)
    assert list(net.state_dict()) == keys and [n for n, _ in net.named_parameters()] == params
    assert [n for n, _ in net.named_modules()] == modules
    assert all(type(m) is torch.nn.BatchNorm2d for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))


def test_convert_refuses_the_torch_backend():
    net = train.OrienMaskYOLO(3, 80, backend="torch")
    with pytest.raises(ValueError, match="backend 'torch'"):
        train.convert_sync_batchnorm(net)
    assert not any(m.sync for m in net.modules() if isinstance(m, train.ConvBNLeaky))
    # a marked block outside a process group exchanges nothing: the 'hip' block refuses a CPU tensor as before
    blk = train.convert_sync_batchnorm(train.ConvBNLeaky(4, 8, 1))
    assert blk.sync and train._sync_world_size(None) == 1


def test_entries_are_declared_bound_and_exported(built):
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    L = omlib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in omlib.SIGNATURES and hasattr(L, name)


def test_null_pointers_and_rank_counts_are_refused_by_name(built):
    L = omlib.load()
    assert L.om_bn_sync_stats(None, 2, 4, 3, 3, None, None, 0, None) != 0 and b"om_bn_sync_stats" in L.om_last_error()
    rc = L.om_bn_sync_forward(None, 2, 4, 3, 3, None, 1, None, None, None, None, None, 0.1, 1e-5, 0.1, None, None, None, None, None, None)
    assert rc != 0 and b"om_bn_sync_forward" in L.om_last_error()
    rc = L.om_bn_sync_backward_sums(None, None, 2, 4, 3, 3, None, None, None, None, 0.1, None, None, None, None, 0, None)
    assert rc != 0 and b"om_bn_sync_backward_sums" in L.om_last_error()
    rc = L.om_bn_sync_backward_dx(None, None, 2, 4, 3, 3, None, None, None, None, 0.1, None, 1, None, None, None)
    assert rc != 0 and b"om_bn_sync_backward_dx" in L.om_last_error()
