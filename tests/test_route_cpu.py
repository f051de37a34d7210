"""Without a GPU: the numpy restatement of csrc/route.hip (tests/route_np.py) against torch's own composition on the CPU, and the
host side of route_backend='hip' (orienmask_amd/train.py)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
import route_np as R
import train_step as T
from orienmask_amd import lib as omlib, train
from orienmask_amd.train import split_channels, upsample_concat  # noqa: F401  (the feature under test: absent, nothing here runs)


def _torch_composition(srcs, scales, dy):
    """torch.cat of F.interpolate on the CPU under autograd -> (y, [d src])."""
    ts = [torch.from_numpy(s).requires_grad_(True) for s in srcs]
    y = torch.cat([F.interpolate(t, scale_factor=s, mode="nearest") if s > 1 else t for t, s in zip(ts, scales)], dim=1)
    y.backward(torch.from_numpy(dy))
    return y.detach().numpy(), [t.grad.numpy() for t in ts]


@pytest.fixture(scope="module", params=R.CASES, ids=R.case_id)
def composed(request):
    case = request.param
    srcs, dy = R.inputs(case, 7 + sum(case[:3]))
    return case, srcs, dy, _torch_composition(srcs, R.chans_scales(case)[1], dy)


def test_forward_restatement_equals_torch_cpu(composed):
    case, srcs, _, (y, _) = composed
    chans, scales = R.chans_scales(case)
    got = R.forward(srcs, chans, scales, *case[:3])
    assert got.shape == y.shape and np.array_equal(R.bits(got), R.bits(y))


def test_backward_restatement_equals_torch_cpu_autograd(composed):
    case, _, dy, (_, grads) = composed
    got = R.backward(dy, *R.chans_scales(case))
    for i, (g, t) in enumerate(zip(got, grads)):
        assert g.shape == t.shape and np.array_equal(R.bits(g), R.bits(t)), (case, i)


def test_backward_restatement_is_within_the_sequential_sum_bound(composed):
    case, _, dy, _ = composed
    chans, scales = R.chans_scales(case)
    worst = R.within_bound(R.backward(dy, chans, scales), dy, chans, scales)
    print("%s: worst error / bound %.3f" % (R.case_id(case), worst))
    assert worst <= 1.0


def test_forward_with_a_null_source_is_zeros_there():
    case = R.CASES[9]
    chans, scales = R.chans_scales(case)
    srcs, _ = R.inputs(case, 3)
    y = R.forward([srcs[0], None, srcs[2], srcs[3]], chans, scales, *case[:3])
    full = R.forward(srcs, chans, scales, *case[:3])
    assert not y[:, 7:8].any()
    assert np.array_equal(y[:, :7], full[:, :7]) and np.array_equal(y[:, 8:], full[:, 8:])


@pytest.mark.parametrize("absent", [None, 1], ids=["all-outputs", "one-output-unused"])
def test_split_restatement_equals_torch_split_and_its_autograd(absent):
    """split = the backward at scale 1, its gradient = the forward; an output without a gradient contributes zeros."""
    B, C, H, W, sizes = 2, 18, 5, 7, [6, 6, 6]
    rng = np.random.Generator(np.random.PCG64(11))
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    cots = [rng.standard_normal((B, c, H, W)).astype(np.float32) for c in sizes]
    t = torch.from_numpy(x).requires_grad_(True)
    outs = torch.split(t, sizes, dim=1)
    used = [i for i in range(3) if i != absent]
    torch.autograd.backward([outs[i] for i in used], [torch.from_numpy(cots[i]) for i in used])
    got = R.backward(x, sizes, [1, 1, 1])
    for g, o in zip(got, outs):
        assert np.array_equal(R.bits(g), R.bits(o.detach().numpy()))
    dx = R.forward([cots[i] if i in used else None for i in range(3)], sizes, [1, 1, 1], B, H, W)
    assert np.array_equal(R.bits(dx), R.bits(t.grad.numpy()))


# ---------------------------------------------------------------------------------------------------------------- host logic
def test_route_backend_is_accepted_validated_and_defaults_to_torch():
    for net in T.models():
        assert net.route_backend == "torch"
    for net in T.models(route_backend="hip"):
        assert net.route_backend == "hip" and net.conv_backend == "torch" and net.conv_forward == "torch"
    for cls in (train.OrienMaskYOLOFPNPlus, train.OrienMaskYOLO):
        with pytest.raises(ValueError, match="route_backend"):
            cls(3, 80, route_backend="bogus")


def test_route_backend_leaves_the_module_tree_alone():
    for a, b in zip(T.models(route_backend="hip"), T.models()):
        assert list(a.state_dict().keys()) == list(b.state_dict().keys())
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        assert [tuple(p.shape) for p in a.parameters()] == [tuple(p.shape) for p in b.parameters()]
        assert [type(m) for m in a.modules()] == [type(m) for m in b.modules()]


def test_hip_route_backend_has_no_cpu_fallback():
    x = torch.rand(2, 3, 64, 64)
    for net in T.models(route_backend="hip", backend="torch"):
        with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
            net(x)
    t = torch.rand(2, 4, 3, 3)
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.upsample_concat([t, t], [1, 1])
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.split_channels(t, [2, 2])


def test_counts_are_checked_before_anything_else():
    t = torch.rand(2, 4, 3, 3)
    with pytest.raises(ValueError, match="1 to 4"):
        train.upsample_concat([], [])
    with pytest.raises(ValueError, match="1 to 4"):
        train.upsample_concat([t] * 5, [1] * 5)
    with pytest.raises(ValueError, match="as many scales"):
        train.upsample_concat([t, t], [1])
    with pytest.raises(ValueError, match="1 to 4"):
        train.split_channels(t, [])
    with pytest.raises(ValueError, match="1 to 4"):
        train.split_channels(t, [1, 1, 1, 1, 0])


def test_the_functions_are_exported_and_the_symbols_declared_and_bound():
    assert "upsample_concat" in train.__all__ and "split_channels" in train.__all__
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    for name in ("om_route_concat_forward", "om_route_concat_backward"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in omlib.SIGNATURES and len(omlib.SIGNATURES[name][1]) == 9
