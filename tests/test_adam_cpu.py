"""HipAdam / HipAdamW without a GPU: the numpy restatement of the step (tests/adam_np.py) against live torch-CPU, the bias table of
the device-counted step, the mutants the restatement must tell apart, the names, the builder and the refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch

import adam_np as A
import optim_np as N
from conftest import REPO
from orienmask_amd import builder, lib as omlib
from orienmask_amd import optim as O

SIZES = (1, 7, 64, 4099)


def _grads_with_a_gap(n, seed):
    p0, grads = A.seeded_inputs(seed, n)
    grads[2] = None                                          # no gradient in the middle step
    return p0, grads


# ---- the restatement against torch-CPU --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(A.HYPER_SETS))
def test_restatement_with_torchs_sqrt_is_torch_cpu_bit_for_bit(name, n):
    """p, exp_avg and exp_avg_sq over 5 steps (lr from a schedule, no gradient in step 3) with torch's own Tensor.sqrt on the same
    values: every other operation of the restatement is torch-CPU's, in the vector body and in the loop tail."""
    hyper, decoupled = A.HYPER_SETS[name]
    p0, grads = _grads_with_a_gap(n, 11 + n)
    want = A.torch_cpu_run(p0, grads, hyper, decoupled, lrs=A.SCHEDULE)
    got = A.numpy_run(p0, grads, hyper, decoupled, lrs=A.SCHEDULE, sqrt=A.torch_sqrt)
    for s in range(A.ADAM_STEPS):
        for what, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got[s], want[s]):
            assert N.same_bits(a, b), (name, n, s, what)
    assert N.same_bits(got[2][0], got[1][0]) and N.same_bits(got[2][1], got[1][1])       # the step without a gradient moved nothing


@pytest.mark.parametrize("n", (1, 3, 7))
@pytest.mark.parametrize("name", sorted(A.HYPER_SETS))
def test_restatement_with_ieee_sqrt_is_torch_cpu_on_short_tensors(name, n):
    """Tensors short enough for torch's scalar path: the IEEE sqrt of the contract is then torch's too."""
    hyper, decoupled = A.HYPER_SETS[name]
    p0, grads = _grads_with_a_gap(n, 23 + n)
    want = A.torch_cpu_run(p0, grads, hyper, decoupled, lrs=A.SCHEDULE)
    got = A.numpy_run(p0, grads, hyper, decoupled, lrs=A.SCHEDULE)
    for s in range(A.ADAM_STEPS):
        for what, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got[s], want[s]):
            assert N.same_bits(a, b), (name, n, s, what)


def test_specials_propagate_as_in_torch():
    p0, grads = A.special_inputs()
    hyper, decoupled = A.HYPER_SETS["adamw"]
    want = A.torch_cpu_run(p0, grads, hyper, decoupled)
    got = A.numpy_run(p0, grads, hyper, decoupled, sqrt=A.torch_sqrt)
    for s in range(len(grads)):
        for what, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got[s], want[s]):
            assert N.same_bits(a, b), (s, what)
    assert np.isnan(got[0][0]).any() and np.isinf(got[0][2]).any()


# ---- mutants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ["lerp_mul_add", "addcmul_square_first", "fma_last"])
def test_the_restatement_tells_the_mutants_apart(mutant):
    """One operation swapped for a near-equivalent one: torch-CPU (and so the contract) differs in some element, in both branches
    of lerp."""
    for name in ("adam_wd", "beta1_low"):
        hyper, decoupled = A.HYPER_SETS[name]
        p0, grads = A.seeded_inputs(5, 4099)
        want = A.torch_cpu_run(p0, grads, hyper, decoupled)
        good = A.numpy_run(p0, grads, hyper, decoupled, sqrt=A.torch_sqrt)
        bad = A.numpy_run(p0, grads, hyper, decoupled, sqrt=A.torch_sqrt, mutant=mutant)
        assert all(N.same_bits(a, b) for a, b in zip(good[-1], want[-1])), (name, "the unmutated restatement")
        assert not all(N.same_bits(a, b) for a, b in zip(bad[-1], want[-1])), (name, mutant)


def test_pow_one_half_is_not_sqrt():
    """bc2s is ``bias_correction2 ** 0.5`` as torch writes it; at some step counts that is not sqrt's double.  The restatement and
    the bias table hold the former."""
    beta2 = 0.999
    ks = [k for k in range(1, 3000) if math.sqrt(1 - beta2 ** float(k)) != (1 - beta2 ** float(k)) ** 0.5]
    assert ks, "no step count below 3000 tells ** 0.5 from sqrt on this host"
    k = ks[0]
    table = O.adam_bias_table(0.9, beta2)
    assert table[k, 1] == (1 - beta2 ** float(k)) ** 0.5 == A.corrections(0.9, beta2, float(k))[1]
    assert table[k, 1] != math.sqrt(1 - beta2 ** float(k))


# ---- the bias table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.4, 0.99), (0.0, 0.5), (0.95, 0.9)])
def test_bias_table_rows_are_the_host_scalars(betas):
    table = O.adam_bias_table(*betas)
    assert table.dtype == np.float64 and table.ndim == 2 and table.shape[1] == 2
    want = np.asarray([A.corrections(betas[0], betas[1], float(k)) for k in range(table.shape[0])], dtype=np.float64)
    assert np.array_equal(table.view(np.int64), want.view(np.int64))
    both_one = (table[:, 0] == 1.0) & (table[:, 1] == 1.0)
    assert both_one[-1] and not both_one[:-1].any()          # it ends at the first row where both are exactly 1.0
    for k in (table.shape[0], table.shape[0] + 1, 10 * table.shape[0]):
        assert A.corrections(betas[0], betas[1], float(k)) == (1.0, 1.0)                 # and both stay 1.0 beyond it
    if betas == (0.9, 0.999):
        assert 30000 < table.shape[0] < 45000


def test_bias_table_refuses_betas_that_need_too_many_rows():
    with pytest.raises(omlib.OrienMaskHipError, match="rows"):
        O.adam_bias_table(0.9, 0.99999)
    with pytest.raises(omlib.OrienMaskHipError, match="rows"):
        O.adam_bias_table(0.999999, 0.999)
    assert O.adam_bias_table(0.9, 0.9999).shape[0] <= O.ADAM_BIAS_MAX_ROWS == 2 ** 20


# ---- names, builder, refusals ---------------------------------------------------------------------------------------------------------
def test_names():
    assert O.Adam is torch.optim.Adam and O.AdamW is torch.optim.AdamW
    assert issubclass(O.HipAdam, torch.optim.Adam) and issubclass(O.HipAdamW, torch.optim.AdamW)
    assert not issubclass(O.HipAdam, torch.optim.AdamW)
    for name in ("om_adam_step", "om_adam_clip_step", "om_adam_ema_swap"):
        assert name in omlib.SIGNATURES
    for cls in (O.HipAdam, O.HipAdamW, O.SGD):
        for method in ("ema_swap", "ema_applied", "ema_state_dict", "load_ema_state_dict", "ema_updates", "grad_norm_stats"):
            assert getattr(cls, method) is getattr(O._HipStep, method)                  # shared, not copied


def test_row_layout_is_the_kernel_files():
    """ADAM_ROW against struct om_adam_tensor of csrc/optim.hip (the header documents it; the struct itself lives there)."""
    from test_abi_cpu import mirror_layout, struct_layout, struct_mismatches
    with open(os.path.join(REPO, "orienmask_amd", "csrc", "optim.hip")) as f:
        body = re.search(r"struct\s+om_adam_tensor\s*\{([^{}]*)\}", f.read()).group(1)
    body = re.sub(r"//[^\n]*", " ", body)
    assert struct_mismatches("om_adam_tensor", struct_layout(body, {}), mirror_layout(O.ADAM_ROW)) == []
    assert O.ADAM_ROW.itemsize == O.OM_ADAM_ROW_BYTES == 96


def test_build_optimizer_reaches_the_class(monkeypatch):
    monkeypatch.setattr(O, "_check_param", lambda *a: None)          # a host without a GPU: nothing here steps
    model = N.groups_module()
    config = dict(type="HipAdamW", lr=1e-3, weight_decay=1e-2, max_grad_norm=10.0, nonfinite="skip", ema_decay=0.999)
    opt = builder.build_optimizer(config, 2, model)
    assert type(opt) is O.HipAdamW and isinstance(opt, torch.optim.AdamW)
    assert opt.param_groups[0]["lr"] == 5e-4 and opt.param_groups[0]["weight_decay"] == 1e-2
    assert (opt.max_grad_norm, opt.nonfinite, opt.ema_decay, opt.ema_warmup) == (10.0, "skip", 0.999, True)
    assert config["lr"] == 1e-3
    assert set(opt.state_dict()["param_groups"][0]) == set(torch.optim.AdamW(model.parameters()).state_dict()["param_groups"][0])
    plain = builder.build_optimizer(dict(type="HipAdam", lr=1e-3, weight_decay=0.0), 1, model)
    assert type(plain) is O.HipAdam and not plain.param_groups[0]["decoupled_weight_decay"]
    assert opt.param_groups[0]["decoupled_weight_decay"]


def test_on_a_host_without_a_gpu_the_class_refuses_the_model():
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU or eager fallback"):
        builder.build_optimizer(dict(type="HipAdamW", lr=1e-3, weight_decay=1e-2), 1, N.groups_module())
    with pytest.raises(omlib.OrienMaskHipError, match="HipAdam"):
        O.HipAdam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)


@pytest.mark.parametrize("cls", ["HipAdam", "HipAdamW"])
def test_refusals(cls, monkeypatch):
    C = getattr(O, cls)
    cpu = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(omlib.OrienMaskHipError, match="float32"):
        C([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=1e-3)
    with pytest.raises(omlib.OrienMaskHipError):
        C([cpu], lr=1e-3)                                    # not on the GPU
    monkeypatch.setattr(O, "_check_param", lambda *a: None)  # past the device check
    with pytest.raises(omlib.OrienMaskHipError, match="amsgrad"):
        C([cpu], lr=1e-3, amsgrad=True)
    for key in ("capturable", "differentiable", "foreach", "fused"):
        with pytest.raises(omlib.OrienMaskHipError, match=key):
            C([cpu], lr=1e-3, **{key: True})
    with pytest.raises(omlib.OrienMaskHipError, match="tensor"):
        C([cpu], lr=torch.tensor(1e-3))
    with pytest.raises(omlib.OrienMaskHipError, match="tensor"):
        C([cpu], lr=1e-3, betas=(torch.tensor(0.9), torch.tensor(0.999)))
    with pytest.raises(omlib.OrienMaskHipError, match="rows"):
        C([cpu], lr=1e-3, betas=(0.9, 0.99999), max_grad_norm=1.0, nonfinite="skip")
    C([cpu], lr=1e-3, betas=(0.9, 0.99999), max_grad_norm=1.0)                           # host-known counts need no table
    with pytest.raises(ValueError, match="max_grad_norm"):
        C([cpu], lr=1e-3, nonfinite="skip")
    with pytest.raises(ValueError, match="ema_decay"):
        C([cpu], lr=1e-3, ema_decay=1.5)
    opt = C([cpu], lr=1e-3)
    with pytest.raises(omlib.OrienMaskHipError, match="amsgrad"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "amsgrad": True})
    with pytest.raises(omlib.OrienMaskHipError, match="sparse"):
        opt._conform_grad(cpu, torch.zeros(4).to_sparse())
    with pytest.raises(omlib.OrienMaskHipError, match=cls):
        opt.grad_norm_stats()


def test_state_dict_interchanges_with_torch(monkeypatch):
    """The state layout is torch's: keys step / exp_avg / exp_avg_sq, a state_dict loads both ways.  (CPU tensors with the device
    check lifted: nothing here steps.)"""
    monkeypatch.setattr(O, "_check_param", lambda *a: None)
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    theirs = torch.optim.AdamW(ps, lr=1e-3, weight_decay=1e-2, foreach=False)
    for p in ps:
        p.grad = torch.randn_like(p)
    theirs.step()
    theirs.step()
    mine = O.HipAdamW(ps, lr=5e-4, weight_decay=0.0, max_grad_norm=1.0, nonfinite="skip")
    mine.load_state_dict(theirs.state_dict())
    assert mine.param_groups[0]["lr"] == 1e-3 and mine.param_groups[0]["weight_decay"] == 1e-2
    for p in ps:
        assert set(mine.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(mine.state[p]["step"]) == 2.0
        assert torch.equal(mine.state[p]["exp_avg"], theirs.state[p]["exp_avg"])
    back = torch.optim.AdamW(ps, lr=1.0, foreach=False)
    back.load_state_dict(mine.state_dict())
    assert float(back.state[ps[1]]["step"]) == 2.0 and torch.equal(back.state[ps[1]]["exp_avg_sq"], theirs.state[ps[1]]["exp_avg_sq"])
    assert (mine.max_grad_norm, mine.nonfinite) == (1.0, "skip")                          # attributes, not state
