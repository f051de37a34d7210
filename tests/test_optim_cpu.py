"""CPU tests of orienmask_amd.optim / orienmask_amd.builder.build_optimizer: the numpy yardstick (tests/optim_np.py) against
torch.optim.SGD on CPU and the recorded fixtures, the schedulers and param_groups against what the reference's own classes
produced (tests/golden/optim_*.npz, tools/gen_golden_optim.py), the chunk planner, state_dict interchange and the refusals."""
import copy
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
import optim_np as N
from orienmask_amd import builder, lib as omlib
from orienmask_amd import optim as O


def _same_run(a, b):
    for (pa, ba), (pb, bb) in zip(a, b):
        if not N.same_bits(pa, pb):
            return False
        if (ba is None) != (bb is None) or (ba is not None and not N.same_bits(ba, bb)):
            return False
    return len(a) == len(b)


def _fixture_run(name):
    g = np.load(os.path.join(GOLDEN, "optim_sgd_%s.npz" % name))
    hyper = json.loads(bytes(g["hyper"]).decode())
    run = [(g["param"][s], g["buf"][s] if "buf" in g.files else None) for s in range(g["param"].shape[0])]
    return g["p0"], list(g["grads"]), hyper, run


@pytest.mark.parametrize("foreach", [False, True])
@pytest.mark.parametrize("name", sorted(N.HYPER_SETS))
def test_numpy_yardstick_equals_torch_cpu(name, foreach):
    """(b) == (a), parameters and momentum buffers after every step, bit for bit: 400,003 elements with magnitudes over five decades
    (vector bodies and scalar tails of torch's CPU kernels), with and without foreach."""
    p0, grads = N.seeded_inputs(100 + sorted(N.HYPER_SETS).index(name), n=400003)
    hyper = N.HYPER_SETS[name]
    assert _same_run(N.numpy_run(p0, grads, hyper), N.torch_cpu_run(p0, grads, hyper, foreach=foreach))


@pytest.mark.parametrize("n", [1, 3, 18, 255])
def test_numpy_yardstick_equals_torch_cpu_small(n):
    for name, hyper in N.HYPER_SETS.items():
        p0, grads = N.seeded_inputs(n, n=n)
        assert _same_run(N.numpy_run(p0, grads, hyper), N.torch_cpu_run(p0, grads, hyper)), name


@pytest.mark.parametrize("name", sorted(N.HYPER_SETS) + ["specials"])
def test_fixture_equals_torch_cpu_and_numpy(name):
    """(c) == (a) run live on this host == (b).  A host whose torch rounds otherwise fails HERE, not in the kernel's tests."""
    p0, grads, hyper, run = _fixture_run(name)
    if name != "specials":
        assert hyper == {k: v for k, v in N.HYPER_SETS[name].items()}
        q0, qgrads = N.seeded_inputs(20 + list(N.HYPER_SETS).index(name))
        assert N.same_bits(p0, q0) and all(N.same_bits(a, b) for a, b in zip(grads, qgrads))
    else:
        q0, qgrads = N.special_inputs()
        assert N.same_bits(p0, q0) and all(N.same_bits(a, b) for a, b in zip(grads, qgrads))
        assert np.isnan(run[0][0]).any() and np.isinf(run[0][0]).any()
    assert _same_run(run, N.torch_cpu_run(p0, grads, hyper)), "torch on this host does not round as the fixture's host did"
    assert _same_run(run, N.numpy_run(p0, grads, hyper))


def test_fma32_is_a_single_rounding():
    """Cases where a float64 multiply-add rounded to float32 (a double rounding) differs from the fused result."""
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)           # a * b = 1 + 2^-11 + 2^-24: a float32 tie ...
    c = np.float32(2.0 ** -60)                                              # ... broken upwards only by c
    assert N.fma32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(1 + 2.0 ** -11)     # the double rounding
    assert N.fma32(a, b, -c) == np.float32(1 + 2.0 ** -11)
    assert np.isnan(N.fma32(np.float32(np.inf), np.float32(0), np.float32(1)))
    assert np.signbit(N.fma32(np.float32(-0.0), np.float32(1), np.float32(-0.0)))
    tiny = np.float32(1e-45)
    assert N.fma32(tiny, np.float32(0.5), tiny) == 2 * tiny and N.fma32(tiny, np.float32(0.25), tiny) == tiny      # 1.5 ties to even, 1.25 down


# ---- schedulers and param_groups against the reference's own results --------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(N.STEP_WARMUP_CASES))
def test_step_warmup_lr_equals_reference(name):
    want = np.load(os.path.join(GOLDEN, "optim_lr_schedules.npz"))["step_" + name]
    case = N.STEP_WARMUP_CASES[name]
    got = N.lr_sequence(lambda opt: O.StepWarmUpLR(optimizer=opt, **case), N.STEP_WARMUP_ITERS)
    assert got.shape == want.shape and (got == want).all(), (got, want)
    # the sequence crosses the warm-up boundary and both milestones
    assert N.STEP_WARMUP_ITERS > max(case["milestones"]) > case["warmup_iter"]
    assert len({float(v) for v in want[case["warmup_iter"] + 1:, 0]}) == 3


def test_step_warmup_lr_positional_signature():
    """the reference's argument order: (warmup_type, warmup_iter, warmup_ratio, optimizer, milestones, gamma, last_epoch)"""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-3)
    sch = O.StepWarmUpLR("linear", 4, 0.1, opt, [6, 8], 0.1)
    assert sch.warmup.type == "linear" and sch.warmup.iter == 4 and sch.warmup.ratio == 0.1 and sch.gamma == 0.1
    assert O.WarmupLR("const", 3, 0.5).get_warmup_lr(2, 1e-2) == 1e-2 * 0.5
    with pytest.raises(AssertionError):
        O.WarmupLR("cosine", 3, 0.5)


def test_poly_lr_equals_reference():
    want = np.load(os.path.join(GOLDEN, "optim_lr_schedules.npz"))["poly"]
    got = N.lr_sequence(lambda opt: O.PolyLR(opt, **N.POLY_CASE), N.POLY_ITERS)
    assert got.shape == want.shape and (got == want).all(), (got, want)


def test_param_groups_equals_reference():
    g = np.load(os.path.join(GOLDEN, "optim_param_groups.npz"))
    model = N.groups_module()
    groups = O.param_groups(model, **N.GROUPS_KWARGS)
    got = N.groups_listing(model, groups)
    want = list(zip([str(s) for s in g["names"]], g["lr"].tolist(), g["weight_decay"].tolist()))
    assert got == want, (got, want)
    names = [n for n, _, _ in got]
    assert "scale.frozen" not in names and "bn2.bias" not in names            # frozen parameters are left out
    assert "tied.weight" not in names and names.count("conv3.weight") == 1    # a shared parameter once
    decays = dict((n, w) for n, _, w in got)
    # both carry-overs of the reference (kept, not repaired): the norm's decay on the weight after a norm, the bias's after a bias
    assert decays["conv1.weight"] == 5e-4 and decays["conv2.weight"] == 0.0 and decays["conv3.weight"] == 1e-4
    assert all(len(x["params"]) == 1 and set(x) == {"params", "lr", "weight_decay"} for x in groups)


def test_reexports_resolve_to_torch():
    assert O.Adam is torch.optim.Adam and O.AdamW is torch.optim.AdamW
    assert O.CosineAnnealingLR is torch.optim.lr_scheduler.CosineAnnealingLR and O.MultiStepLR is torch.optim.lr_scheduler.MultiStepLR
    assert issubclass(O.SGD, torch.optim.SGD) and O.SGD is not torch.optim.SGD
    assert issubclass(O.StepWarmUpLR, torch.optim.lr_scheduler.MultiStepLR)
    p = torch.nn.Parameter(torch.zeros(1))
    sch = builder.build(dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=1000, warmup_ratio=0.1, milestones=[10, 20]),
                        O, optimizer=torch.optim.SGD([p], lr=1e-3))
    assert isinstance(sch, O.StepWarmUpLR)


# ---- build_optimizer ------------------------------------------------------------------------------------------------------------
def test_build_optimizer_divides_by_accumulate_and_keeps_config(monkeypatch):
    model = N.groups_module()
    config = dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4)
    frozen = copy.deepcopy(config)
    monkeypatch.setattr(O, "SGD", torch.optim.SGD)         # a CPU box: look at what the class is called with
    opt = builder.build_optimizer(config, 4, model)
    assert config == frozen
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 1e-3 / 4 and opt.param_groups[0]["momentum"] == 0.9
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in trainable]

    config = dict(type="SGD", lr=8e-3, momentum=0.9, weight_decay=5e-4,
                  param_groups=dict(norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4))
    frozen = copy.deepcopy(config)
    opt = builder.build_optimizer(config, 4, model)
    assert config == frozen
    got = N.groups_listing(model, opt.param_groups)
    want = N.groups_listing(model, O.param_groups(model, base_lr=8e-3 / 4, weight_decay=5e-4, norm_weight_decay=0.0,
                                                  bias_lr_factor=2.0, bias_weight_decay=1e-4))
    assert got == want and got[0][1] == 2e-3 and got[4][1] == 4e-3

    class Wrapper:                                          # what DistributedDataParallel looks like to the builder
        def __init__(self, module):
            self.module = module
    opt = builder.build_optimizer(dict(type="Adam", lr=1e-3, weight_decay=0.0), 2, Wrapper(model), is_distributed=True)
    assert type(opt) is torch.optim.Adam and opt.param_groups[0]["lr"] == 5e-4


def test_build_optimizer_sgd_is_the_hip_class():
    """On a host without a GPU the HIP class refuses the CPU model: there is no eager fallback to torch's step."""
    with pytest.raises(omlib.OrienMaskHipError):
        builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), 1, N.groups_module())


# ---- state_dict interchange -----------------------------------------------------------------------------------------------------
def test_state_dict_interchanges_with_torch_sgd(monkeypatch):
    """The state layout is torch's: a state_dict of the new class loads into torch.optim.SGD and back.  (Built on CPU tensors with
    the device check lifted: nothing here steps.)"""
    monkeypatch.setattr(O, "_check_param", lambda p: None)
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    groups = [{"params": [ps[0]], "lr": 1e-2, "weight_decay": 0.0}, {"params": [ps[1]]}]
    mine = O.SGD(groups, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    for p in ps:
        mine.state[p]["momentum_buffer"] = torch.randn_like(p)
    sd = mine.state_dict()
    theirs = torch.optim.SGD([{"params": [ps[0]]}, {"params": [ps[1]]}], lr=1.0)
    theirs.load_state_dict(sd)
    assert theirs.param_groups[0]["lr"] == 1e-2 and theirs.param_groups[1]["nesterov"] is True
    for p in ps:
        assert torch.equal(theirs.state[p]["momentum_buffer"], mine.state[p]["momentum_buffer"])
    ref_sd = theirs.state_dict()
    assert ref_sd["param_groups"] == sd["param_groups"]
    back = O.SGD([{"params": [ps[0]]}, {"params": [ps[1]]}], lr=1.0)
    back.load_state_dict(ref_sd)
    assert back.param_groups[1]["weight_decay"] == 5e-4 and back._plans is None
    for p in ps:
        assert torch.equal(back.state[p]["momentum_buffer"], mine.state[p]["momentum_buffer"])
    # a scheduler of torch's drives it as it is
    sch = torch.optim.lr_scheduler.MultiStepLR(back, [1], 0.1)
    assert sch.base_lrs == [1e-2, 1e-3]


# ---- chunk planner --------------------------------------------------------------------------------------------------------------
def _assert_exact_cover(counts):
    plan = O.plan_chunks(counts)
    assert plan.dtype == np.int32 and plan.flags["C_CONTIGUOUS"] and plan.shape[1] == 2
    tensor, start, stop = O.chunk_ranges(plan, counts)
    assert (start % 4 == 0).all() and (stop > start).all() and (stop - start <= O.OM_SGD_CHUNK).all()
    for t, n in enumerate(counts):
        sel = tensor == t
        order = np.argsort(start[sel])
        s, e = start[sel][order], stop[sel][order]
        assert s[0] == 0 and e[-1] == n and (s[1:] == e[:-1]).all(), (t, n)       # every element exactly once
    assert int((stop - start).sum()) == int(np.sum(counts))


def test_chunk_plan_covers_the_model_exactly_once():
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    net = OrienMaskYOLOFPNPlus(num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False, backbone_batchnorm_eval=False)
    counts = [p.numel() for p in net.parameters()]
    assert len(counts) == 266 and sum(counts) == 63662063 and min(counts) == 18 and max(counts) == 4718592
    assert sorted(c for c in counts if c % 4) == [18, 255, 255, 255]
    _assert_exact_cover(counts)


def test_chunk_plan_adversarial_counts():
    c = O.OM_SGD_CHUNK
    _assert_exact_cover([1, 3, 18, 255, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 1, 5 * c + 3])
    _assert_exact_cover([c])
    _assert_exact_cover([1])
    for bad in ([], [0], [4, -1]):
        with pytest.raises(ValueError):
            O.plan_chunks(bad)


def test_table_layout_matches_header(built):
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    defines = dict(re.findall(r"#define (OM_SGD_[A-Z_]+) (\d+)", header))
    assert int(defines["OM_SGD_CHUNK"]) == O.OM_SGD_CHUNK
    for name in ("SKIP", "FIRST", "NESTEROV", "MAXIMIZE", "HAS_MOMENTUM", "HAS_WD"):
        assert int(defines["OM_SGD_" + name]) == getattr(O, "OM_SGD_" + name)
    assert O.TENSOR_ROW.itemsize == 64
    assert [O.TENSOR_ROW.fields[f][1] for f in ("param", "grad", "buf", "n", "neg_lr", "weight_decay", "momentum",
                                                "one_minus_dampening", "flags")] == [0, 8, 16, 24, 32, 36, 40, 44, 48]
    assert "om_sgd_step" in omlib.SIGNATURES and len(omlib.SIGNATURES["om_sgd_step"][1]) == 6
    L = omlib.load()
    assert L.om_sgd_step(None, None, 1, None, 1, None) != 0 and b"om_sgd_step" in L.om_last_error()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    cpu = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU or eager fallback"):
        O.SGD([cpu], lr=1e-3)
    with pytest.raises(omlib.OrienMaskHipError):
        O.SGD([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))], lr=1e-3)
    with pytest.raises(TypeError):
        O.SGD([np.zeros(3)], lr=1e-3)
    assert O._is_dense(torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last))
    assert O._is_dense(torch.zeros(4, 6).t()) and not O._is_dense(torch.zeros(4, 6)[:, ::2]) and not O._is_dense(torch.zeros(4, 6)[:, :3])
    monkeypatch.setattr(O, "_check_param", lambda p: None)          # past the device check, on a host without a GPU
    with pytest.raises(omlib.OrienMaskHipError, match="differentiable"):
        O.SGD([cpu], lr=1e-3, differentiable=True)
    opt = O.SGD([cpu], lr=1e-3)
    with pytest.raises(omlib.OrienMaskHipError, match="differentiable"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "differentiable": True})
    assert len(opt.param_groups) == 1
