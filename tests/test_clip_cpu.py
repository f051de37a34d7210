"""CPU tests of gradient-norm clipping in orienmask_amd.optim.SGD: the numpy yardstick (tests/clip_np.py) against exact arithmetic
for the norm and against torch itself (torch.nn.utils.clip_grads_with_norm_ + torch.optim.SGD on CPU) for the clipped step, the
mutants the comparison has to catch, and the host logic (refusals, state_dict, build_optimizer, tools/train.py's flags)."""
import importlib.util
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import REPO
import clip_np as C
import optim_np as N
from orienmask_amd import builder, lib as omlib
from orienmask_amd import optim as O

F32 = np.float32


# ---- the norm against exact arithmetic ------------------------------------------------------------------------------------------
def _exact_norm(g):
    """float32(sqrt(sum of the exact squares)): math.fsum returns the correctly rounded float64 of the exact sum, math.sqrt the
    correctly rounded root of that."""
    return F32(math.sqrt(math.fsum(float(x) * float(x) for x in np.asarray(g, F32).reshape(-1))))


def _norm_cases():
    rs = np.random.RandomState(11)
    tiny = (rs.uniform(0.2, 1.0, 5000) * 1e-39).astype(F32)
    assert (np.abs(tiny) < np.float32(1.1754944e-38)).all() and (tiny != 0).all()
    huge = (rs.standard_normal(9000) * 1e-3).astype(F32)
    huge[4567] = F32(3.0e38)
    return {
        "random": [(np.where(rs.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3.0, 2.0, n)).astype(F32) for n in (1, 18, 4097, 70001)],
        "zeros": [np.zeros(5000, F32), -np.zeros(3, F32)],
        "denormals": [tiny],
        "one_huge": [huge],
    }


@pytest.mark.parametrize("name", ["random", "zeros", "denormals", "one_huge"])
def test_norm_is_within_one_ulp_of_the_exact_norm(name):
    """|yardstick - exact| <= 2^-23 * exact.  The terms are positive, so float64 accumulation of n <= 2^26 terms errs by at most
    n * 2^-53 <= 2^-27 relative, negligible beside the single float32 rounding of 2^-24: the bound is one ulp."""
    grads = _norm_cases()[name]
    got, _ = C.norm_of(grads)
    want = _exact_norm(np.concatenate(grads))
    print(name, float(got), float(want))
    assert np.isfinite(got) and abs(float(got) - float(want)) <= 2.0 ** -23 * float(want)
    if name == "zeros":
        assert got == 0 and not np.signbit(got)


def test_norm_of_two_to_the_24_equal_elements():
    v = F32(0.1)
    got, s = C.norm_of([np.full(2 ** 24, v, F32)])
    exact = Fraction(float(v)) ** 2 * 2 ** 24                             # sqrt = 4096 * v exactly
    assert Fraction(float(s)) == exact or abs(Fraction(float(s)) - exact) <= exact * Fraction(1, 2 ** 27)
    want = F32(4096.0 * float(v))
    print(float(got), float(want))
    assert abs(float(got) - float(want)) <= 2.0 ** -23 * float(want)


def test_norm_ignores_where_a_tensor_starts_but_not_the_chunk_grid():
    """The restated order: an element's lane is (j // 4) % 256 inside its chunk, and chunks are summed in table order; a tensor
    without a gradient keeps its place in that order."""
    rs = np.random.RandomState(12)
    a, b = rs.standard_normal(5000).astype(F32), rs.standard_normal(300).astype(F32)
    with_gap, _ = C.norm_of([a, None, b], [5000, 9000, 300])
    without, _ = C.norm_of([a, b])
    assert abs(float(with_gap) - float(without)) <= 2.0 ** -23 * float(without)
    lanes = rs.standard_normal(256)
    want = sum(sum(lanes[w * 64 + i] for i in range(64)) for w in range(4))
    assert abs(float(C.tree_sum(lanes)) - want) < 1e-12
    one = np.zeros(256)
    one[200] = 1.0
    assert C.tree_sum(one) == 1.0


# ---- the clipped step against torch itself --------------------------------------------------------------------------------------
COUNTS = [1003, 18, 5000, 1]


def _inputs(seed, scale, steps=3, poison=None):
    rs = np.random.RandomState(seed)
    ps = [rs.standard_normal(n).astype(F32) for n in COUNTS]
    gs = [[(rs.standard_normal(n) * scale).astype(F32) for n in COUNTS] for _ in range(steps)]
    if poison is not None:
        gs[1][2][77] = poison
    return ps, gs


def _torch_run(ps, gs, hyper, max_norms, norms):
    """clip_grads_with_norm_(params, max_norm, total_norm=<the given float32 norm>) + torch.optim.SGD.step() on CPU."""
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = torch.optim.SGD(params, **hyper)
    out = []
    for step_grads, max_norm, norm in zip(gs, max_norms, norms):
        for p, g in zip(params, step_grads):
            p.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grads_with_norm_(params, max_norm, total_norm=torch.tensor(float(norm), dtype=torch.float32))
        opt.step()
        out.append(([p.detach().numpy().copy() for p in params],
                    [opt.state[p]["momentum_buffer"].numpy().copy() if "momentum_buffer" in opt.state.get(p, {}) else None
                     for p in params]))
    return out


def _yardstick_run(ps, gs, hyper, max_norms, **mutant):
    cur, bufs, out, norms = [p.copy() for p in ps], [None] * len(ps), [], []
    for step_grads, max_norm in zip(gs, max_norms):
        cur, bufs, norm, coef, _ = C.clipped_step(cur, step_grads, bufs, hyper, max_norm, **mutant)
        norms.append(norm)
        out.append((cur, bufs))
    return out, norms


def _agree(a, b):
    for (pa, ba), (pb, bb) in zip(a, b):
        for x, y in zip(pa, pb):
            if not N.same_bits(x, y):
                return False
        for x, y in zip(ba, bb):
            if (x is None) != (y is None) or (x is not None and not N.same_bits(x, y)):
                return False
    return len(a) == len(b)


def _straddle(norm, k):
    """max_norm k float32 steps away from norm + 1e-6: max / (norm + 1e-6) is within a few ulps of 1.0, on either side."""
    m = F32(F32(norm) + F32(1e-6))
    for _ in range(abs(k)):
        m = np.nextafter(m, F32(np.inf if k > 0 else 0), dtype=F32)
    return float(m)


def _cases():
    """name -> (params, per-step gradients, per-step max_norm)."""
    out = {}
    ps, gs = _inputs(1, 3.0)
    out["far_above"] = (ps, gs, [0.5, 1e-3, 7.0])                          # norms around 230
    ps, gs = _inputs(2, 0.01)
    out["small_norm_clipped"] = (ps, gs, [0.01, 0.3, 0.05])                # norms around 0.78: the 1e-6 is 16 ulps of the norm
    ps, gs = _inputs(3, 0.01)
    out["below"] = (ps, gs, [10.0, 1.0, 100.0])                            # coefficient 1
    ps, gs = _inputs(4, 0.1)
    norms = [C.norm_of(g)[0] for g in gs]
    for k in (-3, -1, 0, 1, 2):
        out["straddle_%+d" % k] = (ps, gs, [_straddle(n, k + d) for d, n in zip((0, 1, -1), norms)])
    ps, gs = _inputs(5, 1.0)
    out["zero_gradients"] = (ps, [[np.zeros_like(g) for g in step] for step in gs], [1.0, 1.0, 1.0])
    ps, gs = _inputs(6, 1.0, poison=F32(np.inf))
    out["inf"] = (ps, gs, [1.0, 1.0, 1.0])
    ps, gs = _inputs(7, 1.0, poison=F32(np.nan))
    out["nan"] = (ps, gs, [1.0, 1.0, 1.0])
    return out


CASES = _cases()


@pytest.mark.parametrize("hyper_name", sorted(N.HYPER_SETS))
def test_yardstick_equals_torch_clip_and_step(hyper_name):
    """Three steps of every case, parameters and momentum buffers after every step, bit for bit; torch is given the yardstick's
    float32 norm, so this pins the coefficient, the product and where it enters the update."""
    hyper = N.HYPER_SETS[hyper_name]
    for name, (ps, gs, max_norms) in CASES.items():
        mine, norms = _yardstick_run(ps, gs, hyper, max_norms)
        coefs = [C.coefficient(n, m) for n, m in zip(norms, max_norms)]
        if name in ("far_above", "small_norm_clipped"):
            assert all(c < 1 for c in coefs)
        if name in ("below", "zero_gradients"):
            assert all(c == 1 for c in coefs)
        if name == "inf":
            assert np.isinf(norms[1]) and coefs[1] == 0 and np.isnan(mine[1][0][2]).any()
        if name == "nan":
            assert np.isnan(norms[1]) and np.isnan(coefs[1]) and all(np.isnan(p).all() for p in mine[1][0])
        assert _agree(mine, _torch_run(ps, gs, hyper, max_norms, norms)), (hyper_name, name)


def test_straddle_cases_fall_on_both_sides_of_one():
    coefs = []
    for name, (ps, gs, max_norms) in CASES.items():
        if name.startswith("straddle"):
            for g, m in zip(gs, max_norms):
                coefs.append(float(C.coefficient(C.norm_of(g)[0], m)))
    print(sorted(set(coefs)))
    assert max(coefs) == 1.0 and min(coefs) < 1.0 and min(coefs) > 1.0 - 1e-6 and len(set(coefs)) >= 3


def test_coefficient_equals_torch_on_random_norms():
    """2000 random (norm, max_norm): the expression torch's clip_grads_with_norm_ evaluates, bit for bit; a true division differs
    on some of them (so the mutant below is distinguishable)."""
    rs = np.random.RandomState(13)
    norms = (10.0 ** rs.uniform(-4, 4, 2000)).astype(F32)
    maxes = (10.0 ** rs.uniform(-3, 3, 2000)).astype(np.float64)
    differ = 0
    for n, m in zip(norms, maxes):
        want = torch.clamp(float(m) / (torch.tensor(float(n), dtype=torch.float32) + 1e-6), max=1.0).numpy()
        assert N.same_bits(C.coefficient(n, float(m)), want), (n, m)
        differ += not N.same_bits(C.coefficient(n, float(m), divide="true"), want)
    print("true division differs on", differ, "of 2000")
    assert differ > 50


@pytest.mark.parametrize("mutant", [dict(divide="true"), dict(eps=0.0), dict(clamp=False), dict(after_decay=True)],
                         ids=["true_division", "no_epsilon", "no_clamp", "coefficient_after_decay"])
def test_the_comparison_catches_mutants(mutant):
    """Each mutant of the yardstick disagrees with torch on at least one case of the set above (momentum and weight decay)."""
    hyper = N.HYPER_SETS["momentum_decay"]
    caught = []
    for name, (ps, gs, max_norms) in CASES.items():
        _, norms = _yardstick_run(ps, gs, hyper, max_norms)
        wrong, _ = _yardstick_run(ps, gs, hyper, max_norms, **mutant)
        if not _agree(wrong, _torch_run(ps, gs, hyper, max_norms, norms)):
            caught.append(name)
    print(mutant, "caught by", caught)
    assert caught


# ---- host logic -----------------------------------------------------------------------------------------------------------------
def _cpu_params():
    return [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]


def test_refusals(monkeypatch):
    cpu = torch.nn.Parameter(torch.zeros(4))
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "1.0", True, 1e39, [1.0]):
        with pytest.raises(ValueError, match="max_grad_norm"):
            O.SGD([cpu], lr=1e-3, max_grad_norm=bad)
    with pytest.raises(omlib.OrienMaskHipError, match="tensor"):
        O.SGD([cpu], lr=1e-3, max_grad_norm=torch.tensor(1.0))
    with pytest.raises(ValueError, match="nonfinite"):
        O.SGD([cpu], lr=1e-3, max_grad_norm=1.0, nonfinite="drop")
    with pytest.raises(ValueError, match="needs max_grad_norm"):
        O.SGD([cpu], lr=1e-3, nonfinite="skip")
    # keyword-only, and not constructor positions of torch.optim.SGD
    kinds = inspect.signature(O.SGD.__init__).parameters
    assert kinds["max_grad_norm"].kind is kinds["nonfinite"].kind is inspect.Parameter.KEYWORD_ONLY
    assert kinds["max_grad_norm"].default is None and kinds["nonfinite"].default == "propagate"
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU or eager fallback"):
        O.SGD([cpu], lr=1e-3, max_grad_norm=1.0, nonfinite="skip")           # valid options: the device check is what refuses
    monkeypatch.setattr(O, "_check_param", lambda p: None)                   # past the device check, on a host without a GPU
    opt = O.SGD([cpu], lr=1e-3, max_grad_norm=2, nonfinite="skip")
    assert opt.max_grad_norm == 2 and opt.nonfinite == "skip"
    assert "max_grad_norm" not in opt.defaults and "nonfinite" not in opt.defaults
    assert all("max_grad_norm" not in g and "nonfinite" not in g for g in opt.param_groups)
    # the attributes are checked again at step(): a value assigned later is refused in the same way, before anything is launched
    monkeypatch.setattr(omlib, "load", lambda: None)
    opt.max_grad_norm = torch.tensor(1.0)
    with pytest.raises(omlib.OrienMaskHipError, match="tensor"):
        opt.step()
    opt.max_grad_norm, opt.nonfinite = 1.0, "sometimes"
    with pytest.raises(ValueError, match="nonfinite"):
        opt.step()
    # parameters on more than one device: the norm is global
    two = O.SGD([cpu, torch.nn.Parameter(torch.zeros(4, device="meta"))], lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(omlib.OrienMaskHipError, match="one device"):
        two._build_plans()
    with pytest.raises(omlib.OrienMaskHipError, match="not enabled"):
        O.SGD([cpu], lr=1e-3).grad_norm_stats()
    fresh = O.SGD([cpu], lr=1e-3, max_grad_norm=1.0).grad_norm_stats()       # no step yet: nothing on a device to read
    assert fresh["steps"] == 0 and fresh["first_nonfinite_step"] == 0 and math.isnan(fresh["mean_norm"])
    assert sorted(fresh) == sorted(["steps", "mean_norm", "max_norm", "clipped_steps", "nonfinite_steps", "first_nonfinite_step",
                                    "last_norm", "last_coef"])


def test_state_dict_is_unchanged_by_clipping(monkeypatch):
    """The two options are attributes: state_dict() has exactly the keys it has without them, and loads into torch.optim.SGD."""
    monkeypatch.setattr(O, "_check_param", lambda p: None)
    ps = _cpu_params()
    hyper = dict(lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    plain = O.SGD([{"params": [ps[0]], "lr": 1e-2}, {"params": [ps[1]]}], **hyper)
    clipped = O.SGD([{"params": [ps[0]], "lr": 1e-2}, {"params": [ps[1]]}], max_grad_norm=10.0, nonfinite="skip", **hyper)
    for opt in (plain, clipped):
        for p in ps:
            opt.state[p]["momentum_buffer"] = torch.full_like(p, 0.25)
    a, b = plain.state_dict(), clipped.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"]
    assert a["param_groups"] == b["param_groups"] and [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert sorted(b["state"]) == [0, 1] and all(sorted(v) == ["momentum_buffer"] for v in b["state"].values())
    theirs = torch.optim.SGD([{"params": [ps[0]]}, {"params": [ps[1]]}], lr=1.0)
    theirs.load_state_dict(b)
    assert theirs.param_groups[0]["lr"] == 1e-2 and theirs.param_groups[1]["nesterov"] is True
    assert theirs.state_dict()["param_groups"] == b["param_groups"]
    for p in ps:
        assert torch.equal(theirs.state[p]["momentum_buffer"], clipped.state[p]["momentum_buffer"])
    back = O.SGD([{"params": [ps[0]]}, {"params": [ps[1]]}], lr=1.0, max_grad_norm=3.0)
    back.load_state_dict(theirs.state_dict())
    assert back.max_grad_norm == 3.0 and back.nonfinite == "propagate" and back._plans is None


def test_build_optimizer_passes_the_two_keys(monkeypatch):
    monkeypatch.setattr(O, "_check_param", lambda p: None)
    model = N.groups_module()
    config = dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0, nonfinite="skip",
                  param_groups=dict(norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4))
    opt = builder.build_optimizer(config, 2, model)
    assert type(opt) is O.SGD and opt.max_grad_norm == 10.0 and opt.nonfinite == "skip"
    assert opt.param_groups[0]["lr"] == 5e-4 and "max_grad_norm" not in opt.param_groups[0]
    plain = builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), 1, model)
    assert plain.max_grad_norm is None and plain.nonfinite == "propagate"
    with pytest.raises(ValueError, match="max_grad_norm"):
        builder.build_optimizer(dict(type="SGD", lr=1e-3, max_grad_norm=-1.0), 1, model)


def test_train_tool_parses_the_two_flags():
    spec = importlib.util.spec_from_file_location("om_train_tool_clip", os.path.join(REPO, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    config = dict(model=dict(type="OrienMaskYOLOFPNPlus"), optimizer=dict(type="SGD", lr=1e-3, max_grad_norm=5.0))
    args = tool.parse_args(["--config", "c.json", "--max-grad-norm", "2.5", "--nonfinite-grads", "skip"])
    assert args.max_grad_norm == 2.5 and args.nonfinite_grads == "skip"
    out = tool.apply_overrides(config, args)
    assert out["optimizer"] == dict(type="SGD", lr=1e-3, max_grad_norm=2.5, nonfinite="skip")
    assert config["optimizer"] == dict(type="SGD", lr=1e-3, max_grad_norm=5.0)          # the caller's dict is not mutated
    none = tool.parse_args(["--config", "c.json"])
    assert none.max_grad_norm is None and none.nonfinite_grads is None and tool.apply_overrides(config, none) is config
    with pytest.raises(SystemExit):
        tool.parse_args(["--config", "c.json", "--nonfinite-grads", "drop"])


def test_constants_match_the_header():
    header = open(os.path.join(REPO, "include", "orienmask_hip.h")).read()
    import re
    defines = {k: int(v) for k, v in re.findall(r"#define (OM_(?:CLIP|SGD)_[A-Z_]+) (\d+)", header)}
    for name in ("OM_SGD_DEVICE_FIRST", "OM_CLIP_SKIP_NONFINITE", "OM_CLIP_NORM_OFF", "OM_CLIP_COEF_OFF", "OM_CLIP_SKIP_OFF",
                 "OM_CLIP_STEPS_OFF", "OM_CLIP_SUM_OFF", "OM_CLIP_MAX_OFF", "OM_CLIP_CLIPPED_OFF", "OM_CLIP_NONFINITE_OFF",
                 "OM_CLIP_FIRST_NONFINITE_OFF", "OM_CLIP_STATE_DOUBLES"):
        assert defines[name] == getattr(O, name), name
    assert "om_sgd_clip_step" in omlib.SIGNATURES and len(omlib.SIGNATURES["om_sgd_clip_step"][1]) == 12
    assert C.CHUNK == O.OM_SGD_CHUNK


def test_launcher_validates(built):
    L = omlib.load()
    assert L.om_sgd_clip_step(None, None, 1, None, 1, None, None, None, 1.0, 0, 1, None) != 0
    assert b"om_sgd_clip_step" in L.om_last_error()
    # the scalar arguments are refused before anything is enqueued (the pointers are never followed: 64 is just not null)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.om_sgd_clip_step(None, 64, 1, 64, 1, 64, 64, 64, bad, 0, 1, None) != 0 and b"max_norm" in L.om_last_error(), bad
    assert L.om_sgd_clip_step(None, 64, 1, 64, 1, 64, 64, 64, 1.0, 0, 0, None) != 0 and b"step" in L.om_last_error()
    assert L.om_sgd_clip_step(None, 64, 1, 64, 1, 64, 64, 64, 1.0, 2, 1, None) != 0 and b"mode" in L.om_last_error()
    assert L.om_sgd_clip_step(None, 64, 1, 64, 1, 68, 64, 64, 1.0, 0, 1, None) != 0 and b"misaligned" in L.om_last_error()
    assert L.om_sgd_clip_step(None, 64, 0, 64, 1, 64, 64, 64, 1.0, 0, 1, None) != 0 and b"tensors" in L.om_last_error()
