"""HipAdam / HipAdamW on the GPU against tests/adam_np.py, bit for bit: shapes around the chunk and the 16-byte path, each stream
misaligned in turn, several groups in one launch, clipping, the skipped step with its device-side counts, the EMA, streams and
synchronisation, checkpoints both ways with torch's classes, the model's 266 shapes once, live torch-CPU, and the trainer."""
import copy
import os
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import adam_np as A
import clip_np as C
import ema_np as E
import loss_counter_cases as cases
import optim_np as N
from orienmask_amd import optim as O
from optim_harness import dev, _param, _np, _np_grad, _set_grads  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu


def _hyper_of(group):
    return dict(lr=group["lr"], betas=tuple(group["betas"]), eps=group["eps"], weight_decay=group["weight_decay"],
                maximize=group["maximize"])


def _reference(opt, params, sqrt=A.ieee_sqrt):
    group_of = {id(p): g for g in opt.param_groups for p in g["params"]}
    ref = A.Reference([_np(p) for p in params], [_hyper_of(group_of[id(p)]) for p in params],
                      isinstance(opt, torch.optim.AdamW), sqrt=sqrt)
    ref.group_of = group_of
    return ref


def _ref_step(ref, params, grads, coef=None, threads=1):
    """One step of the yardstick with the hyper-parameters the optimizer's groups hold now."""
    for i, p in enumerate(params):
        ref.hypers[i] = _hyper_of(ref.group_of[id(p)])
    if threads == 1:
        ref.step(grads, coef=coef)
        return

    def one(i):
        if grads[i] is not None:
            ref.k[i] += 1.0
            ref.p[i], ref.m[i], ref.v[i] = A.adam_step(ref.p[i], grads[i], ref.m[i], ref.v[i], ref.k[i], decoupled=ref.decoupled,
                                                       coef=coef, **ref.hypers[i])
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(len(params))))


def _assert_state(opt, params, ref, what, counts=True):
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        st = opt.state.get(p, {})
        assert N.same_bits(_np(p), ref.p[i]), (what, "param", i, tuple(p.shape))
        if ref.k[i] == 0 and "exp_avg" not in st:
            continue
        assert N.same_bits(_np(st["exp_avg"]), ref.m[i]), (what, "exp_avg", i, tuple(p.shape))
        assert N.same_bits(_np(st["exp_avg_sq"]), ref.v[i]), (what, "exp_avg_sq", i, tuple(p.shape))
        if counts:
            assert float(st["step"]) == ref.k[i], (what, "step", i, float(st["step"]), ref.k[i])


def _drive(dev, opt, params, grads_per_step, ref=None, what="", after_step=None):
    ref = _reference(opt, params) if ref is None else ref
    for s, grads in enumerate(grads_per_step):
        _set_grads(dev, params, grads)
        flat = [None if p.grad is None else _np_grad(p) for p in params]
        _ref_step(ref, params, flat)
        opt.step()
        _assert_state(opt, params, ref, (what, "step", s))
        if after_step is not None:
            after_step(s)
    return ref


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
SHAPE_COUNTS = (1, 3, 4, 5, 4095, 4096, 4097, 8193)


@pytest.mark.parametrize("cls", ["HipAdam", "HipAdamW"])
def test_counts_around_the_chunk_and_the_vector_path(dev, cls):
    assert O.OM_SGD_CHUNK == 4096
    rs = np.random.RandomState(1)
    params = [_param(dev, rs.standard_normal(n)) for n in SHAPE_COUNTS]
    opt = getattr(O, cls)(params, lr=1e-2, weight_decay=1e-2)
    _drive(dev, opt, params, [[rs.standard_normal(n).astype(np.float32) for n in SHAPE_COUNTS] for _ in range(3)], what=cls)


@pytest.mark.parametrize("stream", ["param", "grad", "exp_avg", "exp_avg_sq"])
def test_each_stream_one_float_off_the_16_byte_grid(dev, stream):
    """Views one float into a flat buffer: each of the four streams in turn is the one that forces the 4-byte path."""
    rs = np.random.RandomState(2)
    counts = [1003, 4097, 6]
    flat = torch.from_numpy(rs.standard_normal(3 * 8192).astype(np.float32)).to(dev)

    def view(i, n):
        v = flat[8192 * i + 1: 8192 * i + 1 + n]
        assert v.data_ptr() % 16 == 4
        return v
    if stream == "param":
        params = [torch.nn.Parameter(view(i, n)) for i, n in enumerate(counts)]
    else:
        params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.HipAdamW(params, lr=1e-2, weight_decay=1e-2)
    ref = _reference(opt, params)
    for s in range(3):
        grads = [torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev) for n in counts]
        if stream == "grad":
            for i, n in enumerate(counts):
                view(i, n).copy_(grads[i])
            grads = [view(i, n) for i, n in enumerate(counts)]
        if stream in ("exp_avg", "exp_avg_sq") and s == 1:       # the moment becomes the caller's misaligned view
            for i, (p, n) in enumerate(zip(params, counts)):
                view(i, n).copy_(opt.state[p][stream])
                opt.state[p][stream] = view(i, n)
        _set_grads(dev, params, grads)
        _ref_step(ref, params, [_np(g) for g in grads])
        opt.step()
        _assert_state(opt, params, ref, (stream, s))
    for p in params:
        assert all(t.data_ptr() % 16 == (4 if name == stream else 0)
                   for name, t in (("param", p), ("exp_avg", opt.state[p]["exp_avg"]), ("exp_avg_sq", opt.state[p]["exp_avg_sq"])))


def test_channels_last_weight_and_strided_gradient(dev):
    rs = np.random.RandomState(3)
    w = torch.from_numpy(rs.standard_normal((16, 8, 3, 3)).astype(np.float32)).to(dev)
    p_cl = torch.nn.Parameter(w.contiguous(memory_format=torch.channels_last))
    p_ct = torch.nn.Parameter(w.clone())
    opt = O.HipAdam([p_cl, p_ct], lr=1e-2, weight_decay=5e-4)
    ref = _reference(opt, [p_cl, p_ct])
    for s in range(3):
        g = torch.from_numpy(rs.standard_normal((16, 8, 3, 3)).astype(np.float32)).to(dev)
        p_cl.grad = g.clone()                               # a contiguous gradient for a channels_last parameter
        p_ct.grad = g.contiguous(memory_format=torch.channels_last)
        _ref_step(ref, [p_cl, p_ct], [_np_grad(p_cl), _np_grad(p_ct)])
        opt.step()
        _assert_state(opt, [p_cl, p_ct], ref, ("layout", s))
        assert torch.equal(p_cl.detach(), p_ct.detach())    # the same values, element for element, in two storage orders
        assert opt.state[p_cl]["exp_avg"].stride() == p_cl.stride() == w.contiguous(memory_format=torch.channels_last).stride()


@pytest.mark.parametrize("cls", ["HipAdam", "HipAdamW"])
def test_specials(dev, cls):
    """+-0, denormals, squares that underflow, large values, NaN and Inf: kept, rounded and propagated as the contract says."""
    p0, grads = A.special_inputs()
    p = _param(dev, p0)
    opt = getattr(O, cls)([p], lr=1e-3, weight_decay=1e-2)
    ref = _drive(dev, opt, [p], [[g] for g in grads], what="specials")
    assert np.isnan(ref.p[0]).any() and np.isinf(ref.v[0]).any()
    tiny = np.abs(ref.v[0][np.isfinite(ref.v[0]) & (ref.v[0] != 0)]).min()
    assert tiny < 1.1754944e-38                             # a denormal second moment survived


# ---- several groups in one launch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["HipAdam", "HipAdamW"])
def test_groups_with_their_own_hypers_and_a_missing_gradient(dev, cls):
    rs = np.random.RandomState(4)
    counts = [18, 255, 5000, 4099, 70001]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    groups = [dict(params=[params[0]], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
              dict(params=[params[1]], lr=3e-3, betas=(0.4, 0.99), eps=1e-3, weight_decay=5e-4),
              dict(params=[params[2], params[3]], lr=1e-3, betas=(0.8, 0.9), eps=1e-6, weight_decay=1e-2, maximize=True),
              dict(params=[params[4]])]
    opt = getattr(O, cls)(groups, lr=2e-3, weight_decay=1e-3)
    sch = O.StepWarmUpLR("linear", 2, 0.1, opt, [3], 0.5)
    steps = [[rs.standard_normal(n).astype(np.float32) for n in counts] for _ in range(5)]
    steps[2][3] = None                                      # no gradient in step 3 of 5
    before = {}

    def after(s):
        sch.step()
        if s == 1:
            before.update(m=_np(opt.state[params[3]]["exp_avg"]).copy(), v=_np(opt.state[params[3]]["exp_avg_sq"]).copy(),
                          p=_np(params[3]).copy())
        if s == 2:                                          # count and moments stayed
            assert float(opt.state[params[3]]["step"]) == 2.0 and float(opt.state[params[2]]["step"]) == 3.0
            assert N.same_bits(_np(opt.state[params[3]]["exp_avg"]), before["m"])
            assert N.same_bits(_np(opt.state[params[3]]["exp_avg_sq"]), before["v"]) and N.same_bits(_np(params[3]), before["p"])
    ref = _drive(dev, opt, params, steps, what=cls, after_step=after)
    assert ref.k == [5.0, 5.0, 5.0, 4.0, 5.0]               # the later corrections of the tensor used its own count


# ---- clipping -----------------------------------------------------------------------------------------------------------------------------
def test_clipped_step_is_clip_grad_norm_then_the_step(dev):
    rs = np.random.RandomState(5)
    counts = [18, 4097, 70001, 1003]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    twins = [_param(dev, _np(p)) for p in params]
    opt = O.HipAdamW(params, lr=1e-2, weight_decay=1e-2, max_grad_norm=2.0)
    sgd = O.SGD(twins, lr=1e-3, max_grad_norm=2.0)
    ref = _reference(opt, params)
    coefs = []
    for s in range(4):
        scale = (10.0, 1e-3, 1.0, 3.0)[s]                   # clipped, not clipped, clipped, clipped
        grads = [(rs.standard_normal(n) * scale).astype(np.float32) for n in counts]
        if s == 2:
            grads[1] = None
        _set_grads(dev, params, grads)
        _set_grads(dev, twins, grads)
        kept = [None if p.grad is None else p.grad.clone() for p in params]
        norm, _ = C.norm_of(grads, counts)
        coef = C.coefficient(norm, 2.0)
        coefs.append(float(coef))
        _ref_step(ref, params, grads, coef=coef)
        opt.step()
        sgd.step()
        _assert_state(opt, params, ref, ("clip", s))
        for p, k in zip(params, kept):
            assert (p.grad is None and k is None) or torch.equal(p.grad, k)              # p.grad is not modified
        # torch's own clip on copies of the gradients: the same norm to float32 accuracy (its summation order is its own)
        copies = [torch.nn.Parameter(torch.zeros(n, device=dev)) for n in counts]
        _set_grads(dev, copies, grads)
        total = torch.nn.utils.clip_grad_norm_(copies, 2.0)
        assert abs(float(total) - float(norm)) <= 1e-5 * float(norm)     # float32 sums of up to 2**17 squares: ~17 roundings of 6e-8
    assert coefs[1] == 1.0 and coefs[0] < 1.0
    mine, theirs = opt.grad_norm_stats(), sgd.grad_norm_stats()
    assert mine == theirs and mine["steps"] == 4 and mine["clipped_steps"] == 3


# ---- the skipped step ---------------------------------------------------------------------------------------------------------------------
def _skip_setup(dev, nonfinite, seed=6):
    rs = np.random.RandomState(seed)
    counts = [18, 4097, 30001]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    groups = [dict(params=params[:2]), dict(params=params[2:], betas=(0.8, 0.99), lr=3e-3)]
    opt = O.HipAdamW(groups, lr=1e-2, weight_decay=1e-2, max_grad_norm=5.0, nonfinite=nonfinite, ema_decay=0.9)
    steps = [[(rs.standard_normal(n) * 3.0).astype(np.float32) for n in counts] for _ in range(6)]
    steps[1][0] = None                                      # counts differ between tensors
    return counts, params, opt, steps


def _snapshot(opt, params):
    torch.cuda.synchronize()
    out = []
    for p in params:
        st = opt.state[p]
        out.append((_np(p).copy(), _np(st["exp_avg"]).copy(), _np(st["exp_avg_sq"]).copy(), _np(opt.ema_shadow(p)).copy()))
    return out


def test_skipped_step_leaves_everything_and_later_steps_follow_the_applied_ones(dev):
    counts, params, opt, steps = _skip_setup(dev, "skip")
    ref = _reference(opt, params)
    shadows = [r.copy() for r in ref.p]
    k_ema = 0
    for s, grads in enumerate(steps):
        grads = list(grads)
        if s == 2:
            grads[1] = grads[1].copy()
            grads[1][77] = np.inf
        _set_grads(dev, params, grads)
        before = _snapshot(opt, params) if s == 2 else None
        opt.step()
        if s == 2:
            after = _snapshot(opt, params)
            for b, a in zip(before, after):
                assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(b, a))
            assert opt.ema_updates() == 2
            sd = opt.state_dict()["state"]
            assert [float(sd[i]["step"]) for i in range(3)] == [1.0, 2.0, 2.0]            # every count stayed
            continue
        norm, _ = C.norm_of(grads, counts)
        _ref_step(ref, params, grads, coef=C.coefficient(norm, 5.0))
        omd = E.omd_at(k_ema, 0.9)
        k_ema += 1
        shadows = [sh if g is None else E.ema_update(sh, p, omd) for sh, p, g in zip(shadows, ref.p, grads)]
        _assert_state(opt, params, ref, ("skip", s), counts=False)
        for p, sh in zip(params, shadows):
            assert N.same_bits(_np(opt.ema_shadow(p)), sh), ("shadow", s)
    assert opt.ema_updates() == 5
    sd = opt.state_dict()["state"]                          # one small read brings the device's counts into state['step']
    assert [float(sd[i]["step"]) for i in range(3)] == ref.k == [4.0, 5.0, 5.0]
    stats = opt.grad_norm_stats()
    assert stats["nonfinite_steps"] == 1 and stats["first_nonfinite_step"] == 3 and stats["steps"] == 6


def test_skip_mode_without_a_nonfinite_step_is_propagate_mode(dev):
    runs = []
    for mode in ("skip", "propagate"):
        counts, params, opt, steps = _skip_setup(dev, mode)
        for grads in steps:
            _set_grads(dev, params, grads)
            opt.step()
        runs.append((_snapshot(opt, params), [float(opt.state_dict()["state"][i]["step"]) for i in range(3)], opt.ema_updates()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    assert runs[0][1:] == runs[1][1:] == ([5.0, 6.0, 6.0], 6)


# ---- EMA ------------------------------------------------------------------------------------------------------------------------------------
def test_ema_follows_sgds_rule_and_leaves_the_step_alone(dev):
    rs = np.random.RandomState(7)
    counts = [18, 4097, 1003]
    p0 = [rs.standard_normal(n).astype(np.float32) for n in counts]
    steps = [[rs.standard_normal(n).astype(np.float32) for n in counts] for _ in range(4)]
    steps[1][2] = None
    with_ema = [_param(dev, a) for a in p0]
    without = [_param(dev, a) for a in p0]
    opt = O.HipAdam(with_ema, lr=1e-2, weight_decay=5e-4, ema_decay=0.99)
    plain = O.HipAdam(without, lr=1e-2, weight_decay=5e-4)
    ref = _reference(opt, with_ema)
    shadows = [a.copy() for a in p0]
    for s, grads in enumerate(steps):
        _set_grads(dev, with_ema, grads)
        _set_grads(dev, without, grads)
        _ref_step(ref, with_ema, grads)
        omd = E.omd_at(s, 0.99)
        shadows = [sh if g is None else E.ema_update(sh, p, omd) for sh, p, g in zip(shadows, ref.p, grads)]
        opt.step()
        plain.step()
        _assert_state(opt, with_ema, ref, ("ema", s))
        _assert_state(plain, without, ref, ("no ema", s))       # the bits parameters and moments have without ema_decay
        for p, sh in zip(with_ema, shadows):
            assert N.same_bits(_np(opt.ema_shadow(p)), sh), ("shadow", s)
    assert opt.ema_updates() == 4
    live = [_np(p).copy() for p in with_ema]
    opt.ema_swap()
    torch.cuda.synchronize()
    for p, sh, lv in zip(with_ema, shadows, live):
        assert N.same_bits(_np(p), sh) and N.same_bits(_np(opt.ema_shadow(p)), lv)
    opt.ema_swap()
    torch.cuda.synchronize()
    for p, sh, lv in zip(with_ema, shadows, live):
        assert N.same_bits(_np(p), lv) and N.same_bits(_np(opt.ema_shadow(p)), sh)      # twice is the identity


# ---- streams, synchronisation, allocation -------------------------------------------------------------------------------------------------
FORMS = {"plain": {}, "clip_skip_ema": dict(max_grad_norm=5.0, nonfinite="skip", ema_decay=0.99),
         "clip_propagate": dict(max_grad_norm=5.0)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_step_neither_synchronises_nor_allocates(dev, monkeypatch, form):
    """After the first step: no device-to-host copy, no synchronisation, no allocation, with a scheduler between the steps and
    zero_grad(set_to_none=True) -- torch's sync debug mode "error" around step() and patched counters, as for SGD."""
    rs = np.random.RandomState(8)
    counts = [18, 255, 4096, 100003]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.HipAdamW(params, lr=1e-2, weight_decay=1e-2, **FORMS[form])
    sch = O.StepWarmUpLR("linear", 3, 0.1, opt, [5], 0.1)
    grads = [[torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev) for n in counts] for _ in range(7)]
    _set_grads(dev, params, grads[0])
    opt.step()
    sch.step()
    torch.cuda.synchronize()
    calls = []
    for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "cpu"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"),
                        (torch.cuda, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")):
        orig = getattr(owner, name)

        def counted(*a, _orig=orig, _name=name, **k):
            calls.append(_name)
            return _orig(*a, **k)
        monkeypatch.setattr(owner, name, counted)
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        calls.clear()
        for s in range(1, 7):
            _set_grads(dev, params, grads[s])
            opt.step()
            sch.step()
            opt.zero_grad(set_to_none=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == [], calls
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before
    monkeypatch.undo()
    # and the steps behind the check are right
    fresh = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt2 = O.HipAdamW(fresh, lr=1e-2, weight_decay=1e-2, **FORMS[form])
    sch2 = O.StepWarmUpLR("linear", 3, 0.1, opt2, [5], 0.1)
    ref = _reference(opt2, fresh)
    for s in range(7):
        g = [_np(t) for t in grads[s]]
        _set_grads(dev, fresh, grads[s])
        coef = None if "max_grad_norm" not in FORMS[form] else C.coefficient(C.norm_of(g, counts)[0], 5.0)
        _ref_step(ref, fresh, g, coef=coef)
        opt2.step()
        sch2.step()
        opt2.zero_grad(set_to_none=True)
        _assert_state(opt2, fresh, ref, (form, s), counts=form != "clip_skip_ema")


def test_non_default_stream(dev):
    rs = np.random.RandomState(9)
    counts = [18, 255, 5000, 70001]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.HipAdamW(params, lr=1e-2, weight_decay=1e-2)
    ref = _reference(opt, params)
    stream = torch.cuda.Stream(dev)
    for s in range(6):                                     # more steps than staging buffers
        gs = [rs.standard_normal(n).astype(np.float32) for n in counts]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            _set_grads(dev, params, gs)
            opt.step()
        stream.synchronize()
        _ref_step(ref, params, gs)
        _assert_state(opt, params, ref, ("stream", s))


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------------------
def test_checkpoints_move_both_ways(dev):
    rs = np.random.RandomState(10)
    counts = [18, 4097, 1003]
    p0 = [rs.standard_normal(n).astype(np.float32) for n in counts]
    steps = [[rs.standard_normal(n).astype(np.float32) for n in counts] for _ in range(5)]
    hyper = dict(lr=1e-2, weight_decay=1e-2)
    # torch.optim.AdamW on the GPU for two steps -> HipAdamW
    theirs_p = [_param(dev, a) for a in p0]
    theirs = torch.optim.AdamW(theirs_p, **hyper)
    for grads in steps[:2]:
        _set_grads(dev, theirs_p, grads)
        theirs.step()
    mine_p = [_param(dev, _np(p)) for p in theirs_p]
    mine = O.HipAdamW(mine_p, lr=1.0, max_grad_norm=1e30, nonfinite="skip")
    mine.load_state_dict(copy.deepcopy(theirs.state_dict()))    # load_state_dict keeps tensors that already fit: no sharing here
    ref = _reference(mine, mine_p)
    for i, p in enumerate(theirs_p):
        ref.m[i], ref.v[i], ref.k[i] = _np(theirs.state[p]["exp_avg"]).copy(), _np(theirs.state[p]["exp_avg_sq"]).copy(), 2.0
    for grads in steps[2:4]:
        _set_grads(dev, mine_p, grads)
        coef = C.coefficient(C.norm_of(grads, counts)[0], 1e30)
        assert coef == 1.0
        _ref_step(ref, mine_p, grads, coef=coef)
        mine.step()
        _assert_state(mine, mine_p, ref, "after loading torch's state", counts=False)
    # ... and back: the counts come out of the device with state_dict()
    sd = mine.state_dict()
    assert [float(sd["state"][i]["step"]) for i in range(3)] == [4.0, 4.0, 4.0]
    back_p = [_param(dev, _np(p)) for p in mine_p]
    back = torch.optim.AdamW(back_p, lr=1.0)
    back.load_state_dict(copy.deepcopy(sd))
    host = O.HipAdamW([_param(dev, _np(p)) for p in mine_p], lr=1.0)        # and into the host-counted form
    host.load_state_dict(copy.deepcopy(sd))
    host_p = [p for g in host.param_groups for p in g["params"]]
    _set_grads(dev, back_p, steps[4])
    _set_grads(dev, host_p, steps[4])
    back.step()
    host.step()
    _ref_step(ref, mine_p, steps[4])
    ref_host = ref
    _assert_state(host, host_p, ref_host, "host-counted after the device-counted checkpoint")
    torch.cuda.synchronize()
    for i, p in enumerate(back_p):
        assert float(back.state[p]["step"]) == 5.0
        np.testing.assert_allclose(_np(p), ref.p[i], rtol=1e-5, atol=1e-7)      # torch's GPU kernel rounds in its own way
        np.testing.assert_allclose(_np(back.state[p]["exp_avg_sq"]), ref.v[i], rtol=1e-5, atol=0)


# ---- the model's shapes at full size ----------------------------------------------------------------------------------------------------------
def test_model_shapes_full_size(dev):
    """The 266 tensors (63,662,063 elements) take one step as 266 groups with the lr / decay split of param_groups."""
    from test_optim import _model_counts_and_groups
    shapes, split = _model_counts_and_groups()
    assert len(shapes) == 266
    rs = np.random.RandomState(5)
    params = [_param(dev, (rs.standard_normal(s) * 0.05).astype(np.float32)) for s in shapes]
    opt = O.HipAdamW([{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(params, split)], lr=1e-3)
    gen = torch.Generator(device=dev).manual_seed(9)
    grads = [torch.randn(s, device=dev, generator=gen) * (10.0 ** float(rs.uniform(-3, 0))) for s in shapes]
    ref = _reference(opt, params)
    _set_grads(dev, params, grads)
    _ref_step(ref, params, [_np(g) for g in grads], threads=8)
    opt.step()
    _assert_state(opt, params, ref, "full size")


# ---- live torch-CPU ---------------------------------------------------------------------------------------------------------------------------
def test_against_live_torch_cpu(dev, capsys):
    """Not a tolerance but a condition: where the GPU differs from torch-CPU after one step, torch's vectorised sqrt differs from
    the IEEE value of the same argument, and the restatement with torch's sqrt in place has no difference left."""
    n = 4099
    differing = total = 0
    for name in sorted(A.HYPER_SETS):
        hyper, decoupled = A.HYPER_SETS[name]
        p0, grads = A.seeded_inputs(31, n, steps=1)
        p = _param(dev, p0)
        opt = (O.HipAdamW if decoupled else O.HipAdam)([p], **hyper)
        p.grad = torch.from_numpy(grads[0]).to(dev)
        opt.step()
        torch.cuda.synchronize()
        got = _np(p)
        want = A.torch_cpu_run(p0, grads, hyper, decoupled)[0]
        ieee = A.numpy_run(p0, grads, hyper, decoupled)[0]
        with_torch_sqrt = A.numpy_run(p0, grads, hyper, decoupled, sqrt=A.torch_sqrt)[0]
        assert N.same_bits(got, ieee[0]), name
        assert N.same_bits(with_torch_sqrt[0], want[0]) and N.same_bits(with_torch_sqrt[2], want[2]), name
        differs = got.view(np.uint32) != want[0].view(np.uint32)
        sqrt_differs = A.torch_sqrt(want[2]).view(np.uint32) != A.ieee_sqrt(want[2]).view(np.uint32)
        assert not (differs & ~sqrt_differs).any(), name
        differing += int(differs.sum())
        total += n
    with capsys.disabled():
        print("\nHipAdam vs live torch-CPU: %d of %d elements of p differ after one step (%.4f %%), all where torch's sqrt is not "
              "the IEEE value" % (differing, total, 100.0 * differing / total))


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------
HIP = dict(backend="hip", conv_backend="hip", conv_forward="hip", route_backend="hip")


class _Scalars:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), step))


def test_trainer_runs_two_steps_with_clipping_skip_and_ema(dev, tmp_path):
    from orienmask_amd import builder, train
    from orienmask_amd.tester import SyntheticLossLoader
    from orienmask_amd.trainer import Trainer
    config = dict(n_gpu=1, accumulate=1, epochs=1, val_freq=1, save_freq=1, monitor="loss", monitor_mode="off", log_freq=2,
                  log_dir=str(tmp_path), name="adamw",
                  model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=cases.NUM_CLASSES, **HIP),
                  loss=dict(type="OrienMaskYOLOMultiScaleLoss", **cases.loss_kwargs()),
                  optimizer=dict(type="HipAdamW", lr=1e-4, weight_decay=1e-2, max_grad_norm=10.0, nonfinite="skip", ema_decay=0.9),
                  lr_scheduler=dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=2, warmup_ratio=0.1, milestones=[4], gamma=0.5))
    kw = dict(size=(cases.IMAGE, cases.IMAGE), gts_per_image=cases.GTS_PER_IMAGE, num_classes=cases.NUM_CLASSES, device=dev)
    torch.manual_seed(7)
    model = builder.build(config["model"], train).to(dev)
    loss = builder.build(config["loss"], train)
    optimizer = builder.build_optimizer(config["optimizer"], config["accumulate"], model)
    assert type(optimizer) is O.HipAdamW
    scheduler = builder.build(config["lr_scheduler"], O, optimizer=optimizer)
    loaders = SyntheticLossLoader(4, cases.BATCH, seed=0, **kw), SyntheticLossLoader(2, cases.BATCH, seed=50, **kw)
    t = Trainer(model, loss, optimizer, scheduler, config, *loaders, lambda predict: None, dev,
                types.SimpleNamespace(resume=None, weights=None))
    t.tensorboard = _Scalars()
    t._log_result = lambda result: None
    assert len(t.train_loader) == 2                         # a two-step run
    t.train()
    torch.cuda.synchronize()
    tags = {tag for tag, _, _ in t.tensorboard.rows}
    assert {"train/grad_norm", "train/grad_norm_max", "train/clipped_steps", "train/skipped_steps", "train/ema_updates"} <= tags
    assert ("train/ema_updates", 2.0, 2) in t.tensorboard.rows and t.optimizer.ema_updates() == 2
    ck = torch.load(os.path.join(t.checkpoint_dir, "epoch1.pth"), map_location=dev, weights_only=False)
    assert "ema" in ck and ck["ema"]["updates"] == 2
    counts = {float(st["step"]) for st in ck["optimizer"]["state"].values()}
    assert counts == {2.0}                                  # the device's counts, read back for the checkpoint
