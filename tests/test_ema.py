"""GPU tests of the weight EMA inside the HIP SGD step (om_sgd_ema_step, om_sgd_clip_ema_step, om_ema_swap, csrc/optim.hip;
orienmask_amd.optim.SGD(ema_decay=..., ema_warmup=...)).  Every comparison is BIT FOR BIT (NaN equal to NaN) against tests/ema_np.py
over the case table of tests/ema_cases.py -- which tests/test_ema_cpu.py shows to tell the yardstick from each of its mutants:
parameters, momentum buffers and shadows after every step, and for every case the parameters and buffers of the same run WITHOUT the
average."""
import copy
import os
import types

import numpy as np
import pytest
import torch

import ema_cases as K
import ema_np as E
import loss_counter_cases as cases
import optim_np as N
from orienmask_amd import lib as omlib
from orienmask_amd import optim as O

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# ---- tensors in a case's layout -------------------------------------------------------------------------------------------------
def _place(dev, flat, offset, shape):
    """A float32 array in storage order as a device tensor: a view `offset` elements into a flat buffer, channels-last for a 4-D
    `shape`."""
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    if offset:
        store = torch.zeros(flat.size + 8, device=dev)
        t = store[offset: offset + flat.size]
        t.copy_(torch.from_numpy(flat))
        assert t.data_ptr() % 16 == 4 * offset
    else:
        t = torch.from_numpy(flat).to(dev)
    if shape is not None:
        n, c, h, w = shape
        t = t.view(n, h, w, c).permute(0, 3, 1, 2)          # permuted-dense: NCHW sizes over NHWC storage
        assert not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)
    return t


def _flat(t):
    """The tensor's elements in storage order, on the host."""
    t = t.detach()
    if t.dim() == 4 and not t.is_contiguous():
        t = t.permute(0, 2, 3, 1)
    return t.reshape(-1).cpu().numpy()


def _optimizer(case, params, ema=True, per_tensor=None):
    hypers = case["hypers"]
    kw = dict(max_grad_norm=case["max_norm"], nonfinite=case["nonfinite"])
    if ema:
        kw.update(ema_decay=case["decay"], ema_warmup=case["warmup"])
    if isinstance(hypers, dict):
        groups = [{"params": [p]} for p in params] if per_tensor else params
        return O.SGD(groups, **hypers, **kw)
    return O.SGD([dict(params=[p], **h) for p, h in zip(params, hypers)], lr=1.0, **kw)


def _run(dev, case, ema=True, per_tensor=None):
    """The case on the device -> per step (parameters, buffers, shadows or None, updates or None) as host arrays in storage order."""
    params = [torch.nn.Parameter(_place(dev, p, o, s)) for p, o, s in zip(case["params"], case["offset"], case["shapes"])]
    opt = _optimizer(case, params, ema, per_tensor)
    out = []
    for grads in case["grads"]:
        for p, g, s in zip(params, grads, case["shapes"]):
            p.grad = None if g is None else _place(dev, g, 0, s)
        opt.step()
        torch.cuda.synchronize()
        bufs = [_flat(opt.state[p]["momentum_buffer"]) if "momentum_buffer" in opt.state.get(p, {}) else None for p in params]
        shadows = updates = None
        if ema:
            shadows = [opt.ema_shadow(p) for p in params]
            assert all(e.stride() == p.stride() and e.shape == p.shape and e.dtype == torch.float32 for e, p in zip(shadows, params))
            shadows, updates = [_flat(e) for e in shadows], opt.ema_updates()
        out.append(([_flat(p) for p in params], bufs, shadows, updates))
    return out, opt, params


def _check_buffers(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            # no applied step yet: no buffer, or (nonfinite="skip") the zeros it was allocated with
            assert g is None or not g.view(np.uint32).any(), (what, "buffer before any applied step", i)
        else:
            assert g is not None and N.same_bits(g, w), (what, "buffer", i)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case_equals_the_yardstick_and_leaves_the_step_alone(dev, name):
    case = K.CASES[name]
    want = K.reference(name)
    got, _, _ = _run(dev, case)
    plain, _, _ = _run(dev, case, ema=False)
    assert len(got) == len(want) == len(plain)
    for s, ((ps, bufs, shadows, updates), (wp, wb, we, wk, skipped), (pp, pb, _, _)) in enumerate(zip(got, want, plain)):
        what = (name, "step", s)
        for i in range(len(ps)):
            assert N.same_bits(ps[i], wp[i]), (what, "parameter", i)
            assert N.same_bits(shadows[i], we[i]), (what, "shadow", i)
            # the same run without the average: the step is not disturbed
            assert N.same_bits(ps[i], pp[i]), (what, "parameter with and without the average", i)
            assert (bufs[i] is None) == (pb[i] is None) and (bufs[i] is None or N.same_bits(bufs[i], pb[i])), (what, "buffer", i)
        _check_buffers(bufs, wb, what)
        assert updates == wk, (what, "updates", updates, wk)
    if name == "skip":
        assert [k for _, _, _, k in got] == [1, 1, 2, 2, 3]
        for before, after in ((0, 1), (2, 3)):              # across a skipped step: shadows, parameters and buffers bit-unchanged
            for x, y in zip(got[before][0] + got[before][1] + got[before][2], got[after][0] + got[after][1] + got[after][2]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_one_group_and_one_group_per_tensor_give_the_same_bits(dev):
    case = K.CASES["counts"]
    one, _, _ = _run(dev, case)
    many, opt, _ = _run(dev, case, per_tensor=True)
    assert len(opt.param_groups) == len(K.COUNTS)
    for (pa, ba, ea, ka), (pb, bb, eb, kb) in zip(one, many):
        assert ka == kb and all(N.same_bits(x, y) for x, y in zip(pa + ba + ea, pb + bb + eb))


def test_two_runs_give_the_same_bits(dev):
    for name in ("counts", "skip"):
        a, _, _ = _run(dev, K.CASES[name])
        b, _, _ = _run(dev, K.CASES[name])
        for (pa, _, ea, ka), (pb, _, eb, kb) in zip(a, b):
            assert ka == kb and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(pa + ea, pb + eb))


# ---- the C entry: a shadow that alone is misaligned, a tensor without a shadow ------------------------------------------------------
def test_misaligned_shadow_and_null_shadow_through_the_entry(dev):
    rs = np.random.RandomState(31)
    counts = [2 * 4096 + 5, 1003]
    hyper = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)
    p0 = [K._draw(rs, n) for n in counts]
    e0 = [K._draw(rs, n) for n in counts]                   # not a copy of the parameter: the entry takes what it is given
    grads = [[K._draw(rs, n) for n in counts] for _ in range(2)]
    ps = [torch.from_numpy(p).to(dev) for p in p0]
    bufs = [torch.zeros(n, device=dev) for n in counts]
    shadow = _place(dev, e0[0], 1, None)
    assert ps[0].data_ptr() % 16 == 0 and bufs[0].data_ptr() % 16 == 0 and shadow.data_ptr() % 16 == 4
    ptrs = torch.from_numpy(np.asarray([shadow.data_ptr(), 0], dtype=np.int64)).to(dev)         # the second tensor is not averaged
    chunks = O.plan_chunks(counts)
    chunks_dev = torch.from_numpy(chunks).to(dev)
    table = torch.empty(2 * O.TENSOR_ROW.itemsize, dtype=torch.uint8, device=dev)
    host = torch.empty(2 * O.TENSOR_ROW.itemsize, dtype=torch.uint8).pin_memory()
    rows = host.numpy().view(O.TENSOR_ROW)
    cur, nb, e = [p.copy() for p in p0], [None, None], e0[0].copy()
    omds = [E.omd_at(k, 0.9, warmup=True) for k in range(2)]
    for s, step in enumerate(grads):
        gs = [torch.from_numpy(g).to(dev) for g in step]
        assert all(g.data_ptr() % 16 == 0 for g in gs)
        rows["param"], rows["grad"], rows["buf"] = [[t.data_ptr() for t in ts] for ts in (ps, gs, bufs)]
        rows["n"] = counts
        rows["neg_lr"], rows["weight_decay"], rows["momentum"], rows["one_minus_dampening"] = -hyper["lr"], hyper["weight_decay"], 0.9, 1.0
        rows["flags"] = O.OM_SGD_HAS_MOMENTUM | O.OM_SGD_HAS_WD | (O.OM_SGD_FIRST if s == 0 else 0)
        omlib.launch("om_sgd_ema_step", dev, host, table, 2, chunks_dev, int(chunks.shape[0]), ptrs,
                     float(omds[s]))
        torch.cuda.synchronize()
        cur, nb = N.sgd_step_many(cur, step, nb, hyper)
        e = E.ema_update(e, cur[0], omds[s])
        for i in range(2):
            assert N.same_bits(ps[i].cpu().numpy(), cur[i]) and N.same_bits(bufs[i].cpu().numpy(), nb[i]), (s, i)
        assert N.same_bits(shadow.cpu().numpy(), e), s
    # the swap through the entry: the misaligned pair is exchanged, the tensor without a shadow is left alone
    omlib.launch("om_ema_swap", dev, None, table, 2, chunks_dev, int(chunks.shape[0]), ptrs)
    torch.cuda.synchronize()
    assert N.same_bits(ps[0].cpu().numpy(), e) and N.same_bits(shadow.cpu().numpy(), cur[0]) and N.same_bits(ps[1].cpu().numpy(), cur[1])


# ---- swap -----------------------------------------------------------------------------------------------------------------------
def _nan_payloads(n, seed):
    rs = np.random.RandomState(seed)
    bits = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    bits[::5] = 0x7FC00000 | rs.randint(1, 2 ** 22, bits[::5].size).astype(np.uint32)          # quiet NaNs with payloads
    bits[1::7] = 0xFF800001 + rs.randint(0, 2 ** 22, bits[1::7].size).astype(np.uint32)        # signalling ones, sign set
    return bits


def test_swap_exchanges_and_twice_restores_every_bit(dev):
    """Bit patterns of every kind, NaN payloads included, in aligned, unaligned and channels-last tensors; a tensor without a
    gradient in the latest step is exchanged like any other."""
    layouts = [(1, 0, None), (3, 0, None), (1003, 1, None), (4096, 0, None), (4097, 1, None), (2 * 4096 + 5, 0, None),
               (2 * 3 * 4 * 5, 0, (2, 3, 4, 5))]
    p_bits = [_nan_payloads(n, 40 + i) for i, (n, _, _) in enumerate(layouts)]
    e_bits = [_nan_payloads(n, 60 + i) for i, (n, _, _) in enumerate(layouts)]
    params = [torch.nn.Parameter(_place(dev, b.view(F32), o, s)) for b, (_, o, s) in zip(p_bits, layouts)]
    opt = O.SGD(params, lr=1e-3, momentum=0.9, ema_decay=0.99)
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    opt.ema_swap()                                          # builds the plan: the shadows are bit copies, so nothing moves
    torch.cuda.synchronize()
    assert all(np.array_equal(_flat(p).view(np.uint32), b) for p, b in zip(params, p_bits))
    assert all(np.array_equal(_flat(opt.ema_shadow(p)).view(np.uint32), b) for p, b in zip(params, p_bits))
    for p, b, (_, _, s) in zip(params, e_bits, layouts):    # now shadows of their own
        opt.ema_shadow(p).copy_(_place(dev, b.view(F32), 0, s))
    torch.cuda.synchronize()
    ptrs = [(p.data_ptr(), opt.ema_shadow(p).data_ptr()) for p in params]
    plans = opt._plans
    allocated = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    assert allocated > before
    opt.ema_swap()
    torch.cuda.synchronize()
    assert all(np.array_equal(_flat(p).view(np.uint32), b) for p, b in zip(params, e_bits))
    assert all(np.array_equal(_flat(opt.ema_shadow(p)).view(np.uint32), b) for p, b in zip(params, p_bits))
    with opt.ema_applied():                                 # swaps back in, and out again
        torch.cuda.synchronize()
        assert all(np.array_equal(_flat(p).view(np.uint32), b) for p, b in zip(params, p_bits))
    opt.ema_swap()
    torch.cuda.synchronize()
    assert all(np.array_equal(_flat(p).view(np.uint32), b) for p, b in zip(params, p_bits))
    assert all(np.array_equal(_flat(opt.ema_shadow(p)).view(np.uint32), b) for p, b in zip(params, e_bits))
    # pointers stay, no plan is rebuilt, nothing is allocated
    assert ptrs == [(p.data_ptr(), opt.ema_shadow(p).data_ptr()) for p in params] and opt._plans is plans
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == allocated and opt.ema_updates() == 0


def test_a_step_after_swap_and_back_equals_one_without(dev):
    case = K.CASES["grad_none"]
    want = K.reference("grad_none")
    params = [torch.nn.Parameter(_place(dev, p, 0, None)) for p in case["params"]]
    opt = _optimizer(case, params)
    for s, grads in enumerate(case["grads"]):
        for p, g in zip(params, grads):
            p.grad = None if g is None else _place(dev, g, 0, None)
        opt.step()
        with opt.ema_applied():                             # after step 1 and 2 the middle row is under OM_SGD_SKIP: still swapped
            torch.cuda.synchronize()
            assert all(N.same_bits(_flat(p), e) for p, e in zip(params, want[s][2]))
            assert all(N.same_bits(_flat(opt.ema_shadow(p)), q) for p, q in zip(params, want[s][0]))
        torch.cuda.synchronize()
        assert all(N.same_bits(_flat(p), q) for p, q in zip(params, want[s][0]))
        assert all(N.same_bits(_flat(opt.ema_shadow(p)), e) for p, e in zip(params, want[s][2]))
    assert opt.ema_updates() == 4


# ---- the count across the forms of the step; no synchronisation, no allocation -------------------------------------------------------
def test_the_count_carries_over_when_the_form_of_the_step_changes(dev):
    """plain, clipped, clipped with skip (one step of it skipped), plain again: the decay of every applied step comes from one
    count, 0, 1, 2, 3 (the skipped step has none), whoever keeps it."""
    rs = np.random.RandomState(33)
    counts = [1003, 4097]
    p0 = [K._draw(rs, n) for n in counts]
    grads = [[K._draw(rs, n, 1e-2) for n in counts] for _ in range(5)]
    grads[3][0][5] = np.inf
    hyper = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)
    forms = [(None, "propagate"), (10.0, "propagate"), (10.0, "skip"), (10.0, "skip"), (None, "propagate")]
    params = [torch.nn.Parameter(torch.from_numpy(p).to(dev)) for p in p0]
    opt = O.SGD(params, ema_decay=0.9998, ema_warmup=True, **hyper)
    import clip_np as C
    cur, bufs, shadows, k = [p.copy() for p in p0], [None, None], [p.copy() for p in p0], 0
    for s, ((max_norm, nonfinite), step) in enumerate(zip(forms, grads)):
        opt.max_grad_norm, opt.nonfinite = max_norm, nonfinite
        for p, g in zip(params, step):
            p.grad = torch.from_numpy(g).to(dev)
        opt.step()
        if max_norm is None:
            new, bufs, skipped = *N.sgd_step_many(cur, step, bufs, hyper), False
        else:
            new, bufs, _, _, skipped = C.clipped_step(cur, step, bufs, hyper, max_norm, nonfinite)
        if not skipped:
            shadows = [E.ema_update(e, p, E.omd_at(k, 0.9998)) for e, p in zip(shadows, new)]
            k += 1
        cur = new
        torch.cuda.synchronize()
        assert all(N.same_bits(_flat(p), q) for p, q in zip(params, cur)), s
        assert all(N.same_bits(_flat(opt.ema_shadow(p)), e) for p, e in zip(params, shadows)), s
        if s not in (2, 3):                                 # after the two skip-mode steps the count is left on the device: the plain
            assert opt.ema_updates() == k, (s, k)           # step that follows has to fetch it itself
    assert k == 4 and opt.ema_updates() == 4


@pytest.mark.parametrize("form", ["plain", "clip", "skip"])
def test_averaging_step_neither_synchronises_nor_allocates(dev, monkeypatch, form):
    """After the first step, six averaging steps with a scheduler and zero_grad(set_to_none=True) make no device-to-host copy, no
    synchronisation and no allocation (the harness of tests/test_clip.py); ema_updates() afterwards is the one read."""
    rs = np.random.RandomState(4)
    counts = [18, 255, 4096, 100003]
    params = [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev)) for n in counts]
    kw = dict(plain={}, clip=dict(max_grad_norm=1.0), skip=dict(max_grad_norm=1.0, nonfinite="skip"))[form]
    opt = O.SGD(params, lr=1e-2, momentum=0.9, weight_decay=5e-4, ema_decay=0.9998, **kw)
    sch = O.StepWarmUpLR("linear", 3, 0.1, opt, [5], 0.1)
    grads = [[torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev) for n in counts] for _ in range(7)]
    for p, g in zip(params, grads[0]):
        p.grad = g
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
        for s in range(1, 7):
            for p, g in zip(params, grads[s]):
                p.grad = g
            opt.step()
            sch.step()
            opt.zero_grad(set_to_none=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == [], calls
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before
    monkeypatch.undo()
    assert opt.ema_updates() == 7


# ---- state dict -----------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_on_the_groups_module(dev):
    """optim_np.groups_module(): a weight shared by two modules, a frozen parameter, BatchNorm buffers."""
    def build():
        model = N.groups_module().to(dev)
        opt = O.SGD(O.param_groups(model, **N.GROUPS_KWARGS), lr=1e-3, momentum=0.9, ema_decay=0.9, ema_warmup=False)
        return model, opt

    def steps(model, opt, seeds):
        for seed in seeds:
            gen = torch.Generator(device=dev).manual_seed(seed)
            for p in model.parameters():
                if p.requires_grad:
                    p.grad = torch.randn(p.shape, device=dev, generator=gen)
            opt.step()

    model, opt = build()
    steps(model, opt, [1, 2, 3])
    sd = opt.ema_state_dict(model)
    live = model.state_dict()
    assert list(sd) == list(live)
    held = {id(p) for g in opt.param_groups for p in g["params"]}
    names = dict(model.named_parameters(remove_duplicate=False))
    assert "tied.weight" in names and names["tied.weight"] is names["conv3.weight"]
    for key in sd:
        if key in names and id(names[key]) in held:
            assert torch.equal(sd[key], opt.ema_shadow(names[key])) and not torch.equal(sd[key], live[key]), key
            assert sd[key].data_ptr() != opt.ema_shadow(names[key]).data_ptr()         # a copy
        else:                                               # buffers and frozen parameters: the live tensors
            assert sd[key].data_ptr() == live[key].data_ptr(), key
    assert {"scale.frozen", "bn2.bias", "bn1.running_mean", "bn1.num_batches_tracked"} <= {k for k in sd if not (k in names and id(names[k]) in held)}
    assert torch.equal(sd["tied.weight"], sd["conv3.weight"])
    # into a fresh optimizer that then goes on: equal to the run that was never interrupted
    model2, opt2 = build()
    model2.load_state_dict(live)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))  # state_dict() hands out the live momentum buffers, and load keeps them
    opt2.load_ema_state_dict(model2, sd, opt.ema_updates())
    assert opt2.ema_updates() == 3
    steps(model, opt, [4, 5])
    steps(model2, opt2, [4, 5])
    torch.cuda.synchronize()
    a, b = opt.ema_state_dict(model), opt2.ema_state_dict(model2)
    assert all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in a)
    assert opt.ema_updates() == opt2.ema_updates() == 5
    # refusals
    short = {k: v for k, v in sd.items() if k != "conv2.bias"}
    with pytest.raises(omlib.OrienMaskHipError, match="conv2.bias"):
        opt2.load_ema_state_dict(model2, short, 3)
    with pytest.raises(omlib.OrienMaskHipError, match="shape"):
        opt2.load_ema_state_dict(model2, dict(sd, **{"conv1.weight": torch.zeros(1, device=dev)}), 3)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------
HIP = dict(backend="hip", conv_backend="hip", conv_forward="hip", route_backend="hip")


class _Scalars:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), step))


def test_trainer_validates_and_checkpoints_the_averaged_weights(dev, tmp_path):
    from orienmask_amd import builder, train
    from orienmask_amd.tester import SyntheticLossLoader
    from orienmask_amd.trainer import Trainer
    config = dict(n_gpu=1, accumulate=1, epochs=1, val_freq=1, save_freq=1, monitor="loss", monitor_mode="off", log_freq=2,
                  log_dir=str(tmp_path), name="ema",
                  model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=cases.NUM_CLASSES, **HIP),
                  loss=dict(type="OrienMaskYOLOMultiScaleLoss", **cases.loss_kwargs()),
                  optimizer=dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4, ema_decay=0.9, ema_warmup=False),
                  lr_scheduler=dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=2, warmup_ratio=0.1, milestones=[4], gamma=0.5))
    kw = dict(size=(cases.IMAGE, cases.IMAGE), gts_per_image=cases.GTS_PER_IMAGE, num_classes=cases.NUM_CLASSES, device=dev)

    def make(resume=None):
        torch.manual_seed(7)
        model = builder.build(config["model"], train).to(dev)
        loss = builder.build(config["loss"], train)
        optimizer = builder.build_optimizer(config["optimizer"], config["accumulate"], model)
        scheduler = builder.build(config["lr_scheduler"], O, optimizer=optimizer)
        loaders = SyntheticLossLoader(4, cases.BATCH, seed=0, **kw), SyntheticLossLoader(2, cases.BATCH, seed=50, **kw)
        return Trainer(model, loss, optimizer, scheduler, config, *loaders, lambda predict: None, dev,
                       types.SimpleNamespace(resume=resume, weights=None))

    t = make()
    t.tensorboard = _Scalars()
    t._log_result = lambda result: None
    watched = [(k, p) for k, p in t.model.named_parameters() if p.requires_grad][:3]
    seen = []
    t.model.register_forward_pre_hook(lambda m, a: None if m.training else seen.append([p.detach().clone() for _, p in watched]))
    t.train()
    torch.cuda.synchronize()
    steps = len(t.train_loader)
    assert t.optimizer.ema_updates() == steps and len(seen) == len(t.val_loader)
    sd = t.optimizer.ema_state_dict(t.model)
    for at_val in seen:                                     # validation ran on the averaged weights ...
        for (k, p), v in zip(watched, at_val):
            assert torch.equal(v, sd[k]) and not torch.equal(v, p.detach()), k
    ck = torch.load(os.path.join(t.checkpoint_dir, "epoch1.pth"), map_location=dev, weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "lr_scheduler", "monitor_best", "config", "ema"}
    live = t.model.state_dict()
    assert all(torch.equal(ck["state_dict"][k], live[k]) for k in live)                 # ... and the parameters came back
    assert ck["ema"]["updates"] == steps and all(torch.equal(ck["ema"]["state_dict"][k], sd[k]) for k in sd)
    assert ("train/ema_updates", 2.0, 2) in t.tensorboard.rows
    # the checkpoint's entry reloads
    again = make(resume=os.path.join(t.checkpoint_dir, "epoch1.pth"))
    assert again.start_epoch == 2 and again.optimizer.ema_updates() == steps
    back = again.optimizer.ema_state_dict(again.model)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
