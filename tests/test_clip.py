"""GPU tests of gradient-norm clipping inside the HIP SGD step (om_sgd_clip_step, csrc/optim.hip;
orienmask_amd.optim.SGD(max_grad_norm=..., nonfinite=...)).  Every comparison is BIT FOR BIT (NaN equal to NaN) against
tests/clip_np.py -- which tests/test_clip_cpu.py ties to torch's clip_grads_with_norm_ + SGD.step() on the CPU: parameters and momentum
buffers after every step, and the float32 ``last_norm`` / ``last_coef`` of ``grad_norm_stats()``."""
import types

import numpy as np
import pytest
import torch

import clip_np as C
import optim_np as N
import train_step as T
from orienmask_amd import builder, lib as omlib
from orienmask_amd import optim as O
from optim_harness import dev, _param, _np, _set_grads  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32
HYPER = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)


def _hyper_of(group):
    return dict(lr=group["lr"], weight_decay=group["weight_decay"], momentum=group["momentum"], dampening=group["dampening"],
                nesterov=group["nesterov"], maximize=group["maximize"])


def _assert_state(opt, params, want_p, want_buf, what):
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        assert N.same_bits(_np(p), np.asarray(want_p[i]).reshape(-1)), (what, "param", i, tuple(p.shape))
        buf = opt.state[p].get("momentum_buffer") if p in opt.state else None
        if want_buf[i] is None:
            # no applied step yet: no buffer, or (nonfinite="skip") the zeros it was allocated with
            assert buf is None or not _np(buf).view(np.uint32).any(), (what, "buffer before any applied step", i)
        else:
            assert buf is not None and N.same_bits(_np(buf), np.asarray(want_buf[i]).reshape(-1)), (what, "buffer", i, tuple(p.shape))


def _drive(dev, opt, params, grads_per_step, after_step=None, what=""):
    """Steps `opt` with the given gradients (tensor, array or None) and checks parameters, buffers, last_norm and last_coef after
    every step against the yardstick.  -> (parameters, buffers, [(norm, coef, skipped)])."""
    cur = [_np(p).copy() for p in params]
    bufs = [None] * len(params)
    seen = []
    for s, grads in enumerate(grads_per_step):
        _set_grads(dev, params, grads)
        hyper = _hyper_of(opt.param_groups[0])
        assert len(opt.param_groups) == 1
        opt.step()
        stats = opt.grad_norm_stats(reset=False)
        flat = [None if p.grad is None else _np(p.grad) for p in params]
        cur, bufs, norm, coef, skipped = C.clipped_step(cur, flat, bufs, hyper, opt.max_grad_norm, opt.nonfinite)
        print(what, "step", s, "norm", float(norm), "coef", float(coef), "device", stats["last_norm"], stats["last_coef"])
        assert N.same_bits(F32(stats["last_norm"]), norm), (what, s, "norm", stats["last_norm"], float(norm))
        assert N.same_bits(F32(stats["last_coef"]), coef), (what, s, "coef", stats["last_coef"], float(coef))
        assert stats["steps"] == s + 1
        _assert_state(opt, params, cur, bufs, (what, "step", s))
        seen.append((norm, coef, skipped))
        if after_step is not None:
            after_step(s)
    return cur, bufs, seen


# ---- 1, 2: small, unaligned, missing --------------------------------------------------------------------------------------------
COUNTS = [1, 3, 18, 255, O.OM_SGD_CHUNK - 1, O.OM_SGD_CHUNK, O.OM_SGD_CHUNK + 1, 2 * O.OM_SGD_CHUNK + 3]


def _views(dev, values, offsets):
    """values[i] as a view offsets[i] elements into a fresh flat buffer (0: an aligned tensor of its own)."""
    out = []
    for v, k in zip(values, offsets):
        if k == 0:
            out.append(torch.from_numpy(v).to(dev))
        else:
            flat = torch.zeros(v.size + 8, device=dev)
            view = flat[k: k + v.size]
            view.copy_(torch.from_numpy(v))
            assert view.data_ptr() % 16 == 4 * k
            out.append(view)
    return out


def test_small_and_unaligned_tensors(dev):
    """1 ... 2 chunks + 3 elements; gradients that are views 1, 2 and 3 elements into a flat buffer; some grad None; momentum, weight
    decay, nesterov; three steps of which the first and the last are clipped and the middle one is not."""
    rs = np.random.RandomState(1)
    params = [_param(dev, rs.standard_normal(n)) for n in COUNTS]
    opt = O.SGD(params, lr=1e-2, momentum=0.9, weight_decay=5e-4, nesterov=True, max_grad_norm=5.0)
    offsets = [0, 1, 2, 3, 1, 2, 3, 1]
    steps = []
    for s, scale in enumerate((1.0, 1e-3, 0.5)):
        values = [(rs.standard_normal(n) * scale).astype(F32) for n in COUNTS]
        grads = _views(dev, values, offsets if s != 2 else [0] * len(COUNTS))
        if s == 1:
            grads[2] = grads[5] = None
        steps.append(grads)
    _, _, seen = _drive(dev, opt, params, steps, what="small")
    assert seen[0][1] < 1 and seen[1][1] == 1 and seen[2][1] < 1
    stats = opt.grad_norm_stats()
    assert stats["steps"] == 3 and stats["clipped_steps"] == 2 and stats["nonfinite_steps"] == 0 and stats["first_nonfinite_step"] == 0
    norms = [float(n) for n, _, _ in seen]
    assert stats["max_norm"] == max(norms) and abs(stats["mean_norm"] - sum(norms) / 3) <= 1e-12 * sum(norms)
    again = opt.grad_norm_stats()                          # reset=True above: the running counts start again, the last values stay
    assert again["steps"] == 0 and again["clipped_steps"] == 0 and again["last_norm"] == stats["last_norm"]


def test_alignment_does_not_change_the_norm(dev):
    """The same gradient values through aligned tensors and through views 1, 2, 3 elements into flat buffers: the same last_norm
    bits and the same parameters."""
    rs = np.random.RandomState(2)
    values = [(rs.standard_normal(n) * 0.3).astype(F32) for n in COUNTS]
    start = [rs.standard_normal(n).astype(F32) for n in COUNTS]
    results = []
    for offsets in ([0] * 8, [1, 2, 3, 1, 2, 3, 1, 2], [3, 3, 3, 3, 3, 3, 3, 3]):
        params = [_param(dev, a) for a in start]
        opt = O.SGD(params, max_grad_norm=1.0, **HYPER)
        for p, g in zip(params, _views(dev, values, offsets)):
            p.grad = g
        opt.step()
        stats = opt.grad_norm_stats()
        results.append((F32(stats["last_norm"]), F32(stats["last_coef"]), [_np(p).copy() for p in params]))
    want = C.norm_of(values)[0]
    for norm, coef, ps in results:
        assert N.same_bits(norm, want) and N.same_bits(coef, results[0][1])
        assert all(N.same_bits(a, b) for a, b in zip(ps, results[0][2]))


# ---- 3, 4: more chunks than the finish kernel has lanes, more than the grid has workgroups; the model ------------------------------
def test_more_chunks_than_lanes_and_workgroups(dev):
    rs = np.random.RandomState(3)
    counts = [2049 * O.OM_SGD_CHUNK + 5, 18, 255, 5000]
    assert O.plan_chunks(counts).shape[0] > 2048 > 256          # SGD_MAX_BLOCKS workgroups, the finish kernel's lanes
    params = [_param(dev, rs.standard_normal(n) * 0.05) for n in counts]
    opt = O.SGD(params, max_grad_norm=20.0, **HYPER)
    steps = [[(rs.standard_normal(n) * sc).astype(F32) for n in counts] for sc in (0.1, 1e-3)]
    _, _, seen = _drive(dev, opt, params, steps, what="grid")
    assert seen[0][1] < 1 and seen[1][1] == 1


def _model_shapes():
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    net = OrienMaskYOLOFPNPlus(num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False, backbone_batchnorm_eval=False)
    return [tuple(p.shape) for p in net.parameters()]


def test_model_shapes_full_size(dev):
    """The 266 tensors (63,662,063 elements) as one group, two steps, the first clipped."""
    shapes = _model_shapes()
    assert len(shapes) == 266
    rs = np.random.RandomState(5)
    params = [_param(dev, (rs.standard_normal(s) * 0.05).astype(np.float32)) for s in shapes]
    opt = O.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0)
    gen = torch.Generator(device=dev).manual_seed(9)
    steps = [[torch.randn(s, device=dev, generator=gen) * sc for s in shapes] for sc in (1e-2, 1e-4)]
    _, _, seen = _drive(dev, opt, params, steps, what="model")
    assert seen[0][1] < 1 and seen[1][1] == 1              # norms about 80 and 0.8


# ---- 5: propagate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [np.inf, np.nan], ids=["inf", "nan"])
def test_propagate_equals_the_yardstick(dev, poison):
    rs = np.random.RandomState(6)
    counts = [18, 255, 5000]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.SGD(params, max_grad_norm=1.0, **HYPER)
    steps = [[rs.standard_normal(n).astype(F32) for n in counts] for _ in range(2)]
    steps[1][1][100] = poison
    cur, _, seen = _drive(dev, opt, params, steps, what="propagate")
    assert not np.isfinite(seen[1][0]) and not seen[1][2]
    assert np.isnan(cur[1]).any()                          # Inf: coefficient 0, Inf * 0 = NaN in that element; NaN: everywhere
    if np.isnan(poison):
        assert all(np.isnan(c).all() for c in cur)
    stats = opt.grad_norm_stats()
    assert stats["nonfinite_steps"] == 1 and stats["first_nonfinite_step"] == 2 and stats["steps"] == 2


# ---- 6, 7: skip -----------------------------------------------------------------------------------------------------------------
def _bits(params, opt):
    torch.cuda.synchronize()
    return ([_np(p).view(np.uint32).copy() for p in params],
            [_np(opt.state[p]["momentum_buffer"]).view(np.uint32).copy() if "momentum_buffer" in opt.state.get(p, {}) else None
             for p in params])


def test_skip_with_a_poisoned_first_step(dev):
    """dampening 0.5: a first step that is `buf = d` differs from `buf = 0.5 d`, which a zero buffer read as a later step would give."""
    rs = np.random.RandomState(7)
    counts = [18, 255, O.OM_SGD_CHUNK + 1, 3 * O.OM_SGD_CHUNK + 7]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.SGD(params, lr=1e-2, momentum=0.9, dampening=0.5, weight_decay=5e-4, max_grad_norm=1.0, nonfinite="skip")
    steps = [[rs.standard_normal(n).astype(F32) for n in counts] for _ in range(3)]
    steps[0][3][5000] = np.nan
    before = [_np(p).view(np.uint32).copy() for p in params]
    seen_after_first = []

    def after(s):
        if s == 0:
            ps, bs = _bits(params, opt)
            assert all((a == b).all() for a, b in zip(before, ps))                 # every parameter bit-unchanged
            assert all(b is not None and not b.any() for b in bs)                  # buffers: allocated, zeros
            seen_after_first.append(1)
    cur, bufs, seen = _drive(dev, opt, params, steps, after_step=after, what="skip_first")
    assert seen_after_first and seen[0][2] and not seen[1][2] and not seen[2][2]
    # the second call was torch's FIRST step: the yardstick's buffers were None going into it, so buf = d (checked bit for bit above);
    # restated here for one tensor without the yardstick's bookkeeping
    first = N.sgd_step(_np_u32(before[0]), C.scale(steps[1][0], seen[1][1]), None, lr=1e-2, momentum=0.9, dampening=0.5,
                       weight_decay=5e-4)
    again = N.sgd_step(first[0], C.scale(steps[2][0], seen[2][1]), first[1], lr=1e-2, momentum=0.9, dampening=0.5, weight_decay=5e-4)
    assert N.same_bits(again[0], cur[0]) and N.same_bits(again[1], bufs[0])
    stats = opt.grad_norm_stats()
    assert stats["nonfinite_steps"] == 1 and stats["first_nonfinite_step"] == 1 and stats["steps"] == 3


def _np_u32(bits):
    return bits.view(np.float32)


def test_skip_with_a_poisoned_middle_step(dev):
    rs = np.random.RandomState(8)
    counts = [18, 255, O.OM_SGD_CHUNK + 1, 3 * O.OM_SGD_CHUNK + 7]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.SGD(params, lr=1e-2, momentum=0.9, weight_decay=5e-4, nesterov=True, max_grad_norm=1.0, nonfinite="skip")
    steps = [[rs.standard_normal(n).astype(F32) for n in counts] for _ in range(4)]
    steps[1][0][3] = np.inf
    steps[2][2][17] = np.nan
    held = {}

    def after(s):
        if s == 0:
            held["bits"] = _bits(params, opt)
        if s in (1, 2):
            ps, bs = _bits(params, opt)
            assert all((a == b).all() for a, b in zip(held["bits"][0], ps)) and all((a == b).all() for a, b in zip(held["bits"][1], bs))
    _, _, seen = _drive(dev, opt, params, steps, after_step=after, what="skip_middle")
    assert [k for _, _, k in seen] == [False, True, True, False]
    stats = opt.grad_norm_stats()
    assert stats["nonfinite_steps"] == 2 and stats["first_nonfinite_step"] == 2 and stats["steps"] == 4
    assert np.isinf(seen[1][0]) and np.isnan(seen[2][0]) and np.isfinite(stats["max_norm"]) and np.isfinite(stats["mean_norm"])


# ---- 8, 9: the gradient is left alone; a run repeats ----------------------------------------------------------------------------------
def test_the_gradient_is_not_modified(dev):
    rs = np.random.RandomState(9)
    counts = [18, 255, 5000, O.OM_SGD_CHUNK * 2 + 3]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.SGD(params, max_grad_norm=0.5, **HYPER)
    for p in params:
        p.grad = torch.from_numpy(rs.standard_normal(p.numel()).astype(F32)).to(dev)
    before = [_np(p.grad).view(np.uint32).copy() for p in params]
    opt.step()
    torch.cuda.synchronize()
    assert opt.grad_norm_stats()["last_coef"] < 1
    assert all((_np(p.grad).view(np.uint32) == b).all() for p, b in zip(params, before))


def test_two_runs_give_the_same_bits(dev):
    counts = [18, 255, 5000, 70001, 300 * O.OM_SGD_CHUNK + 1]
    runs = []
    for _ in range(2):
        rs = np.random.RandomState(10)
        params = [_param(dev, rs.standard_normal(n)) for n in counts]
        opt = O.SGD(params, max_grad_norm=2.0, nonfinite="skip", **HYPER)
        norms = []
        for s in range(3):
            for p in params:
                p.grad = torch.from_numpy((rs.standard_normal(p.numel()) * (1e-3 if s == 1 else 1.0)).astype(F32)).to(dev)
            opt.step()
            st = opt.grad_norm_stats(reset=False)
            norms.append((F32(st["last_norm"]).view(np.uint32), F32(st["last_coef"]).view(np.uint32)))
        runs.append((norms, _bits(params, opt)))
    (na, (pa, ba)), (nb, (pb, bb)) = runs
    assert na == nb and all((x == y).all() for x, y in zip(pa, pb)) and all((x == y).all() for x, y in zip(ba, bb))


# ---- 10: no synchronisation, no allocation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonfinite", ["propagate", "skip"])
def test_clipped_step_neither_synchronises_nor_allocates(dev, monkeypatch, nonfinite):
    """After the first step, six clipped steps with a scheduler and zero_grad(set_to_none=True) make no device-to-host copy, no
    synchronisation and no allocation: torch's sync debug mode "error" around them (probed with an .item() that has to raise; where
    the build does not honour the mode that is printed and the counters hold), and counted .item() / .cpu() / .tolist() / .numpy() /
    synchronize calls."""
    rs = np.random.RandomState(4)
    counts = [18, 255, 4096, 100003]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.SGD(params, max_grad_norm=1.0, nonfinite=nonfinite, **HYPER)
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
    probe = torch.ones(1, device=dev)
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            honoured = False
            probe.item()
        except RuntimeError:
            honoured = True
        calls.clear()
        for s in range(1, 7):
            for p, g in zip(params, grads[s]):
                p.grad = g
            opt.step()
            sch.step()
            opt.zero_grad(set_to_none=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode honoured on this build:", honoured)
    assert calls == [], calls
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before
    monkeypatch.undo()
    stats = opt.grad_norm_stats()
    assert stats["steps"] == 7 and stats["clipped_steps"] == 7 and stats["nonfinite_steps"] == 0


def test_refusals_on_the_device(dev):
    p = _param(dev, np.ones(8))
    with pytest.raises(ValueError, match="max_grad_norm"):
        O.SGD([p], lr=0.1, max_grad_norm=0.0)
    with pytest.raises(omlib.OrienMaskHipError, match="tensor"):
        O.SGD([p], lr=0.1, max_grad_norm=torch.tensor(1.0, device=dev))
    with pytest.raises(ValueError, match="nonfinite"):
        O.SGD([p], lr=0.1, max_grad_norm=1.0, nonfinite="ignore")
    # no gradient anywhere: nothing is launched and nothing is counted
    opt = O.SGD([p], lr=0.1, momentum=0.9, max_grad_norm=1.0, nonfinite="skip")
    opt.step()
    assert opt.grad_norm_stats()["steps"] == 0 and torch.equal(p.detach().cpu(), torch.ones(8))
    # max_grad_norm=None is the plain step: the yardstick of tests/test_optim.py
    q = _param(dev, np.arange(8))
    plain = O.SGD([q], lr=0.5)
    q.grad = torch.ones_like(q)
    plain.step()
    torch.cuda.synchronize()
    assert plain._clip_state is None and torch.equal(q.detach().cpu(), torch.arange(8.0) - 0.5)


# ---- 11: the trainer ------------------------------------------------------------------------------------------------------------
HIP = dict(backend="hip", conv_backend="hip", conv_forward="hip", route_backend="hip")


class _Scalars:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), step))


def _trainer_run(dev, tmp_path, name, optimizer_cfg, poison_first):
    """trainer.Trainer on the 96 x 96 harness of tests/train_step.py (FPN-Plus, HIP backends, the HIP loss, B = 2): four batches,
    one optimizer step each, the counter read every second step.  poison_first: the first batch's image is NaN."""
    from orienmask_amd import train
    from orienmask_amd.tester import SyntheticLossLoader
    from orienmask_amd.trainer import Trainer
    h = w = 96
    config = dict(n_gpu=1, accumulate=1, epochs=1, val_freq=1, save_freq=5, monitor="loss", monitor_mode="off", log_freq=2,
                  log_dir=str(tmp_path), name=name,
                  model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False,
                             backbone_batchnorm_eval=False, **HIP),
                  loss=T.loss_cfg(h, w), optimizer=optimizer_cfg,
                  lr_scheduler=dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=2, warmup_ratio=0.1, milestones=[8]))
    torch.manual_seed(3)
    with torch.cuda.device(dev):
        model = builder.build_train_model(config["model"])
    loss = builder.build(config["loss"], train)
    optimizer = builder.build_optimizer(config["optimizer"], 1, model)
    scheduler = builder.build(config["lr_scheduler"], O, optimizer=optimizer)
    loader = SyntheticLossLoader(8, 2, size=(h, w), seed=0, gts_per_image=6, num_classes=80, device=dev)
    if poison_first:
        image, target, info = loader._batches[0]
        loader._batches[0] = (torch.full_like(image, float("nan")), target, info)
    t = Trainer(model, loss, optimizer, scheduler, config, loader, None, None, dev, types.SimpleNamespace(resume=None, weights=None))
    assert t.sync_free
    t.tensorboard = _Scalars()
    return t


def test_trainer_writes_the_four_scalars(dev, tmp_path):
    opt_cfg = dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=1.0, nonfinite="skip")
    t = _trainer_run(dev, tmp_path, "clip", opt_cfg, poison_first=False)
    t.train()
    rows = t.tensorboard.rows
    tags = [tag for tag, _, _ in rows]
    for tag in ("train/grad_norm", "train/grad_norm_max", "train/clipped_steps", "train/skipped_steps"):
        assert tags.count(tag) == 2, (tag, tags)                            # the reads at steps 2 and 4
    by = {(tag, at): v for tag, v, at in rows}
    for at in (2, 4):
        assert 0 < by[("train/grad_norm", at)] <= by[("train/grad_norm_max", at)] < float("inf")
        assert by[("train/skipped_steps", at)] == 0 and by[("train/clipped_steps", at)] in (0, 1, 2)
    # without clipping the scalars are today's
    plain = _trainer_run(dev, tmp_path, "plain", dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), poison_first=False)
    plain.train()
    assert not [tag for tag, _, _ in plain.tensorboard.rows if "grad_norm" in tag or "_steps" in tag]
    assert [tag for tag in tags if "grad_norm" not in tag and "_steps" not in tag] == [tag for tag, _, _ in plain.tensorboard.rows]


def test_trainer_skip_keeps_the_last_finite_parameters(dev, tmp_path):
    """A NaN batch at step 1, noticed at the read of step 2: with nonfinite="skip" the run ends in the trainer's FloatingPointError
    with every parameter finite, and the message says so; with "propagate" the same run ends with NaN parameters."""
    base = dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=1.0)
    t = _trainer_run(dev, tmp_path, "skip", dict(base, nonfinite="skip"), poison_first=True)
    with pytest.raises(FloatingPointError) as err:
        t.train()
    print(err.value)
    assert "last finite state" in str(err.value) and "first at its step 1" in str(err.value) and "epoch 1 batch 1" in str(err.value)
    assert all(torch.isfinite(p).all() for p in t.model.parameters())
    stats = t.optimizer.grad_norm_stats()
    assert stats["first_nonfinite_step"] == 1 and stats["nonfinite_steps"] == 1 and stats["steps"] == 2
    u = _trainer_run(dev, tmp_path, "propagate", dict(base, nonfinite="propagate"), poison_first=True)
    with pytest.raises(FloatingPointError) as err:
        u.train()
    assert "last finite state" not in str(err.value)
    assert any(torch.isnan(p).any() for p in u.model.parameters())
