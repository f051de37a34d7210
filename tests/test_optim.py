"""GPU tests of the optimizer step (om_sgd_step, csrc/optim.hip; orienmask_amd.optim.SGD).  Every comparison is BIT FOR BIT
(NaN equal to NaN) against tests/optim_np.py -- torch.optim.SGD's update with a true single rounding per fused multiply-add -- and,
where recorded, the fixtures tests/golden/optim_sgd_*.npz (what torch.optim.SGD on CPU produced), for parameters and momentum
buffers after every step."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import optim_np as N
import train_step as T
from orienmask_amd import builder, lib as omlib
from orienmask_amd import optim as O
from optim_harness import dev, _param, _np, _np_grad, _set_grads  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu


def _hyper_of(group):
    return dict(lr=group["lr"], weight_decay=group["weight_decay"], momentum=group["momentum"], dampening=group["dampening"],
                nesterov=group["nesterov"], maximize=group["maximize"])


def _assert_state(opt, params, want_p, want_buf, what):
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        assert N.same_bits(_np(p), np.asarray(want_p[i]).reshape(-1)), (what, "param", i, tuple(p.shape))
        buf = opt.state[p].get("momentum_buffer") if p in opt.state else None
        if want_buf[i] is None:
            assert buf is None, (what, "buffer", i)
        else:
            assert buf is not None and N.same_bits(_np(buf), np.asarray(want_buf[i]).reshape(-1)), (what, "buffer", i, tuple(p.shape))


def _drive(dev, opt, params, grads_per_step, after_step=None, what=""):
    """Steps `opt` with the given gradients (None: no gradient) and checks parameters and buffers after every step against the
    numpy yardstick driven with the hyper-parameters the optimizer holds at that step."""
    group_of = {}
    for g in opt.param_groups:
        for p in g["params"]:
            group_of[id(p)] = g
    cur = [_np(p).copy() for p in params]
    bufs = [None] * len(params)
    for s, grads in enumerate(grads_per_step):
        _set_grads(dev, params, grads)
        hypers = [_hyper_of(group_of[id(p)]) for p in params]
        opt.step()
        flat = [None if p.grad is None else _np_grad(p) for p in params]
        cur, bufs = N.sgd_step_many(cur, flat, bufs, hypers)
        _assert_state(opt, params, cur, bufs, (what, "step", s))
        if after_step is not None:
            after_step(s)
    return cur, bufs


# ---- hyper-parameter sets, fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(N.HYPER_SETS) + ["specials"])
def test_fixture_sets_first_and_later_steps(dev, name):
    """Each hyper-parameter set (and the zeros / denormals / +-Inf / NaN inputs): first step and later steps against the recorded
    torch-CPU results (c) and the numpy yardstick (b)."""
    g = np.load(os.path.join(GOLDEN, "optim_sgd_%s.npz" % name))
    hyper = json.loads(bytes(g["hyper"]).decode())
    p = _param(dev, g["p0"])
    opt = O.SGD([p], **hyper)
    want = N.numpy_run(g["p0"], list(g["grads"]), hyper)
    for s in range(g["grads"].shape[0]):
        p.grad = torch.from_numpy(g["grads"][s]).to(dev)
        opt.step()
        torch.cuda.synchronize()
        buf = opt.state[p].get("momentum_buffer") if p in opt.state else None
        assert N.same_bits(_np(p), want[s][0]), (name, s, "param vs numpy")
        assert N.same_bits(_np(p), g["param"][s]), (name, s, "param vs fixture")
        if "buf" in g.files:
            assert N.same_bits(_np(buf), want[s][1]) and N.same_bits(_np(buf), g["buf"][s]), (name, s, "buffer")
        else:
            assert buf is None
        if name == "specials" and s == 0:
            assert np.isnan(_np(p)).any() and np.isinf(_np(p)).any()       # they propagate (later steps turn Inf - Inf into NaN)


# ---- the model's 266 shapes at full size ----------------------------------------------------------------------------------------
def _model_counts_and_groups():
    from orienmask_amd.model import OrienMaskYOLOFPNPlus
    net = OrienMaskYOLOFPNPlus(num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False, backbone_batchnorm_eval=False)
    plist = list(net.parameters())
    for p in plist:
        p.requires_grad_(True)                              # the inference model holds its weights frozen
    index = {id(p): i for i, p in enumerate(plist)}
    groups = O.param_groups(net, base_lr=1e-3, weight_decay=5e-4, norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4)
    split = [None] * len(plist)
    for g in groups:
        split[index[id(g["params"][0])]] = (g["lr"], g["weight_decay"])
    return [tuple(p.shape) for p in plist], split


@pytest.mark.parametrize("grouping", ["one_group", "per_tensor_groups"])
def test_model_shapes_full_size(dev, grouping):
    """The 266 tensors (63,662,063 elements, 18 to 4,718,592 each), three steps with a scheduler step between optimizer steps:
    as one group, and as 266 groups with the lr / decay split of param_groups."""
    shapes, split = _model_counts_and_groups()
    assert len(shapes) == 266 and all(s is not None for s in split)
    rs = np.random.RandomState(5)
    params = [_param(dev, (rs.standard_normal(s) * 0.05).astype(np.float32)) for s in shapes]
    if grouping == "one_group":
        opt = O.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4)
    else:
        opt = O.SGD([{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(params, split)], lr=1e-3, momentum=0.9,
                    weight_decay=5e-4)
        assert len(opt.param_groups) == 266 and len({(g["lr"], g["weight_decay"]) for g in opt.param_groups}) >= 3
    sch = O.StepWarmUpLR("linear", 2, 0.1, opt, [3], 0.1)
    lrs = []

    def after(step):
        lrs.append(opt.param_groups[0]["lr"])
        sch.step()
    gen = torch.Generator(device=dev).manual_seed(9)
    steps = [[torch.randn(s, device=dev, generator=gen) * (10.0 ** float(rs.uniform(-3, 0))) for s in shapes] for _ in range(3)]
    _drive(dev, opt, params, steps, after_step=after, what=grouping)
    assert len(set(lrs)) == 3                               # every step ran at another learning rate


# ---- small, unaligned, strided, missing -----------------------------------------------------------------------------------------
def test_small_and_unaligned_tensors(dev):
    """1, 3, 18 and 255 elements; one chunk +- 1; views one, two and three elements into a flat buffer for the parameter, the
    gradient or the momentum buffer, each alone; parameters without a gradient."""
    rs = np.random.RandomState(1)
    c = O.OM_SGD_CHUNK
    counts = [1, 3, 18, 255, c - 1, c, c + 1, 2 * c + 3, 1001, 1002, 1003]
    flat = torch.from_numpy(rs.standard_normal(40000).astype(np.float32)).to(dev)
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    off = 0
    for k in (1, 2, 3):                                    # parameters that are views k elements into a flat buffer
        n = 1000 + k
        params.append(torch.nn.Parameter(flat[off + k: off + k + n]))
        assert params[-1].data_ptr() % 16 == 4 * k
        off += 2048
    opt = O.SGD(params, lr=1e-2, momentum=0.9, weight_decay=5e-4, nesterov=True)
    gflat = torch.from_numpy(rs.standard_normal(40000).astype(np.float32)).to(dev)

    def grads(step):
        out = []
        for i, p in enumerate(params):
            if step == 1 and i % 4 == 1:
                out.append(None)                            # some grad is None
            elif i in (8, 9, 10):                           # an aligned parameter with a gradient 1, 2, 3 elements into a flat buffer
                k = i - 7
                g = gflat[4096 * k + k: 4096 * k + k + p.numel()]
                assert g.data_ptr() % 16 == 4 * k and p.data_ptr() % 16 == 0
                out.append(g)
            else:
                out.append(torch.from_numpy(rs.standard_normal(p.numel()).astype(np.float32)).to(dev))
        return out
    cur, bufs = _drive(dev, opt, params, [grads(0)], what="first")
    # momentum buffers that are views 1, 2, 3 elements into a flat buffer, alone (parameter and gradient aligned)
    for k, i in ((1, 4), (2, 5), (3, 6)):
        p = params[i]
        view = torch.zeros(p.numel() + 8, device=dev)[k: k + p.numel()]
        view.copy_(opt.state[p]["momentum_buffer"])
        opt.state[p]["momentum_buffer"] = view
        assert view.data_ptr() % 16 == 4 * k and p.data_ptr() % 16 == 0
    for s in (1, 2):
        gs = grads(s)
        for p, g in zip(params, gs):
            p.grad = g
        hyp = _hyper_of(opt.param_groups[0])
        opt.step()
        cur, bufs = N.sgd_step_many(cur, [None if g is None else _np(g) for g in gs], bufs, hyp)
        _assert_state(opt, params, cur, bufs, ("later", s))
    for k, i in ((1, 4), (2, 5), (3, 6)):
        assert opt.state[params[i]]["momentum_buffer"].data_ptr() % 16 == 4 * k      # still the caller's views


def test_channels_last_weight_and_strided_gradient(dev):
    """A channels_last weight is updated in storage order; a gradient whose strides differ from its parameter's is brought to the
    parameter's layout first."""
    rs = np.random.RandomState(2)
    w = torch.from_numpy(rs.standard_normal((16, 8, 3, 3)).astype(np.float32)).to(dev)
    p_cl = torch.nn.Parameter(w.contiguous(memory_format=torch.channels_last))
    p_ct = torch.nn.Parameter(w.clone())
    assert p_cl.stride() != p_ct.stride()
    opt = O.SGD([p_cl, p_ct], lr=1e-2, momentum=0.9, weight_decay=5e-4)
    ref = torch.optim.SGD([torch.nn.Parameter(w.cpu().clone())], lr=1e-2, momentum=0.9, weight_decay=5e-4)
    for s in range(3):
        g = torch.from_numpy(rs.standard_normal((16, 8, 3, 3)).astype(np.float32)).to(dev)
        p_cl.grad = g.clone()                               # contiguous gradient for a channels_last parameter
        p_ct.grad = g.contiguous(memory_format=torch.channels_last)
        ref.param_groups[0]["params"][0].grad = g.cpu()
        opt.step()
        ref.step()
        torch.cuda.synchronize()
        want = ref.param_groups[0]["params"][0].detach()
        assert p_cl.stride() == w.contiguous(memory_format=torch.channels_last).stride()
        assert torch.equal(p_cl.detach().cpu(), want) and torch.equal(p_ct.detach().cpu(), want), s
        wb = ref.state[ref.param_groups[0]["params"][0]]["momentum_buffer"]
        assert torch.equal(opt.state[p_cl]["momentum_buffer"].cpu(), wb) and torch.equal(opt.state[p_ct]["momentum_buffer"].cpu(), wb)
        assert opt.state[p_cl]["momentum_buffer"].stride() == p_cl.stride()


# ---- streams, synchronisation, allocation ---------------------------------------------------------------------------------------
def test_non_default_stream(dev):
    rs = np.random.RandomState(3)
    counts = [18, 255, 5000, 70001]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.SGD(params, lr=1e-2, momentum=0.9, weight_decay=5e-4)
    cur, bufs = [_np(p).copy() for p in params], [None] * len(params)
    stream = torch.cuda.Stream(dev)
    for s in range(6):                                     # more steps than staging buffers
        gs = [rs.standard_normal(n).astype(np.float32) for n in counts]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for p, g in zip(params, gs):
                p.grad = torch.from_numpy(g).to(dev, non_blocking=False)
            opt.step()
        stream.synchronize()
        cur, bufs = N.sgd_step_many(cur, gs, bufs, _hyper_of(opt.param_groups[0]))
        _assert_state(opt, params, cur, bufs, ("stream", s))


def test_step_neither_synchronises_nor_allocates(dev, monkeypatch):
    """After a tensor's first step, step() makes no device-to-host copy, no synchronisation and no allocation.  Checked twice:
    torch's sync debug mode "error" around step() -- if this torch build does not honour the mode on ROCm (probed here with an
    .item() that has to raise; torch 2.10 on ROCm 7 does honour it), that is printed and the patched counters below are what holds --
    and by counting .item() /
    .cpu() / .tolist() / synchronize calls through patches."""
    rs = np.random.RandomState(4)
    counts = [18, 255, 4096, 100003]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.SGD(params, lr=1e-2, momentum=0.9, weight_decay=5e-4)
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


def test_steps_behind_the_sync_check_are_right(dev):
    """The same drive as the synchronisation test (scheduler between steps, zero_grad(set_to_none=True)) against the yardstick."""
    rs = np.random.RandomState(4)
    counts = [18, 255, 4096, 100003]
    params = [_param(dev, rs.standard_normal(n)) for n in counts]
    opt = O.SGD(params, lr=1e-2, momentum=0.9, weight_decay=5e-4)
    sch = O.StepWarmUpLR("linear", 3, 0.1, opt, [5], 0.1)

    def after(step):
        sch.step()
        opt.zero_grad(set_to_none=True)
    _drive(dev, opt, params, [[rs.standard_normal(n).astype(np.float32) for n in counts] for _ in range(7)], after_step=after)


# ---- state interchange ----------------------------------------------------------------------------------------------------------
def test_resume_from_torch_sgd_state(dev):
    """load_state_dict of a state torch.optim.SGD produced (what the reference's trainer checkpoints), then two more steps equal to
    torch continuing; and the state written here loads back into torch.optim.SGD."""
    rs = np.random.RandomState(6)
    counts = [18, 255, 9001]
    hyper = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4, nesterov=True)
    cpu = [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(n).astype(np.float32))) for n in counts]
    ref = torch.optim.SGD([{"params": cpu[:1], "lr": 2e-2, "weight_decay": 0.0}, {"params": cpu[1:]}], **hyper)
    grads = [[torch.from_numpy(rs.standard_normal(n).astype(np.float32)) for n in counts] for _ in range(4)]
    for s in range(2):
        for p, g in zip(cpu, grads[s]):
            p.grad = g.clone()
        ref.step()
    params = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in cpu]
    opt = O.SGD([{"params": params[:1]}, {"params": params[1:]}], lr=1.0)
    opt.load_state_dict(ref.state_dict())
    assert opt.param_groups[0]["lr"] == 2e-2 and opt.param_groups[1]["nesterov"] is True
    assert all(opt.state[p]["momentum_buffer"].is_cuda for p in params)
    for s in (2, 3):
        for p, q, g in zip(cpu, params, grads[s]):
            p.grad = g.clone()
            q.grad = g.to(dev)
        ref.step()
        opt.step()
        torch.cuda.synchronize()
        for p, q in zip(cpu, params):
            assert torch.equal(q.detach().cpu(), p.detach()), s
            assert torch.equal(opt.state[q]["momentum_buffer"].cpu(), ref.state[p]["momentum_buffer"]), s
    back = torch.optim.SGD([{"params": cpu[:1]}, {"params": cpu[1:]}], lr=1.0)
    back.load_state_dict(opt.state_dict())
    for p, q in zip(cpu, params):
        assert torch.equal(back.state[p]["momentum_buffer"], opt.state[q]["momentum_buffer"].cpu())


def test_closure_and_refusals(dev):
    p = _param(dev, np.ones(10))
    opt = O.SGD([p], lr=0.5)
    seen = []

    def closure():
        assert torch.is_grad_enabled()
        loss = (p * p).sum()
        opt.zero_grad()
        loss.backward()
        seen.append(1)
        return loss
    loss = opt.step(closure)
    torch.cuda.synchronize()
    assert seen == [1] and float(loss) == 10.0 and torch.equal(p.detach().cpu(), torch.zeros(10))       # 1 - 0.5 * 2
    # sparse gradients
    emb = torch.nn.Embedding(8, 4, sparse=True).to(dev)
    sopt = O.SGD(emb.parameters(), lr=0.1)
    emb(torch.tensor([1, 3], device=dev)).sum().backward()
    with pytest.raises(omlib.OrienMaskHipError, match="sparse"):
        sopt.step()
    # a tensor learning rate
    q = _param(dev, np.ones(4))
    topt = O.SGD([q], lr=0.1)
    topt.param_groups[0]["lr"] = torch.tensor(0.1, device=dev)
    q.grad = torch.ones_like(q)
    with pytest.raises(omlib.OrienMaskHipError, match="tensor"):
        topt.step()
    with pytest.raises(omlib.OrienMaskHipError):
        O.SGD([torch.nn.Parameter(torch.ones(4, device=dev, dtype=torch.float16))], lr=0.1)
    with pytest.raises(omlib.OrienMaskHipError):
        O.SGD([torch.nn.Parameter(torch.ones(4, 6, device=dev)[:, ::2])], lr=0.1)
    with pytest.raises(omlib.OrienMaskHipError, match="differentiable"):
        O.SGD([_param(dev, np.ones(4))], lr=0.1, differentiable=True)
    # no gradient anywhere: nothing to do, nothing launched
    r = _param(dev, np.ones(4))
    O.SGD([r], lr=0.1, momentum=0.9).step()
    torch.cuda.synchronize()
    assert torch.equal(r.detach().cpu(), torch.ones(4))


# ---- the three swapped pieces in one training step ------------------------------------------------------------------------------
class _Heads(torch.nn.Module):
    """A small torch network that produces the three scales' heads at 96 x 96 (the network's own backward is torch's)."""

    def __init__(self, C=80):
        super().__init__()
        torch.manual_seed(1)
        self.stem = torch.nn.Conv2d(3, 8, 3, padding=1, bias=False)
        self.bn = torch.nn.BatchNorm2d(8)
        self.box = torch.nn.ModuleList([torch.nn.Conv2d(8, 3 * (5 + C), 1) for _ in range(3)])
        self.orien = torch.nn.ModuleList([torch.nn.Conv2d(8, 6, 1) for _ in range(3)])

    def forward(self, x):
        f = torch.relu(self.bn(self.stem(x)))
        q = torch.nn.functional.avg_pool2d(f, 4)
        return [(self.box[s](torch.nn.functional.avg_pool2d(f, k)) - 2.0, self.orien[s](q)) for s, k in enumerate((32, 16, 8))]


def test_training_step_with_hip_loss_and_optimizer(dev):
    """loss.backward() through orienmask_amd.train's loss on a small torch head, then build_optimizer's SGD (with the param_groups
    split) and StepWarmUpLR from config dicts: the step applied to those gradients is the yardstick's, for two iterations."""
    from orienmask_amd import synth, train
    h = w = 96
    net = _Heads().to(dev)
    loss_fn = builder.build(T.loss_cfg(h, w), train)
    opt_cfg = dict(type="SGD", lr=4e-3, momentum=0.9, weight_decay=5e-4,
                   param_groups=dict(norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4))
    optimizer = builder.build_optimizer(opt_cfg, 2, net)
    assert type(optimizer) is O.SGD and len(optimizer.param_groups) == len(list(net.parameters()))
    scheduler = builder.build(dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=4, warmup_ratio=0.1, milestones=[6, 8]),
                              O, optimizer=optimizer)
    params = [g["params"][0] for g in optimizer.param_groups]
    target = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.synth_targets(51, 2, h, w, 6))
    cur, bufs = [_np(p).copy() for p in params], [None] * len(params)
    for it in range(2):
        x = torch.from_numpy(np.random.default_rng(it).standard_normal((2, 3, h, w)).astype(np.float32)).to(dev)
        loss, _, _ = loss_fn(net(x), target, training=True)
        loss.backward()
        grads = [_np_grad(p) for p in params]
        assert all(np.isfinite(g).all() for g in grads)
        assert sum(bool(np.abs(g).max() > 0) for g in grads) > len(grads) // 2      # (a scale without a positive has zero head gradients)
        hypers = [_hyper_of(g) for g in optimizer.param_groups]
        optimizer.step()
        scheduler.step()
        optimizer.zero_grad()
        cur, bufs = N.sgd_step_many(cur, grads, bufs, hypers)
        _assert_state(optimizer, params, cur, bufs, ("train", it))
