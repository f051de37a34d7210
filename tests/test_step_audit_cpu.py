"""CPU tests of the step audit's own parts (tests/loss_f64.py, tests/step_audit.py): the differentiable loss against the
restatements, the closed-form schedule against the recorded one, the written-out updates against torch's optimizers, and the
teeth of the judgement: with a small torch model and the float32 CPU transition in the kernels' place, step_audit.judge passes
the honest transition and rejects every planted fault (step_audit.FAULTS) by at least twice its bar."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_files
import loss_f64
import loss_grad_np
import optim_np
import step_audit as A
import train_step as T
from test_loss_grad import _random_case
from orienmask_amd import synth

UNIT = 2.0 ** -24
# The float32 rounding LossNP / LossGradNP carry, in units of 2^-24 of the compared tensor's scale.
# Values: a term is a float64 sum rounded to float32, divided by B and multiplied by its weight in float32 (1.5 units), of
# elements whose logarithm (half a unit of the element) and whose sigmoid (half a unit, through t / p - (1 - t) / (1 - p)) are
# rounded: 8 units of the term cover it with a factor of about two to spare.
# Gradients: the sigmoid's half unit reaches d (p - t) as at most d 2^-25, half a unit of a head whose largest entry is d;
# objectness adds its positive and negative route; the orientation head's up-sample is three float32 roundings into 16 taps:
# 4 units of max|g|.
VALUE_UNITS, GRAD_UNITS = 8.0, 4.0

LOSS_CASES = [("fixture", n) for n in golden_files("grad_loss_")] + [("seed", s) for s in range(8)]


def _loss_case(kind, which):
    if kind == "fixture":
        g, cfg, heads, target, gout = loss_grad_np.load_grad_fixture(os.path.join(GOLDEN, which))
        return cfg, heads, target, gout, float(g["loss_sum"])
    cfg, heads, target = _random_case(which)
    return cfg, heads, target, 1.25, None


@pytest.mark.parametrize("kind,which", LOSS_CASES, ids=lambda v: str(v))
def test_loss_f64_equals_the_restatements(kind, which):
    cfg, heads, target, gout, recorded = _loss_case(kind, which)
    as_np = [(b.numpy(), o.numpy()) for b, o in heads]
    with A.cpu_threads():
        forced = loss_f64.forced_targets(cfg, as_np, target)
        leaves = [(b.double().requires_grad_(), o.double().requires_grad_()) for b, o in heads]
        total, terms = loss_f64.loss(cfg, leaves, forced)
        grads = torch.autograd.grad(total * gout, [t for pair in leaves for t in pair])
    ln = loss_grad_np.LossGradNP(**cfg)
    values = ln(as_np, target)
    want = ln.grad(as_np, target, gout)
    if recorded is not None:
        assert abs(float(total.detach()) - recorded) <= VALUE_UNITS * UNIT * abs(recorded)
    worst_v = worst_g = 0.0
    for s in range(len(heads)):
        w = values[s][0].astype(np.float64)
        d = np.abs(terms[s].numpy() - w)
        assert ((w == 0) == (terms[s].numpy() == 0)).all()
        worst_v = max(worst_v, float((d / np.maximum(np.abs(w), 1e-300)).max()) / UNIT)
        for g, r in zip((grads[2 * s], grads[2 * s + 1]), want[s][:2]):
            scale = float(np.abs(r).max())
            if scale == 0.0:
                assert float(g.abs().max()) == 0.0
                continue
            worst_g = max(worst_g, float(np.abs(g.numpy() - r).max()) / scale / UNIT)
    print("%s %s: values %.2f units of 2^-24 (bound %g), gradients %.2f (bound %g)" % (kind, which, worst_v, VALUE_UNITS, worst_g,
                                                                                      GRAD_UNITS))
    assert worst_v <= VALUE_UNITS and worst_g <= GRAD_UNITS


def test_loss_f64_in_float32_is_the_same_function():
    """The float32 evaluation (the yardstick's) stays within float32 rounding of the float64 one: same code, another dtype."""
    cfg, heads, target, _, _ = _loss_case("seed", 5)
    forced = loss_f64.forced_targets(cfg, [(b.numpy(), o.numpy()) for b, o in heads], target)
    a, _ = loss_f64.loss(cfg, [(b.double(), o.double()) for b, o in heads], forced)
    b, _ = loss_f64.loss(cfg, heads, forced)
    assert b.dtype == torch.float32 and abs(float(a) - float(b)) <= 64 * UNIT * abs(float(a))


def test_closed_form_schedule_equals_the_recorded_one():
    g = np.load(os.path.join(GOLDEN, "optim_lr_schedules.npz"))
    for name, case in optim_np.STEP_WARMUP_CASES.items():
        sched = dict(type="StepWarmUpLR", **case)
        got = [[A.lr_at(sched, k, base) for base in optim_np.SCHEDULE_BASE_LRS] for k in range(optim_np.STEP_WARMUP_ITERS + 1)]
        assert np.array_equal(np.asarray(got, np.float64), g["step_" + name]), name
    sched = dict(type="PolyLR", **optim_np.POLY_CASE)
    got = [[A.lr_at(sched, k, base) for base in optim_np.SCHEDULE_BASE_LRS] for k in range(optim_np.POLY_ITERS + 1)]
    assert np.array_equal(np.asarray(got, np.float64), g["poly"])


# ---- the written-out updates against torch's --------------------------------------------------------------------------------------
GROUPS = dict(norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4)
TORCH_CASES = {
    "sgd": (dict(type="SGD", lr=0.05, momentum=0.9, weight_decay=5e-4, max_grad_norm=0.5), torch.optim.SGD),
    "sgd-nesterov-groups": (dict(type="SGD", lr=0.05, momentum=0.9, weight_decay=5e-4, nesterov=True, param_groups=GROUPS),
                            torch.optim.SGD),
    "adam-groups": (dict(type="HipAdam", lr=1e-3, weight_decay=5e-4, max_grad_norm=0.5, param_groups=GROUPS), torch.optim.Adam),
    "adamw": (dict(type="HipAdamW", lr=1e-3, weight_decay=1e-2, betas=(0.8, 0.99)), torch.optim.AdamW),
}
SCHEDULE = dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=2, warmup_ratio=0.25, milestones=[3], gamma=0.5)


@pytest.mark.parametrize("case", sorted(TORCH_CASES))
def test_update_equals_torch_in_float64(case):
    """step_audit.update over four steps of seeded gradients on optim_np.groups_module in float64 against clip_grad_norm_ and
    torch.optim's step, the learning rate set from the closed form: parameters and optimizer state to 1e-13 of their scale."""
    opt_cfg, torch_class = TORCH_CASES[case]
    cfg = dict(optimizer=opt_cfg, accumulate=2, lr_scheduler=SCHEDULE)
    net = optim_np.groups_module().double()
    hyper = A.hypers(net, cfg)
    named = dict(net.named_parameters())
    kw = {k: v for k, v in opt_cfg.items() if k not in ("type", "max_grad_norm", "param_groups", "lr")}
    theirs = torch_class([dict(params=[named[n]], lr=lr, weight_decay=wd) for n, lr, wd in hyper], lr=1.0, **kw)
    from orienmask_amd import optim as O
    ours = O.param_groups(net, base_lr=opt_cfg["lr"] / 2, weight_decay=opt_cfg["weight_decay"], **GROUPS)
    if "param_groups" in opt_cfg:        # the restated carry-over is the package's (tests/golden/optim_param_groups.npz pins that one)
        assert [(lr, wd) for _, lr, wd in hyper] == [(g["lr"], g["weight_decay"]) for g in ours]
    else:
        assert all((lr, wd) == (opt_cfg["lr"] / 2, opt_cfg["weight_decay"]) for _, lr, wd in hyper) and len(hyper) == len(ours)
    S = dict(params={n: p.detach().clone() for n, p in net.named_parameters()}, buffers={}, opt={}, ema=None, ema_updates=0,
             last_epoch=0)
    rng = np.random.default_rng(3)
    for k in range(4):
        grads = {n: torch.from_numpy(rng.standard_normal(tuple(named[n].shape))) for n, _, _ in hyper}
        res = A.update(S, dict(sum=grads, last=None, losses=[0.0], buffers=[{}]), hyper, cfg, torch.float64, "cpu")
        for (n, base, _), group in zip(hyper, theirs.param_groups):
            named[n].grad = grads[n].clone()
            group["lr"] = A.lr_at(SCHEDULE, k, base)
        if "max_grad_norm" in opt_cfg:
            norm = torch.nn.utils.clip_grad_norm_([named[n] for n, _, _ in hyper], opt_cfg["max_grad_norm"])
            assert abs(float(norm) - res["norm"]) <= 1e-13 * float(norm) and res["clipped"]
        theirs.step()
        S = res["S"]
        for n, _, _ in hyper:
            assert torch.allclose(S["params"][n], named[n].detach(), rtol=0, atol=1e-13 * float(named[n].abs().max())), (k, n)
            for key, v in theirs.state[named[n]].items():
                if key == "step":
                    assert float(v) == S["opt"][n]["step"] == k + 1
                elif v is not None:
                    assert torch.allclose(S["opt"][n][key], v, rtol=0, atol=1e-13 * max(float(v.abs().max()), 1e-30)), (k, n, key)
        assert S["last_epoch"] == k + 1


# ---- the teeth ----------------------------------------------------------------------------------------------------------------------
class _Small(torch.nn.Module):
    """A convolution, a BatchNorm and the three scales' heads at 96 x 96: running statistics, a normalisation module ahead of
    biased convolutions (both carry-overs of param_groups), a few thousand parameters."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        nn = torch.nn
        self.stem = nn.Conv2d(3, 8, 3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(8)
        self.mix = nn.Conv2d(8, 8, 1, bias=False)
        self.box = nn.ModuleList([nn.Conv2d(8, 255, 1) for _ in range(3)])
        self.orien = nn.ModuleList([nn.Conv2d(8, 6, 1) for _ in range(3)])
        with torch.no_grad():
            for m in self.box:
                m.bias.view(3, 85)[:, 4] -= 4.0

    def forward(self, x):
        F = torch.nn.functional
        f = self.mix(F.leaky_relu(self.bn(self.stem(x)), 0.1))
        q = F.avg_pool2d(f, 4)
        return [(self.box[s](F.avg_pool2d(f, k)), self.orien[s](q)) for s, k in enumerate((32, 16, 8))]


def _teeth_cfg(optimizer):
    return dict(model=_Small, loss=T.loss_cfg(96, 96), accumulate=2, lr_scheduler=SCHEDULE, optimizer=optimizer)


TEETH = {
    "sgd": _teeth_cfg(dict(type="SGD", lr=0.2, momentum=0.9, weight_decay=5e-3, max_grad_norm=1.0, nonfinite="skip",
                           ema_decay=0.999, ema_warmup=True, param_groups=GROUPS)),
    "adam": _teeth_cfg(dict(type="HipAdam", lr=2e-3, weight_decay=5e-3, param_groups=GROUPS)),
}
TEETH_FAULTS = {"sgd": ("previous_lr", "lr_not_divided", "last_batch_only", "tail_skipped", "decay_everywhere", "clip_after_decay",
                        "ema_old_param", "stats_once"),
                "adam": ("adam_bias_behind", "previous_lr", "decay_everywhere")}
STEP_BATCHES = ((0, 1), (2,), (0, 1), (2,))          # three batches an epoch, accumulate 2: the second and fourth are epoch tails


@pytest.fixture(scope="module")
def teeth_runs():
    """Per configuration the chain S_0 ... S_4 of the honest float32 transition and, for every step, the float32 and float64
    gradients from S_k (shared by the mutants) with the float64 result."""
    images = [synth.synth_image_batch(30 + i, 2, 96, 96) for i in range(3)]
    targets = [synth.synth_targets(60 + i, 2, 96, 96, 5) for i in range(3)]
    out = {}
    with A.cpu_threads():
        for name, cfg in TEETH.items():
            nets = {dt: A.build_model(cfg, dt, "cpu") for dt in (torch.float32, torch.float64)}
            hyper = A.hypers(nets[torch.float32], cfg)
            S = dict(params={n: p.detach().clone() for n, p in nets[torch.float32].named_parameters()},
                     buffers={n: b.detach().clone() for n, b in nets[torch.float32].named_buffers()}, opt={}, ema_updates=0, last_epoch=0)
            S["ema"] = {n: S["params"][n].clone() for n, _, _ in hyper} if "ema_decay" in cfg["optimizer"] else None
            steps = []
            for which in STEP_BATCHES:
                xs = [images[i] for i in which]
                with torch.no_grad():
                    nets[torch.float32].load_state_dict({**S["params"], **S["buffers"]})
                    heads = [[(b.numpy(), o.numpy()) for b, o in nets[torch.float32](x)] for x in xs]
                forced = [loss_f64.forced_targets(cfg["loss"], h, targets[i]) for h, i in zip(heads, which)]
                assert all(f["near_ignore"] == 0 for per in forced for f in per)
                g32 = A.gradients(S, xs, forced, cfg, torch.float32, "cpu", nets[torch.float32], keep_last=True)
                g64 = A.gradients(S, xs, forced, cfg, torch.float64, "cpu", nets[torch.float64])
                honest = A.update(S, g32, hyper, cfg, torch.float32, "cpu")
                truth = A.update(S, g64, hyper, cfg, torch.float64, "cpu")
                steps.append(dict(S=S, g32=g32, honest=honest, truth=truth))
                S = honest["S"]
            out[name] = (cfg, hyper, steps)
    return out


def _factors(steps):
    """The configuration's factors, as the GPU test takes them: from the honest reports of all its transitions."""
    return A.spread_factors([A.judge(s["S"], s["honest"]["S"], s["honest"], s["truth"], s["honest"]) for s in steps])


def _verdict(step, got, factors):
    report = A.apply_spread(A.judge(step["S"], got["S"], got, step["truth"], step["honest"]), factors)
    return report, max(report["worst"].values())


@pytest.mark.parametrize("name", sorted(TEETH))
def test_judge_passes_the_honest_transition(teeth_runs, name):
    cfg, hyper, steps = teeth_runs[name]
    factors = _factors(steps)
    print(name, "factors", factors)
    for k, step in enumerate(steps):
        report, worst = _verdict(step, step["honest"], factors)
        A.show(report, "%s step %d" % (name, k + 1))
        assert not report["failed"] and not report["exact"] and worst <= 0.5 + 1e-12
        assert report["median_spacings"] >= 100, report["median_spacings"]
        assert step["truth"]["clipped"] == ("max_grad_norm" in cfg["optimizer"])
    assert [s["S"]["last_epoch"] for s in steps] == [0, 1, 2, 3] and len(set(steps[k]["truth"]["lrs"][0] for k in range(4))) == 4


@pytest.mark.parametrize("name,fault", [(n, f) for n in sorted(TEETH_FAULTS) for f in TEETH_FAULTS[n]])
def test_judge_rejects_a_planted_fault(teeth_runs, name, fault):
    """Every fault, at every step where it changes the result, is over a bar by a factor of two; at least one step shows it."""
    cfg, hyper, steps = teeth_runs[name]
    caught, factors = 0, _factors(steps)
    for k, step in enumerate(steps):
        mutant = A.update(step["S"], step["g32"], hyper, cfg, torch.float32, "cpu", fault=fault)
        if A.same_state(mutant["S"], step["honest"]["S"]) or mutant["lrs"] != step["honest"]["lrs"]:
            report, worst = _verdict(step, dict(mutant, lrs=None), factors)       # without the exact check of the rates: the bars decide
            print("%s %s step %d: worst ratio to bar %.3g, exact %s" % (name, fault, k + 1, worst, report["exact"][:2]))
            assert worst >= 2.0, (fault, k, worst)
            caught += 1
    assert caught >= 1


def test_judge_rejects_an_ema_count_that_advances_on_a_skipped_step(teeth_runs):
    """A non-finite gradient: the honest step is skipped and leaves everything but the schedule's count bit-unchanged; the mutant
    that counts the skipped step as an EMA update fails the exact check of the count."""
    cfg, hyper, steps = teeth_runs["sgd"]
    step = steps[2]
    bad = copy.copy(step["g32"])
    bad["sum"] = dict(bad["sum"])
    first = hyper[0][0]
    bad["sum"][first] = bad["sum"][first].clone()
    bad["sum"][first].view(-1)[0] = float("inf")
    honest = A.update(step["S"], bad, hyper, cfg, torch.float32, "cpu")
    truth = A.update(step["S"], dict(bad, sum={n: g.double() for n, g in bad["sum"].items()}), hyper, cfg, torch.float64, "cpu")
    assert honest["skipped"] and truth["skipped"] and honest["S"]["last_epoch"] == step["S"]["last_epoch"] + 1
    skipped = dict(step, truth=truth, honest=honest)
    factors = _factors(steps)
    report, _ = _verdict(skipped, honest, factors)
    assert not report["exact"] and not report["failed"]
    mutant = A.update(step["S"], bad, hyper, cfg, torch.float32, "cpu", fault="ema_counts_skipped")
    report, _ = _verdict(skipped, mutant, factors)
    assert any(line.startswith("ema_updates") for line in report["exact"]), report["exact"]


@pytest.mark.parametrize("name", ["f32-sgd", "yolo-sgd"])
def test_audit_batches_are_far_from_the_ignore_threshold(name):
    """The GPU audit leaves out a step whose batch has an IoU within 4 ulp of obj_ignore_threshold.  On the float32 torch model's
    heads (the yardstick's, here on the CPU) at the start weights none of the three batches has one, and every batch has
    positives on two scales."""
    cfg = A.CONFIGS[name]
    with A.cpu_threads(), torch.no_grad():
        net = A.build_model(cfg, torch.float32, "cpu")
        net.load_state_dict(A.start_weights(cfg), strict=True)
        for x, target in A.audit_batches():
            forced = loss_f64.forced_targets(cfg["loss"], [(b.numpy(), o.numpy()) for b, o in net(x)], target)
            assert [f["near_ignore"] for f in forced] == [0, 0, 0]
            assert sum(int(f["pos"].sum()) > 0 for f in forced) >= 2
    assert A.step_batches(2) == [(0, 1), (2,), (0, 1), (2,)] and A.step_batches(1) == [(0,), (1,), (2,)] * 2
