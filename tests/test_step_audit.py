"""GPU: every optimizer-step transition of orienmask_amd.trainer.Trainer against float64, teacher-forced in time.

Per configuration the product is built through `builder` as tests/test_trainer.py builds it and run with sync_free=True over a
fixed list of three 2 x 3 x 96 x 96 batches for two epochs, from the train_step_f96_b2 weights.  The state S_k after every
optimizer step is recorded (step_audit.capture), with the step's .grad tensors, its learning rates, its gradient norm, every
batch's heads and loss value.  Each transition S_k -> S_{k+1} is then recomputed from the run's OWN S_k by step_audit.transition,
in float64 on the CPU (the truth) and in float32 on the GPU without any kernel of this package (the yardstick), with the loss's
discrete decisions forced from the run's own heads, and step_audit.judge compares the three: an error is that step's alone.
The root mean square of every quantity is held to twice max(yardstick's error, floor); a single tensor or scalar to the factor
that step_audit.spread_factors takes from the yardstick's own spread over the configuration's transitions (printed with -s).

A step with a batch whose IoU lies within 4 ulp of obj_ignore_threshold on the run's heads is left out of the judgement (its
forced decision could be another rounding's); at most one step per configuration, asserted.
"""
import os
import time
import types

import numpy as np
import pytest
import torch

import loss_f64
import optim_np
import step_audit as A

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def audits():
    return {}


class _Loader(list):
    """A fixed in-memory list of (image, target) batches: what the epoch loop needs of a loader."""


def _product(dev, name, tmp, epochs, resume=None, observe=False):
    """One run of the product's Trainer.  observe: record S_0 and, at every scheduler step, what the audit needs."""
    from orienmask_amd import builder, optim, train
    from orienmask_amd.trainer import Trainer
    cfg = A.CONFIGS[name]
    config = dict(n_gpu=1, accumulate=cfg["accumulate"], epochs=epochs, val_freq=1, save_freq=1, monitor="loss", monitor_mode="off",
                  log_freq=1, log_dir=str(tmp), name=name, model=cfg["model"], loss=cfg["loss"], optimizer=cfg["optimizer"],
                  lr_scheduler=cfg["lr_scheduler"])
    torch.manual_seed(7)
    model = builder.build(config["model"], train).to(dev)
    model.load_state_dict(A.start_weights(cfg), strict=True)
    loss = builder.build(config["loss"], train)
    optimizer = builder.build_optimizer(config["optimizer"], config["accumulate"], model)
    scheduler = builder.build(config["lr_scheduler"], optim, optimizer=optimizer)
    loader = _Loader((x, tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in t)) for x, t in A.audit_batches())
    rec = types.SimpleNamespace(states=[], steps=[], pending=[], losses=[])
    if observe:
        rec.states.append(A.capture(model, optimizer, scheduler, first=True))
        model.register_forward_hook(lambda m, inp, out: rec.pending.append(
            dict(x=inp[0].detach().cpu().clone(), heads=[(b.detach().cpu().clone(), o.detach().cpu().clone()) for b, o in out])))
        enqueue, sched_step = loss.enqueue, scheduler.step          # bound methods of the classes

        def recording_enqueue(*a, **kw):
            value = enqueue(*a, **kw)
            rec.losses.append(value.detach().clone())
            return value

        def recording_step(self, *a, **kw):
            # between optimizer.step() and zero_grad(): the gradients the step took, its rates and its norm
            held = [p for g in optimizer.param_groups for p in g["params"]]
            step = dict(batches=rec.pending, losses=[float(v) for v in rec.losses], grads=[p.grad.detach().clone() for p in held],
                        lrs=[float(g["lr"]) for g in optimizer.param_groups for _ in g["params"]],
                        wds=[float(g["weight_decay"]) for g in optimizer.param_groups for _ in g["params"]])
            if getattr(optimizer, "max_grad_norm", None) is not None:
                stats = optimizer.grad_norm_stats(reset=False)
                step.update(norm=stats["last_norm"], clipped=stats["last_coef"] < 1.0)
            else:
                total = sum(float(g.double().pow(2).sum()) for g in step["grads"])
                step.update(norm=total ** 0.5, clipped=False)
            rec.pending, rec.losses = [], []
            sched_step(*a, **kw)
            rec.steps.append(step)
            rec.states.append(A.capture(model, optimizer, scheduler))

        # a subclass, not an attribute of the instance: the scheduler's state_dict (its __dict__) goes into every checkpoint
        loss.enqueue = recording_enqueue
        scheduler.__class__ = type("Recording" + type(scheduler).__name__, (type(scheduler),), dict(step=recording_step))
    t = Trainer(model, loss, optimizer, scheduler, config, loader, None, None, dev, types.SimpleNamespace(resume=resume, weights=None),
                sync_free=True)
    t.train()
    torch.cuda.synchronize(dev)
    rec.final = A.capture(model, optimizer, scheduler)
    rec.names = {id(p): n for n, p in model.named_parameters()}
    rec.held = [rec.names[id(p)] for g in optimizer.param_groups for p in g["params"]]
    rec.checkpoint_dir = t.checkpoint_dir
    return rec


def _audit(dev, audits, name, tmp_path_factory):
    if name in audits:
        return audits[name]
    began = time.monotonic()
    cfg = A.CONFIGS[name]
    amp = bool(cfg["model"].get("amp"))
    targets = [t for _, t in A.audit_batches()]
    which = A.step_batches(cfg["accumulate"])
    with A.cpu_threads():
        rec = _product(dev, name, tmp_path_factory.mktemp(name), epochs=2, observe=True)
        product_s = time.monotonic() - began
        assert len(rec.steps) == len(which) and [len(s["batches"]) for s in rec.steps] == [len(w) for w in which]
        nets = {torch.float64: A.build_model(cfg, torch.float64, "cpu"), torch.float32: A.build_model(cfg, torch.float32, dev)}
        hyper = A.hypers(nets[torch.float64], cfg)
        assert [n for n, _, _ in hyper] == rec.held                      # the optimizer holds these parameters, in this order
        reports, left_out, bits = [], [], []
        for k, (step, batch_ids) in enumerate(zip(rec.steps, which)):
            S0, S1 = rec.states[k], rec.states[k + 1]
            forced = [loss_f64.forced_targets(cfg["loss"], [(b.numpy(), o.numpy()) for b, o in rec_b["heads"]], targets[i])
                      for rec_b, i in zip(step["batches"], batch_ids)]
            if any(f["near_ignore"] for per in forced for f in per):
                left_out.append(k)
                continue
            xs = [b["x"] for b in step["batches"]]
            truth = A.transition(S0, xs, forced, cfg, torch.float64, "cpu", nets[torch.float64])
            with torch.backends.cudnn.flags(deterministic=True):          # one draw of the yardstick's error, the same in every run
                yard = A.transition(S0, xs, forced, cfg, torch.float32, dev, nets[torch.float32])
            assert step["wds"] == [wd for _, _, wd in hyper]
            reports.append((k, A.judge(S0, S1, step, truth, yard, amp=amp), list(batch_ids)))
            if name == "yolo-sgd":
                bits.append((k, _sgd_bits(cfg, rec, k)))
        factors = A.spread_factors([r for _, r, _ in reports])
        print("%s: factors from the yardstick's spread: %s" % (name, ", ".join("%s %.3g" % kv for kv in sorted(factors.items()))))
        judged = []
        for k, report, batch_ids in reports:
            report = A.apply_spread(report, factors)
            A.show(report, "%s step %d (batches %s)" % (name, k + 1, batch_ids))
            judged.append((k, report))
        reports = judged
        _summary(name, reports)
        audits[name] = types.SimpleNamespace(rec=rec, reports=reports, left_out=left_out, bits=bits, factors=factors)
        rec.states, rec.steps = None, None                                # only the final state is kept for the resume test
    print("%s: %d transitions, product run %.1f s, whole audit %.1f s" % (name, len(reports), product_s, time.monotonic() - began))
    return audits[name]


def _summary(name, reports):
    """Per quantity over the configuration's transitions: the largest rms error over its bar, and the largest error of one tensor
    (or scalar) over max(its own yardstick error, floor) -- the figure the plain factor 2 would have had to cover."""
    rms, single = {}, {}
    for _, report in reports:
        for q, kind, err, yerr, floor, _, ratio in report["records"]:
            if kind == "rms":
                rms[q] = max(rms.get(q, 0.0), ratio)
            else:
                q = A._family(q)
                single[q] = max(single.get(q, 0.0), err / max(yerr, floor))
    for q in single:
        print("%s summary: %-16s rms over bar %s   worst single over its own yardstick %.3g" % (
            name, q, "%.3f" % rms[q] if q in rms else "  -  ", single[q]))


def _sgd_bits(cfg, rec, k):
    """optim_np.sgd_step_many on the run's own gradients and S_k with the step's rate -> the tensors of S_{k+1} it does not
    reproduce bit for bit."""
    opt = cfg["optimizer"]
    S0, S1, step = rec.states[k], rec.states[k + 1], rec.steps[k]
    flat = lambda t: t.detach().cpu().contiguous().view(-1).numpy()                 # noqa: E731
    ps = [flat(S0["params"][n]) for n in rec.held]
    bufs = [flat(S0["opt"][n]["momentum_buffer"]) if n in S0["opt"] else None for n in rec.held]
    hyper = [dict(lr=lr, momentum=opt["momentum"], weight_decay=opt["weight_decay"], nesterov=opt.get("nesterov", False))
             for lr in step["lrs"]]
    new_p, new_b = optim_np.sgd_step_many(ps, [flat(g) for g in step["grads"]], bufs, hyper, threads=A.MAX_THREADS)
    return [n for n, p, b in zip(rec.held, new_p, new_b)
            if not (optim_np.same_bits(p, flat(S1["params"][n])) and optim_np.same_bits(b, flat(S1["opt"][n]["momentum_buffer"])))]


@pytest.mark.parametrize("name", sorted(A.CONFIGS))
def test_every_transition_against_float64(dev, audits, name, tmp_path_factory):
    """Per transition: the change of every parameter, moment estimate, running statistic and shadow, the gradient norm and every
    batch's loss as the quantity's root mean square within twice max(yardstick's error, floor) and per tensor within the factor
    from the yardstick's spread; the counters, the clip decision, the frozen and eval-mode tensors and every learning rate
    exactly (step_audit.judge, step_audit.spread_factors)."""
    audit = _audit(dev, audits, name, tmp_path_factory)
    assert len(audit.left_out) <= 1, audit.left_out
    assert audit.reports
    problems = []
    for k, report in audit.reports:
        assert report["median_spacings"] >= 100, (k, report["median_spacings"])     # the step moves the parameters: asserted, not assumed
        problems += [(k,) + r for r in report["failed"]] + [(k, line) for line in report["exact"]]
    assert not problems, problems[:20]
    if name == "yolo-sgd":
        assert len(audit.bits) == len(audit.reports) and all(not bad for _, bad in audit.bits), audit.bits


@pytest.mark.parametrize("name", sorted(A.CONFIGS))
def test_resumed_run_ends_in_the_straight_runs_state(dev, audits, name, tmp_path_factory):
    """A second run stopped after epoch 1 and resumed from its epoch1.pth: parameters, buffers, optimizer state, shadows and counts
    of the straight run, bit for bit."""
    audit = _audit(dev, audits, name, tmp_path_factory)
    began = time.monotonic()
    with A.cpu_threads():
        half = _product(dev, name, tmp_path_factory.mktemp(name + "_half"), epochs=1)
        resumed = _product(dev, name, half.checkpoint_dir, epochs=2, resume=os.path.join(half.checkpoint_dir, "epoch1.pth"))
    print("%s: stopped and resumed in %.1f s" % (name, time.monotonic() - began))
    assert half.final["last_epoch"] * 2 == resumed.final["last_epoch"] == audit.rec.final["last_epoch"]
    assert A.same_state(audit.rec.final, resumed.final) == [] and A.same_state(resumed.final, audit.rec.final) == []
