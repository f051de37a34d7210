"""The truth, the yardstick and the judgement of ONE optimizer-step transition of the trainer (tests/test_step_audit.py on the GPU,
tests/test_step_audit_cpu.py for the arithmetic and the teeth).  DESIGN.md section 3.33.

The state S is what orienmask_amd.trainer.Trainer carries from one optimizer step to the next:

    params        {name: tensor}                      every parameter of the model
    buffers       {name: tensor}                      BatchNorm running_mean / running_var / num_batches_tracked
    opt           {name: {key: tensor or number}}     momentum_buffer, or exp_avg / exp_avg_sq / step; {} before the first step
    ema           {name: tensor} or None              the shadows (a bit copy of the parameters before the first step)
    ema_updates   int
    last_epoch    int                                 the scheduler's count = optimizer steps taken so far

``transition(S, batches, forced, cfg, dtype, device)`` is one optimizer step of the reference's loop (trainer/trainer.py:42-60:
backward after every batch, then step, schedule and zero_grad every ``accumulate`` batches and after the epoch's last), written
out on its own: the torch-backend model cast to `dtype`, tests/loss_f64.py with the forced targets, gradients summed over the
step's batches, the learning rate from a closed form of the schedule divided by ``accumulate``, the reference's param_groups, the
global L2 norm and clip coefficient in clip_np.coefficient's form, the SGD / Adam / AdamW update and the EMA (ema_np.decay_at)
in a few lines each.  In float64 on the CPU it is the truth; in float32 on the GPU (with amp: the torch-backend bf16 model, loss
and optimizer float32) it is the yardstick.  It calls no HIP kernel of this package and reads no code of orienmask_amd.optim,
.builder or .trainer.

``judge`` applies the project's rule (tests/test_conv_grad.py, tests/test_amp_model.py) to a transition of the code under test:
per quantity and tensor, the relative L2 error of the CHANGE S_k -> S_{k+1} against the truth's change may be at most twice
max(yardstick's error, floor), and so may the root mean square over the quantity's tensors.  ``spread_factors`` /
``apply_spread`` replace the 2 of the single tensors and scalars (never of the root mean squares) by the factor the yardstick's
own spread over a configuration's transitions gives.

The keyword `fault` of ``update`` exists for tests/test_step_audit_cpu.py's mutants only (FAULTS).
"""
import contextlib
import math

import numpy as np
import torch

import ema_np
import loss_f64
from orienmask_amd import train

FLOOR_F32 = 2e-7             # tests/test_conv_grad.py
FLOOR_AMP = 2.0 ** -8        # tests/test_amp_model.py: the bf16 unit
MAX_THREADS = 16
SPACING_STRIDE = 7           # the displacement's median is taken over every 7th element of every held parameter
FAULTS = ("previous_lr", "lr_not_divided", "last_batch_only", "tail_skipped", "decay_everywhere", "clip_after_decay",
          "ema_old_param", "ema_counts_skipped", "adam_bias_behind", "stats_once")
NORM_TYPES = (torch.nn.BatchNorm2d, torch.nn.GroupNorm)
MOMENT_KEYS = ("momentum_buffer", "exp_avg", "exp_avg_sq")


@contextlib.contextmanager
def cpu_threads():
    """At most MAX_THREADS torch CPU threads inside the block."""
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, MAX_THREADS))
    try:
        yield
    finally:
        torch.set_num_threads(before)


# ---- the schedule, closed form ---------------------------------------------------------------------------------------------------
def lr_at(sched, k, base_lr):
    """The learning rate of optimizer step number k (from 0) of a group whose configured rate is base_lr (already divided by
    accumulate).  StepWarmUpLR: the warm-up rate while k <= warmup_iter; after it the LAST warm-up rate times gamma for every
    milestone m with warmup_iter < m <= k (a milestone inside the warm-up never acts).  PolyLR: base_lr (1 - k / max_iter)^power."""
    kind = sched["type"]
    if kind == "PolyLR":
        return base_lr * math.pow(1 - k / sched["max_iter"], sched.get("power", 0.9))
    if kind != "StepWarmUpLR":
        raise ValueError("no closed form for %r" % kind)
    n, ratio, form = sched["warmup_iter"], sched["warmup_ratio"], sched["warmup_type"]
    j = min(k, n)
    if form == "const":
        lr = base_lr * ratio
    elif form == "linear":
        lr = base_lr * (ratio + (1 - ratio) * j / n)
    else:
        lr = base_lr * ((j / n) ** ratio)
    milestones = sorted(sched["milestones"])
    for m in sorted(set(milestones)):
        if n < m <= k:
            lr = lr * sched.get("gamma", 0.1) ** milestones.count(m)
    return lr


# ---- the model and the parameters' hyper-parameters ------------------------------------------------------------------------------
def build_model(cfg, dtype, device):
    """cfg['model'] as the torch-backend model in `dtype` on `device`, in training mode: a model config dict (its kernel choices
    dropped; amp kept for float32 only: the float64 truth has none), or a callable that returns a fresh module (the CPU teeth)."""
    spec = cfg["model"]
    if callable(spec):
        net = spec()
    else:
        kw = {k: spec[k] for k in ("frozen_stages", "backbone_batchnorm_eval") if k in spec}
        if spec.get("amp") and dtype == torch.float32:
            kw["amp"] = spec["amp"]
        net = getattr(train, spec["type"])(spec["num_anchors"], spec["num_classes"], backend="torch", **kw)
    return net.to(device=device, dtype=dtype).train()


def hypers(net, cfg):
    """[(name, base lr, weight decay)] of the parameters the optimizer holds, in its order.  With a `param_groups` entry this is
    the reference's optim/param_groups.py, its carry-over included: the decay is a variable that a normalisation module sets to
    norm_weight_decay and a parameter named bias to bias_weight_decay, and that nothing sets back."""
    opt = cfg["optimizer"]
    lr, wd = opt["lr"] / cfg["accumulate"], opt.get("weight_decay", 0.0)
    groups = opt.get("param_groups")
    names = {id(p): n for n, p in net.named_parameters()}
    if not groups:
        return [(n, lr, wd) for n, p in net.named_parameters() if p.requires_grad]
    out, seen, decay = [], set(), wd
    for module in net.modules():
        for leaf, p in module.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            rate = lr
            if isinstance(module, NORM_TYPES):
                decay = groups.get("norm_weight_decay", 0.0)
            elif leaf == "bias":
                rate = lr * groups.get("bias_lr_factor", 1.0)
                decay = groups.get("bias_weight_decay", 1e-4)
            out.append((names[id(p)], rate, decay))
    return out


def _load(net, S, dtype, device):
    sd = {k: v.to(device=device, dtype=dtype) for k, v in S["params"].items()}
    sd.update({k: v.to(device=device, dtype=v.dtype if k.endswith("num_batches_tracked") else dtype) for k, v in S["buffers"].items()})
    net.load_state_dict(sd, strict=True)
    net.zero_grad(set_to_none=True)


def _buffers(net):
    return {k: v.detach().clone() for k, v in net.named_buffers()}


# ---- one step: the gradients, then the update --------------------------------------------------------------------------------------
def gradients(S, batches, forced, cfg, dtype, device, net=None, keep_last=False):
    """The step's forwards and backwards from state S: `batches` the images of the step's batches, `forced` loss_f64's forced
    targets per batch.  -> dict(sum={name: grad}, last={name: grad of the last batch alone} (keep_last), losses=[float],
    buffers=[the buffers after each forward])."""
    net = build_model(cfg, dtype, device) if net is None else net
    _load(net, S, dtype, device)
    losses, buffers, before = [], [], None
    for i, (x, f) in enumerate(zip(batches, forced)):
        if keep_last and i == len(batches) - 1 and i > 0:
            before = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        value, _ = loss_f64.loss(cfg["loss"], net(x.to(device=device, dtype=dtype)), f)
        value.backward()
        losses.append(float(value.detach()))
        buffers.append(_buffers(net))
    total = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    last = None
    if keep_last:
        last = total if before is None else {n: g - before[n] for n, g in total.items()}
    net.zero_grad(set_to_none=True)
    return dict(sum=total, last=last, losses=losses, buffers=buffers)


def update(S, grads, hyper, cfg, dtype, device, fault=None):
    """The optimizer step, the EMA and the schedule's count on the step's gradients.  -> dict(S=S', losses, norm, clipped,
    skipped, lrs=[the rate of every held parameter at this step], grads={name: the gradient the step took})."""
    opt, acc = cfg["optimizer"], cfg["accumulate"]
    kind = opt["type"]
    k = S["last_epoch"]
    g_of = grads["last"] if fault == "last_batch_only" else grads["sum"]
    to = lambda t: t.to(device=device, dtype=dtype)                                 # noqa: E731
    out = dict(params={n: v.clone() for n, v in S["params"].items()},
               buffers={n: v.clone() for n, v in grads["buffers"][0 if fault == "stats_once" else -1].items()},
               opt={n: dict(v) for n, v in S["opt"].items()}, ema=None if S["ema"] is None else dict(S["ema"]),
               ema_updates=S["ema_updates"], last_epoch=k + 1)
    result = dict(S=out, losses=list(grads["losses"]), norm=float("nan"), clipped=False, skipped=False, grads=g_of)
    step_k = k - 1 if fault == "previous_lr" and k > 0 else k
    scale = acc if fault == "lr_not_divided" else 1
    result["lrs"] = [lr_at(cfg["lr_scheduler"], step_k, base) * scale for _, base, _ in hyper]
    if fault == "tail_skipped" and len(grads["losses"]) < acc:
        out["last_epoch"] = k
        return result
    norms = torch.stack([torch.linalg.vector_norm(to(g_of[n])) for n, _, _ in hyper])
    norm = torch.linalg.vector_norm(norms)
    result["norm"] = float(norm)
    coef = None
    max_norm = opt.get("max_grad_norm")
    if max_norm is not None:
        coef = torch.clamp(1.0 / (norm + 1e-6) * max_norm, max=1.0)                 # clip_np.coefficient's form
        result["clipped"] = bool(coef < 1.0)
        if opt.get("nonfinite", "propagate") == "skip" and not math.isfinite(result["norm"]):
            result["skipped"] = True
            if fault == "ema_counts_skipped":
                out["ema_updates"] += 1
            return result
    decay = opt.get("ema_decay")
    omd = None
    if decay is not None:
        omd = float(1.0 - ema_np.decay_at(S["ema_updates"], decay, opt.get("ema_warmup", True)))
        out["ema_updates"] += 1
    default_wd = opt.get("weight_decay", 0.0)
    for (name, _, wd), lr in zip(hyper, result["lrs"]):
        p, g = to(S["params"][name]), to(g_of[name])
        st = out["opt"].setdefault(name, {})
        if fault == "decay_everywhere":
            wd = default_wd
        late = coef is not None and fault == "clip_after_decay"
        if coef is not None and not late:
            g = g * coef
        if kind == "SGD":
            d = g + wd * p if wd else g
            if late:
                d = d * coef
            momentum = opt.get("momentum", 0.0)
            if momentum:
                buf = st.get("momentum_buffer")
                buf = d.clone() if buf is None else momentum * to(buf) + (1.0 - opt.get("dampening", 0.0)) * d
                st["momentum_buffer"] = buf
                d = d + momentum * buf if opt.get("nesterov", False) else buf
            new = p - lr * d
        else:
            decoupled = kind.endswith("AdamW")
            beta1, beta2 = opt.get("betas", (0.9, 0.999))
            t = float(st.get("step", 0.0)) + 1.0
            if decoupled:
                p = p * (1.0 - lr * wd)
            elif wd:
                g = g + wd * p
            if late:
                g = g * coef
            m = to(st["exp_avg"]) if "exp_avg" in st else torch.zeros_like(p)
            v = to(st["exp_avg_sq"]) if "exp_avg_sq" in st else torch.zeros_like(p)
            m = m + (g - m) * (1.0 - beta1)
            v = beta2 * v + (1.0 - beta2) * g * g
            tb = t - 1.0 if fault == "adam_bias_behind" and t > 1 else t
            bc1, bc2 = 1.0 - beta1 ** tb, 1.0 - beta2 ** tb
            new = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + opt.get("eps", 1e-8))
            st.update(step=t, exp_avg=m, exp_avg_sq=v)
        out["params"][name] = new
        if omd is not None:
            e = to(S["ema"][name])
            out["ema"][name] = e + ((to(S["params"][name]) if fault == "ema_old_param" else new) - e) * omd
    return result


def transition(S, batches, forced, cfg, dtype, device, net=None, fault=None):
    """One optimizer step from S over `batches` (see the module docstring).  `net`: a model from build_model to reuse."""
    net = build_model(cfg, dtype, device) if net is None else net
    grads = gradients(S, batches, forced, cfg, dtype, device, net, keep_last=fault == "last_batch_only")
    return update(S, grads, hypers(net, cfg), cfg, dtype, device, fault)


# ---- the state of a live run ------------------------------------------------------------------------------------------------------
def capture(model, optimizer, scheduler, first=False):
    """S of a live model / optimizer / scheduler as CPU tensors.  first=True: before the first step, where the shadows are by
    definition bit copies of the parameters and the optimizer has not been touched."""
    cpu = lambda t: t.detach().cpu().clone()                                        # noqa: E731
    params = {n: cpu(p) for n, p in model.named_parameters()}
    averaging = getattr(optimizer, "ema_decay", None) is not None
    S = dict(params=params, buffers={n: cpu(b) for n, b in model.named_buffers()}, opt={}, ema=None, ema_updates=0,
             last_epoch=int(scheduler.last_epoch))
    if averaging:
        S["ema"] = {n: cpu(p) for n, p in model.named_parameters() if p.requires_grad}
    if first:
        return S
    state = optimizer.state_dict()["state"]
    held = [p for g in optimizer.param_groups for p in g["params"]]
    names = {id(p): n for n, p in model.named_parameters()}
    for i, p in enumerate(held):
        st = state.get(i, {})
        S["opt"][names[id(p)]] = {key: (float(v) if key == "step" else cpu(v)) for key, v in st.items()
                                  if key == "step" or (key in MOMENT_KEYS and v is not None)}
    if averaging:
        S["ema"] = {names[id(p)]: cpu(optimizer.ema_shadow(p)) for p in held}
        S["ema_updates"] = int(optimizer.ema_updates())
    return S


def same_state(a, b):
    """The names of everything in which two states differ by a bit (parameters, buffers, optimizer state, shadows, counts)."""
    bad = []
    for part in ("params", "buffers", "ema"):
        if (a[part] is None) != (b[part] is None):
            bad.append(part)
            continue
        for n in (a[part] or {}):
            if n not in b[part] or not torch.equal(a[part][n], b[part][n]):
                bad.append("%s.%s" % (part, n))
    for n in a["opt"]:
        for key, v in a["opt"][n].items():
            w = b["opt"].get(n, {}).get(key)
            if w is None or not (torch.equal(v, w) if torch.is_tensor(v) else v == w):
                bad.append("opt.%s.%s" % (n, key))
    bad += [key for key in ("ema_updates", "last_epoch") if a[key] != b[key]]
    if sorted(a["opt"]) != sorted(b["opt"]):
        bad.append("opt keys")
    return bad


# ---- the audited configurations (tests/test_step_audit.py; their first batches also tests/test_step_audit_cpu.py) ------------------
SIZE, BATCH, BATCHES, EPOCHS = 96, 2, 3, 2
_HIP = dict(backend="hip", conv_backend="hip", conv_forward="hip", route_backend="hip")
_MODEL = dict(num_anchors=3, num_classes=80)
_GROUPS = dict(norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4)
_STEP_LR = dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=2, warmup_ratio=0.25, milestones=[3], gamma=0.5)


def _loss_cfg():
    import train_step
    return train_step.loss_cfg(SIZE, SIZE)


# Every kernel choice is HIP where one exists; the rate differs at every step of every schedule (0.25, 0.625, 1, 0.5 of the base
# rate; the polynomial decays); the rates move the median parameter element by more than 100 float32 spacings (asserted).
CONFIGS = {
    "f32-sgd": dict(model=dict(type="OrienMaskYOLOFPNPlus", **_MODEL, **_HIP), accumulate=2, lr_scheduler=_STEP_LR,
                    optimizer=dict(type="SGD", lr=0.1, momentum=0.9, weight_decay=5e-4, max_grad_norm=1.0, nonfinite="skip",
                                   ema_decay=0.999, ema_warmup=True)),
    "amp-adamw": dict(model=dict(type="OrienMaskYOLOFPNPlus", **_MODEL, amp="bf16", conv_forward="hip", conv_grad="hip",
                                 route_backend="hip"), accumulate=2, lr_scheduler=dict(type="PolyLR", max_iter=8, power=0.9),
                      optimizer=dict(type="HipAdamW", lr=1e-4, weight_decay=1e-2, max_grad_norm=1.0, ema_decay=0.999,
                                     ema_warmup=False)),
    "frozen-adam": dict(model=dict(type="OrienMaskYOLOFPNPlus", **_MODEL, **_HIP, frozen_stages=2, backbone_batchnorm_eval=True),
                        accumulate=2, lr_scheduler=_STEP_LR,
                        optimizer=dict(type="HipAdam", lr=1e-4, weight_decay=5e-4, param_groups=_GROUPS)),
    "yolo-sgd": dict(model=dict(type="OrienMaskYOLO", **_MODEL, **_HIP), accumulate=1,
                     lr_scheduler=dict(type="PolyLR", max_iter=12, power=0.9),
                     optimizer=dict(type="SGD", lr=1e-5, momentum=0.9, weight_decay=5e-4, nesterov=True)),
}
for _cfg in CONFIGS.values():
    _cfg["loss"] = _loss_cfg()


def start_weights(cfg):
    """The train_step_f96_b2 weights (its seeds), for the configuration's model."""
    import os
    from conftest import GOLDEN
    from orienmask_amd import synth
    g = np.load(os.path.join(GOLDEN, "train_step_f96_b2.npz"))
    return synth.synth_state_dict(int(g["wseed"]), obj_bias=float(g["obj_bias"]), head_gain=float(g["head_gain"]),
                                  model=cfg["model"]["type"])


def audit_batches():
    """The epoch's three batches: [(image [2, 3, 96, 96] float32, target numpy tuple)]."""
    from orienmask_amd import synth
    return [(synth.synth_image_batch(100 + i, BATCH, SIZE, SIZE), synth.synth_targets(200 + i, BATCH, SIZE, SIZE, 6))
            for i in range(BATCHES)]


def step_batches(accumulate):
    """The batches (indices into audit_batches) of every optimizer step of the run: a step after every accumulate-th batch of an
    epoch and after its last."""
    steps = []
    for _ in range(EPOCHS):
        pending = []
        for b in range(BATCHES):
            pending.append(b)
            if (b + 1) % accumulate == 0 or b + 1 == BATCHES:
                steps.append(tuple(pending))
                pending = []
    return steps


# ---- the judgement ------------------------------------------------------------------------------------------------------------------
def _f64(t):
    return torch.as_tensor(t).detach().to(device="cpu", dtype=torch.float64)


def _norm(t):
    return float(torch.linalg.vector_norm(t))


def _half_ulp32(t):
    return torch.from_numpy(np.spacing(np.abs(t.to(torch.float32).numpy())).astype(np.float64)) * 0.5


def judge(S0, S1, got, truth, yard, amp=False, factor=2.0):
    """The transition S0 -> S1 of the code under test (`got`: its dict(losses, norm, clipped, lrs); lrs may be None) against the
    truth's and the yardstick's results from the same S0.

    -> dict(records=[(quantity, tensor, error, yardstick's error, floor, bar, error / bar)], failed=[records over their bar],
    exact=[what an exact check found], worst={quantity: largest error / bar}, median_spacings=the median over the held parameters'
    elements (every SPACING_STRIDE-th) of |truth's change| in float32 spacings of the parameter).  A record named "rms" is the quantity's root mean square
    over its tensors.  Floors: 2e-7, under amp 2^-8; parameters and shadows also the storage rounding itself,
    |0.5 ulp32(p')| / |truth's change|, because the code under test keeps them in float32."""
    base = FLOOR_AMP if amp else FLOOR_F32
    T, Y = truth["S"], yard["S"]
    records, exact = [], []
    held = [n for n in T["params"] if n in T["opt"]] if T["opt"] else []
    groups = {}

    def compare(quantity, name, a0, a1, t1, y1, storage=False):
        a0 = _f64(a0)
        dt = _f64(t1) - a0
        scale = _norm(dt)
        dg, dy = _f64(a1) - a0, _f64(y1) - a0
        if scale == 0.0:
            if _norm(dg) != 0.0:
                exact.append("%s %s: the truth does not move it, the code under test does" % (quantity, name))
            return dt
        floor = max(base, _norm(_half_ulp32(_f64(t1))) / scale) if storage else base
        groups.setdefault(quantity, []).append((name, _norm(dg - dt) / scale, _norm(dy - dt) / scale, floor))
        return dt

    spacings = []
    for n in S0["params"]:
        if n not in held:
            if not torch.equal(S0["params"][n], S1["params"][n]):
                exact.append("param %s: not held by the optimizer, yet changed" % n)
            continue
        dt = compare("param", n, S0["params"][n], S1["params"][n], T["params"][n], Y["params"][n], storage=True)
        spacings.append((dt.reshape(-1)[::SPACING_STRIDE].abs() / (2.0 * _half_ulp32(_f64(S0["params"][n]).reshape(-1)[::SPACING_STRIDE]))))
        for key in MOMENT_KEYS:
            if key in T["opt"][n]:
                zero = torch.zeros_like(S0["params"][n])
                have = S1["opt"].get(n, {}).get(key)
                if have is None:
                    exact.append("%s %s: missing" % (key, n))
                    continue
                compare(key, n, S0["opt"].get(n, {}).get(key, zero), have, T["opt"][n][key], Y["opt"][n][key])
        if "step" in T["opt"][n] and S1["opt"].get(n, {}).get("step") != T["opt"][n]["step"]:
            exact.append("step %s: %r, expected %r" % (n, S1["opt"].get(n, {}).get("step"), T["opt"][n]["step"]))
        if T["ema"] is not None:
            compare("ema", n, S0["ema"][n], S1["ema"][n], T["ema"][n], Y["ema"][n], storage=True)
    for n in S0["buffers"]:
        if n.endswith("num_batches_tracked"):
            if int(S1["buffers"][n]) != int(T["buffers"][n]):
                exact.append("%s: %d, expected %d" % (n, int(S1["buffers"][n]), int(T["buffers"][n])))
            continue
        counter = n.rsplit(".", 1)[0] + ".num_batches_tracked"
        if counter in T["buffers"] and int(T["buffers"][counter]) == int(S0["buffers"][counter]):
            if not torch.equal(S0["buffers"][n], S1["buffers"][n]):       # a frozen or eval-mode block: bit-unchanged
                exact.append("buffer %s: its block saw no training forward, yet it changed" % n)
            continue
        compare(n.rsplit(".", 1)[1], n, S0["buffers"][n], S1["buffers"][n], T["buffers"][n], Y["buffers"][n])
    for quantity, rows in groups.items():
        for name, err, yerr, floor in rows:
            bar = factor * max(yerr, floor)
            records.append((quantity, name, err, yerr, floor, bar, err / bar))
        rms = lambda i: math.sqrt(sum(r[i] ** 2 for r in rows) / len(rows))      # noqa: E731
        bar = 2.0 * max(rms(2), rms(3))
        records.append((quantity, "rms", rms(1), rms(2), rms(3), bar, rms(1) / bar))
    scalars = [("grad_norm", got["norm"], truth["norm"], yard["norm"])]
    scalars += [("loss[%d]" % i, g, t, y) for i, (g, t, y) in enumerate(zip(got["losses"], truth["losses"], yard["losses"]))]
    if len(got["losses"]) != len(truth["losses"]):
        exact.append("%d loss values, expected %d" % (len(got["losses"]), len(truth["losses"])))
    for name, g, t, y in scalars:
        if not (math.isfinite(t) and t != 0.0):
            if not (g == t or (math.isnan(g) and math.isnan(t))):
                exact.append("%s: %r, expected %r" % (name, g, t))
            continue
        err, yerr = abs(g - t) / abs(t), abs(y - t) / abs(t)
        bar = 2.0 * max(yerr, base)
        records.append((name, "scalar", err, yerr, base, bar, err / bar))
    for key in ("ema_updates", "last_epoch"):
        if S1[key] != T[key]:
            exact.append("%s: %r, expected %r" % (key, S1[key], T[key]))
    if bool(got["clipped"]) != bool(truth["clipped"]):
        exact.append("clipped: %r, expected %r" % (got["clipped"], truth["clipped"]))
    if got.get("lrs") is not None and list(got["lrs"]) != list(truth["lrs"]):
        exact.append("learning rates: %r..., expected %r..." % (list(got["lrs"])[:3], list(truth["lrs"])[:3]))
    worst = {}
    for r in records:
        worst[r[0]] = max(worst.get(r[0], 0.0), r[6])
    median = float(torch.cat(spacings).median()) if spacings else float("nan")
    return dict(records=records, failed=[r for r in records if not r[2] <= r[5]], exact=exact, worst=worst, median_spacings=median)


def _family(quantity):
    return "loss" if quantity.startswith("loss[") else quantity


def spread_factors(reports):
    """The per-tensor and per-scalar factors of one configuration, from the yardstick's own spread over its transitions.

    One run of the yardstick is ONE draw of its error.  On the MI355X the kernels' gradients are as accurate as torch's tensor by
    tensor (median ratio 0.8 to 1.0), yet a tensor's own pair of draws differs by far more than 2: the element
    whose gradient is a thousandth of its tensor's takes either sign under Adam, exp(objectness logit) carries the whole gradient
    of a head bias.  So, with e^ = max(error, floor):
      tensors   F = 2 max over transitions and tensors of (yardstick's e^ of the tensor / its quantity's rms bar e^): how far
                one tensor stands above its quantity in the yardstick; a tensor passes within twice its own yardstick e^ OR
                within F times the quantity's rms e^ -- worse than the yardstick's worst tensor by two is a mishandled tensor;
      scalars   F = 2 (largest yardstick e^ / smallest yardstick e^ over the transitions), the bar is F times the step's e^.
    -> {quantity or "loss" or "grad_norm": F}."""
    spread, lo, hi = {}, {}, {}
    for report in reports:
        rms = {r[0]: max(r[3], r[4]) for r in report["records"] if r[1] == "rms"}
        for q, name, _, yerr, floor, _, _ in report["records"]:
            e = max(yerr, floor)
            if name == "scalar":
                lo[_family(q)], hi[_family(q)] = min(lo.get(_family(q), e), e), max(hi.get(_family(q), e), e)
            elif name != "rms":
                spread[q] = max(spread.get(q, 1.0), e / rms[q])
    factors = {q: 2.0 * v for q, v in spread.items()}
    factors.update({q: 2.0 * hi[q] / lo[q] for q in lo})
    return factors


def apply_spread(report, factors):
    """The report with its per-tensor and scalar bars widened as spread_factors describes (the rms records keep factor 2)."""
    rms = {r[0]: max(r[3], r[4]) for r in report["records"] if r[1] == "rms"}
    records = []
    for q, name, err, yerr, floor, bar, ratio in report["records"]:
        if name == "scalar":
            bar = factors[_family(q)] * max(yerr, floor)
        elif name != "rms":
            bar = max(bar, factors[q] * rms[q])
        records.append((q, name, err, yerr, floor, bar, err / bar))
    worst = {}
    for r in records:
        worst[r[0]] = max(worst.get(r[0], 0.0), r[6])
    return dict(report, records=records, failed=[r for r in records if not r[2] <= r[5]], worst=worst)


def show(report, label):
    """Every ratio of a report, one line per record whose ratio is among its quantity's three largest, and the exact findings."""
    print("%s: median displacement %.0f float32 spacings" % (label, report["median_spacings"]))
    by = {}
    for r in report["records"]:
        by.setdefault(r[0], []).append(r)
    for quantity, rows in by.items():
        rows = sorted(rows, key=lambda r: -r[6])
        keep = [r for r in rows if r[1] in ("rms", "scalar")] + [r for r in rows if r[1] not in ("rms", "scalar")][:3]
        for r in keep:
            print("  %-14s %-44s err %.3g  yardstick %.3g  floor %.3g  ratio to bar %.3f" % (r[0], r[1], r[2], r[3], r[4], r[6]))
    for line in report["exact"]:
        print("  EXACT", line)
