"""Time one optimizer step on the model's 266 parameter tensors (63,662,063 float32 elements): orienmask_amd.optim.SGD (one launch
of om_sgd_step, csrc/optim.hip) against torch.optim.SGD on the same tensors on the same GPU -- its single-tensor loop
(foreach=False), its default (foreach) and fused=True where this torch offers it -- as ONE parameter group and as 266 groups with
the lr / weight_decay split of param_groups.  torch is the baseline: the parent commit has no optimizer.

Method: momentum 0.9 and weight decay, so a step reads parameter, gradient and momentum buffer and writes parameter and buffer
(5 x 4 bytes per element = 1.27 GB).  Every variant is warmed up, then timed in ROUNDS interleaved rounds (variant after variant
inside a round, so drift hits all alike); a round times INNER back-to-back steps between two HIP events on the current stream
and divides.  Reported per variant: median, min and max of the rounds' per-step times, the spread (max - min) / median, the
bytes per second at the median, and the host time per step (what the Python side of step() costs; where it exceeds the device
time the event figure is host-bound and says so).  The device clock is read before and after where the runtime exposes it.

    python tools/bench_optim.py [--optimizer sgd|adamw] [--rounds 15] [--inner 20] [--warmup 5] [--max-grad-norm X] [--ema-decay X]

prints one JSON line.  ``--max-grad-norm X`` adds, per grouping, ``hip_clip_*`` -- the same class with ``max_grad_norm=X``: three
launches of om_sgd_clip_step, one more read of the gradients -- and ``torch_clip_foreach_*``: torch.nn.utils.clip_grad_norm_ on the
tensors followed by torch's default step (on gradients of its own: it scales them in place), and reports ``clip_over_plain``, the
ratio of the medians of hip_clip_* and hip_* of the same run.  ``--ema-decay X`` adds ``hip_ema_*`` -- the same class with
``ema_decay=X``: om_sgd_ema_step, one more stream read and written (7 x 4 bytes per element) -- with ``--max-grad-norm`` also
``hip_clip_ema_*``, and ``torch_foreach_ema_*``: torch's default step followed by ``torch._foreach_lerp_(shadows, params, 1 - X)``
(8 x 4 bytes per element, more launches), and reports ``ema_over_plain`` and ``ema_over_torch``.  GBps_at_median counts the bytes
each variant's own arithmetic has to move.

``--optimizer adamw`` times orienmask_amd.optim.HipAdamW (om_adam_step / om_adam_clip_step) against torch.optim.AdamW in the same
variants: a step reads parameter, gradient and both moments and writes parameter and both moments (7 x 4 bytes per element =
1.78 GB); with ``--max-grad-norm`` also ``hip_clip_skip_*``, the form whose step counts live on the device (nonfinite="skip").
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from orienmask_amd import optim as O  # noqa: E402
from orienmask_amd.model import OrienMaskYOLOFPNPlus  # noqa: E402

HYPERS = {"sgd": dict(lr=1e-3, momentum=0.9, weight_decay=5e-4), "adamw": dict(lr=1e-3, weight_decay=1e-2)}
STREAMS = {"sgd": 5, "adamw": 7}                                  # 4-byte streams per element of the plain step
SPLIT = dict(base_lr=1e-3, weight_decay=5e-4, norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4)


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", choices=sorted(HYPERS), default="sgd",
                    help="sgd: orienmask_amd.optim.SGD against torch.optim.SGD; adamw: HipAdamW against torch.optim.AdamW")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="also time the step with gradient-norm clipping at X, and torch's clip_grad_norm_ + step")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="X",
                    help="also time the step with the weight EMA fused in (decay X), and torch's step + _foreach_lerp_")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs an MI355X: there is nothing to time on a CPU")
    dev = torch.device("cuda:0")
    HYPER = HYPERS[args.optimizer]
    hip_cls, torch_cls = (O.SGD, torch.optim.SGD) if args.optimizer == "sgd" else (O.HipAdamW, torch.optim.AdamW)
    net = OrienMaskYOLOFPNPlus(num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False, backbone_batchnorm_eval=False)
    cpu_params = list(net.parameters())
    for p in cpu_params:
        p.requires_grad_(True)                                # the inference model holds its weights frozen
    index = {id(p): i for i, p in enumerate(cpu_params)}
    split = [None] * len(cpu_params)
    for g in O.param_groups(net, **SPLIT):
        split[index[id(g["params"][0])]] = (g["lr"], g["weight_decay"])
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = [tuple(p.shape) for p in cpu_params]
    elements = sum(p.numel() for p in cpu_params)
    del net, cpu_params
    grads = [torch.randn(s, device=dev, generator=gen) * 1e-2 for s in shapes]

    def fresh_params():
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.05) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g
        return ps

    class TorchClipped:
        """torch.nn.utils.clip_grad_norm_ + torch.optim.SGD.step() as one step()."""

        def __init__(self, ps, per_tensor, max_norm):
            for p in ps:
                p.grad = p.grad.clone()                       # clip_grad_norm_ scales in place
            self.params, self.max_norm = ps, max_norm
            self.opt = torch_cls(groups(ps, per_tensor), **HYPER)

        def step(self):
            torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
            self.opt.step()

    class TorchAveraged:
        """torch.optim.SGD.step() + torch._foreach_lerp_ of the shadows towards the parameters as one step()."""

        def __init__(self, ps, per_tensor, decay):
            self.params, self.weight = [p.detach() for p in ps], 1.0 - decay
            self.shadows = [p.detach().clone() for p in ps]
            self.opt = torch_cls(groups(ps, per_tensor), **HYPER)

        def step(self):
            self.opt.step()
            torch._foreach_lerp_(self.shadows, self.params, self.weight)

    def groups(ps, per_tensor):
        if not per_tensor:
            return ps
        return [{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(ps, split)]

    variants = {}
    skipped = {}
    for per_tensor, tag in ((False, "1group"), (True, "266groups")):
        variants["hip_" + tag] = hip_cls(groups(fresh_params(), per_tensor), **HYPER)
        if args.max_grad_norm is not None:
            variants["hip_clip_" + tag] = hip_cls(groups(fresh_params(), per_tensor), max_grad_norm=args.max_grad_norm, **HYPER)
            if args.optimizer == "adamw":
                variants["hip_clip_skip_" + tag] = hip_cls(groups(fresh_params(), per_tensor), max_grad_norm=args.max_grad_norm,
                                                           nonfinite="skip", **HYPER)
            variants["torch_clip_foreach_" + tag] = TorchClipped(fresh_params(), per_tensor, args.max_grad_norm)
        if args.ema_decay is not None:
            variants["hip_ema_" + tag] = hip_cls(groups(fresh_params(), per_tensor), ema_decay=args.ema_decay, **HYPER)
            if args.max_grad_norm is not None:
                variants["hip_clip_ema_" + tag] = hip_cls(groups(fresh_params(), per_tensor), max_grad_norm=args.max_grad_norm,
                                                          ema_decay=args.ema_decay, **HYPER)
            variants["torch_foreach_ema_" + tag] = TorchAveraged(fresh_params(), per_tensor, args.ema_decay)
        variants["torch_single_" + tag] = torch_cls(groups(fresh_params(), per_tensor), foreach=False, **HYPER)
        variants["torch_foreach_" + tag] = torch_cls(groups(fresh_params(), per_tensor), **HYPER)
        try:
            opt = torch_cls(groups(fresh_params(), per_tensor), fused=True, **HYPER)
            opt.step()
            torch.cuda.synchronize()
            variants["torch_fused_" + tag] = opt
        except Exception as e:                                # this torch build has no fused step on this device
            skipped["torch_fused_" + tag] = "%s: %s" % (type(e).__name__, str(e)[:200])

    for opt in variants.values():
        for _ in range(args.warmup):
            opt.step()
    torch.cuda.synchronize()
    clock_before = clock_mhz()
    dev_ms = {k: [] for k in variants}
    host_ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, opt in variants.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            for _ in range(args.inner):
                opt.step()
            stop.record()
            t1 = time.perf_counter()
            stop.synchronize()
            dev_ms[name].append(start.elapsed_time(stop) / args.inner)
            host_ms[name].append((t1 - t0) * 1e3 / args.inner)
    clock_after = clock_mhz()
    nbytes = STREAMS[args.optimizer] * 4 * elements
    out = {"bench": "optim_step", "optimizer": args.optimizer, "tensors": len(shapes), "elements": elements,
           "bytes_per_step": nbytes, "rounds": args.rounds, "inner": args.inner, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "clock_mhz_before": clock_before, "clock_mhz_after": clock_after, "floor_ms_at_6.3TBps": nbytes / 6.3e12 * 1e3,
           "variants": {}, "skipped": skipped}
    for name in variants:
        v = sorted(dev_ms[name])
        med = statistics.median(v)
        # 4-byte streams per element: p, g, buf (adamw: both moments) read and p, buf (both moments) written; + g again for the
        # norm; + shadow read and written (torch's lerp reads the parameter once more)
        ema_streams = 3 if name.startswith("torch_foreach_ema") else 2 if "ema" in name else 0
        streams = STREAMS[args.optimizer] + ("clip" in name) + ema_streams
        moved = streams * 4 * elements
        out["variants"][name] = {"ms_median": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                                 "spread_pct": round(100 * (v[-1] - v[0]) / med, 1), "bytes": moved,
                                 "GBps_at_median": round(moved / med / 1e6, 1),
                                 "host_ms_median": round(statistics.median(host_ms[name]), 4),
                                 "host_bound": statistics.median(host_ms[name]) > 0.9 * med}
    if args.max_grad_norm is not None:
        out["max_grad_norm"] = args.max_grad_norm
        out["clip_over_plain"] = {tag: round(out["variants"]["hip_clip_" + tag]["ms_median"] /
                                             out["variants"]["hip_" + tag]["ms_median"], 3) for tag in ("1group", "266groups")}
    if args.ema_decay is not None:
        def ratio(a, b):
            return {tag: round(out["variants"][a + tag]["ms_median"] / out["variants"][b + tag]["ms_median"], 3)
                    for tag in ("1group", "266groups")}
        out["ema_decay"] = args.ema_decay
        out["ema_over_plain"] = ratio("hip_ema_", "hip_")
        out["ema_over_torch"] = ratio("hip_ema_", "torch_foreach_ema_")
        if args.max_grad_norm is not None:
            out["clip_ema_over_clip"] = ratio("hip_clip_ema_", "hip_clip_")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
