"""Steps per second of the training loop, sync-free against the reference's per-step host bookkeeping, on the same build.

    python tools/bench_train_step.py [--batch 8] [--size 544] [--steps 30] [--warmup 5] [--rounds 3] [--frozen-stages K]
                                     [--default-backends] [--amp bf16] [--conv-forward {torch,hip}] [--conv-grad {torch,hip}]
                                     [--out profiles/train_step_bench.json]

Both loops are orienmask_amd.trainer.Trainer._train_epoch over the same SyntheticLossLoader batches (made once, on the device),
the trainable OrienMaskYOLOFPNPlus with every HIP backend, the HIP SGD step, accumulate 1 and log_freq = steps, so the sync-free
loop reads its counter twice per timed epoch (at the last batch, where step % writer_freq == 0, and at the end of the epoch): the
only difference is ``sync_free``.  An epoch of `warmup` batches runs first; then `rounds` timed epochs of
`steps` batches per loop, alternating, each between two device synchronisations.  Prints one JSON line: per loop the median,
minimum and maximum steps per second over the rounds, and the spread that any comparison of the two has to clear, and the peak
device memory of the timed epochs.  --frozen-stages K builds the model with frozen_stages=K (0, the default, leaves the model
dict as it was); --default-backends leaves the four backend options at the model's defaults instead of every HIP backend.

--amp bf16 compares precisions instead of loops: both loops are sync-free and use the model's default backends (amp needs torch's
convolutions), one with the float32 model ("fp32") and one with amp='bf16' ("amp_bf16"), in the same alternating rounds; each
loop's peak device memory is that of its own timed epochs (both models stay resident, so subtract nothing: compare the two).

--amp bf16 --conv-forward hip compares the forward convolutions under amp instead: both loops are sync-free amp='bf16' models with
the default backends, one with torch's bf16 convolutions ("amp_bf16_conv_torch") and one with conv_forward='hip'
("amp_bf16_conv_hip": csrc/conv_fwd_bf16.hip, frozen stages one fused kernel per layer), in the same alternating rounds; default
--out profiles/train_step_amp_conv_bench.json.

--amp bf16 --conv-forward hip --conv-grad hip compares the convolution gradients behind that forward instead: both loops are
sync-free amp='bf16', conv_forward='hip' models, one with torch's bf16 gradients ("amp_bf16_grad_torch") and one with
conv_grad='hip' ("amp_bf16_grad_hip": csrc/conv_grad_bf16.hip), in the same alternating rounds; default --out
profiles/train_step_amp_conv_grad_bench.json.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=544)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frozen-stages", type=int, default=0, help="freeze backbone.conv1 ... conv{K} (0: none)")
    ap.add_argument("--default-backends", action="store_true", help="the model's default backends instead of every HIP backend")
    ap.add_argument("--amp", choices=["bf16"], default=None, help="time the float32 model against amp (see above)")
    ap.add_argument("--conv-forward", choices=["torch", "hip"], default="torch",
                    help="with --amp: 'hip' times amp with torch's convolutions against amp with conv_forward='hip' (see above)")
    ap.add_argument("--conv-grad", choices=["torch", "hip"], default="torch",
                    help="with --amp and --conv-forward hip: 'hip' times conv_grad='torch' against conv_grad='hip' (see above)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    conv_ab = args.conv_forward == "hip"
    grad_ab = args.conv_grad == "hip"
    if grad_ab and not (args.amp and conv_ab):
        raise SystemExit("--conv-grad hip compares the gradients behind the bf16 forward kernel: add --amp bf16 --conv-forward hip")
    if grad_ab and args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "train_step_amp_conv_grad_bench.json")
    if conv_ab and not args.amp:
        raise SystemExit("--conv-forward hip compares the forward convolutions under amp: add --amp bf16")
    if conv_ab and args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "train_step_amp_conv_bench.json")

    import torch
    from orienmask_amd import builder
    from orienmask_amd.tester import SyntheticLossLoader
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    dev = torch.device("cuda", 0)
    s = args.size
    anchors = [[12, 16], [19, 36], [40, 28], [36, 75], [76, 55], [72, 146], [142, 110], [192, 243], [459, 401]]
    log_dir = tempfile.mkdtemp(prefix="om_train_bench_")
    config = dict(seed=0, n_gpu=1, accumulate=1, epochs=1, val_freq=1000, save_freq=1000, monitor="loss", monitor_mode="off",
                  log_freq=args.steps, log_dir=log_dir, name="bench",
                  model=dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, backend="hip", conv_backend="hip",
                             conv_forward="hip", route_backend="hip"),
                  loss=dict(type="OrienMaskYOLOMultiScaleLoss", grid_size=[[s // 32] * 2, [s // 16] * 2, [s // 8] * 2],
                            image_size=[s, s], anchors=anchors, anchor_mask=[[6, 7, 8], [3, 4, 5], [0, 1, 2]], num_classes=80,
                            weight=[1, 1, 1, 1, 1, 20, 20], scales_weight=[1, 1, 1]),
                  optimizer=dict(type="SGD", lr=1e-4, momentum=0.9, weight_decay=5e-4),
                  lr_scheduler=dict(type="StepWarmUpLR", warmup_type="linear", warmup_iter=1000, warmup_ratio=0.1,
                                    milestones=[100000], gamma=0.1))

    if args.default_backends or args.amp:
        config["model"] = dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80)
    if args.frozen_stages:
        config["model"]["frozen_stages"] = args.frozen_stages

    def loader(n):
        return SyntheticLossLoader(n * args.batch, args.batch, size=(s, s), seed=1, device=dev)

    warm, timed = loader(args.warmup), loader(args.steps)
    trainers = {}
    if grad_ab:
        loops = (("amp_%s_grad_torch" % args.amp, True, dict(amp=args.amp, conv_forward="hip")),
                 ("amp_%s_grad_hip" % args.amp, True, dict(amp=args.amp, conv_forward="hip", conv_grad="hip")))
    elif conv_ab:
        loops = (("amp_%s_conv_torch" % args.amp, True, dict(amp=args.amp)),
                 ("amp_%s_conv_hip" % args.amp, True, dict(amp=args.amp, conv_forward="hip")))
    elif args.amp:
        loops = (("fp32", True, {}), ("amp_" + args.amp, True, dict(amp=args.amp)))
    else:
        loops = (("sync_free", True, {}), ("host_loop", False, {}))
    for name, sync_free, model_kw in loops:
        t = builder.build_trainer(dict(config, name="bench_" + name, model=dict(config["model"], **model_kw)),
                                  types.SimpleNamespace(resume=None, weights=None), dev, train_loader=warm, sync_free=sync_free)
        t._train_epoch(1)
        t.train_loader = timed
        trainers[name] = t
    rates = {name: [] for name in trainers}
    peaks = {name: 0 for name in trainers}
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    for _ in range(args.rounds):
        for name, t in trainers.items():
            torch.cuda.synchronize(dev)
            if args.amp:
                torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            t._train_epoch(2)
            torch.cuda.synchronize(dev)
            rates[name].append(args.steps / (time.perf_counter() - t0))
            peaks[name] = max(peaks[name], int(torch.cuda.max_memory_allocated(dev)))
    shutil.rmtree(log_dir, ignore_errors=True)          # the trainers' run directories: nothing in them is a result
    out = dict(bench="train_step", batch=args.batch, size=s, steps=args.steps, warmup=args.warmup, rounds=args.rounds,
               device=torch.cuda.get_device_name(0), torch=torch.__version__, frozen_stages=args.frozen_stages,
               backends="default" if args.default_backends or args.amp else "hip", amp=args.amp, conv_forward=args.conv_forward, conv_grad=args.conv_grad,
               peak_bytes=max(peaks.values()))
    for name, r in rates.items():
        out[name] = dict(steps_per_s_median=round(statistics.median(r), 3), steps_per_s_min=round(min(r), 3),
                         steps_per_s_max=round(max(r), 3), images_per_s_median=round(statistics.median(r) * args.batch, 2),
                         ms_per_step_median=round(1e3 / statistics.median(r), 3))
        if args.amp:
            out[name]["peak_bytes"] = peaks[name]
    first, second = [n for n, _, _ in loops]
    # sync_free over host_loop; with --amp, amp over fp32; with --conv-forward hip, conv_forward 'hip' over 'torch'
    out["ratio_of_medians"] = round(out[second if args.amp else first]["steps_per_s_median"]
                                    / out[first if args.amp else second]["steps_per_s_median"], 4)
    out["spread"] = round(max((max(r) - min(r)) / statistics.median(r) for r in rates.values()), 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as handle:
            handle.write(line + "\n")


if __name__ == "__main__":
    main()
