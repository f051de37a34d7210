"""Time the forward convolution per distinct convolution geometry of the FPNPlus model at 544 x 544: om_conv2d_forward
(csrc/conv_fwd.hip, what orienmask_amd.train.conv2d(forward='hip') enqueues) against F.conv2d (MIOpen, what forward='torch' runs) on
the same GPU and the same tensors, and against om_conv2d_grad_input of the same geometry (csrc/conv_grad.hip), which does the same
flops on the same matrix instruction.

Method (tools/bench_conv_grad.py's): per geometry, WARMUP calls of each of the three, then ROUNDS interleaved rounds (hip forward,
torch forward, hip dx, hip forward, ... so drift hits all alike); a round times INNER back-to-back calls between two HIP events and
divides.  Reported: median / min / max per call, TFLOP/s at the median (2 * B*Ho*Wo * cout * cin * taps), the sum over the model's
90 convolutions (median x multiplicity), the geometries where the HIP forward is slower than torch's, and one whole-model training
step (forward + backward, median of interleaved rounds) with its peak memory for (conv_backend, conv_forward) = ('torch', 'torch'),
('hip', 'torch') and ('hip', 'hip'), all in this run.

The frozen column: on the geometries the backbone contains (what frozen_stages can freeze), om_conv2d_frozen_forward (hip_frozen:
the convolution with the fixed BatchNorm affine, LeakyReLU and, on a DarkNet block's second layer, the residual add in its epilogue)
against the two kernels it replaces, om_conv2d_forward followed by om_bn_act_forward(training=0) (hip_fwd_bn), in the same
interleaved rounds; the geometries where the fused kernel is slower by more than the rounds' own min-max spread are listed.  A row's
`backbone_layers` counts the backbone's layers of the geometry (52 in all; `layers` counts the whole model's, which also has the
geometry in its necks, where nothing can be frozen), and the two frozen columns' sums over layers are weighted by it.
--only-frozen times these two on the backbone's geometries and nothing else.

--dtype bf16 times the bf16 forward instead (csrc/conv_fwd_bf16.hip, what amp='bf16' with conv_forward='hip' enqueues), per
geometry and in the same interleaved rounds: om_conv2d_bf16_forward on a bf16 x and the float32 master weight, bf16 out (hip_bf16),
against F.conv2d on bf16 tensors (MIOpen: torch_bf16) and om_conv2d_forward on the float32 tensors (hip_f32); and on the backbone's
geometries om_conv2d_bf16_frozen_forward (hip_bf16_frozen) against torch's bf16 convolution followed by om_bn_act_forward_bf16 in
eval mode (torch_bf16_conv_bn: what a frozen block runs under amp with conv_forward='torch').  No training step (that is
tools/bench_train_step.py --amp bf16 --conv-forward hip).  Default --out: profiles/conv_fwd_bf16_bench.json.

    python tools/bench_conv_fwd.py [--batches 8 32] [--rounds 5] [--inner 3] [--warmup 2] [--only-frozen] [--dtype {f32,bf16}]
                                   [--out profiles/conv_fwd_bench.json]

prints one JSON line (and writes it to --out); a progress line per geometry goes to stderr.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from orienmask_amd import arch, lib as omlib, train  # noqa: E402

BACKBONE_COLUMNS = ("hip_frozen", "hip_fwd_bn", "hip_bf16_frozen", "torch_bf16_conv_bn")   # summed over the backbone's layers
STEP_CONFIGS = (("torch", "torch"), ("hip", "torch"), ("hip", "hip"))      # (conv_backend, conv_forward)


def layer_table(size):
    """(cin, cout, ksize, stride, H, W) with H, W the input's -> number of convolutions."""
    table = {}
    for spec in arch.fpnplus_convs():
        d = arch.layer_div(spec)
        key = (spec.cin, spec.cout, spec.ksize, spec.stride, size // d * spec.stride, size // d * spec.stride)
        table[key] = table.get(key, 0) + 1
    return table


def backbone_table(size):
    """The backbone's geometries (what frozen_stages=6 fuses) -> (number of BACKBONE layers, residual): residual True for a DarkNet
    block's second layer.  Within the backbone a geometry is either always or never such a layer."""
    table = {}
    for spec in arch.fpnplus_convs():
        if spec.name.startswith("backbone."):
            d = arch.layer_div(spec)
            key = (spec.cin, spec.cout, spec.ksize, spec.stride, size // d * spec.stride, size // d * spec.stride)
            count, residual = table.get(key, (0, spec.name.endswith(".conv.1")))
            assert residual == spec.name.endswith(".conv.1"), key
            table[key] = (count + 1, residual)
    return table


def time_calls(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def bench_geometry(dev, B, key, args, frozen=None):
    cin, cout, ks, stride, H, W = key
    L = omlib.load()
    gen = torch.Generator(device=dev).manual_seed(cin + cout + H)
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    x = torch.randn(B, cin, H, W, device=dev, generator=gen)
    w = torch.randn(cout, cin, ks, ks, device=dev, generator=gen) * (cin * ks * ks) ** -0.5
    dy = torch.randn(B, cout, Ho, Wo, device=dev, generator=gen)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    geom = (B, cin, H, W, cout, ks, stride)
    st = omlib.current_stream_ptr(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    calls = {
        "hip_fwd": lambda: omlib.check(L.om_conv2d_forward(vp(x), vp(w), None, *geom, vp(y), st), "fwd"),
        "torch_fwd": lambda: F.conv2d(x, w, None, stride, pad),
        "hip_dx": lambda: omlib.check(L.om_conv2d_grad_input(vp(dy), vp(w), *geom, vp(dx), None, 0, st), "dx"),
    }
    if args.dtype == "bf16":
        xb, wb, yb = x.to(torch.bfloat16), w.to(torch.bfloat16), torch.empty_like(dy, dtype=torch.bfloat16)
        calls = {
            "hip_bf16": lambda: omlib.check(L.om_conv2d_bf16_forward(vp(xb), vp(w), None, *geom, vp(yb), 0, st), "bf16 fwd"),
            "torch_bf16": lambda: F.conv2d(xb, wb, None, stride, pad),
            "hip_f32": calls["hip_fwd"],
        }
        if frozen is not None:
            gamma, beta, mean = (torch.randn(cout, device=dev, generator=gen) for _ in range(3))
            var = torch.rand(cout, device=dev, generator=gen) + 0.5
            res = torch.randn(B, cout, Ho, Wo, device=dev, generator=gen).to(torch.bfloat16) if frozen else None
            save = torch.empty(4 * cout, device=dev)
            rp = vp(res) if frozen else None

            def torch_conv_bn():
                h = F.conv2d(xb, wb, None, stride, pad)
                omlib.check(L.om_bn_act_forward_bf16(vp(h), B, cout, Ho, Wo, vp(gamma), vp(beta), vp(mean), vp(var), None, 0, 0.1, 1e-5,
                                                     0.1, rp, vp(yb), save.data_ptr(), save.data_ptr() + 8 * cout, None, 0, st), "bn")

            calls["hip_bf16_frozen"] = lambda: omlib.check(L.om_conv2d_bf16_frozen_forward(
                vp(xb), vp(w), *geom, vp(gamma), vp(beta), vp(mean), vp(var), 1e-5, 0.1, rp, vp(yb), st), "bf16 frozen")
            calls["torch_bf16_conv_bn"] = torch_conv_bn
    elif frozen is not None:
        gamma, beta, mean = (torch.randn(cout, device=dev, generator=gen) for _ in range(3))
        var = torch.rand(cout, device=dev, generator=gen) + 0.5
        res = torch.randn(B, cout, Ho, Wo, device=dev, generator=gen) if frozen else None
        h, save = torch.empty_like(dy), torch.empty(4 * cout, device=dev)
        rp = vp(res) if frozen else None

        def two_kernels():
            omlib.check(L.om_conv2d_forward(vp(x), vp(w), None, *geom, vp(h), st), "fwd")
            omlib.check(L.om_bn_act_forward(vp(h), B, cout, Ho, Wo, vp(gamma), vp(beta), vp(mean), vp(var), None, 0, 0.1, 1e-5, 0.1, rp,
                                            vp(y), save.data_ptr(), save.data_ptr() + 8 * cout, None, 0, st), "bn")

        calls["hip_frozen"] = lambda: omlib.check(L.om_conv2d_frozen_forward(vp(x), vp(w), *geom, vp(gamma), vp(beta), vp(mean), vp(var),
                                                                             1e-5, 0.1, rp, vp(y), st), "frozen")
        calls["hip_fwd_bn"] = two_kernels
        if args.only_frozen:
            calls = {k: calls[k] for k in ("hip_frozen", "hip_fwd_bn")}
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    samples = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            samples[k].append(time_calls(fn, args.inner))
    flops = 2.0 * B * Ho * Wo * cout * cin * ks * ks
    out = {}
    for name, v in samples.items():
        v = sorted(v)
        med = statistics.median(v)
        out[name] = {"ms_median": round(med, 5), "ms_min": round(v[0], 5), "ms_max": round(v[-1], 5),
                     "TFLOPs_at_median": round(flops / (med * 1e-3) / 1e12, 2)}
    return out


def step_times_and_memory(dev, B, size, rounds):
    """One training step (forward + backward of the whole model) per (conv_backend, conv_forward): median ms of interleaved
    rounds, peak memory."""
    x = torch.rand(B, 3, size, size, device=dev)
    nets = {}
    for cfg in STEP_CONFIGS:
        torch.manual_seed(0)
        nets[cfg] = train.OrienMaskYOLOFPNPlus(3, 80, backend="hip", conv_backend=cfg[0], conv_forward=cfg[1]).to(dev).train()

    def step(cfg):
        out = nets[cfg](x)
        sum(t.square().mean() for pair in out for t in pair).backward()

    result = {cfg: {"conv_backend": cfg[0], "conv_forward": cfg[1], "batch": B} for cfg in nets}
    for cfg in nets:
        for _ in range(2):                # the second step is the steady state (gradients exist, the allocator is warm)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            step(cfg)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev)
        result[cfg].update(peak_bytes=int(peak), peak_above_resident_bytes=int(peak - base))
    samples = {cfg: [] for cfg in nets}
    for _ in range(rounds):
        for cfg in nets:
            samples[cfg].append(time_calls(lambda: step(cfg), 1))
    for cfg, v in samples.items():
        v = sorted(v)
        result[cfg].update(step_ms_median=round(statistics.median(v), 3), step_ms_min=round(v[0], 3), step_ms_max=round(v[-1], 3))
    return [result[cfg] for cfg in STEP_CONFIGS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--size", type=int, default=544)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--only-frozen", action="store_true", help="only the frozen column, on the backbone's geometries")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32", help="bf16: the bf16 forward's columns (see above)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bf16 = args.dtype == "bf16"
    if bf16 and args.only_frozen:
        raise SystemExit("--only-frozen is a float32 column")
    if bf16 and args.out is None:
        args.out = os.path.join(REPO, "profiles", "conv_fwd_bf16_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_fwd.py needs an MI355X: there is nothing to time on a CPU")
    dev = torch.device("cuda:0")
    table = layer_table(args.size)
    backbone = backbone_table(args.size)
    if args.only_frozen:
        table = {k: backbone[k][0] for k in table if k in backbone}
    result = {"bench": "conv_fwd_bf16" if bf16 else "conv_fwd", "size": args.size, "rounds": args.rounds, "inner": args.inner, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batches": {}}
    for B in args.batches:
        rows, sums = [], {}
        for key, count in sorted(table.items(), key=lambda kv: -kv[0][0] * kv[0][1] * kv[0][2] ** 2 * kv[0][4] * kv[0][5]):
            r = bench_geometry(dev, B, key, args, backbone[key][1] if key in backbone else None)
            rows.append(dict(zip(("cin", "cout", "ksize", "stride", "H", "W"), key), layers=count, **r))
            if key in backbone:
                rows[-1].update(backbone_layers=backbone[key][0], residual=backbone[key][1])
            print("B=%d %s x%d: %s" % (B, key, count, {k: v["ms_median"] for k, v in r.items()}), file=sys.stderr, flush=True)
            for k, v in r.items():
                s = sums.setdefault(k, {"ms_median": 0.0, "ms_min": 0.0, "ms_max": 0.0})
                for f in s:
                    s[f] += (backbone[key][0] if k in BACKBONE_COLUMNS else count) * v[f]
            torch.cuda.empty_cache()
        slower = [dict(zip(("cin", "cout", "ksize", "stride", "H"), (r["cin"], r["cout"], r["ksize"], r["stride"], r["H"])),
                       hip_ms=r["hip_fwd"]["ms_median"], torch_ms=r["torch_fwd"]["ms_median"], hip_dx_ms=r["hip_dx"]["ms_median"])
                  for r in rows if not args.only_frozen and not bf16 and r["hip_fwd"]["ms_median"] > r["torch_fwd"]["ms_median"]]
        # slower by more than the rounds' own spread: the fused kernel's fastest round is above the two kernels' slowest
        fused_slower = [dict(zip(("cin", "cout", "ksize", "stride", "H"), (r["cin"], r["cout"], r["ksize"], r["stride"], r["H"])),
                             frozen_ms=r["hip_frozen"], two_kernels_ms=r["hip_fwd_bn"])
                        for r in rows if "hip_frozen" in r and r["hip_frozen"]["ms_min"] > r["hip_fwd_bn"]["ms_max"]]
        if bf16:
            geo = lambda r: "%dx%d s%d %d->%d @%d" % (r["ksize"], r["ksize"], r["stride"], r["cin"], r["cout"], r["H"])      # noqa: E731
            for r in rows:
                r["hip_bf16_over_torch_bf16"] = round(r["hip_bf16"]["ms_median"] / r["torch_bf16"]["ms_median"], 3)
                r["hip_bf16_over_hip_f32"] = round(r["hip_bf16"]["ms_median"] / r["hip_f32"]["ms_median"], 3)
            result["batches"][str(B)] = {"geometries": rows, "layers": sum(table.values()),
                                         "backbone_layers": sum(n for n, _ in backbone.values()),
                                         "sum_over_layers_ms": {k: {f: round(x, 4) for f, x in v.items()} for k, v in sums.items()},
                                         "geometries_where_bf16_is_not_faster_than_the_f32_kernel":
                                             [geo(r) for r in rows if r["hip_bf16"]["ms_median"] >= r["hip_f32"]["ms_median"]],
                                         "geometries_where_bf16_is_slower_than_torch_bf16":
                                             [geo(r) for r in rows if r["hip_bf16"]["ms_median"] > r["torch_bf16"]["ms_median"]]}
            continue
        result["batches"][str(B)] = {"geometries": rows, "layers": sum(table.values()),
                                     "backbone_layers": sum(n for n, _ in backbone.values()),
                                     "sum_over_layers_ms": {k: {f: round(x, 4) for f, x in v.items()} for k, v in sums.items()},
                                     "geometries_where_hip_is_slower": slower,
                                     "geometries_where_the_fused_frozen_kernel_is_slower_beyond_spread": fused_slower}
    if not args.only_frozen and not bf16:
        result["training_step"] = step_times_and_memory(dev, args.step_batch, args.size, args.rounds)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
