"""Time the convolution gradients per distinct convolution geometry of the FPNPlus model at 544 x 544: om_conv2d_grad_input and
om_conv2d_grad_weight (csrc/conv_grad.hip and csrc/conv_dw.hip, what orienmask_amd.train.conv2d's backward enqueues) against torch's own convolution
backward (aten.convolution_backward with one output selected) on the same GPU and the same tensors, the data gradient and the weight
gradient separately.  torch is the baseline: it is what conv_backend='torch' runs.

Method: per geometry, WARMUP calls of each of the four (backend, gradient) pairs, then ROUNDS interleaved rounds (hip dx, torch dx,
hip dw, torch dw, hip dx, ... so drift hits all alike); a round times INNER back-to-back calls between two HIP events and divides.
Reported: median / min / max per call, TFLOP/s at the median (2 * B*Ho*Wo * cout * cin * taps per gradient), the sum over the
model's 90 convolutions (median x multiplicity; the input gradient of backbone.conv1 is never needed and is left out), the
geometries where 'hip' is slower, and one whole-model training step (forward + backward, median of interleaved rounds) with its peak
memory for conv_backend 'hip' and 'torch'.

    python tools/bench_conv_grad.py [--batches 8 32] [--rounds 5] [--inner 3] [--warmup 2] [--out profiles/conv_grad_bench.json]
                                    [--dtype {f32,bf16}]

prints one JSON line (and writes it to --out); a progress line per geometry goes to stderr.

--dtype bf16 times the bf16 gradients instead (csrc/conv_grad_bf16.hip and csrc/conv_dw.hip, what amp='bf16' with conv_forward='hip', conv_grad='hip'
enqueues), per geometry and in the same interleaved rounds: om_conv2d_bf16_grad_input (bf16 dx) and om_conv2d_bf16_grad_weight on
bf16 dy and x and the float32 master weight (hip_bf16), aten.convolution_backward on bf16 tensors with one output selected
(torch_bf16: what conv_grad='torch' runs), and om_conv2d_grad_* on the float32 tensors (hip_f32).  Reported besides: the geometries
where hip_bf16 is slower than torch_bf16, and those where it is slower than hip_f32.  No whole-model step (that is
tools/bench_train_step.py --amp bf16 --conv-forward hip --conv-grad hip).  Default --out: profiles/conv_grad_bf16_bench.json.
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

from orienmask_amd import arch, lib as omlib, train  # noqa: E402


def layer_table(size):
    """(cin, cout, ksize, stride, H, W) with H, W the input's -> [number of convolutions, number of them that need dx]."""
    table = {}
    for spec in arch.fpnplus_convs():
        d = arch.layer_div(spec)
        key = (spec.cin, spec.cout, spec.ksize, spec.stride, size // d * spec.stride, size // d * spec.stride)
        e = table.setdefault(key, [0, 0])
        e[0] += 1
        e[1] += 0 if spec.name == "backbone.conv1" else 1
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


def bench_geometry(dev, B, key, args):
    cin, cout, ks, stride, H, W = key
    L = omlib.load()
    gen = torch.Generator(device=dev).manual_seed(cin + cout + H)
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    x = torch.randn(B, cin, H, W, device=dev, generator=gen)
    w = torch.randn(cout, cin, ks, ks, device=dev, generator=gen) * (cin * ks * ks) ** -0.5
    dy = torch.randn(B, cout, Ho, Wo, device=dev, generator=gen)
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    geom = (B, cin, H, W, cout, ks, stride)
    ws = torch.empty(max(L.om_conv2d_grad_workspace_bytes(*geom), 16), dtype=torch.uint8, device=dev)
    st = omlib.current_stream_ptr(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    conv_bwd = torch.ops.aten.convolution_backward

    def torch_grad(mask):
        return conv_bwd(dy, x, w, None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1, mask)

    calls = {
        ("hip", "dx"): lambda: omlib.check(L.om_conv2d_grad_input(vp(dy), vp(w), *geom, vp(dx), vp(ws), ws.numel(), st), "dx"),
        ("torch", "dx"): lambda: torch_grad([True, False, False]),
        ("hip", "dw"): lambda: omlib.check(L.om_conv2d_grad_weight(vp(x), vp(dy), *geom, vp(dw), None, vp(ws), ws.numel(), st), "dw"),
        ("torch", "dw"): lambda: torch_grad([False, True, False]),
    }
    if args.dtype == "bf16":
        xb, dyb, wb, dxb = x.to(torch.bfloat16), dy.to(torch.bfloat16), w.to(torch.bfloat16), torch.empty_like(x, dtype=torch.bfloat16)
        wsb = torch.empty(max(L.om_conv2d_bf16_grad_workspace_bytes(*geom), 16), dtype=torch.uint8, device=dev)

        def torch_bf16(mask):
            return conv_bwd(dyb, xb, wb, None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1, mask)

        calls = {
            ("hip_bf16", "dx"): lambda: omlib.check(L.om_conv2d_bf16_grad_input(vp(dyb), vp(w), *geom, vp(dxb), 0, vp(wsb), wsb.numel(),
                                                                                st), "bf16 dx"),
            ("torch_bf16", "dx"): lambda: torch_bf16([True, False, False]),
            ("hip_f32", "dx"): calls[("hip", "dx")],
            ("hip_bf16", "dw"): lambda: omlib.check(L.om_conv2d_bf16_grad_weight(vp(xb), vp(dyb), *geom, vp(dw), None, vp(wsb), wsb.numel(),
                                                                                 st), "bf16 dw"),
            ("torch_bf16", "dw"): lambda: torch_bf16([False, True, False]),
            ("hip_f32", "dw"): calls[("hip", "dw")],
        }
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    samples = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            samples[k].append(time_calls(fn, args.inner))
    flops = 2.0 * B * Ho * Wo * cout * cin * ks * ks
    out = {}
    for (name, grad), v in samples.items():
        v = sorted(v)
        med = statistics.median(v)
        out["%s_%s" % (name, grad)] = {"ms_median": round(med, 5), "ms_min": round(v[0], 5), "ms_max": round(v[-1], 5),
                                       "TFLOPs_at_median": round(flops / (med * 1e-3) / 1e12, 2)}
    return out


def step_times_and_memory(dev, B, size, rounds):
    """One training step (forward + backward of the whole model) per conv_backend: median ms of interleaved rounds, peak memory."""
    x = torch.rand(B, 3, size, size, device=dev)
    nets = {}
    for cb in ("hip", "torch"):
        torch.manual_seed(0)
        nets[cb] = train.OrienMaskYOLOFPNPlus(3, 80, backend="hip", conv_backend=cb).to(dev).train()

    def step(cb):
        out = nets[cb](x)
        sum(t.square().mean() for pair in out for t in pair).backward()

    result = {cb: {"batch": B} for cb in nets}
    for cb in nets:
        for _ in range(2):                # the second step is the steady state (gradients exist, the allocator is warm)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            step(cb)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev)
        result[cb].update(peak_bytes=int(peak), peak_above_resident_bytes=int(peak - base))
    samples = {cb: [] for cb in nets}
    for _ in range(rounds):
        for cb in nets:
            samples[cb].append(time_calls(lambda: step(cb), 1))
    for cb, v in samples.items():
        v = sorted(v)
        result[cb].update(step_ms_median=round(statistics.median(v), 3), step_ms_min=round(v[0], 3), step_ms_max=round(v[-1], 3))
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--size", type=int, default=544)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    args = ap.parse_args()
    bf16 = args.dtype == "bf16"
    if bf16 and args.out is None:
        args.out = os.path.join(REPO, "profiles", "conv_grad_bf16_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_grad.py needs an MI355X: there is nothing to time on a CPU")
    dev = torch.device("cuda:0")
    table = layer_table(args.size)
    result = {"bench": "conv_grad_bf16" if bf16 else "conv_grad", "size": args.size, "rounds": args.rounds, "inner": args.inner,
              "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batches": {}}
    for B in args.batches:
        rows, sums = [], {}
        for key, (count, count_dx) in sorted(table.items(), key=lambda kv: -kv[0][0] * kv[0][1] * kv[0][2] ** 2 * kv[0][4] * kv[0][5]):
            r = bench_geometry(dev, B, key, args)
            rows.append(dict(zip(("cin", "cout", "ksize", "stride", "H", "W"), key), layers=count, layers_with_dx=count_dx, **r))
            print("B=%d %s x%d: %s" % (B, key, count, {k: v["ms_median"] for k, v in r.items()}), file=sys.stderr, flush=True)
            for k, v in r.items():
                s = sums.setdefault(k, {"ms_median": 0.0, "ms_min": 0.0, "ms_max": 0.0})
                for f in s:
                    s[f] += (count_dx if k.endswith("dx") else count) * v[f]
            torch.cuda.empty_cache()
        def slower_than(mine, other):
            return [dict(zip(("cin", "cout", "ksize", "stride", "H"), (r["cin"], r["cout"], r["ksize"], r["stride"], r["H"])), gradient=g,
                         **{mine + "_ms": r["%s_%s" % (mine, g)]["ms_median"], other + "_ms": r["%s_%s" % (other, g)]["ms_median"]})
                    for r in rows for g in ("dx", "dw") if r["%s_%s" % (mine, g)]["ms_median"] > r["%s_%s" % (other, g)]["ms_median"]]
        if bf16:
            result["batches"][str(B)] = {"geometries": rows, "layers": sum(c for c, _ in table.values()),
                                         "sum_over_layers_ms": {k: {f: round(x, 4) for f, x in v.items()} for k, v in sums.items()},
                                         "geometries_where_hip_bf16_is_slower_than_torch_bf16": slower_than("hip_bf16", "torch_bf16"),
                                         "geometries_where_hip_bf16_is_slower_than_hip_f32": slower_than("hip_bf16", "hip_f32")}
            continue
        slower = [dict(zip(("cin", "cout", "ksize", "stride", "H"), (r["cin"], r["cout"], r["ksize"], r["stride"], r["H"])), gradient=g,
                       hip_ms=r["hip_" + g]["ms_median"], torch_ms=r["torch_" + g]["ms_median"])
                  for r in rows for g in ("dx", "dw") if r["hip_" + g]["ms_median"] > r["torch_" + g]["ms_median"]]
        result["batches"][str(B)] = {"geometries": rows, "layers": sum(c for c, _ in table.values()),
                                     "sum_over_layers_ms": {k: {f: round(x, 4) for f, x in v.items()} for k, v in sums.items()},
                                     "geometries_where_hip_is_slower": slower}
    if not bf16:
        result["training_step"] = step_times_and_memory(dev, args.step_batch, args.size, args.rounds)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
