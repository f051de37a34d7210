"""Time the part of the Conv -> BatchNorm -> LeakyReLU block that is not the convolution, forward and backward, per distinct layer
shape of the FPNPlus model at 544 x 544: orienmask_amd.train.bn_leaky (csrc/bn_act.hip) against torch's batch_norm + in-place
leaky_relu (+ residual add) on the same GPU, both under autograd on a ready convolution output.  torch is the baseline: the parent
commit has no training forward.

Method: per shape and backend, WARMUP calls, then ROUNDS interleaved rounds (hip, torch, hip, ... so drift hits both alike); a round
times INNER back-to-back calls between two HIP events and divides.  Reported: median / min / max per call, bytes per second at the
median against the fused pass counts (forward 3 passes over the activation tensor, 4 with a residual; backward 5) and against torch's
(5 / 8, +2 / +0 with a residual), the host time per call (where it exceeds the device time the event figure is host-bound), the sum
over the BatchNorm layers (median x multiplicity; 86 in the FPNPlus model) with the sum of the per-shape minima and maxima as its run-to-run range, and the peak
memory of one full training step (forward + backward of the whole model) for both backends.

--dtype fp32 (default) times float32 activations; --dtype bf16 the bf16 entry points (the models' amp='bf16') against torch's bf16
batch_norm + leaky_relu, under the names hip_bf16 / torch_bf16; --dtype both times all four in the same interleaved rounds, which
is what a comparison of the two types needs.  Bytes are counted with the type's element size; the passes are the same.

    python tools/bench_bn_act.py [--batches 8 32] [--rounds 7] [--inner 5] [--warmup 3] [--dtype fp32|bf16|both]
                                 [--out profiles/bn_act_bench.json]

prints one JSON line (and writes it to --out).
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
import torch.nn.functional as F  # noqa: E402

from orienmask_amd import arch, train  # noqa: E402

HBM_BYTES_PER_S = 6.3e12      # achievable, MI355X


def layer_table(size):
    """(C, H, W, residual) -> number of BatchNorm layers with that shape."""
    table = {}
    for spec in arch.fpnplus_convs():
        if spec.bn:
            d = arch.layer_div(spec)
            key = (spec.cout, size // d, size // d, arch.is_residual_tail(spec))
            table[key] = table.get(key, 0) + 1
    return table


def torch_block(h, bn, res):
    y = F.leaky_relu(F.batch_norm(h, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps), 0.1, inplace=True)
    return y if res is None else y + res


def hip_block(h, bn, res):
    return train.bn_leaky(h, bn, residual=res)


def time_calls(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    t1 = time.perf_counter()
    stop.synchronize()
    return start.elapsed_time(stop) / inner, (t1 - t0) * 1e3 / inner


DTYPES = {"fp32": (torch.float32, ""), "bf16": (torch.bfloat16, "_bf16")}


def variants(dtype):
    """name -> (block, tensor dtype): hip / torch for float32, hip_bf16 / torch_bf16 for bf16."""
    kinds = ("fp32", "bf16") if dtype == "both" else (dtype,)
    return {name + DTYPES[k][1]: (fn, DTYPES[k][0]) for k in kinds for name, fn in (("hip", hip_block), ("torch", torch_block))}


def bench_shape(dev, B, C, H, W, residual, args):
    gen = torch.Generator(device=dev).manual_seed(C + H)
    blocks = variants(args.dtype)
    data = {}
    for dt in {d for _, d in blocks.values()}:          # the same values in either type, up to bf16's rounding
        gen.manual_seed(C + H)
        data[dt] = (torch.randn(B, C, H, W, device=dev, generator=gen).to(dt).requires_grad_(True),
                    torch.randn(B, C, H, W, device=dev, generator=gen).to(dt) if residual else None,
                    torch.randn(B, C, H, W, device=dev, generator=gen).to(dt))
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    out = {}
    state = {}

    def fwd(name):
        fn, dt = blocks[name]
        h, res, _ = data[dt]
        state[name] = fn(h, bn, res)

    def bwd(name):
        h, _, gy = data[blocks[name][1]]
        h.grad = None
        state[name].backward(gy, retain_graph=True)

    for name in blocks:
        for _ in range(args.warmup):
            fwd(name)
            bwd(name)
    samples = {(n, p): [] for n in blocks for p in ("fwd", "bwd")}
    host = {(n, p): [] for n in blocks for p in ("fwd", "bwd")}
    for _ in range(args.rounds):
        for name in blocks:
            d, hst = time_calls(lambda: fwd(name), args.inner)
            samples[(name, "fwd")].append(d); host[(name, "fwd")].append(hst)
            d, hst = time_calls(lambda: bwd(name), args.inner)
            samples[(name, "bwd")].append(d); host[(name, "bwd")].append(hst)
    passes = {("hip", "fwd"): 3 + (1 if residual else 0), ("hip", "bwd"): 5, ("torch", "fwd"): 5 + (3 if residual else 0), ("torch", "bwd"): 8}
    for key, v in samples.items():
        v = sorted(v)
        med = statistics.median(v)
        hm = statistics.median(host[key])
        tensor_bytes = blocks[key[0]][1].itemsize * B * C * H * W
        n_pass = passes[(key[0].split("_")[0], key[1])]
        out["%s_%s" % key] = {"ms_median": round(med, 5), "ms_min": round(v[0], 5), "ms_max": round(v[-1], 5),
                              "passes_counted": n_pass, "GBps_at_median": round(n_pass * tensor_bytes / med / 1e6, 1),
                              "share_of_6.3TBps": round(n_pass * tensor_bytes / (med * 1e-3) / HBM_BYTES_PER_S, 3),
                              "host_ms_median": round(hm, 5), "host_bound": hm > 0.9 * med}
    return out


def step_peak_memory(dev, backend, B, size, amp=None):
    torch.manual_seed(0)
    net = train.OrienMaskYOLOFPNPlus(3, 80, backend=backend, amp=amp).to(dev).train()
    x = torch.rand(B, 3, size, size, device=dev)
    for _ in range(2):                    # the second step is the steady state (gradients exist, the allocator is warm)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = net(x)
        sum(t.square().mean() for pair in out for t in pair).backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev)
    del net, out
    torch.cuda.empty_cache()
    return {"batch": B, "peak_bytes": int(peak), "peak_above_model_bytes": int(peak - base)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--size", type=int, default=544)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--memory-batch", type=int, default=8)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "both"], default="fp32", help="the activations' type (see above)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bn_act.py needs an MI355X: there is nothing to time on a CPU")
    dev = torch.device("cuda:0")
    table = layer_table(args.size)
    names = list(variants(args.dtype))
    result = {"bench": "bn_act", "dtype": args.dtype, "size": args.size, "rounds": args.rounds, "inner": args.inner, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batches": {}}
    for B in args.batches:
        rows, sums = [], {}
        for (C, H, W, residual), count in sorted(table.items(), key=lambda kv: -kv[0][0] * kv[0][1] * kv[0][2]):
            r = bench_shape(dev, B, C, H, W, residual, args)
            rows.append({"C": C, "H": H, "W": W, "residual": residual, "layers": count, **r})
            for k, v in r.items():
                s = sums.setdefault(k, {"ms_median": 0.0, "ms_min": 0.0, "ms_max": 0.0})
                for f in s:
                    s[f] += count * v[f]
            torch.cuda.empty_cache()
        slower = [{"C": r["C"], "H": r["H"], "residual": r["residual"], "pass": p, "sfx": sfx, "hip_ms": r["hip%s_%s" % (sfx, p)]["ms_median"],
                   "torch_ms": r["torch%s_%s" % (sfx, p)]["ms_median"]} for r in rows for p in ("fwd", "bwd")
                  for sfx in ("", "_bf16") if "hip" + sfx in names
                  if r["hip%s_%s" % (sfx, p)]["ms_median"] > r["torch%s_%s" % (sfx, p)]["ms_median"]]
        batch = {"shapes": rows, "layers": sum(table.values()), "sum_over_layers_ms": {k: {f: round(x, 4) for f, x in v.items()} for k, v in sums.items()},
                 "shapes_where_hip_is_slower": slower}
        if args.dtype == "both":
            batch["shapes_where_hip_bf16_is_slower_than_hip_fp32"] = [
                {"C": r["C"], "H": r["H"], "residual": r["residual"], "pass": p, "bf16_ms": r["hip_bf16_" + p]["ms_median"],
                 "fp32_ms": r["hip_" + p]["ms_median"]} for r in rows for p in ("fwd", "bwd")
                if r["hip_bf16_" + p]["ms_median"] > r["hip_" + p]["ms_median"]]
        result["batches"][str(B)] = batch
    result["training_step_peak_memory"] = {n: step_peak_memory(dev, n.split("_")[0], args.memory_batch, args.size,
                                                               "bf16" if n.endswith("_bf16") else None) for n in names}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
