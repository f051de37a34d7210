"""Time the up-sampling / concat / split of the training models at 544 x 544: train.upsample_concat and train.split_channels
(csrc/route.hip, what route_backend='hip' runs) against torch's composition (F.interpolate + torch.cat, torch.split + .contiguous(),
and autograd's backward of them: what route_backend='torch' runs) on the same GPU and the same tensors.

Sites: cat16 (256 x 17^2 x2 with 512 x 34^2), cat8 (128 x 34^2 x2 with 256 x 68^2), the Plus model's cat4 (64 x 17^2 x8, 64 x 34^2
x4, 64 x 68^2 x2, 64 x 136^2) and the orientation split 18 -> 6, 6, 6 at 136^2; forward and backward each.

Method (tools/bench_conv_fwd.py's): per site, WARMUP calls of each side, then ROUNDS interleaved rounds; a round times INNER
back-to-back calls between two HIP events and divides.  Three sides: 'hip' (the train function under autograd), 'torch' (the
composition under autograd) and 'hip_kernel' (the C entry point alone, without the Python around it).  The backward is
torch.autograd.grad through a retained graph, so it is the backward alone.  Reported: median / min / max per call and algorithmic
bytes over the median.  Algorithmic bytes, by count, S1 the scale-1 sources and Su the up-sampled ones (|t| the bytes of t, |up(t)|
of t up-sampled):
    hip, either direction        every source once and y once: sum |src| + |y|
    torch concat forward         interpolate reads src and writes up(src); cat reads every part and writes y:
                                 sum over Su (|src| + |up(src)|) + 2 |y|
    torch concat backward        at least: the slice of dy read and d src written per up-sampled source; a scale-1 source gets a
                                 VIEW of dy, no bytes (its consumer pays for the copy later):  sum over Su (|up(src)| + |src|).
                                 A lower bound: what torch's kernels move beyond it is not counted
    torch split, either way      each output copied (forward), the gradients gathered into one tensor (backward): 2 |x|
And one whole training step (forward + backward, backend / conv_backend / conv_forward all 'hip') with route_backend 'torch'
against 'hip': median of interleaved rounds and peak memory.

    python tools/bench_route.py [--batches 8 32] [--rounds 5] [--inner 3] [--warmup 2] [--out profiles/route_bench.json]

prints one JSON line (and writes it to --out); a progress line per site goes to stderr.
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

from orienmask_amd import lib as omlib, train  # noqa: E402


def sites(size):
    """name -> ('concat' | 'split', H, [(channels, scale)]) at this image size."""
    s32, s16, s8, s4 = size // 32, size // 16, size // 8, size // 4
    assert s32 * 32 == size
    return {"cat16": ("concat", s16, [(256, 2), (512, 1)]),
            "cat8": ("concat", s8, [(128, 2), (256, 1)]),
            "cat4_plus": ("concat", s4, [(64, 8), (64, 4), (64, 2), (64, 1)]),
            "orien_split": ("split", s4, [(6, 1), (6, 1), (6, 1)])}


def time_calls(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def algorithmic_bytes(kind, B, H, parts):
    y = 4 * B * sum(c for c, _ in parts) * H * H
    if kind == "split":
        return {"hip": 2 * y, "torch_fwd": 2 * y, "torch_bwd": 2 * y}
    src = [4 * B * c * (H // s) ** 2 for c, s in parts]
    up = [4 * B * c * H * H for c, _ in parts]
    ups = [i for i, (_, s) in enumerate(parts) if s > 1]
    return {"hip": sum(src) + y,
            "torch_fwd": sum(src[i] + up[i] for i in ups) + 2 * y,
            "torch_bwd": sum(up[i] + src[i] for i in ups)}


def bench_site(dev, B, kind, H, parts, args):
    L = omlib.load()
    gen = torch.Generator(device=dev).manual_seed(B + H)
    chans, scales = [c for c, _ in parts], [s for _, s in parts]
    srcs = [torch.randn(B, c, H // s, H // s, device=dev, generator=gen).requires_grad_(True) for c, s in parts]
    whole = torch.randn(B, sum(chans), H, H, device=dev, generator=gen)       # dy of the concat, x of the split
    st = omlib.current_stream_ptr(dev)
    ci, si = (ctypes.c_int * 4)(*chans + [0] * (4 - len(chans))), (ctypes.c_int * 4)(*scales + [0] * (4 - len(chans)))
    table = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts] + [None] * (4 - len(ts)))      # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    out_whole = torch.empty_like(whole)
    out_parts = [torch.empty_like(t) for t in srcs]
    n = len(parts)
    k_gather = lambda: omlib.check(L.om_route_concat_forward(table([t.detach() for t in srcs]), ci, si, n, B, H, H, vp(out_whole), st), "fwd")      # noqa: E731
    k_scatter = lambda: omlib.check(L.om_route_concat_backward(vp(whole), ci, si, n, B, H, H, table(out_parts), st), "bwd")      # noqa: E731
    if kind == "concat":
        compose = lambda: torch.cat([F.interpolate(t, scale_factor=s, mode="nearest") if s > 1 else t      # noqa: E731
                                     for t, s in zip(srcs, scales)], dim=1)
        y_hip, y_torch = train.upsample_concat(srcs, scales), compose()
        assert torch.equal(y_hip, y_torch)
        calls = {
            "fwd": {"hip": lambda: train.upsample_concat(srcs, scales), "torch": compose, "hip_kernel": k_gather},
            "bwd": {"hip": lambda: torch.autograd.grad(y_hip, srcs, whole, retain_graph=True),
                    "torch": lambda: torch.autograd.grad(y_torch, srcs, whole, retain_graph=True), "hip_kernel": k_scatter},
        }
    else:
        x = whole.requires_grad_(True)
        cots = [t.detach() for t in srcs]
        o_hip = train.split_channels(x, chans)
        o_torch = [t.contiguous() for t in torch.split(x, chans, dim=1)]
        assert all(torch.equal(a, b) for a, b in zip(o_hip, o_torch))
        calls = {
            "fwd": {"hip": lambda: train.split_channels(x, chans),
                    "torch": lambda: [t.contiguous() for t in torch.split(x, chans, dim=1)], "hip_kernel": k_scatter},
            "bwd": {"hip": lambda: torch.autograd.grad(o_hip, x, cots, retain_graph=True),
                    "torch": lambda: torch.autograd.grad(o_torch, x, cots, retain_graph=True), "hip_kernel": k_gather},
        }
    nbytes = algorithmic_bytes(kind, B, H, parts)
    out = {}
    for direction, sides in calls.items():
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        samples = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                samples[k].append(time_calls(fn, args.inner))
        row = {}
        for k, v in samples.items():
            v = sorted(v)
            med = statistics.median(v)
            moved = nbytes["hip"] if k != "torch" else nbytes["torch_" + direction]
            row[k] = {"ms_median": round(med, 5), "ms_min": round(v[0], 5), "ms_max": round(v[-1], 5), "algorithmic_bytes": moved,
                      "GBps_at_median": round(moved / (med * 1e-3) / 1e9, 1)}
        out[direction] = row
    return out


def step_times_and_memory(dev, B, size, rounds):
    """One training step (forward + backward of the whole model, everything else HIP) per route_backend: median ms of interleaved
    rounds, peak memory."""
    x = torch.rand(B, 3, size, size, device=dev)
    nets = {}
    for rb in ("torch", "hip"):
        torch.manual_seed(0)
        nets[rb] = train.OrienMaskYOLOFPNPlus(3, 80, backend="hip", conv_backend="hip", conv_forward="hip", route_backend=rb).to(dev).train()

    def step(rb):
        out = nets[rb](x)
        sum(t.square().mean() for pair in out for t in pair).backward()

    result = {rb: {"route_backend": rb, "batch": B} for rb in nets}
    for rb in nets:
        for _ in range(2):                # the second step is the steady state (gradients exist, the allocator is warm)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            step(rb)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev)
        result[rb].update(peak_bytes=int(peak), peak_above_resident_bytes=int(peak - base))
    samples = {rb: [] for rb in nets}
    for _ in range(rounds):
        for rb in nets:
            samples[rb].append(time_calls(lambda: step(rb), 1))
    for rb, v in samples.items():
        v = sorted(v)
        result[rb].update(step_ms_median=round(statistics.median(v), 3), step_ms_min=round(v[0], 3), step_ms_max=round(v[-1], 3))
    return [result[rb] for rb in ("torch", "hip")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--size", type=int, default=544)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_route.py needs an MI355X: there is nothing to time on a CPU")
    dev = torch.device("cuda:0")
    result = {"bench": "route", "size": args.size, "rounds": args.rounds, "inner": args.inner, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batches": {}}
    for B in args.batches:
        rows, slower = {}, []
        for name, (kind, H, parts) in sites(args.size).items():
            r = bench_site(dev, B, kind, H, parts, args)
            rows[name] = dict(kind=kind, H=H, parts=parts, **r)
            print("B=%d %s: %s" % (B, name, {d: {k: v["ms_median"] for k, v in row.items()} for d, row in r.items()}),
                  file=sys.stderr, flush=True)
            for d, row in r.items():
                # slower than torch by more than the rounds' own spread: the medians differ by more than either side's min-max
                spread = max(row["hip"]["ms_max"] - row["hip"]["ms_min"], row["torch"]["ms_max"] - row["torch"]["ms_min"])
                if row["hip"]["ms_median"] - row["torch"]["ms_median"] > spread:
                    slower.append({"site": name, "direction": d, "hip_ms": row["hip"]["ms_median"], "torch_ms": row["torch"]["ms_median"],
                                   "hip_kernel_ms": row["hip_kernel"]["ms_median"], "spread_ms": round(spread, 5)})
            torch.cuda.empty_cache()
        result["batches"][str(B)] = {"sites": rows, "sites_where_hip_is_slower_beyond_the_spread": slower}
    result["training_step"] = step_times_and_memory(dev, args.step_batch, args.size, args.rounds)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
