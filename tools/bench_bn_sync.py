"""Time the synchronised BatchNorm + LeakyReLU block (om_bn_sync_* of csrc/bn_act.hip).

1. One device, R == 1, through the C ABI, per distinct BatchNorm layer shape of the FPNPlus model at 544 x 544: the staged pair
   (om_bn_sync_stats + om_bn_sync_forward; om_bn_sync_backward_sums + om_bn_sync_backward_dx) against om_bn_act_forward /
   om_bn_act_backward on the same buffers.  The passes over memory are the same; the staged form has one more (per-channel) launch
   where a channel takes several workgroups, and cannot fuse the two phases where a channel takes one.
2. --ranks 2 (needs two devices): one training forward + backward of the whole model at --batch images per rank, the converted 'hip'
   model against the same model on torch's SyncBatchNorm + LeakyReLU, both inside DistributedDataParallel.  The script starts one
   fresh child process of itself per rank (nccl, one device each) and reports rank 0's timings.

Method (tools/bench_bn_act.py): WARMUP calls, then ROUNDS interleaved rounds (a, b, a, ...), each timing INNER back-to-back calls
between two HIP events; median / min / max per call.

    python tools/bench_bn_sync.py [--batch 8] [--rounds 7] [--inner 5] [--warmup 3] [--ranks 2] [--out profiles/bn_sync_bench.json]
    python tools/bench_bn_sync.py --ranks 2 --profile-steps 3      # children only run steps of the 'hip' model (for a kernel trace)

prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import subprocess
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from orienmask_amd import arch, lib as omlib, train  # noqa: E402

MOMENTUM, EPS, SLOPE = 0.1, 1e-5, 0.1


def layer_table(size):
    """(C, H, W, residual) -> number of BatchNorm layers with that shape."""
    table = {}
    for spec in arch.fpnplus_convs():
        if spec.bn:
            d = arch.layer_div(spec)
            key = (spec.cout, size // d, size // d, arch.is_residual_tail(spec))
            table[key] = table.get(key, 0) + 1
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


def interleaved(fns, args):
    """name -> {ms_median, ms_min, ms_max} of the callables, rounds interleaved."""
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    samples = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            samples[k].append(time_calls(fn, args.inner))
    return {k: {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5)}
            for k, v in samples.items()}


# ---------------------------------------------------------------------------------------------------------------- 1: C ABI, R == 1
def bench_shape(dev, B, C, H, W, residual, args):
    L = omlib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(C + H)
    x = torch.randn(B, C, H, W, device=dev, generator=gen)
    dy = torch.randn(B, C, H, W, device=dev, generator=gen)
    res = torch.randn(B, C, H, W, device=dev, generator=gen) if residual else None
    y, dx = torch.empty_like(x), torch.empty_like(x)
    gamma, beta, rm, rv = (torch.rand(C, device=dev) + 0.5 for _ in range(4))
    sm, si, dg, db = (torch.empty(2 * C, device=dev) for _ in range(4))
    nbt = torch.zeros((), dtype=torch.long, device=dev)
    rec, sums, nt = (torch.empty(n, dtype=torch.float64, device=dev) for n in (3 * C, 2 * C, 1))
    ws = torch.empty(max(L.om_bn_act_workspace_bytes(B, C, H, W), 16), dtype=torch.uint8, device=dev)
    st = omlib.current_stream_ptr(dev)

    def plain_fwd():
        omlib.check(L.om_bn_act_forward(vp(x), B, C, H, W, vp(gamma), vp(beta), vp(rm), vp(rv), vp(nbt), 1, MOMENTUM, EPS, SLOPE, vp(res),
                                        vp(y), vp(sm), vp(si), vp(ws), ws.numel(), st), "om_bn_act_forward")

    def sync_fwd():
        omlib.check(L.om_bn_sync_stats(vp(x), B, C, H, W, vp(rec), vp(ws), ws.numel(), st), "om_bn_sync_stats")
        omlib.check(L.om_bn_sync_forward(vp(x), B, C, H, W, vp(rec), 1, vp(gamma), vp(beta), vp(rm), vp(rv), vp(nbt), MOMENTUM, EPS, SLOPE,
                                         vp(res), vp(y), vp(sm), vp(si), vp(nt), st), "om_bn_sync_forward")

    def plain_bwd():
        omlib.check(L.om_bn_act_backward(vp(x), vp(dy), B, C, H, W, vp(gamma), vp(beta), vp(sm), vp(si), 1, SLOPE, vp(dx), vp(dg), vp(db),
                                         vp(ws), ws.numel(), st), "om_bn_act_backward")

    def sync_bwd():
        omlib.check(L.om_bn_sync_backward_sums(vp(x), vp(dy), B, C, H, W, vp(gamma), vp(beta), vp(sm), vp(si), SLOPE, vp(sums), vp(dg),
                                               vp(db), vp(ws), ws.numel(), st), "om_bn_sync_backward_sums")
        omlib.check(L.om_bn_sync_backward_dx(vp(x), vp(dy), B, C, H, W, vp(gamma), vp(beta), vp(sm), vp(si), SLOPE, vp(sums), 1, vp(nt),
                                             vp(dx), st), "om_bn_sync_backward_dx")

    sync_fwd()                                  # the save vectors and n_total the backward calls read
    r = interleaved({"plain_fwd": plain_fwd, "sync_fwd": sync_fwd}, args)
    r.update(interleaved({"plain_bwd": plain_bwd, "sync_bwd": sync_bwd}, args))
    for p in ("fwd", "bwd"):
        r["ratio_" + p] = round(r["sync_" + p]["ms_median"] / r["plain_" + p]["ms_median"], 3)
        r["plain_spread_" + p] = round(r["plain_" + p]["ms_max"] / r["plain_" + p]["ms_min"], 3)
    r["launches"] = "two" if B * H * W > 16384 else "one"
    return r


def bench_kernels(dev, args):
    rows, sums = [], {}
    for (C, H, W, residual), count in sorted(layer_table(args.size).items(), key=lambda kv: -kv[0][0] * kv[0][1] * kv[0][2]):
        r = bench_shape(dev, args.batch, C, H, W, residual, args)
        rows.append({"C": C, "H": H, "W": W, "residual": residual, "layers": count, **r})
        for k in ("plain_fwd", "sync_fwd", "plain_bwd", "sync_bwd"):
            sums[k] = sums.get(k, 0.0) + count * r[k]["ms_median"]
        torch.cuda.empty_cache()
    return {"batch": args.batch, "shapes": rows, "sum_over_layers_ms": {k: round(v, 4) for k, v in sums.items()},
            "ratio_fwd": round(sums["sync_fwd"] / sums["plain_fwd"], 3), "ratio_bwd": round(sums["sync_bwd"] / sums["plain_bwd"], 3)}


# ---------------------------------------------------------------------------------------------------------------- 2: two ranks
class _TorchBlock(nn.Module):
    """Conv -> torch.nn.SyncBatchNorm -> LeakyReLU (+ residual): the comparator block."""

    def __init__(self, blk):
        super().__init__()
        conv, bn = blk.conv_block[0], blk.conv_block[1]
        norm = nn.SyncBatchNorm(bn.num_features)
        norm.load_state_dict(bn.state_dict())
        self.conv_block = nn.Sequential(conv, norm, nn.LeakyReLU(SLOPE, inplace=True))

    def forward(self, x, residual=None):
        y = self.conv_block(x)
        return y if residual is None else y + residual


def _torch_sync_model():
    net = train.OrienMaskYOLOFPNPlus(3, 80, backend="torch")
    for name, blk in list(net._by_name.items()):
        if isinstance(blk, train.ConvBNLeaky):
            new = _TorchBlock(blk)
            *path, leaf = name.split(".")
            node = net
            for p in path:
                node = node._modules[p]
            node._modules[leaf] = new
            net._by_name[name] = new
    return net


def rank_child(args):
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=int(os.environ["WORLD_SIZE"]), device_id=dev)
    try:
        torch.manual_seed(0)
        x = torch.rand(args.batch, 3, args.size, args.size, device=dev)
        nets = {"hip": DistributedDataParallel(train.convert_sync_batchnorm(train.OrienMaskYOLOFPNPlus(3, 80)).to(dev), device_ids=[rank])}
        if not args.profile_steps:
            nets["torch"] = DistributedDataParallel(_torch_sync_model().to(dev), device_ids=[rank])

        def step(net):
            out = net(x)
            sum(t.square().mean() for pair in out for t in pair).backward()

        if args.profile_steps:
            for _ in range(args.profile_steps):
                step(nets["hip"])
            torch.cuda.synchronize()
            return
        r = interleaved({k: (lambda n=n: step(n)) for k, n in nets.items()}, args)
        r["ratio"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 3)
        if rank == 0:
            print("RANK0 " + json.dumps(r), flush=True)
    finally:
        dist.destroy_process_group()


def bench_ranks(args):
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, os.path.abspath(__file__), "--rank-child", "--batch", str(args.batch), "--size", str(args.size), "--rounds",
           str(args.rounds), "--inner", str(args.inner), "--warmup", str(args.warmup), "--profile-steps", str(args.profile_steps)]
    children = [subprocess.Popen(cmd, env=dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.ranks), MASTER_ADDR="127.0.0.1",
                                               MASTER_PORT=str(port)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                for r in range(args.ranks)]
    outs = []
    for p in children:
        try:
            outs.append(p.communicate(timeout=args.child_timeout)[0])
        except subprocess.TimeoutExpired:
            for q in children:
                q.kill()
            raise SystemExit("a rank did not finish within %d s" % args.child_timeout)
        if p.returncode != 0:
            for q in children:
                q.terminate()
            raise SystemExit("a rank failed (%s):\n%s" % (p.returncode, outs[-1][-3000:]))
    for line in outs[0].splitlines():
        if line.startswith("RANK0 "):
            return dict(json.loads(line[6:]), ranks=args.ranks, batch_per_rank=args.batch)
    return {"ranks": args.ranks, "profile_steps": args.profile_steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=544)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ranks", type=int, default=0, help="2: also time the two-rank training step (needs two devices)")
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--rank-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bn_sync.py needs an MI355X: there is nothing to time on a CPU")
    if args.rank_child:
        return rank_child(args)
    result = {"bench": "bn_sync", "size": args.size, "rounds": args.rounds, "inner": args.inner, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if args.ranks:
        if torch.cuda.device_count() < args.ranks:
            raise SystemExit("--ranks %d needs %d devices, %d visible" % (args.ranks, args.ranks, torch.cuda.device_count()))
        result["two_ranks"] = bench_ranks(args)
    if not args.profile_steps:
        result["kernels_one_rank"] = bench_kernels(torch.device("cuda:0"), args)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
