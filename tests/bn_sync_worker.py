"""One rank of the two-device tests of tests/test_bn_sync.py: `python bn_sync_worker.py TASK OUTDIR` with RANK, WORLD_SIZE, LOCAL_RANK,
MASTER_ADDR and MASTER_PORT in the environment (nccl backend, one device per rank).  Writes OUTDIR/TASK_rank<RANK>.npz; the parent
judges.  Not a test module."""
import hashlib
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.nn as nn  # noqa: E402

import bn_act_np as N  # noqa: E402
from orienmask_amd import builder, synth, train  # noqa: E402

SD_SEED = 1
SIZE = 96


def _np(t):
    return t.detach().cpu().numpy()


def _digest(t):
    a = np.ascontiguousarray(_np(t))
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


class _Count:
    """Counts the calls of dist.all_gather_into_tensor while active."""

    def __enter__(self):
        self.calls, self.real = 0, dist.all_gather_into_tensor

        def counted(*args, **kwargs):
            self.calls += 1
            return self.real(*args, **kwargs)

        dist.all_gather_into_tensor = counted
        return self

    def __exit__(self, *exc):
        dist.all_gather_into_tensor = self.real


def block(rank, dev):
    torch.manual_seed(1)                                   # the same weights on both ranks
    hip = train.ConvBNLeaky(16, 32, 3, padding=1)
    with torch.no_grad():
        bn = hip.conv_block[1]
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
    ref = nn.Sequential(nn.Conv2d(16, 32, 3, padding=1, bias=False), nn.SyncBatchNorm(32), nn.LeakyReLU(0.1))
    ref[0].load_state_dict(hip.conv_block[0].state_dict())
    ref[1].load_state_dict(bn.state_dict())
    out = dict(weight=_np(hip.conv_block[0].weight), gamma=_np(bn.weight), beta=_np(bn.bias), rm0=_np(bn.running_mean),
               rv0=_np(bn.running_var))
    hip, ref = train.convert_sync_batchnorm(hip).to(dev).train(), ref.to(dev).train()
    gen = torch.Generator().manual_seed(10 + rank)         # another batch on each rank
    x = torch.randn(2, 16, 12, 12, generator=gen)
    gy = torch.randn(2, 32, 12, 12, generator=gen)
    out.update(x=x.numpy(), gy=gy.numpy())
    x, gy = x.to(dev), gy.to(dev)
    for side, m, (conv, norm) in (("hip", hip, (hip.conv_block[0], hip.conv_block[1])), ("torch", ref, (ref[0], ref[1]))):
        xi = x.clone().requires_grad_(True)
        with _Count() as count:
            y = m(xi)
            y.backward(gy)
        if side == "hip":
            out["train_gathers"] = count.calls
        out.update({side + "_y": _np(y), side + "_dx": _np(xi.grad), side + "_dweight": _np(conv.weight.grad),
                    side + "_dgamma": _np(norm.weight.grad), side + "_dbeta": _np(norm.bias.grad), side + "_rm": _np(norm.running_mean),
                    side + "_rv": _np(norm.running_var), side + "_nbt": _np(norm.num_batches_tracked)})
    h = hip.conv_block[0](x).detach()                      # a BatchNorm input that needs no gradient: no second all-gather
    with _Count() as count:
        train.bn_leaky(h, hip.conv_block[1], sync=True).backward(gy)
    out["nograd_gathers"] = count.calls
    hip.eval()
    with _Count() as count:
        hip(x.clone().requires_grad_(True)).backward(gy)
    out["eval_gathers"] = count.calls
    return out


def model(rank, dev):
    cfg = dict(type="OrienMaskYOLOFPNPlus", num_anchors=3, num_classes=80, pretrained=None, freeze_backbone=False,
               backbone_batchnorm_eval=False)
    net = builder.build_train_model(cfg, is_distributed=True)
    assert type(net) is torch.nn.parallel.DistributedDataParallel and net.module.backend == "hip"
    assert all(m.sync for m in net.module.modules() if isinstance(m, train.ConvBNLeaky))
    net.module.load_state_dict(synth.synth_state_dict(SD_SEED), strict=True)
    x = synth.synth_image_batch(40 + rank, 2, SIZE, SIZE)
    out = dict(x=x.numpy(), sd_seed=SD_SEED)
    out["nbt_before"] = np.array([int(v) for k, v in net.module.state_dict().items() if k.endswith("num_batches_tracked")])
    heads = [t for pair in net(x.to(dev)) for t in pair]
    cot = N.cotangents(50 + rank, [t.shape for t in heads])
    torch.autograd.backward(heads, [torch.from_numpy(c).to(dev) for c in cot])
    params = list(net.module.named_parameters())
    out["param_names"] = np.array([n for n, _ in params])
    for i, (t, c) in enumerate(zip(heads, cot)):
        out["head%d" % i], out["cot%d" % i] = _np(t), c
    out["grad_digest"] = np.array([_digest(p.grad) for _, p in params])
    if rank == 0:                                          # the gradients are the same on both ranks (the digests say so): once
        for n, p in params:
            out["grad." + n] = _np(p.grad)
    optimizer = builder.build_optimizer(dict(type="SGD", lr=1e-3, momentum=0.9, weight_decay=5e-4), 1, net, is_distributed=True)
    optimizer.step()
    state = net.module.state_dict()
    out["state_keys"] = np.array(list(state))
    out["state_digest"] = np.array([_digest(v) for v in state.values()])
    out["nbt"] = np.array([int(v) for k, v in state.items() if k.endswith("num_batches_tracked")])
    return out


def main():
    task, outdir = sys.argv[1], sys.argv[2]
    rank, local = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", os.environ["RANK"]))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("nccl", rank=rank, world_size=int(os.environ["WORLD_SIZE"]), device_id=dev)
    try:
        out = {"block": block, "model": model}[task](rank, dev)
        torch.cuda.synchronize(dev)
        np.savez(os.path.join(outdir, "%s_rank%d.npz" % (task, rank)), **out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
