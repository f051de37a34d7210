"""The yardstick of the optimizer tests: torch.optim.SGD's update restated in numpy with a TRUE single rounding per fused
multiply-add (orienmask_amd/optim.py, csrc/optim.hip).

    d   = fma(p, wd, g)                              (only if weight_decay != 0;  g negated first if maximize)
    buf = d                                          (first step of this tensor)
    buf = fma(d, 1 - dampening, buf * momentum)      (later steps; the product is rounded to float32 before the fma)
    d   = nesterov ? fma(buf, momentum, d) : buf     (only if momentum != 0)
    p   = fma(d, -lr, p)

with wd, momentum, 1 - dampening (computed in double, then rounded) and -lr as float32.

fma32 computes a * b + c of float32 operands with ONE rounding: the product of two float32 numbers is exact in float64
(24 + 24 bits), the float64 sum is rounded TO ODD (the error of the round-to-nearest sum is recovered exactly by TwoSum; where
it is not zero and the sum's last bit is even, the sum moves one step towards the exact value), and a round-to-odd float64
rounds to the same float32 as the exact value because float64 carries more than 24 + 2 bits.  A plain float64 multiply-add
rounded to float32 is a double rounding and is not the yardstick.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F32 = np.float32


def fma32(a, b, c):
    a = np.asarray(a, F32).astype(np.float64)
    b = np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        prod = a * b                                   # exact
        s = prod + c
        bb = s - prod
        err = (prod - (s - bb)) + (c - bb)             # TwoSum: prod + c == s + err exactly (finite operands)
        odd = (s.view(np.int64) & 1) == 1
        move = np.isfinite(s) & (err != 0) & ~odd
        towards = np.where((err > 0), np.inf, -np.inf)
        s = np.where(move, np.nextafter(s, towards), s)
        return s.astype(F32)


def sgd_step(p, g, buf, lr, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False, maximize=False):
    """One step of one tensor.  p, g: float32 arrays; buf: float32 array or None (first step).  Returns (p, buf) as new arrays;
    buf stays None when momentum == 0."""
    p = np.asarray(p, F32)
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        d = -g if maximize else g
        if weight_decay != 0:
            d = fma32(p, F32(weight_decay), d)
        if momentum != 0:
            if buf is None:
                buf = d.copy()
            else:
                scaled = (np.asarray(buf, F32) * F32(momentum)).astype(F32)
                buf = fma32(d, F32(1.0 - dampening), scaled)
            d = fma32(buf, F32(momentum), d) if nesterov else buf
        return fma32(d, F32(-lr), p), buf


def sgd_step_many(ps, gs, bufs, hypers, threads=8):
    """sgd_step over lists; hypers: one dict for all or a list of dicts.  g None: the tensor is passed through unchanged."""
    if isinstance(hypers, dict):
        hypers = [hypers] * len(ps)

    def one(i):
        if gs[i] is None:
            return ps[i], bufs[i]
        return sgd_step(ps[i], gs[i], bufs[i], **hypers[i])
    with ThreadPoolExecutor(threads) as ex:
        out = list(ex.map(one, range(len(ps))))
    return [o[0] for o in out], [o[1] for o in out]


# the hyper-parameter sets of the issue's probe, plus maximize
HYPER_SETS = {
    "momentum_decay": dict(lr=1e-3, momentum=0.9, weight_decay=5e-4),
    "nesterov": dict(lr=3e-3, momentum=0.9, weight_decay=1e-4, nesterov=True),
    "dampening": dict(lr=1e-2, momentum=0.8, dampening=0.3, weight_decay=5e-4),
    "plain": dict(lr=1e-2),
    "decay_only": dict(lr=1e-2, weight_decay=5e-4),
    "maximize": dict(lr=1e-3, momentum=0.9, weight_decay=5e-4, maximize=True),
}
SGD_STEPS = 4
SGD_N = 1003           # not a multiple of 4, 8 or 16: vector bodies and tails on the CPU and on the GPU


def seeded_inputs(seed, n=SGD_N, steps=SGD_STEPS):
    """Parameter and per-step gradients with magnitudes over five decades, both signs."""
    rs = np.random.RandomState(seed)
    def draw():
        return (np.where(rs.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3.0, 2.0, n)).astype(F32)
    return draw(), [draw() for _ in range(steps)]


def special_inputs(steps=SGD_STEPS):
    """Zeros of both signs, float32 denormals, +-Inf and NaN in parameter and gradient, every pairing of the classes, plus plain
    values around them (they propagate as in torch)."""
    tiny = np.float32(1e-45)
    vals = np.array([0.0, -0.0, tiny, -tiny, np.float32(1.1754942e-38), np.float32(-5.877e-39), 1.0, -2.5, 3.4028235e38,
                     np.inf, -np.inf, np.nan], dtype=F32)
    p = np.repeat(vals, vals.size)
    g = np.tile(vals, vals.size)
    rs = np.random.RandomState(7)
    grads = [g] + [np.where(rs.rand(g.size) < 0.5, g, rs.standard_normal(g.size).astype(F32) * F32(1e-38)).astype(F32)
                   for _ in range(steps - 1)]
    return p, grads


def torch_cpu_run(p0, grads, hyper, foreach=False):
    """(a): torch.optim.SGD on CPU float32 tensors.  Returns per step (param, momentum_buffer or None) as numpy arrays."""
    import torch
    p = torch.nn.Parameter(torch.from_numpy(np.array(p0, F32)))
    opt = torch.optim.SGD([p], foreach=foreach, **hyper)
    out = []
    for g in grads:
        p.grad = torch.from_numpy(np.array(g, F32))
        opt.step()
        b = opt.state[p].get("momentum_buffer") if p in opt.state else None
        out.append((p.detach().numpy().copy(), None if b is None else b.numpy().copy()))
    return out


def numpy_run(p0, grads, hyper):
    """(b): the same through sgd_step."""
    p, buf, out = np.array(p0, F32), None, []
    for g in grads:
        p, buf = sgd_step(p, g, buf, **hyper)
        out.append((p.copy(), None if buf is None else buf.copy()))
    return out


def same_bits(a, b):
    """Bit equality with NaN equal to NaN (any payload), as torch.equal(..., equal_nan) would give."""
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | nan))


# ---- the small module of the param_groups fixture (built the same way by tools/gen_golden_optim.py and by the test) --------------
def groups_module():
    """conv / BatchNorm / conv with bias / conv / GroupNorm / conv with bias / a frozen parameter / a weight shared by two
    modules: ordered so that both carry-overs of the reference's param_groups show (norm decay on the weights after a norm,
    bias decay on the weights after a bias)."""
    import torch
    nn = torch.nn

    class Scale(nn.Module):
        def __init__(self):
            super().__init__()
            self.gain = nn.Parameter(torch.ones(4))
            self.frozen = nn.Parameter(torch.zeros(4), requires_grad=False)

    torch.manual_seed(0)
    m = nn.Sequential()
    m.add_module("conv1", nn.Conv2d(3, 4, 3, bias=False))
    m.add_module("bn1", nn.BatchNorm2d(4))
    m.add_module("conv2", nn.Conv2d(4, 4, 3, bias=True))
    m.add_module("conv3", nn.Conv2d(4, 4, 1, bias=False))
    m.add_module("gn", nn.GroupNorm(2, 4))
    m.add_module("conv4", nn.Conv2d(4, 4, 1, bias=True))
    m.add_module("scale", Scale())
    m.add_module("conv5", nn.Conv2d(4, 4, 1, bias=False))
    m.add_module("tied", nn.Conv2d(4, 4, 1, bias=False))
    m.tied.weight = m.conv3.weight                       # one parameter, two modules
    m.add_module("bn2", nn.BatchNorm2d(4))
    m.bn2.bias.requires_grad_(False)
    return m


GROUPS_KWARGS = dict(base_lr=2e-3, weight_decay=5e-4, norm_weight_decay=0.0, bias_lr_factor=2.0, bias_weight_decay=1e-4)


def groups_listing(model, groups):
    """[(name, lr, weight_decay)] of a param_groups result, names from model.named_parameters()."""
    names = {id(p): k for k, p in model.named_parameters()}
    return [(names[id(g["params"][0])], float(g["lr"]), float(g["weight_decay"])) for g in groups]


# ---- schedules of the lr fixture ----------------------------------------------------------------------------------------------
SCHEDULE_BASE_LRS = (1e-3, 2.5e-4)
STEP_WARMUP_CASES = {
    "const": dict(warmup_type="const", warmup_iter=5, warmup_ratio=0.2, milestones=[8, 12], gamma=0.1),
    "linear": dict(warmup_type="linear", warmup_iter=5, warmup_ratio=0.1, milestones=[8, 12], gamma=0.1),
    "power": dict(warmup_type="power", warmup_iter=6, warmup_ratio=2.0, milestones=[9, 11], gamma=0.5),
}
STEP_WARMUP_ITERS = 16
POLY_CASE = dict(max_iter=20, power=0.9)
POLY_ITERS = 20


def lr_sequence(make_scheduler, iters):
    """[iters + 1, groups] learning rates: after construction, then after each scheduler.step() (an optimizer step before each,
    as a training loop does)."""
    import torch
    ps = [torch.nn.Parameter(torch.zeros(2)) for _ in SCHEDULE_BASE_LRS]
    opt = torch.optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(ps, SCHEDULE_BASE_LRS)], lr=1.0, momentum=0.9)
    sch = make_scheduler(opt)
    seq = [[g["lr"] for g in opt.param_groups]]
    for _ in range(iters):
        opt.step()
        sch.step()
        seq.append([g["lr"] for g in opt.param_groups])
    return np.asarray(seq, dtype=np.float64)
