"""The yardstick of the Adam tests: torch.optim.Adam / AdamW (amsgrad=False) restated in numpy, float32 per element with ONE
rounding per operation, fused multiply-adds through optim_np.fma32 (orienmask_amd/optim.py HipAdam / HipAdamW, csrc/optim.hip;
DESIGN.md section 3.16.3).

    g  = g * coef                                   (clipping only; ahead of everything else)
    g  = -g                                         (maximize)
    p  = p * float32(1 - lr * wd)                   (AdamW, wd != 0)
    g  = fma(p, wd, g)                              (Adam, wd != 0)
    d  = g - m
    m  = |w| < 0.5 ? fma(w, d, m) : fma(w - 1, d, g)          w = float32(1 - beta1)
    v  = fma(float32(1 - beta2) * g, g, v * beta2)
    den = sqrt(v) / float32(bc2s) + eps
    p  = p + (float32(-(lr / bc1)) * m) / den

bc1 = 1 - beta1 ** step and bc2s = (1 - beta2 ** step) ** 0.5 in Python doubles, step the tensor's own count as a float.
``sqrt`` is a parameter: ieee_sqrt is the contract; torch_sqrt (torch's CPU Tensor.sqrt, whose vectorised body is not correctly
rounded) is what makes the restatement equal torch-CPU bit for bit on long tensors.  ``mutant`` swaps one operation for a
near-equivalent one that the tests must tell apart.  ``sqrt(bc2)`` for ``bc2 ** 0.5`` is not among them: the two differ in double at
some step counts, but no count was found at which their float32 values differ, so no element can tell them apart; the doubles of
the bias table can (tests/test_adam_cpu.py::test_pow_one_half_is_not_sqrt).
"""
import numpy as np

from optim_np import F32, fma32, same_bits      # noqa: F401  (same_bits is re-exported for the tests)

MUTANTS = ("lerp_mul_add", "addcmul_square_first", "fma_last")


def ieee_sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(x, F32)).astype(F32)         # the hardware's float32 sqrt: correctly rounded


def torch_sqrt(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).sqrt().numpy()


def corrections(beta1, beta2, step):
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return bias_correction1, bias_correction2 ** 0.5


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, decoupled=False, coef=None,
              sqrt=ieee_sqrt, mutant=None):
    """One step of one tensor; ``step`` is the number of this step for this tensor (1.0 for the first).  Returns new (p, m, v)."""
    assert mutant is None or mutant in MUTANTS
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    beta1, beta2 = betas
    with np.errstate(all="ignore"):
        if coef is not None:
            g = (g * F32(coef)).astype(F32)
        if maximize:
            g = -g
        if weight_decay != 0:
            if decoupled:
                p = (p * F32(1 - lr * weight_decay)).astype(F32)
            else:
                g = fma32(p, F32(weight_decay), g)
        w = F32(1 - beta1)
        d = (g - m).astype(F32)
        if mutant == "lerp_mul_add":
            m = (m + (w * d).astype(F32)).astype(F32) if abs(w) < 0.5 else (g + ((w - F32(1)) * d).astype(F32)).astype(F32)
        elif abs(w) < 0.5:
            m = fma32(w, d, m)
        else:
            m = fma32(F32(w - F32(1)), d, g)
        omb2 = F32(1 - beta2)
        scaled = (v * F32(beta2)).astype(F32)
        if mutant == "addcmul_square_first":
            v = fma32(omb2, (g * g).astype(F32), scaled)
        else:
            v = fma32((omb2 * g).astype(F32), g, scaled)
        bc1, bc2s = corrections(beta1, beta2, step)
        den = ((sqrt(v) / F32(bc2s)).astype(F32) + F32(eps)).astype(F32)
        nss = F32(-(lr / bc1))
        if mutant == "fma_last":
            p = fma32(nss, (m / den).astype(F32), p)        # addcdiv as p + value * (m / den), fused
        else:
            p = (p + ((nss * m).astype(F32) / den).astype(F32)).astype(F32)
        return p, m, v


class Reference:
    """Several tensors stepped together, each with its own hyper-parameters and its own count (a tensor whose gradient is None
    in a step does not advance, as torch's per-parameter ``state['step']``)."""

    def __init__(self, params, hypers, decoupled, sqrt=ieee_sqrt):
        self.p = [np.array(a, F32).reshape(-1) for a in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.k = [0.0] * len(self.p)
        self.hypers = [dict(hypers) for _ in self.p] if isinstance(hypers, dict) else [dict(h) for h in hypers]
        self.decoupled = decoupled
        self.sqrt = sqrt

    def step(self, grads, coef=None):
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.k[i] += 1.0
            self.p[i], self.m[i], self.v[i] = adam_step(self.p[i], np.asarray(g, F32).reshape(-1), self.m[i], self.v[i], self.k[i],
                                                        decoupled=self.decoupled, coef=coef, sqrt=self.sqrt, **self.hypers[i])


def torch_cpu_run(p0, grads, hyper, decoupled, lrs=None):
    """torch.optim.Adam / AdamW (foreach=False) on CPU float32 tensors; grads may hold None (no gradient in that step); lrs: one
    learning rate per step (a schedule).  Returns per step (p, exp_avg, exp_avg_sq) as numpy arrays."""
    import torch
    p = torch.nn.Parameter(torch.from_numpy(np.array(p0, F32)))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], foreach=False, **hyper)
    out = []
    for s, g in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[s]
        p.grad = None if g is None else torch.from_numpy(np.array(g, F32))
        opt.step()
        st = opt.state[p] if p in opt.state else {}
        out.append((p.detach().numpy().copy(),
                    st["exp_avg"].numpy().copy() if "exp_avg" in st else np.zeros_like(p0, dtype=F32),
                    st["exp_avg_sq"].numpy().copy() if "exp_avg_sq" in st else np.zeros_like(p0, dtype=F32)))
    return out


def numpy_run(p0, grads, hyper, decoupled, lrs=None, sqrt=ieee_sqrt, mutant=None):
    p = np.array(p0, F32)
    m, v, k, out = np.zeros_like(p), np.zeros_like(p), 0.0, []
    for s, g in enumerate(grads):
        h = dict(hyper)
        if lrs is not None:
            h["lr"] = lrs[s]
        if g is not None:
            k += 1.0
            p, m, v = adam_step(p, g, m, v, k, decoupled=decoupled, sqrt=sqrt, mutant=mutant, **h)
        out.append((p.copy(), m.copy(), v.copy()))
    return out


# the hyper-parameter sets of the parity tests: (hyper, decoupled)
HYPER_SETS = {
    "adam": (dict(lr=1e-3), False),
    "adam_wd": (dict(lr=2e-3, weight_decay=5e-4), False),
    "adamw": (dict(lr=1e-3, weight_decay=1e-2), True),
    "adamw_wd0": (dict(lr=1e-3, weight_decay=0.0), True),
    "maximize": (dict(lr=1e-3, weight_decay=1e-2, maximize=True), True),
    "beta1_low": (dict(lr=1e-3, betas=(0.4, 0.99), weight_decay=5e-4), False),      # w = 0.6: the other branch of lerp
    "eps_large": (dict(lr=1e-2, eps=1e-3, weight_decay=1e-2), True),
}
SCHEDULE = (1e-4, 4e-4, 7e-4, 1e-3, 5e-4)       # a learning rate per step
ADAM_STEPS = 5


def seeded_inputs(seed, n, steps=ADAM_STEPS):
    """Parameter and per-step gradients with magnitudes over five decades, both signs."""
    rs = np.random.RandomState(seed)

    def draw():
        return (np.where(rs.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3.0, 2.0, n)).astype(F32)
    return draw(), [draw() for _ in range(steps)]


def special_inputs():
    """+-0, denormals, gradients whose square underflows, large values, NaN and Inf, every pairing of parameter and gradient."""
    tiny = np.float32(1e-45)
    vals = np.array([0.0, -0.0, tiny, -tiny, np.float32(1.1754942e-38), np.float32(-5.877e-39), np.float32(1e-25),
                     np.float32(-3e-23), 1.0, -2.5, np.float32(1e18), np.float32(3.4028235e38), np.inf, -np.inf, np.nan], dtype=F32)
    p = np.repeat(vals, vals.size)
    g = np.tile(vals, vals.size)
    rs = np.random.RandomState(7)
    grads = [g] + [np.where(rs.rand(g.size) < 0.5, g, rs.standard_normal(g.size).astype(F32) * F32(1e-20)).astype(F32)
                   for _ in range(2)]
    return p, grads
