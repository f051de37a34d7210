"""The yardstick of the gradient-clipping tests (om_sgd_clip_step, csrc/optim.hip; orienmask_amd.optim.SGD(max_grad_norm=...)):
torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.SGD.step(), restated in numpy.

The norm restates the kernels' ORDER of summation in float64:
    chunk      OM_SGD_CHUNK consecutive elements of one tensor; element j of a chunk belongs to lane (j // 4) % 256, a lane adds the
               exact float64 squares of its elements in ascending order (a missing element adds + 0.0, which changes no sum)
    tree       the 256 lane sums: within each wave of 64, lanes l < d take lane l + d for d = 32, 16, 8, 4, 2, 1; then
               (w0 + w1) + (w2 + w3) over the four waves
    finish     lane l adds the chunks' sums l, l + 256, ... in ascending order (chunks in table order: tensor by tensor, tensors
               without a gradient contribute 0.0), the same tree gives S; total_norm = float32(sqrt(S))
The coefficient and the product are float32 with one rounding per operation, as torch 2.10 computes them on the CPU:
    coef = min(1, float32(1) / (total_norm + float32(1e-6)) * float32(max_norm))        (Tensor.__rdiv__ is reciprocal, then multiply)
    g'   = g * coef
and g' goes through optim_np.sgd_step (the negation of `maximize` and the weight decay come after it).  nonfinite="skip": a step whose
total_norm is not finite changes nothing, and a tensor whose every step so far was skipped has no momentum buffer yet.

The keyword arguments `divide`, `eps`, `clamp` and `after_decay` exist for tests/test_clip_cpu.py's mutants only.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import optim_np as N

F32 = np.float32
CHUNK = 4096
LANES = 256


def tree_sum(lanes):
    """[..., 256] float64 lane sums -> [...] in the kernels' fixed order."""
    a = np.array(lanes, dtype=np.float64).reshape(lanes.shape[:-1] + (4, 64))
    with np.errstate(all="ignore"):
        d = 32
        while d >= 1:
            a[..., :d] = a[..., :d] + a[..., d:2 * d]
            d //= 2
        w = a[..., 0]
        return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def chunk_partials(g):
    """The float64 sum of squares of every chunk of one tensor (float32, any shape, storage order)."""
    g = np.asarray(g, F32).reshape(-1)
    n_chunks = (g.size + CHUNK - 1) // CHUNK
    sq = np.zeros(n_chunks * CHUNK, dtype=np.float64)
    with np.errstate(all="ignore"):
        x = g.astype(np.float64)
        sq[:g.size] = x * x                                              # exact: 24 + 24 bits
        # [chunk, round k, lane, element e] -> a lane's elements in ascending order: k, then e
        by_lane = np.ascontiguousarray(sq.reshape(n_chunks, CHUNK // (4 * LANES), LANES, 4).transpose(1, 3, 0, 2))
        acc = np.zeros((n_chunks, LANES), dtype=np.float64)
        for k in range(by_lane.shape[0]):
            for e in range(4):
                acc = acc + by_lane[k, e]
    return tree_sum(acc)


def norm_of(grads, counts=None, threads=8):
    """(total_norm float32, S float64).  `counts`: element count of every tensor, needed for the tensors whose gradient is None
    (their chunks sit in the table and contribute 0.0)."""
    def one(i):
        g = grads[i]
        if g is None:
            n = int(counts[i])
            return np.zeros((n + CHUNK - 1) // CHUNK, dtype=np.float64)
        return chunk_partials(g)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, range(len(grads))))
    partials = np.concatenate(parts) if parts else np.zeros(0)
    rows = (partials.size + LANES - 1) // LANES
    padded = np.zeros(rows * LANES, dtype=np.float64)
    padded[:partials.size] = partials
    padded = padded.reshape(rows, LANES)
    with np.errstate(all="ignore"):
        acc = np.zeros(LANES, dtype=np.float64)
        for r in range(rows):
            acc = acc + padded[r]
        s = np.float64(tree_sum(acc))
        return F32(np.sqrt(s)), s


def coefficient(norm, max_norm, divide="reciprocal", eps=1e-6, clamp=True):
    """float32 clip coefficient of a float32 total norm."""
    with np.errstate(all="ignore"):
        t = F32(F32(norm) + F32(eps)) if eps else F32(norm)
        if divide == "reciprocal":
            c = F32(F32(F32(1.0) / t) * F32(max_norm))
        else:
            c = F32(F32(max_norm) / t)
        if clamp and c > F32(1.0):                     # NaN stays NaN
            c = F32(1.0)
        return c


def scale(g, coef):
    with np.errstate(all="ignore"):
        return (np.asarray(g, F32) * F32(coef)).astype(F32)


def clipped_step(ps, gs, bufs, hypers, max_norm, nonfinite="propagate", after_decay=False, **coef_kw):
    """One clipped step over lists (optim_np.sgd_step_many's arguments).  -> (ps, bufs, total_norm, coef, skipped)."""
    if isinstance(hypers, dict):
        hypers = [hypers] * len(ps)
    norm, _ = norm_of(gs, [np.asarray(p).size for p in ps])
    coef = coefficient(norm, max_norm, **coef_kw)
    if nonfinite == "skip" and not np.isfinite(norm):
        return list(ps), list(bufs), norm, coef, True
    if after_decay:                                    # the mutant: weight decay first, the coefficient on the decayed gradient
        scaled, hypers2 = [], []
        for p, g, h in zip(ps, gs, hypers):
            if g is None:
                scaled.append(None)
            else:
                d = N.fma32(p, F32(h.get("weight_decay", 0.0)), g) if h.get("weight_decay", 0.0) != 0 else np.asarray(g, F32)
                scaled.append(scale(d, coef))
            hypers2.append(dict(h, weight_decay=0.0))
        hypers = hypers2
    else:
        scaled = [None if g is None else scale(g, coef) for g in gs]
    ps, bufs = N.sgd_step_many(ps, scaled, bufs, hypers)
    return ps, bufs, norm, coef, False
