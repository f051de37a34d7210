"""float64 numpy restatement of the synchronised BatchNorm + LeakyReLU block (om_bn_sync_* of csrc/bn_act.hip): the per-rank record,
the rank-order merge of the gathered records, and the backward with global sums.  A "rank" is a slice of one batch along its first
axis; tests/bn_act_np.py on the whole batch is what the merged values are held to."""
import numpy as np


def _c(v):
    return np.asarray(v, np.float64).reshape(1, -1, 1, 1)


def split(a, counts):
    """The slices of `a` along axis 0 with these per-rank batch sizes."""
    assert sum(counts) == a.shape[0]
    edges = np.cumsum([0] + list(counts))
    return [a[edges[i]:edges[i + 1]] for i in range(len(counts))]


def record(x):
    """[3][C] doubles of one rank's [B,C,H,W]: n, mean, M2 = sum (x - mean)^2 (two-pass)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.mean(axis=(0, 2, 3))
    d = x - _c(mean)
    return np.stack([np.full(x.shape[1], float(n)), mean, (d * d).sum(axis=(0, 2, 3))])


def merge(records):
    """[R][3][C] -> (N, mean, M2): record 0, then every further record in rank order with the pairwise formula."""
    records = np.asarray(records, np.float64)
    n, mean, m2 = records[0, 0].copy(), records[0, 1].copy(), records[0, 2].copy()
    for r in range(1, records.shape[0]):
        nr, mr, qr = records[r]
        delta, tot = mr - mean, n + nr
        m2 = m2 + qr + delta * delta * n * nr / tot
        mean = mean + delta * nr / tot
        n = tot
    return n, mean, m2


def statistics(records, eps):
    """-> (N, mean, biased variance, unbiased variance, invstd) of the merged records."""
    n, mean, m2 = merge(records)
    var = m2 / n
    return n, mean, var, var * (n / (n - 1)), 1.0 / np.sqrt(var + eps)


def backward_sums(x, dy, mean, invstd, positive, slope):
    """[2][C] of one rank: sum dz, sum dz * xhat, under the sign mask `positive`."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    xhat = (x - _c(mean)) * _c(invstd)
    dz = dy * np.where(positive, 1.0, slope)
    return np.stack([dz.sum(axis=(0, 2, 3)), (dz * xhat).sum(axis=(0, 2, 3))])


def backward_dx(x, dy, gamma, mean, invstd, positive, sums_all, n_total, slope):
    """One rank's dx from the gathered [R][2][C] sums, added in rank order."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    sums_all = np.asarray(sums_all, np.float64)
    total = sums_all[0].copy()
    for r in range(1, sums_all.shape[0]):
        total = total + sums_all[r]
    xhat = (x - _c(mean)) * _c(invstd)
    dz = dy * np.where(positive, 1.0, slope)
    return _c(gamma) * _c(invstd) * (dz - _c(total[0]) / _c(n_total) - xhat * _c(total[1]) / _c(n_total))
