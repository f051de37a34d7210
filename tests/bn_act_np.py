"""float64 numpy restatement of the BatchNorm + LeakyReLU (+ residual) block of csrc/bn_act.hip: the forward, the running-buffer
updates and the backward.  The backward takes the sign mask as an INPUT, so an implementation's gradient can be judged under its
own mask (elements with z within rounding of 0 may land on either side in float32) and the mask is judged separately.

Also here, shared by tools/gen_golden.py and the tests: the seeded cotangents and the parameter names of the train_step fixtures."""
import numpy as np

EPS = 1e-5
MOMENTUM = 0.1
SLOPE = 0.1

# parameters whose full gradient the train_step fixtures store: backbone, necks, routes / skips, heads
GRAD_NAMES = (
    "backbone.conv1.conv_block.0.weight",
    "backbone.conv1.conv_block.1.weight",
    "backbone.conv3.1.conv.0.conv_block.0.weight",
    "backbone.conv6.4.conv.1.conv_block.1.bias",
    "neck16.4.conv_block.1.weight",
    "neck4.0.conv_block.1.weight",
    "route32.0.conv_block.1.bias",
    "skip16.0.conv_block.0.weight",
    "bbox_head32.1.bias",
    "orien_head.5.weight",
)
HEAD_KEYS = ("bbox32", "orien32", "bbox16", "orien16", "bbox8", "orien8")


def cotangents(seed, shapes):
    """One float32 N(0,1) tensor per head shape, in HEAD_KEYS order, from one PCG64 stream."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return [rng.standard_normal(tuple(int(v) for v in s)).astype(np.float32) for s in shapes]


def _c(v):
    return np.asarray(v, np.float64).reshape(1, -1, 1, 1)


def batch_stats(x):
    """(mean, biased variance, unbiased variance) per channel of [B,C,H,W], float64, two-pass."""
    x = np.asarray(x, np.float64)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.mean(axis=(0, 2, 3))
    d = x - _c(mean)
    ss = (d * d).sum(axis=(0, 2, 3))
    return mean, ss / n, ss / max(n - 1, 1)


def forward(x, gamma, beta, running_mean, running_var, training, residual=None, eps=EPS, momentum=MOMENTUM, slope=SLOPE):
    """-> dict(y, z, mean, invstd, running_mean, running_var): everything float64; the running buffers are the values AFTER the call
    (unchanged in eval mode)."""
    x = np.asarray(x, np.float64)
    rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    if training:
        mean, var, unbiased = batch_stats(x)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * unbiased
    else:
        mean, var = rm, rv
    invstd = 1.0 / np.sqrt(var + eps)
    z = (x - _c(mean)) * _c(invstd) * _c(gamma) + _c(beta)
    y = np.where(z > 0, z, z * slope)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return dict(y=y, z=z, mean=mean, invstd=invstd, running_mean=rm, running_var=rv)


def backward(x, dy, gamma, mean, invstd, positive, training, slope=SLOPE):
    """positive: bool [B,C,H,W], True where the implementation took z > 0.  -> (dx, dgamma, dbeta), float64."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    xhat = (x - _c(mean)) * _c(invstd)
    dz = dy * np.where(positive, 1.0, slope)
    dbeta = dz.sum(axis=(0, 2, 3))
    dgamma = (dz * xhat).sum(axis=(0, 2, 3))
    w = _c(gamma) * _c(invstd)
    if training:
        dx = w * (dz - _c(dbeta) / n - xhat * _c(dgamma) / n)
    else:
        dx = w * dz
    return dx, dgamma, dbeta


def rel_max(got, want):
    """Maximum error over the tensor's scale (max |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))
