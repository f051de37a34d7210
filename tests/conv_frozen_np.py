"""The truth and the yardstick for the frozen Conv -> BatchNorm -> LeakyReLU (+ residual) kernel, om_conv2d_frozen_forward
(csrc/conv_fwd.hip; tests/test_conv_frozen.py).

Inputs: conv_fwd_np.inputs' x and w plus gamma (standard normal, so about half are negative), beta, running_mean (standard normal),
running_var (uniform in [0.25, 2.25): positive) and, where asked, a standard-normal residual with the output's shape.
Truth: F.conv2d -> F.batch_norm(training=False) -> leaky_relu -> + residual on the float32 inputs widened to float64 (CPU).
Yardstick: the same composition in float32 on the CPU.  Errors are bn_act_np.rel_max."""
import numpy as np
import torch
import torch.nn.functional as F

from bn_act_np import EPS, SLOPE, rel_max  # noqa: F401
from conv_fwd_np import GEOMETRIES, inputs as _conv_inputs, out_hw  # noqa: F401

STATS = ("gamma", "beta", "running_mean", "running_var")


def inputs(B, cin, cout, ksize, stride, H, W, seed, residual=False):
    """dict(x, w, gamma, beta, running_mean, running_var, residual or None, ksize, stride): float32, contiguous."""
    d = _conv_inputs(B, cin, cout, ksize, stride, H, W, seed)
    d.pop("bias")
    rng = np.random.default_rng(seed + 104729)
    d["gamma"] = rng.standard_normal(cout).astype(np.float32)
    d["beta"] = rng.standard_normal(cout).astype(np.float32)
    d["running_mean"] = rng.standard_normal(cout).astype(np.float32)
    d["running_var"] = (0.25 + 2.0 * rng.random(cout)).astype(np.float32)
    Ho, Wo = out_hw(H, W, ksize, stride)
    d["residual"] = rng.standard_normal((B, cout, Ho, Wo)).astype(np.float32) if residual else None
    return d


def forward(d, dtype, eps=EPS, slope=SLOPE):
    x, w, gamma, beta, rm, rv = (torch.from_numpy(d[k]).to(dtype) for k in ("x", "w") + STATS)
    h = F.conv2d(x, w, None, d["stride"], d["ksize"] // 2)
    y = F.leaky_relu(F.batch_norm(h, rm, rv, gamma, beta, False, 0.0, eps), slope)
    if d["residual"] is not None:
        y = y + torch.from_numpy(d["residual"]).to(dtype)
    return y.numpy()


def z_truth(d, eps=EPS):
    """The pre-activation in float64 (the sign the kernel's LeakyReLU must take)."""
    x, w, gamma, beta, rm, rv = (torch.from_numpy(d[k]).to(torch.float64) for k in ("x", "w") + STATS)
    h = F.conv2d(x, w, None, d["stride"], d["ksize"] // 2)
    return F.batch_norm(h, rm, rv, gamma, beta, False, 0.0, eps).numpy()


def truth(d):
    return forward(d, torch.float64)


def yardstick(d):
    return forward(d, torch.float32)
