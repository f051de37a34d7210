"""The truth and the yardstick for the forward convolution of csrc/conv_fwd.hip (tests/test_conv_fwd.py).

Truth: F.conv2d on the float32 inputs widened to float64 (CPU).  Yardstick: F.conv2d in float32 on the CPU.  Inputs are
conv_grad_np.inputs' x and w (x standard normal, w scaled by fan-in^(-1/2)) plus, where the case has one, a standard-normal bias.
Errors are bn_act_np.rel_max: the maximum absolute difference over the truth's maximum magnitude."""
import numpy as np
import torch
import torch.nn.functional as F

from bn_act_np import rel_max  # noqa: F401  (the error measure of the tests that import this module)
from conv_grad_np import GEOMETRIES, inputs as _grad_inputs, out_hw  # noqa: F401


def inputs(B, cin, cout, ksize, stride, H, W, seed, bias=False):
    """dict(x, w, bias or None, ksize, stride): float32, contiguous."""
    d = _grad_inputs(B, cin, cout, ksize, stride, H, W, seed)
    d.pop("dy")
    d["bias"] = np.random.default_rng(seed + 7919).standard_normal(cout).astype(np.float32) if bias else None
    return d


def forward(d, dtype):
    x, w = (torch.from_numpy(d[k]).to(dtype) for k in ("x", "w"))
    b = torch.from_numpy(d["bias"]).to(dtype) if d["bias"] is not None else None
    return F.conv2d(x, w, b, d["stride"], d["ksize"] // 2).numpy()


def truth(d):
    return forward(d, torch.float64)


def yardstick(d):
    return forward(d, torch.float32)
