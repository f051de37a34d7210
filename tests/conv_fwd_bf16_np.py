"""The truth, the scale and the yardstick for the bf16 forward convolution of csrc/conv_fwd_bf16.hip (tests/test_conv_fwd_bf16.py).

Inputs: conv_fwd_np.inputs' float32 draw with x quantised to bf16 (the kernel's x is bf16; its w is the float32 master weight, which
the kernel rounds to bf16 itself).  Truth: F.conv2d in float64 on float(x_bf16) and quantise(w), plus the bias.  S: the same
convolution of the absolute values (the scale of an element's rounding errors).  Yardstick: F.conv2d in float32 on the CPU on the
truth's operands."""
import numpy as np
import torch
import torch.nn.functional as F

import bf16_np as Q
from conv_fwd_np import GEOMETRIES, inputs as _f32_inputs, out_hw  # noqa: F401


def inputs(B, cin, cout, ksize, stride, H, W, seed, bias=False):
    """dict(x (float32 holding bf16 values), x_bits (uint16), w, bias or None, ksize, stride)."""
    d = dict(_f32_inputs(B, cin, cout, ksize, stride, H, W, seed, bias))
    d["x_bits"] = Q.round_bits(d["x"])
    d["x"] = Q.widen(d["x_bits"])
    return d


def integer_inputs(B, cin, cout, ksize, stride, H, W, seed, bias=True):
    """x and w integers from -4 ... 4, the bias from -8 ... 8: all exact in bf16, every product and partial sum an integer below
    2^24 (k * 16 + 8 <= 73 736 at k = 4608), so the float32 sum is exact in any order."""
    rng = np.random.default_rng(seed)
    d = dict(ksize=ksize, stride=stride)
    d["x"] = rng.integers(-4, 5, (B, cin, H, W)).astype(np.float32)
    d["w"] = rng.integers(-4, 5, (cout, cin, ksize, ksize)).astype(np.float32)
    d["bias"] = rng.integers(-8, 9, cout).astype(np.float32) if bias else None
    d["x_bits"] = Q.round_bits(d["x"])
    assert np.array_equal(Q.widen(d["x_bits"]), d["x"]) and np.array_equal(Q.quantise(d["w"]), d["w"])
    return d


def _conv(d, dtype, absolute=False):
    f = (lambda a: np.abs(a)) if absolute else (lambda a: a)
    x, w = torch.from_numpy(f(d["x"])).to(dtype), torch.from_numpy(f(Q.quantise(d["w"]))).to(dtype)
    b = torch.from_numpy(f(d["bias"])).to(dtype) if d["bias"] is not None else None
    return F.conv2d(x, w, b, d["stride"], d["ksize"] // 2).numpy()


def truth(d):
    return _conv(d, torch.float64)


def scale(d):
    """S: per element, the sum of the absolute values of the products (and of the bias)."""
    return _conv(d, torch.float64, absolute=True)


def yardstick(d):
    return _conv(d, torch.float32)


def k_of(d):
    return int(d["w"].shape[1]) * d["ksize"] ** 2
