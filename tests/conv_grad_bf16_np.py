"""The truth, the scale and the yardstick for the bf16 convolution gradients of csrc/conv_grad_bf16.hip and csrc/conv_dw.hip (tests/test_conv_grad_bf16.py).

Inputs: conv_grad_np.inputs' draw with x and dy quantised to bf16 (bf16_np), w left float32 (the master weight; the kernel rounds
it).  Truth: conv_grad_np.gradients in float64 on widen(x), widen(dy), quantise(w).  S: the same gradients of the absolute values
(the sum of the |products| of an element).  Yardstick: the same in float32 on the CPU.  K, the number of products of an element at
most: cout * ksize^2 for dx, B * Ho * Wo for dw and db."""
import numpy as np

import bf16_np as Q
import conv_grad_np as G

WANT = ("dx", "dw", "db")


def _with_bits(d):
    d = dict(d)
    d["x_bits"], d["dy_bits"] = Q.round_bits(d["x"]), Q.round_bits(d["dy"])
    d["x"], d["dy"] = Q.widen(d["x_bits"]), Q.widen(d["dy_bits"])
    return d


def inputs(B, cin, cout, ksize, stride, H, W, seed):
    return _with_bits(G.inputs(B, cin, cout, ksize, stride, H, W, seed))


def integer_inputs(B, cin, cout, ksize, stride, H, W, seed):
    """x, dy, w integers in -4 ... 4 (exact in bf16)."""
    rng = np.random.default_rng(seed)
    Ho, Wo = G.out_hw(H, W, ksize, stride)
    f = lambda shape: np.ascontiguousarray(rng.integers(-4, 5, size=shape), dtype=np.float32)      # noqa: E731
    return _with_bits(dict(x=f((B, cin, H, W)), dy=f((B, cout, Ho, Wo)), w=f((cout, cin, ksize, ksize)), ksize=ksize, stride=stride))


def operands(d):
    """What the kernel multiplies: x and dy as they are (already bf16 values), the weight rounded to bf16."""
    return dict(d, w=Q.quantise(d["w"]))


def truth(d, want=WANT):
    return G.truth(operands(d), want)


def scale(d, want=WANT):
    o = operands(d)
    return G.truth(dict(o, x=np.abs(o["x"]), dy=np.abs(o["dy"]), w=np.abs(o["w"])), want)


def yardstick(d, want=WANT):
    return G.yardstick(operands(d), want)


def k_of(d, which):
    B, cout, Ho, Wo = d["dy"].shape
    return cout * d["ksize"] ** 2 if which == "dx" else B * Ho * Wo
