"""The truth and the yardstick for the convolution gradients of csrc/conv_grad.hip and csrc/conv_dw.hip (tests/test_conv_grad.py).

Truth: torch.nn.grad.conv2d_input / conv2d_weight on the float32 inputs widened to float64 (CPU).  Yardstick: the same two functions
in float32 on the CPU.  The bias gradient is the sum of dy over batch and plane, in float64 and in float32.  Errors are
bn_act_np.rel_max: the maximum absolute difference over the truth's maximum magnitude."""
import numpy as np
import torch

from bn_act_np import rel_max  # noqa: F401  (the error measure of the tests that import this module)

GEOMETRIES = ((1, 1), (3, 1), (3, 2))      # (ksize, stride); padding is ksize // 2


def out_hw(H, W, ksize, stride):
    p = ksize // 2
    return (H + 2 * p - ksize) // stride + 1, (W + 2 * p - ksize) // stride + 1


def inputs(B, cin, cout, ksize, stride, H, W, seed):
    """x and dy standard normal, w scaled by fan-in^(-1/2); float32, contiguous."""
    rng = np.random.default_rng(seed)
    Ho, Wo = out_hw(H, W, ksize, stride)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    return dict(x=f(rng.standard_normal((B, cin, H, W))), dy=f(rng.standard_normal((B, cout, Ho, Wo))),
                w=f(rng.standard_normal((cout, cin, ksize, ksize)) / np.sqrt(cin * ksize * ksize)), ksize=ksize, stride=stride)


def gradients(d, dtype, want=("dx", "dw", "db")):
    """dict of numpy arrays (dx, dw, db) computed on the CPU in `dtype` from the float32 inputs."""
    x, w, dy = (torch.from_numpy(d[k]).to(dtype) for k in ("x", "w", "dy"))
    s, p = d["stride"], d["ksize"] // 2
    out = {}
    if "dx" in want:
        out["dx"] = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=s, padding=p).numpy()
    if "dw" in want:
        out["dw"] = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=s, padding=p).numpy()
    if "db" in want:
        out["db"] = dy.sum(dim=(0, 2, 3)).numpy()
    return out


def truth(d, want=("dx", "dw", "db")):
    return gradients(d, torch.float64, want)


def yardstick(d, want=("dx", "dw", "db")):
    return gradients(d, torch.float32, want)
