"""Without a GPU: the four entry points of the training convolutions (om_conv2d_forward, om_conv2d_frozen_forward,
om_conv2d_grad_input, om_conv2d_grad_weight; csrc/conv_fwd.hip, csrc/conv_grad.hip, csrc/conv_dw.hip) refuse the same shapes by one rule
(csrc/conv_train.h), each under its own name, and the workspace query answers 0 for them.  Only refused shapes are given: an
accepted one would launch."""
import ctypes

import pytest

from orienmask_amd import lib as omlib

# (B, cin, H, W, cout, ksize, stride)
REFUSED = [(1, 1, 4, 4, 1, 5, 1),
           (1, 1, 4, 4, 1, 3, 3),
           (1, 1, 4, 4, 1, 1, 2),
           (0, 1, 4, 4, 1, 1, 1),
           (16384, 1, 1, 1, 1, 1, 1),
           (16, 1, 8192, 8192, 1, 1, 1),             # B * H * W is exactly 2^30
           (1, 16384, 1, 1, 16384, 3, 1),            # cout * cin * 9 >= 2^31
           (1, (1 << 20) + 1, 1, 1, 1, 1, 1),
           (1, 1, 1, 1, (1 << 20) + 1, 1, 1)]


@pytest.mark.parametrize("shape", REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_the_four_entries_refuse_the_same_shapes_by_name(built, shape):
    L = omlib.load()
    # a small host buffer: the entries refuse before anything is launched or dereferenced
    buf = (ctypes.c_float * 64)()
    x = ctypes.cast(buf, ctypes.c_void_p)
    w, y = ctypes.c_void_p(x.value + 64), ctypes.c_void_p(x.value + 128)
    calls = {
        "om_conv2d_forward": lambda: L.om_conv2d_forward(x, w, None, *shape, y, None),
        "om_conv2d_frozen_forward": lambda: L.om_conv2d_frozen_forward(x, w, *shape, x, x, x, x, 1e-5, 0.1, None, y, None),
        "om_conv2d_grad_input": lambda: L.om_conv2d_grad_input(x, w, *shape, y, None, 0, None),
        "om_conv2d_grad_weight": lambda: L.om_conv2d_grad_weight(x, w, *shape, y, None, None, 0, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        err = L.om_last_error()
        assert name.encode() + b":" in err and b"the geometries are" in err, (name, err)
    assert L.om_conv2d_grad_workspace_bytes(*shape) == 0
