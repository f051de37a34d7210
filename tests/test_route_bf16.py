"""GPU tests of the bf16 entry points of the route kernels (om_route_concat_forward_bf16 / om_route_concat_backward_bf16,
csrc/route.hip) through the C ABI and through train.upsample_concat / train.split_channels.

The forward is a copy: its bf16 output has the bits of the float32 restatement (tests/route_np.py) on the widened sources.  The
backward sums each s x s block in float32 in the float32 kernel's order and rounds once: its bf16 gradients are the float32 entry
point's gradients on the widened dy, rounded to nearest even on the CPU (tests/bf16_np.py), bit for bit.  The float32 entry points
themselves are judged in tests/test_route.py."""
import ctypes

import numpy as np
import pytest
import torch

import bf16_np as Q
import route_np as R
from orienmask_amd import lib as omlib, train

pytestmark = pytest.mark.gpu

# (B, H, W, [(C_i, s_i)]): the FPN-Plus model's three cat sites and its 18 -> 6 + 6 + 6 split at a 96 x 96 image (B = 2), the other
# model's cat at 24 x 24, a four-source case at scales 8, 4, 2, 1 with odd channel counts, and rows that are no multiple of 4
CAT_SITES = [(2, 6, 6, [(256, 2), (512, 1)]), (2, 12, 12, [(128, 2), (256, 1)]), (2, 24, 24, [(64, 8), (64, 4), (64, 2), (64, 1)])]
SPLIT = (2, 24, 24, [(6, 1), (6, 1), (6, 1)])
CASES = CAT_SITES + [SPLIT, (2, 24, 24, [(64, 2), (128, 1)]), (3, 16, 8, [(3, 8), (5, 4), (2, 2), (7, 1)]),
                     (3, 6, 10, [(3, 2), (5, 1)])]
_INPUTS = {}      # case -> (sources, dy) holding bf16 values: drawn once, never modified


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _inputs(case):
    key = R.case_id(case)
    if key not in _INPUTS:
        srcs, dy = R.inputs(case, 300 + len(_INPUTS))
        _INPUTS[key] = ([Q.quantise(s) for s in srcs], Q.quantise(dy))
    return _INPUTS[key]


def _dev(dev, a, bf16, offset=0, empty=False):
    dtype = torch.bfloat16 if bf16 else torch.float32
    buf = torch.full((int(np.prod(a)) + offset if empty else a.size + offset,), float("nan"), dtype=dtype, device=dev)
    t = buf[offset:].view(a if empty else a.shape)
    if not empty:
        t.copy_(torch.from_numpy(a).to(dev))
    return t


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _arrays(chans, scales):
    n = len(chans)
    return (ctypes.c_int * 4)(*list(chans) + [0] * (4 - n)), (ctypes.c_int * 4)(*list(scales) + [0] * (4 - n))


def _ptrs(ts):
    return (ctypes.c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in ts] + [None] * (4 - len(ts)))


def _forward(dev, case, srcs, bf16, offset=0):
    B, H, W, _ = case
    chans, scales = R.chans_scales(case)
    c, s = _arrays(chans, scales)
    name = "om_route_concat_forward" + ("_bf16" if bf16 else "")
    ts = [_dev(dev, a, bf16, offset) if a is not None else None for a in srcs]
    y = _dev(dev, (B, sum(chans), H, W), bf16, offset, empty=True)
    omlib.check(getattr(omlib.load(), name)(_ptrs(ts), c, s, len(chans), B, H, W, ctypes.c_void_p(y.data_ptr()),
                                           omlib.current_stream_ptr(dev)), name)
    torch.cuda.synchronize(dev)
    return y


def _backward(dev, case, dy, bf16, offset=0, want=None):
    B, H, W, _ = case
    chans, scales = R.chans_scales(case)
    c, s = _arrays(chans, scales)
    name = "om_route_concat_backward" + ("_bf16" if bf16 else "")
    want = [True] * len(chans) if want is None else want
    d = _dev(dev, dy, bf16, offset)
    outs = [_dev(dev, (B, ch, H // sc, W // sc), bf16, offset, empty=True) for ch, sc in zip(chans, scales)]
    omlib.check(getattr(omlib.load(), name)(ctypes.c_void_p(d.data_ptr()), c, s, len(chans), B, H, W,
                                           _ptrs([o if w else None for o, w in zip(outs, want)]), omlib.current_stream_ptr(dev)), name)
    torch.cuda.synchronize(dev)
    return outs


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_forward_is_the_widened_copy(dev, case, offset):
    """Both forms (4-element groups; one element per lane for a tensor that starts one element in or rows that are no multiple of 4)."""
    srcs, _ = _inputs(case)
    B, H, W, _ = case
    chans, scales = R.chans_scales(case)
    want = R.forward(srcs, chans, scales, B, H, W)
    y = _forward(dev, case, srcs, True, offset)
    assert y.dtype == torch.bfloat16
    assert np.array_equal(_bits(y), Q.round_bits(want)) and np.array_equal(Q.widen(_bits(y)).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(_bits(_forward(dev, case, srcs, True, offset)), _bits(y))          # a rerun gives the same bits


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_backward_is_the_float32_kernels_result_rounded(dev, case, offset):
    _, dy = _inputs(case)
    chans, scales = R.chans_scales(case)
    ref = _backward(dev, case, dy, False, offset)
    got = _backward(dev, case, dy, True, offset)
    restated = R.backward(dy, chans, scales)
    for i, (g, r, w) in enumerate(zip(got, ref, restated)):
        assert g.dtype == torch.bfloat16 and r.dtype == torch.float32
        assert np.array_equal(r.cpu().numpy().view(np.uint32), w.view(np.uint32)), (R.case_id(case), i, "the float32 kernel")
        assert np.array_equal(_bits(g), Q.round_bits(r.cpu().numpy())), (R.case_id(case), i)
    again = _backward(dev, case, dy, True, offset)
    assert all(np.array_equal(_bits(a), _bits(g)) for a, g in zip(again, got))


def test_null_sources_are_zeros_and_null_gradients_are_skipped(dev):
    case = CASES[5]
    srcs, dy = _inputs(case)
    B, H, W, _ = case
    chans, scales = R.chans_scales(case)
    holes = [srcs[0], None, srcs[2], None]
    y = _forward(dev, case, holes, True)
    assert np.array_equal(_bits(y), Q.round_bits(R.forward(holes, chans, scales, B, H, W)))
    want = [True, False, False, True]
    got = _backward(dev, case, dy, True, want=want)
    ref = _backward(dev, case, dy, False, want=want)
    for g, r, w in zip(got, ref, want):
        if w:
            assert np.array_equal(_bits(g), Q.round_bits(r.cpu().numpy()))
        else:
            assert torch.isnan(g).all()                 # untouched


@pytest.mark.parametrize("case", [CAT_SITES[2], CASES[6]], ids=R.case_id)
def test_upsample_concat_in_bf16_under_autograd(dev, case):
    srcs, dy = _inputs(case)
    chans, scales = R.chans_scales(case)
    B, H, W, _ = case
    ts = [torch.from_numpy(a).to(dev).to(torch.bfloat16).requires_grad_(True) for a in srcs]
    y = train.upsample_concat(ts, scales)
    assert y.dtype == torch.bfloat16
    assert np.array_equal(_bits(y.detach()), Q.round_bits(R.forward(srcs, chans, scales, B, H, W)))
    y.backward(torch.from_numpy(dy).to(dev).to(torch.bfloat16))
    for t, w in zip(ts, R.backward(dy, chans, scales)):
        assert t.grad.dtype == torch.bfloat16 and np.array_equal(_bits(t.grad), Q.round_bits(w))
    # one element type per call: no cast
    with pytest.raises(omlib.OrienMaskHipError, match="no cast"):
        train.upsample_concat([ts[0].detach(), ts[1].detach().float()], scales[:2])


def test_split_channels_in_bf16_under_autograd(dev):
    _, x = _inputs(SPLIT)
    t = torch.from_numpy(x).to(dev).to(torch.bfloat16).requires_grad_(True)
    a, b, c = train.split_channels(t, [6, 6, 6])
    for part, want in zip((a, b, c), np.split(x, 3, axis=1)):
        assert part.dtype == torch.bfloat16 and part.is_contiguous()
        assert np.array_equal(_bits(part.detach()), Q.round_bits(want))
    ga, gc = torch.randn_like(a), torch.randn_like(c)
    torch.autograd.backward([a, c], [ga, gc])              # b takes no part: its gradient is zeros
    want = torch.cat([ga, torch.zeros_like(b), gc], 1)
    assert t.grad.dtype == torch.bfloat16 and torch.equal(t.grad, want)
