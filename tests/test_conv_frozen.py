"""GPU tests of the frozen Conv -> BatchNorm -> LeakyReLU (+ residual) kernel (om_conv2d_frozen_forward, csrc/conv_fwd.hip)
through the C ABI and through orienmask_amd.train.conv_bn_leaky_frozen.

Truth is tests/conv_frozen_np.py: F.conv2d -> F.batch_norm(training=False) -> leaky_relu -> + residual in float64 on the float32
inputs.  The yardstick is the same composition in float32 on the CPU; the bar is the project's own (tests/test_conv_fwd.py): the
kernel's maximum error over the truth's scale may be at most TWICE the yardstick's on the same inputs, with a floor of 2e-7.
Every output is pre-filled with NaN, so "every element finite" is "every element written".

Worst kernel / yardstick ratios measured on an MI355X are recorded in DESIGN.md 3.26."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_frozen_np as C
from orienmask_amd import lib as omlib, train

pytestmark = pytest.mark.gpu

FLOOR = 2e-7
OM_EINVAL = -1

# (B, cin, cout, ksize, stride, H, W)
CASES = [(1, 1, 1, 1, 1, 1, 1),
         (3, 5, 7, 1, 1, 17, 17), (3, 5, 7, 3, 1, 17, 17), (3, 5, 7, 3, 2, 17, 17),
         (2, 37, 33, 3, 1, 5, 7),
         (1, 3, 32, 3, 2, 33, 31), (1, 3, 32, 3, 2, 34, 32),
         (7, 16, 32, 3, 1, 1, 1),
         (2, 8, 64, 1, 1, 136, 136),
         (2, 8, 64, 3, 1, 17, 17)]
BLOCK = (2, 64, 128, 3, 1, 24, 24)          # a DarkNet block's second layer: with the residual only
JUDGED = [(c, r) for c in CASES for r in (False, True)] + [(BLOCK, True)]

_REFERENCES = {}      # (case, seed, residual) -> (inputs, truth, yardstick): computed once, never modified


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _reference(case, seed, residual):
    key = (case, seed, residual)
    if key not in _REFERENCES:
        d = C.inputs(*case, seed, residual)
        _REFERENCES[key] = (d, C.truth(d), C.yardstick(d))
    return _REFERENCES[key]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _to(dev, d, keys):
    return [torch.from_numpy(d[k]).to(dev) if d[k] is not None else None for k in keys]


def _call(dev, x, w, stats, res, ks, stride, y, eps=C.EPS, slope=C.SLOPE):
    B, cin, H, W = x.shape
    gamma, beta, rm, rv = stats
    return omlib.load().om_conv2d_frozen_forward(_vp(x), _vp(w), B, cin, H, W, w.shape[0], ks, stride, _vp(gamma), _vp(beta), _vp(rm),
                                                 _vp(rv), eps, slope, _vp(res), _vp(y), omlib.current_stream_ptr(dev))


def _hip(dev, d):
    """y through the C ABI, pre-filled with NaN.  -> numpy array."""
    x, w, res = _to(dev, d, ("x", "w", "residual"))
    stats = _to(dev, d, C.STATS)
    Ho, Wo = C.out_hw(x.shape[2], x.shape[3], d["ksize"], d["stride"])
    y = torch.full((x.shape[0], w.shape[0], Ho, Wo), float("nan"), device=dev)
    omlib.check(_call(dev, x, w, stats, res, d["ksize"], d["stride"], y), "om_conv2d_frozen_forward")
    torch.cuda.synchronize(dev)
    return y.cpu().numpy()


def _two_kernels(dev, d):
    """om_conv2d_forward, then om_bn_act_forward(training=0) on its output: the path the fused kernel replaces.  -> numpy array."""
    L = omlib.load()
    x, w, res = _to(dev, d, ("x", "w", "residual"))
    gamma, beta, rm, rv = _to(dev, d, C.STATS)
    B, cin, H, W = x.shape
    cout = w.shape[0]
    Ho, Wo = C.out_hw(H, W, d["ksize"], d["stride"])
    st = omlib.current_stream_ptr(dev)
    h = torch.full((B, cout, Ho, Wo), float("nan"), device=dev)
    y = torch.full_like(h, float("nan"))
    save = torch.empty(4 * cout, device=dev)
    omlib.check(L.om_conv2d_forward(_vp(x), _vp(w), None, B, cin, H, W, cout, d["ksize"], d["stride"], _vp(h), st), "om_conv2d_forward")
    omlib.check(L.om_bn_act_forward(_vp(h), B, cout, Ho, Wo, _vp(gamma), _vp(beta), _vp(rm), _vp(rv), None, 0, 0.1, C.EPS, C.SLOPE,
                                    _vp(res), _vp(y), save.data_ptr(), save.data_ptr() + 8 * cout, None, 0, st), "om_bn_act_forward")
    torch.cuda.synchronize(dev)
    return h.cpu().numpy(), y.cpu().numpy()


def _id(case):
    return "x".join(map(str, case))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("case,residual", JUDGED, ids=[_id(c) + ("-res" if r else "") for c, r in JUDGED])
def test_against_float64(dev, case, residual):
    """The smallest shape; channel counts below a tile on 289-float planes with tiles that end mid-image, on all three geometries;
    cin no multiple of the 8-channel chunk with cout one past a 32 block; odd and even stride-2 inputs; every cell at an image
    boundary; the 64-channel form (289 tiles) and the 32-channel form at the same cout; a DarkNet block's second layer."""
    d, truth, ref = _reference(case, sum(case) * 3 + 2, residual)
    got = _hip(dev, d)
    assert got.shape == truth.shape, case
    assert np.isfinite(got).all(), (case, "an element was not written")
    e, theirs = C.rel_max(got, truth), C.rel_max(ref, truth)
    print("%-30s res %d  y  hip %.3g  torch-cpu %.3g  ratio %.2f" % (case, residual, e, theirs, e / max(theirs, FLOOR / 2)))
    assert e <= max(2 * theirs, FLOOR), (case, e, theirs)


def _integer_inputs(case, seed, residual):
    """x integer-valued in [-3, 3], w in [-2, 2], cin <= 37: every partial sum is an integer below 2^24, exact in float32 in any
    order.  The statistics and the residual are conv_frozen_np's arbitrary floats."""
    d = dict(C.inputs(*case, seed, residual))
    rng = np.random.default_rng(seed)
    d["x"] = rng.integers(-3, 4, d["x"].shape).astype(np.float32)
    d["w"] = rng.integers(-2, 3, d["w"].shape).astype(np.float32)
    return d


EXACT = [(3, 37, 40, 1, 1, 17, 17), (3, 37, 40, 3, 1, 17, 17), (3, 37, 40, 3, 2, 17, 17), (2, 8, 64, 1, 1, 136, 136)]


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("case", EXACT, ids=_id)
def test_bit_identical_to_the_two_kernel_path(dev, case, residual):
    """Where every convolution sum is an exact float32, the fused kernel's y equals om_bn_act_forward(training=0) of
    om_conv2d_forward's output bit for bit: the per-channel doubles and the expression of z are one definition."""
    assert case[1] <= 37
    d = _integer_inputs(case, 7 + sum(case), residual)
    h64 = F.conv2d(torch.from_numpy(d["x"]).double(), torch.from_numpy(d["w"]).double(), None, d["stride"], d["ksize"] // 2).numpy()
    assert np.array_equal(h64, np.rint(h64)) and np.abs(h64).max() <= 37 * 9 * 6 < 2 ** 24      # exact float32 sums
    assert np.array_equal(h64.astype(np.float32).astype(np.float64), h64)
    h, want = _two_kernels(dev, d)
    assert np.array_equal(h.astype(np.float64), h64), "om_conv2d_forward is not exact on integer inputs"
    got = _hip(dev, d)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert np.array_equal(_bits(got), _bits(want)), (case, int((_bits(got) != _bits(want)).sum()))


def test_directed_channels(dev):
    """One launch whose channels hold running_var = 0, gamma = 0, a negative gamma, mean 1000 with variance 1 on a convolution
    output of 1000 + noise, and z exactly 0 (beta = 0 and mean = 0 on a channel whose convolution output is all zero).  Against
    float64 within the bar, and z's sign is the float64 sign wherever the truth is not within 1e-6 of zero."""
    case = (2, 9, 8, 3, 1, 13, 11)
    d = dict(C.inputs(*case, 77, False))
    x, w = d["x"].copy(), d["w"].copy()
    gamma, beta, rm, rv = (d[k].copy() for k in C.STATS)
    rv[0] = 0.0
    gamma[1] = 0.0
    gamma[2] = -1.5
    x[:, -1] = 1.0                      # a constant input channel: the centre tap sees it at every cell, border cells included
    w[:, -1] = 0.0
    w[3, -1, 1, 1] = 1000.0
    rm[3], rv[3] = 1000.0, 1.0
    w[4] = 0.0
    rm[4], beta[4] = 0.0, 0.0
    d.update(x=x, w=w, gamma=gamma, beta=beta, running_mean=rm, running_var=rv)
    truth, ref, z = C.truth(d), C.yardstick(d), C.z_truth(d)
    assert np.abs(truth[:, 3]).max() < 20 and np.all(z[:, 4] == 0)
    got = _hip(dev, d)
    assert np.isfinite(got).all()
    e, theirs = C.rel_max(got, truth), C.rel_max(ref, truth)
    print("directed channels  hip %.3g  torch-cpu %.3g" % (e, theirs))
    assert e <= max(2 * theirs, FLOOR), (e, theirs)
    assert np.all(got[:, 4] == 0)
    # gamma = 0: z is beta exactly, so y is one value
    flat = beta[1] if beta[1] > 0 else np.float32(np.float64(beta[1]) * np.float64(np.float32(C.SLOPE)))
    assert np.all(got[:, 1] == flat)
    far = np.abs(z) > 1e-6
    assert far.mean() > 0.75
    assert np.array_equal(np.sign(got)[far], np.sign(z)[far])


@pytest.mark.parametrize("case", [(3, 5, 7, 3, 2, 17, 17), (2, 8, 64, 1, 1, 136, 136), (2, 64, 128, 3, 1, 24, 24)], ids=_id)
def test_rerun_is_bit_identical(dev, case):
    d = _reference(case, 23, True)[0]
    a, b = _hip(dev, d), _hip(dev, d)
    assert np.isfinite(a).all()
    assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("case", [(3, 5, 7, 1, 1, 17, 17), (3, 5, 7, 3, 1, 17, 17), (3, 16, 40, 3, 2, 9, 7)], ids=_id)
def test_batch_independence(dev, case):
    """An image alone gives the bits it gives inside a batch of 3, at every place in the batch."""
    d = _reference(case, 41, True)[0]
    whole = _hip(dev, d)
    assert np.isfinite(whole).all()
    for i in range(case[0]):
        alone = _hip(dev, dict(d, x=np.ascontiguousarray(d["x"][i:i + 1]), residual=np.ascontiguousarray(d["residual"][i:i + 1])))
        assert np.array_equal(_bits(alone[0]), _bits(whole[i])), (case, i)


def test_neighbours_untouched(dev):
    """y is a view in the middle of a larger buffer: the sentinel on both sides is intact after the call."""
    d, truth, _ = _reference((3, 5, 7, 3, 2, 17, 17), 43, True)
    x, w, res = _to(dev, d, ("x", "w", "residual"))
    n, guard, sentinel = truth.size, 4099, -12345.5
    buf = torch.full((n + 2 * guard,), sentinel, device=dev)
    y = buf[guard:guard + n]
    y.fill_(float("nan"))
    omlib.check(_call(dev, x, w, _to(dev, d, C.STATS), res, d["ksize"], d["stride"], y), "om_conv2d_frozen_forward")
    torch.cuda.synchronize(dev)
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + n:] == sentinel).all())
    got = y.cpu().numpy().reshape(truth.shape)
    assert np.isfinite(got).all() and C.rel_max(got, truth) <= 1e-5


def test_refusals_on_the_device(dev):
    """An aliased y, a null statistic and a 5 x 5 kernel return OM_EINVAL; nothing is launched, y keeps its NaN fill."""
    L = omlib.load()
    B, c, H, W = 2, 32, 12, 12
    x = torch.randn(B, c, H, W, device=dev)
    w = torch.randn(c, c, 3, 3, device=dev)
    stats = [torch.rand(c, device=dev) + 0.5 for _ in range(4)]
    y = torch.full((B, c, H, W), float("nan"), device=dev)
    keep = x.clone()
    assert _call(dev, x, w, stats, None, 3, 1, x) == OM_EINVAL and b"alias" in L.om_last_error()
    assert _call(dev, x, w, stats, y, 3, 1, y) == OM_EINVAL and b"alias" in L.om_last_error()
    keep_w = w.clone()
    assert _call(dev, x, w, stats, None, 3, 1, w) == OM_EINVAL and b"alias" in L.om_last_error()
    for i in range(4):
        holed = list(stats)
        holed[i] = None
        assert _call(dev, x, w, holed, None, 3, 1, y) == OM_EINVAL, i
        assert b"null" in L.om_last_error()
    for miss in ("x", "w", "y"):
        args = dict(x=x, w=w, y=y)
        args[miss] = None
        B_, cin_, H_, W_ = x.shape
        rc = L.om_conv2d_frozen_forward(_vp(args["x"]), _vp(args["w"]), B_, cin_, H_, W_, c, 3, 1, *[_vp(s) for s in stats], C.EPS, C.SLOPE,
                                        None, _vp(args["y"]), omlib.current_stream_ptr(dev))
        assert rc == OM_EINVAL, miss
    w5 = torch.randn(c, c, 5, 5, device=dev)
    assert _call(dev, x, w5, stats, None, 5, 1, y) == OM_EINVAL and b"ksize" in L.om_last_error()
    assert _call(dev, x, w, stats, None, 3, 3, y) == OM_EINVAL
    torch.cuda.synchronize(dev)
    assert torch.isnan(y).all() and torch.equal(x, keep) and torch.equal(w, keep_w)
    omlib.check(_call(dev, x, w, stats, None, 3, 1, y), "om_conv2d_frozen_forward")
    torch.cuda.synchronize(dev)
    assert torch.isfinite(y).all()


# ---------------------------------------------------------------------------------------------------------------- train.conv_bn_leaky_frozen
def _bn(dev, d, training=False):
    bn = nn.BatchNorm2d(d["w"].shape[0], eps=C.EPS).to(dev)
    with torch.no_grad():
        for name, key in (("weight", "gamma"), ("bias", "beta"), ("running_mean", "running_mean"), ("running_var", "running_var")):
            getattr(bn, name).copy_(torch.from_numpy(d[key]))
    return bn.train(training)


@pytest.mark.parametrize("ks,stride", C.GEOMETRIES, ids=["1x1", "3x3", "3x3s2"])
def test_module_function(dev, ks, stride):
    """conv_bn_leaky_frozen equals the C ABI's bits, has no grad_fn under grad mode, reads bn's statistics whatever its mode and
    leaves its buffers alone."""
    case = (2, 24, 40, ks, stride, 21, 18)
    d, truth, ref = _reference(case, 31, True)
    want = _hip(dev, d)
    x, w, res = _to(dev, d, ("x", "w", "residual"))
    for training in (False, True):
        bn = _bn(dev, d, training).requires_grad_(False)
        before = {k: v.clone() for k, v in bn.state_dict().items()}
        assert torch.is_grad_enabled()
        y = train.conv_bn_leaky_frozen(x, w, bn, residual=res, stride=stride, padding=ks // 2, slope=C.SLOPE)
        assert y.grad_fn is None and not y.requires_grad
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(want))
        assert all(torch.equal(v, before[k]) for k, v in bn.state_dict().items())
    assert C.rel_max(want, truth) <= max(2 * C.rel_max(ref, truth), FLOOR)


def test_module_function_refusals(dev):
    d = _reference((2, 8, 16, 3, 1, 10, 12), 5, True)[0]
    x, w, res = _to(dev, d, ("x", "w", "residual"))
    bn = _bn(dev, d).requires_grad_(False)
    with pytest.raises(omlib.OrienMaskHipError, match="x requires grad"):
        train.conv_bn_leaky_frozen(x.clone().requires_grad_(True), w, bn, stride=1, padding=1)
    with pytest.raises(omlib.OrienMaskHipError, match="residual requires grad"):
        train.conv_bn_leaky_frozen(x, w, bn, residual=res.clone().requires_grad_(True), stride=1, padding=1)
    with pytest.raises(omlib.OrienMaskHipError, match="weight requires grad"):
        train.conv_bn_leaky_frozen(x, w.clone().requires_grad_(True), bn, stride=1, padding=1)
    with pytest.raises(omlib.OrienMaskHipError, match="bn.weight requires grad"):
        train.conv_bn_leaky_frozen(x, w, _bn(dev, d), stride=1, padding=1)
    with torch.no_grad():                   # without grad mode nothing can ask for a backward
        y = train.conv_bn_leaky_frozen(x.clone().requires_grad_(True), w, _bn(dev, d), stride=1, padding=1)
    assert y.grad_fn is None
    with pytest.raises(omlib.OrienMaskHipError, match="running statistics"):
        train.conv_bn_leaky_frozen(x, w, nn.BatchNorm2d(16, track_running_stats=False).to(dev).requires_grad_(False), stride=1, padding=1)
    with pytest.raises(omlib.OrienMaskHipError, match="contiguous"):
        train.conv_bn_leaky_frozen(x.to(memory_format=torch.channels_last), w, bn, stride=1, padding=1)
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.conv_bn_leaky_frozen(x.cpu(), w.cpu(), bn, stride=1, padding=1)
    with pytest.raises(omlib.OrienMaskHipError, match="float32"):
        train.conv_bn_leaky_frozen(x.double(), w.double(), bn, stride=1, padding=1)
    with pytest.raises(omlib.OrienMaskHipError, match="kernel 3 stride 1 padding 0"):
        train.conv_bn_leaky_frozen(x, w, bn, stride=1, padding=0)
    with pytest.raises(omlib.OrienMaskHipError, match="output shape"):
        train.conv_bn_leaky_frozen(x, w, bn, residual=res[:, :, :-1].contiguous(), stride=1, padding=1)
