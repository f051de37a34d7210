"""GPU tests of the convolution gradients (om_conv2d_grad_input / om_conv2d_grad_weight; csrc/conv_grad.hip, csrc/conv_dw.hip) through the C ABI,
through orienmask_amd.train.conv2d and through the training models built with conv_backend='hip'.

Truth is tests/conv_grad_np.py: torch.nn.grad's two functions in float64 on the float32 inputs.  The yardstick is the same two
functions in float32 on the CPU: kernel and yardstick are float32 evaluations that differ in summation order only, so for each of
dx, dw and dbias the kernel's maximum error over the truth's scale may be at most TWICE torch-CPU-float32's on the same inputs, with
a floor of 2e-7 (about three half-units in the last place of the scale).

Worst kernel / torch-CPU ratios measured on an MI355X are recorded in DESIGN.md 3.19."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
import bn_act_np as N
import conv_grad_np as G
import train_step as T
from orienmask_amd import lib as omlib, train

pytestmark = pytest.mark.gpu

FLOOR = 2e-7
OM_EINVAL, OM_ENOMEM = -1, -3


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# (B, cin, cout, ksize, stride, H, W)
SPECIAL = [(1, 1, 1, 1, 1, 1, 1),
           (3, 5, 7, 1, 1, 17, 17), (3, 5, 7, 3, 1, 17, 17), (3, 5, 7, 3, 2, 17, 17),
           (2, 64, 255, 1, 1, 17, 17),
           (2, 256, 18, 1, 1, 24, 24),
           (1, 3, 32, 3, 1, 33, 31), (1, 3, 32, 3, 2, 33, 31),
           (2, 1024, 512, 1, 1, 3, 5),
           (2, 512, 1024, 3, 1, 3, 5),
           (5, 32, 64, 3, 2, 8, 8)]
# the workload's own k: (case, gradients)
LARGE = [((2, 3, 32, 3, 1, 544, 544), ("dw", "db")),
         ((2, 32, 64, 3, 2, 544, 544), ("dx", "dw", "db")),
         ((2, 128, 64, 1, 1, 136, 136), ("dx", "dw", "db")),
         ((2, 512, 1024, 3, 1, 17, 17), ("dx", "dw", "db"))]
ALL = ("dx", "dw", "db")

_REFERENCES = {}      # (case, seed, want) -> (inputs, truth, yardstick): computed once, never modified


def _reference(case, seed, want=ALL):
    key = (case, seed, want)
    if key not in _REFERENCES:
        B, cin, cout, ks, stride, H, W = case
        d = G.inputs(B, cin, cout, ks, stride, H, W, seed)
        _REFERENCES[key] = (d, G.truth(d, want), G.yardstick(d, want))
    return _REFERENCES[key]


def _hip(dev, d, want=ALL, ws=None):
    """The gradients through the C ABI: outputs pre-filled with NaN, the workspace with 0xFF.  -> dict of numpy arrays."""
    L = omlib.load()
    x, w, dy = (torch.from_numpy(d[k]).to(dev) for k in ("x", "w", "dy"))
    B, cin, H, W = x.shape
    cout, ks, stride = w.shape[0], d["ksize"], d["stride"]
    geom = (B, cin, H, W, cout, ks, stride)
    need = L.om_conv2d_grad_workspace_bytes(*geom)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    ws.fill_(255)
    st = omlib.current_stream_ptr(dev)
    nan = lambda t: torch.full_like(t, float("nan"))      # noqa: E731
    dx = nan(x) if "dx" in want else None
    dw = nan(w) if "dw" in want else None
    db = torch.full((cout,), float("nan"), device=dev) if "db" in want else None
    if dx is not None:
        omlib.check(L.om_conv2d_grad_input(T.vp(dy), T.vp(w), *geom, T.vp(dx), T.vp(ws), ws.numel(), st), "om_conv2d_grad_input")
    if dw is not None or db is not None:
        omlib.check(L.om_conv2d_grad_weight(T.vp(x), T.vp(dy), *geom, T.vp(dw), T.vp(db), T.vp(ws), ws.numel(), st), "om_conv2d_grad_weight")
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in (("dx", dx), ("dw", dw), ("db", db)) if v is not None}


def _judge(dev, case, seed, want=ALL):
    """Asserts the bar for every gradient of the case; -> {gradient: kernel error / torch-CPU error}."""
    d, truth, ref = _reference(case, seed, want)
    got = _hip(dev, d, want)
    ratios, missed = {}, []
    for k in want:
        assert got[k].shape == truth[k].shape, (case, k)
        assert np.isfinite(got[k]).all(), (case, k, "an element was not written")
        e, theirs = G.rel_max(got[k], truth[k]), G.rel_max(ref[k], truth[k])
        ratios[k] = e / max(theirs, FLOOR / 2)
        print("%-34s %-3s hip %.3g  torch-cpu %.3g  ratio %.2f" % (case, k, e, theirs, ratios[k]))
        if e > max(2 * theirs, FLOOR):
            missed.append((case, k, e, theirs))
    assert not missed, missed
    return ratios


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("case", T.SWEEP, ids=T.case_id)
def test_every_layer_geometry_against_float64(dev, case):
    """Every distinct convolution of the two models at 96 x 96 and 160 x 128, B = 2."""
    _judge(dev, case, sum(case) * 5 + 1)


@pytest.mark.parametrize("case", SPECIAL, ids=T.case_id)
def test_special_shapes_against_float64(dev, case):
    """The smallest shape, channel counts that are no tile multiple (3, 5, 7, 18, 255), planes of 289 floats, odd stride-2 inputs,
    tiny maps with deep channels, a batch that is no power of two."""
    _judge(dev, case, sum(case) * 3 + 2)


@pytest.mark.parametrize("case,want", LARGE, ids=[T.case_id(c) for c, _ in LARGE])
def test_full_size_shapes_against_float64(dev, case, want):
    """B = 2 at 544 x 544: the split-k and multi-tile paths at the workload's own k."""
    _judge(dev, case, 17, want)


@pytest.mark.parametrize("case", [(2, 32, 64, 3, 2, 48, 48), (2, 128, 64, 1, 1, 24, 24), (2, 3, 32, 3, 1, 544, 544)], ids=T.case_id)
def test_rerun_is_bit_identical(dev, case):
    """The same call twice, and once more after another call has used the same workspace."""
    want = ("dw", "db") if case[-1] == 544 else ALL
    d = _reference(case, 23, want)[0]
    other = G.inputs(3, 40, 24, 3, 1, 20, 28, 5)
    L = omlib.load()
    ws = torch.empty(max(L.om_conv2d_grad_workspace_bytes(*case[:2], *case[5:], case[2], case[3], case[4]),
                         L.om_conv2d_grad_workspace_bytes(3, 40, 20, 28, 24, 3, 1), 16), dtype=torch.uint8, device=dev)
    a = _hip(dev, d, want, ws)
    b = _hip(dev, d, want, ws)
    _hip(dev, other, ALL, ws)
    c = _hip(dev, d, want, ws)
    for k in want:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        assert np.array_equal(a[k].view(np.uint32), c[k].view(np.uint32)), k


def test_non_default_stream(dev):
    d = _reference((2, 32, 64, 3, 2, 48, 48), 23)[0]
    want = _hip(dev, d)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        got = _hip(dev, d)
    for k in ALL:
        assert np.array_equal(got[k], want[k]), k


def test_refusals_on_the_device(dev):
    """Unsupported geometries and null pointers return OM_EINVAL, a workspace one byte short OM_ENOMEM; nothing is launched."""
    L = omlib.load()
    st = omlib.current_stream_ptr(dev)
    B, cin, cout, H, W = 2, 32, 64, 96, 96
    x = torch.randn(B, cin, H, W, device=dev)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=dev)
    for ks, stride in ((5, 1), (3, 3), (1, 2), (3, 0), (2, 1)):
        Ho = (H + 2 * (ks // 2) - ks) // max(stride, 1) + 1
        dy = torch.randn(B, cout, Ho, Ho, device=dev)
        w = torch.randn(cout, cin, ks, ks, device=dev)
        dx, dw = torch.full_like(x, float("nan")), torch.full_like(w, float("nan"))
        assert L.om_conv2d_grad_workspace_bytes(B, cin, H, W, cout, ks, stride) == 0
        assert L.om_conv2d_grad_input(T.vp(dy), T.vp(w), B, cin, H, W, cout, ks, stride, T.vp(dx), T.vp(ws), ws.numel(), st) == OM_EINVAL
        assert b"ksize" in L.om_last_error()
        assert L.om_conv2d_grad_weight(T.vp(x), T.vp(dy), B, cin, H, W, cout, ks, stride, T.vp(dw), None, T.vp(ws), ws.numel(), st) == OM_EINVAL
        torch.cuda.synchronize(dev)
        assert torch.isnan(dx).all() and torch.isnan(dw).all()
    geom = (B, cin, H, W, cout, 3, 1)
    dy = torch.randn(B, cout, H, W, device=dev)
    w = torch.randn(cout, cin, 3, 3, device=dev)
    dx, dw = torch.full_like(x, float("nan")), torch.full_like(w, float("nan"))
    assert L.om_conv2d_grad_input(None, T.vp(w), *geom, T.vp(dx), T.vp(ws), ws.numel(), st) == OM_EINVAL
    assert L.om_conv2d_grad_input(T.vp(dy), None, *geom, T.vp(dx), T.vp(ws), ws.numel(), st) == OM_EINVAL
    assert L.om_conv2d_grad_input(T.vp(dy), T.vp(w), *geom, None, T.vp(ws), ws.numel(), st) == OM_EINVAL
    assert L.om_conv2d_grad_weight(None, T.vp(dy), *geom, T.vp(dw), None, T.vp(ws), ws.numel(), st) == OM_EINVAL
    assert L.om_conv2d_grad_weight(T.vp(x), None, *geom, T.vp(dw), None, T.vp(ws), ws.numel(), st) == OM_EINVAL
    assert L.om_conv2d_grad_weight(T.vp(x), T.vp(dy), *geom, None, None, T.vp(ws), ws.numel(), st) == OM_EINVAL
    need = L.om_conv2d_grad_workspace_bytes(*geom)
    assert 0 < need <= ws.numel()                 # k = 18432: several splits
    assert L.om_conv2d_grad_weight(T.vp(x), T.vp(dy), *geom, T.vp(dw), None, T.vp(ws), need - 1, st) == OM_ENOMEM
    assert b"workspace" in L.om_last_error()
    assert L.om_conv2d_grad_weight(T.vp(x), T.vp(dy), *geom, T.vp(dw), None, None, need, st) == OM_ENOMEM
    torch.cuda.synchronize(dev)
    assert torch.isnan(dx).all() and torch.isnan(dw).all()
    omlib.check(L.om_conv2d_grad_weight(T.vp(x), T.vp(dy), *geom, T.vp(dw), None, T.vp(ws), need, st), "om_conv2d_grad_weight")
    torch.cuda.synchronize(dev)
    assert torch.isfinite(dw).all()


# ---------------------------------------------------------------------------------------------------------------- train.conv2d
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("ks,stride", G.GEOMETRIES, ids=["1x1", "3x3", "3x3s2"])
def test_module_function_against_torch_and_float64(dev, ks, stride, bias):
    """train.conv2d against F.conv2d under autograd on the same GPU tensors: equal outputs (the same forward), gradients within the
    bar against the float64 truth."""
    case = (2, 24, 40, ks, stride, 21, 18)
    d, truth, ref = _reference(case, 31)
    x0, w0, dy = (torch.from_numpy(d[k]).to(dev) for k in ("x", "w", "dy"))
    b0 = torch.linspace(-1, 1, 40, device=dev) if bias else None
    outs = []
    for fn in (train.conv2d, F.conv2d):
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        b = b0.clone().requires_grad_(True) if bias else None
        y = fn(x, w, b, stride, ks // 2)
        y.backward(dy)
        outs.append((y.detach(), x.grad, w.grad, b.grad if bias else None))
    assert torch.equal(outs[0][0], outs[1][0])
    for k, got in zip(ALL if bias else ALL[:2], outs[0][1:]):
        e, theirs = G.rel_max(got.cpu().numpy(), truth[k]), G.rel_max(ref[k], truth[k])
        print("conv2d %dx%d s%d %-3s hip %.3g  torch-cpu %.3g  torch-gpu %.3g" % (
            ks, ks, stride, k, e, theirs, G.rel_max(outs[1][1 + ALL.index(k)].cpu().numpy(), truth[k])))
        assert e <= max(2 * theirs, FLOOR), (k, e, theirs)


def test_module_function_skips_what_needs_no_gradient(dev):
    x = torch.randn(2, 8, 10, 12, device=dev)
    w = torch.randn(16, 8, 3, 3, device=dev)
    b = torch.randn(16, device=dev)
    # an input without requires_grad: no dx
    wi, bi = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = train.conv2d(x, wi, bi, 1, 1)
    assert y.grad_fn.apply(torch.ones_like(y))[0] is None
    # a frozen weight: no dw; the bias gradient is still there
    xi, bi = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = train.conv2d(xi, w, bi, 1, 1)
    grads = y.grad_fn.apply(torch.ones_like(y))
    assert grads[0] is not None and grads[1] is None and grads[2] is not None and grads[3] is None
    assert G.rel_max(grads[2].cpu().numpy(), np.full(16, 2.0 * 10 * 12)) <= FLOOR
    # nothing but the input
    xi = x.clone().requires_grad_(True)
    y = train.conv2d(xi, w, None, 1, 1)
    grads = y.grad_fn.apply(torch.ones_like(y))
    assert grads[0] is not None and grads[1] is None and grads[2] is None


def test_module_function_takes_a_non_contiguous_dy(dev):
    x = torch.randn(2, 8, 10, 12, device=dev, requires_grad=True)
    w = torch.randn(16, 8, 3, 3, device=dev, requires_grad=True)
    gy = torch.randn(2, 10, 12, 16, device=dev).permute(0, 3, 1, 2)      # channels-last strides
    assert not gy.is_contiguous()
    train.conv2d(x, w, None, 1, 1).backward(gy)
    gx, gw = x.grad.clone(), w.grad.clone()
    x.grad = w.grad = None
    train.conv2d(x, w, None, 1, 1).backward(gy.contiguous())
    assert torch.equal(gx, x.grad) and torch.equal(gw, w.grad)


def test_module_function_refusals(dev):
    x = torch.randn(2, 8, 10, 12, device=dev)
    w = torch.randn(16, 8, 3, 3, device=dev)
    with pytest.raises(omlib.OrienMaskHipError, match="float32"):
        train.conv2d(x.half(), w.half(), None, 1, 1)
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.conv2d(x.cpu(), w.cpu(), None, 1, 1)
    with pytest.raises(omlib.OrienMaskHipError, match="contiguous"):
        train.conv2d(x.to(memory_format=torch.channels_last), w, None, 1, 1)
    with pytest.raises(omlib.OrienMaskHipError, match="padding 0"):
        train.conv2d(x, w, None, 1, 0)
    with pytest.raises(omlib.OrienMaskHipError, match="stride 3"):
        train.conv2d(x, w, None, 3, 1)
    with pytest.raises(omlib.OrienMaskHipError, match="kernel 5"):
        train.conv2d(x, torch.randn(16, 8, 5, 5, device=dev), None, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture
def reproducible_forward():
    """torch's own forward convolution is part of both models under comparison, and without this flag MIOpen's choice for the
    512 -> 1024 3x3 layer on a 3 x 3 map differs in its bits from call to call (F.conv2d twice on the same tensors)."""
    with torch.backends.cudnn.flags(deterministic=True):
        yield


@pytest.mark.parametrize("fixture", ["train_step_f96_b2", "train_step_bneval_f96_b2"])
def test_model_against_the_torch_conv_backend_and_the_reference_step(dev, reproducible_forward, fixture):
    """conv_backend 'hip' against 'torch' (both with backend 'hip') on the same GPU: the heads are bit-identical (the forward is
    shared).  Against the reference's recorded step (CPU float32): the 'hip' model's relative-L2 gradient error (root mean square
    over the recorded tensors) is at most twice the 'torch' model's -- both are float32 against a CPU float32 recording."""
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    errs, heads_of = {}, {}
    for cb in ("hip", "torch"):
        heads_of[cb], _, _, errs[cb], _ = T.recorded_step(dev, g, backend="hip", conv_backend=cb)
    for k, a, b in zip(N.HEAD_KEYS, heads_of["hip"], heads_of["torch"]):
        assert torch.equal(a, b), k
    for i, n in enumerate(N.GRAD_NAMES):
        print("%-50s hip %.3g  torch %.3g" % (n, errs["hip"][i], errs["torch"][i]))
    print("%s: gradient error, rms over tensors: conv_backend hip %.3g  torch %.3g" % (fixture, T.rms(errs["hip"]), T.rms(errs["torch"])))
    assert T.rms(errs["hip"]) <= 2 * T.rms(errs["torch"])


def test_one_trainer_step_with_hip_convolution_gradients(dev, reproducible_forward):
    """build_train_model with conv_backend 'hip' -> the HIP loss -> backward -> the HIP SGD step: every parameter changes, and two
    such steps from the same seed leave bit-identical parameters."""
    runs = [T.trainer_steps(dev, dict(conv_backend="hip"), 1) for _ in range(2)]
    for _, _, net in runs:
        assert net.backend == "hip" and net.conv_backend == "hip"
        assert all(m.conv_backend == "hip" for m in net.modules() if isinstance(m, train.ConvBNLeaky))
    differ = [n for (n, _), a, b in zip(runs[0][2].named_parameters(), runs[0][1][0], runs[1][1][0]) if not torch.equal(a, b)]
    assert not differ, differ[:5]
