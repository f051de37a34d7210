"""GPU tests of the forward convolution (om_conv2d_forward, csrc/conv_fwd.hip) through the C ABI, through
orienmask_amd.train.conv2d(forward='hip') and through the training models built with conv_forward='hip'.

Truth is tests/conv_fwd_np.py: F.conv2d in float64 on the float32 inputs.  The yardstick is F.conv2d in float32 on the CPU: kernel
and yardstick are float32 evaluations that differ in summation order only, so the kernel's maximum error over the truth's scale may
be at most TWICE torch-CPU-float32's on the same inputs, with a floor of 2e-7 (the bar of tests/test_conv_grad.py).  Every output is
pre-filled with NaN, so "every element finite" is "every element written".

Worst kernel / torch-CPU ratios measured on an MI355X are recorded in DESIGN.md 3.21."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import conv_fwd_np as C
import train_step as T
from orienmask_amd import arch, lib as omlib, train

pytestmark = pytest.mark.gpu

FLOOR = 2e-7
OM_EINVAL = -1


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# the plain head convolutions are the ones with a bias
_HEADS = {(s.cin, s.cout, s.ksize, s.stride) for s in list(arch.fpnplus_convs()) + list(arch.yolo_convs()) if not s.bn}
# (B, cin, cout, ksize, stride, H, W)
SPECIAL = [(1, 1, 1, 1, 1, 1, 1),
           (3, 5, 7, 1, 1, 17, 17), (3, 5, 7, 3, 1, 17, 17), (3, 5, 7, 3, 2, 17, 17),
           (2, 64, 255, 1, 1, 17, 17),
           (2, 256, 18, 1, 1, 24, 24),
           (1, 3, 32, 3, 1, 33, 31), (1, 3, 32, 3, 2, 33, 31), (1, 3, 32, 3, 2, 34, 32),
           (2, 1024, 512, 1, 1, 3, 5),
           (2, 512, 1024, 3, 1, 3, 5),
           (2, 512, 1024, 3, 1, 3, 3),
           (5, 32, 64, 3, 2, 8, 8),
           (5, 16, 32, 3, 1, 3, 5), (7, 16, 32, 3, 1, 1, 1),
           (3, 8, 8, 3, 1, 2, 40), (3, 8, 8, 3, 1, 40, 2)]
BIASED = {(2, 64, 255, 1, 1, 17, 17), (2, 256, 18, 1, 1, 24, 24)}
LARGE = [(2, 3, 32, 3, 1, 544, 544),
         (2, 32, 64, 3, 2, 544, 544),
         (2, 128, 64, 1, 1, 136, 136),
         (2, 512, 1024, 3, 1, 17, 17),
         (2, 1024, 512, 1, 1, 17, 17)]

_REFERENCES = {}      # (case, seed, bias) -> (inputs, truth, yardstick): computed once, never modified


def _has_bias(case):
    return case in BIASED or case[1:5] in _HEADS


def _reference(case, seed, bias=None):
    bias = _has_bias(case) if bias is None else bias
    key = (case, seed, bias)
    if key not in _REFERENCES:
        B, cin, cout, ks, stride, H, W = case
        d = C.inputs(B, cin, cout, ks, stride, H, W, seed, bias)
        _REFERENCES[key] = (d, C.truth(d), C.yardstick(d))
    return _REFERENCES[key]


def _call(dev, x, w, b, ks, stride, y):
    L = omlib.load()
    B, cin, H, W = x.shape
    return L.om_conv2d_forward(T.vp(x), T.vp(w), T.vp(b), B, cin, H, W, w.shape[0], ks, stride, T.vp(y), omlib.current_stream_ptr(dev))


def _hip(dev, d):
    """y through the C ABI, pre-filled with NaN.  -> numpy array."""
    x, w = (torch.from_numpy(d[k]).to(dev) for k in ("x", "w"))
    b = torch.from_numpy(d["bias"]).to(dev) if d["bias"] is not None else None
    Ho, Wo = C.out_hw(x.shape[2], x.shape[3], d["ksize"], d["stride"])
    y = torch.full((x.shape[0], w.shape[0], Ho, Wo), float("nan"), device=dev)
    omlib.check(_call(dev, x, w, b, d["ksize"], d["stride"], y), "om_conv2d_forward")
    torch.cuda.synchronize(dev)
    return y.cpu().numpy()


def _judge(dev, case, seed):
    """Asserts the bar for the case; -> kernel error / torch-CPU error."""
    d, truth, ref = _reference(case, seed)
    got = _hip(dev, d)
    assert got.shape == truth.shape, case
    assert np.isfinite(got).all(), (case, "an element was not written")
    e, theirs = C.rel_max(got, truth), C.rel_max(ref, truth)
    ratio = e / max(theirs, FLOOR / 2)
    print("%-34s y   hip %.3g  torch-cpu %.3g  ratio %.2f" % (case, e, theirs, ratio))
    assert e <= max(2 * theirs, FLOOR), (case, e, theirs)
    return ratio


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("case", T.SWEEP, ids=T.case_id)
def test_every_layer_geometry_against_float64(dev, case):
    """Every distinct convolution of the two models at 96 x 96 and 160 x 128, B = 2; the head convolutions with a bias."""
    _judge(dev, case, sum(case) * 5 + 1)


@pytest.mark.parametrize("case", SPECIAL, ids=T.case_id)
def test_special_shapes_against_float64(dev, case):
    """The smallest shape, channel counts that are no tile multiple (3, 5, 7, 18, 255), planes of 289 floats, odd and even stride-2
    inputs, tiny maps with deep channels (tiles that span several images and end mid-image; at 1 x 1 every cell is at an image
    boundary), rows much shorter and much longer than a tile."""
    _judge(dev, case, sum(case) * 3 + 2)


@pytest.mark.parametrize("case", LARGE, ids=T.case_id)
def test_full_size_shapes_against_float64(dev, case):
    """B = 2 at 544 x 544: many tiles, and the workload's own k (4608 for the 512 -> 1024 3x3 layer)."""
    _judge(dev, case, 17)


@pytest.mark.parametrize("case", [(5, 16, 32, 3, 1, 3, 5), (3, 5, 7, 3, 1, 17, 17), (5, 32, 64, 3, 2, 8, 8), (4, 64, 32, 1, 1, 17, 17)],
                         ids=T.case_id)
def test_batch_independence(dev, case):
    """The tiles run over the flat (image, cell) index: an image's y must not depend on its neighbours in the batch or its place
    in it.  The batch equals, bit for bit, every image run alone, and the reversed batch reversed back."""
    d = _reference(case, 41, bias=True)[0]
    whole = _hip(dev, d)
    assert np.isfinite(whole).all()
    for i in range(case[0]):
        alone = _hip(dev, dict(d, x=np.ascontiguousarray(d["x"][i:i + 1])))
        assert np.array_equal(alone[0].view(np.uint32), whole[i].view(np.uint32)), (case, i)
    back = _hip(dev, dict(d, x=np.ascontiguousarray(d["x"][::-1])))[::-1]
    assert np.array_equal(back.view(np.uint32), whole.view(np.uint32)), case


@pytest.mark.parametrize("case", [(3, 5, 7, 3, 2, 17, 17), (2, 64, 255, 1, 1, 17, 17)], ids=T.case_id)
def test_neighbours_untouched(dev, case):
    """y is a view in the middle of a larger buffer: the sentinel on both sides is intact after the call."""
    d, truth, _ = _reference(case, 43)
    x, w = (torch.from_numpy(d[k]).to(dev) for k in ("x", "w"))
    b = torch.from_numpy(d["bias"]).to(dev) if d["bias"] is not None else None
    n, guard, sentinel = truth.size, 4099, -12345.5
    buf = torch.full((n + 2 * guard,), sentinel, device=dev)
    y = buf[guard:guard + n]
    y.fill_(float("nan"))
    omlib.check(_call(dev, x, w, b, d["ksize"], d["stride"], y), "om_conv2d_forward")
    torch.cuda.synchronize(dev)
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + n:] == sentinel).all())
    got = y.cpu().numpy().reshape(truth.shape)
    assert np.isfinite(got).all()
    assert C.rel_max(got, truth) <= 1e-5


@pytest.mark.parametrize("case", [(2, 512, 1024, 3, 1, 3, 3), (2, 32, 64, 3, 2, 48, 48), (2, 3, 32, 3, 1, 544, 544)], ids=T.case_id)
def test_rerun_is_bit_identical(dev, case):
    """The same call twice; the first case is the shape on which MIOpen's forward does not repeat its bits."""
    d = _reference(case, 23)[0]
    a, b = _hip(dev, d), _hip(dev, d)
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_non_default_stream(dev):
    d = _reference((2, 32, 64, 3, 2, 48, 48), 23)[0]
    want = _hip(dev, d)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        got = _hip(dev, d)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want)


def test_refusals_on_the_device(dev):
    """Unsupported geometries, B = 0 and null pointers return OM_EINVAL; nothing is launched, y keeps its NaN fill."""
    L = omlib.load()
    B, cin, cout, H, W = 2, 32, 64, 24, 24
    x = torch.randn(B, cin, H, W, device=dev)
    y = torch.full((B, cout, H, W), float("nan"), device=dev)
    for ks, stride in ((5, 1), (3, 3), (1, 2)):
        w = torch.randn(cout, cin, ks, ks, device=dev)
        assert _call(dev, x, w, None, ks, stride, y) == OM_EINVAL, (ks, stride)
        assert b"ksize" in L.om_last_error()
    w = torch.randn(cout, cin, 3, 3, device=dev)
    st = omlib.current_stream_ptr(dev)
    assert L.om_conv2d_forward(T.vp(x), T.vp(w), None, 0, cin, H, W, cout, 3, 1, T.vp(y), st) == OM_EINVAL
    assert L.om_conv2d_forward(None, T.vp(w), None, B, cin, H, W, cout, 3, 1, T.vp(y), st) == OM_EINVAL
    assert L.om_conv2d_forward(T.vp(x), None, None, B, cin, H, W, cout, 3, 1, T.vp(y), st) == OM_EINVAL
    assert L.om_conv2d_forward(T.vp(x), T.vp(w), None, B, cin, H, W, cout, 3, 1, None, st) == OM_EINVAL
    torch.cuda.synchronize(dev)
    assert torch.isnan(y).all()
    omlib.check(_call(dev, x, w, None, 3, 1, y), "om_conv2d_forward")
    torch.cuda.synchronize(dev)
    assert torch.isfinite(y).all()


# ---------------------------------------------------------------------------------------------------------------- train.conv2d
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("ks,stride", C.GEOMETRIES, ids=["1x1", "3x3", "3x3s2"])
def test_module_function_against_float64_and_the_torch_forward(dev, ks, stride, bias):
    """train.conv2d(forward='hip'): y within the bar against float64; dx, dw, db bit-identical to forward='torch' on the same
    (x, w, dy) -- the backward and what it reads are shared."""
    case = (2, 24, 40, ks, stride, 21, 18)
    d, truth, ref = _reference(case, 31, bias=bias)
    x0, w0 = (torch.from_numpy(d[k]).to(dev) for k in ("x", "w"))
    b0 = torch.from_numpy(d["bias"]).to(dev) if bias else None
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal(truth.shape).astype(np.float32)).to(dev)
    outs = []
    for fwd in ("hip", "torch"):
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        b = b0.clone().requires_grad_(True) if bias else None
        y = train.conv2d(x, w, b, stride, ks // 2, forward=fwd)
        y.backward(dy)
        outs.append((y.detach(), x.grad, w.grad, b.grad if bias else None))
    got = outs[0][0].cpu().numpy()
    assert got.shape == truth.shape and np.isfinite(got).all()
    e, theirs = C.rel_max(got, truth), C.rel_max(ref, truth)
    print("conv2d %dx%d s%d y hip %.3g  torch-cpu %.3g  torch-gpu %.3g" % (ks, ks, stride, e, theirs,
                                                                          C.rel_max(outs[1][0].cpu().numpy(), truth)))
    assert e <= max(2 * theirs, FLOOR), (e, theirs)
    for k, a, t in zip(("dx", "dw", "db"), outs[0][1:], outs[1][1:]):
        assert (a is None) == (t is None), k
        if a is not None:
            assert torch.isfinite(a).all() and torch.equal(a, t), k


def test_module_function_refusals(dev):
    x = torch.randn(2, 8, 10, 12, device=dev)
    w = torch.randn(16, 8, 3, 3, device=dev)
    with pytest.raises(omlib.OrienMaskHipError, match="contiguous"):
        train.conv2d(x.to(memory_format=torch.channels_last), w, None, 1, 1, forward="hip")
    with pytest.raises(omlib.OrienMaskHipError, match="no CPU fallback"):
        train.conv2d(x.cpu(), w.cpu(), None, 1, 1, forward="hip")
    with pytest.raises(ValueError, match="forward"):
        train.conv2d(x, w, None, 1, 1, forward="bogus")


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("fixture", ["train_step_f96_b2", "train_step_bneval_f96_b2"])
def test_model_against_the_torch_forward_and_the_reference_step(dev, fixture):
    """conv_forward 'hip' against 'torch' (both models with backend 'hip' and conv_backend 'hip') on the same GPU, the 'torch' run
    under cudnn.flags(deterministic=True), the 'hip' run without it.  Against the reference's recorded step (CPU float32): the rms
    over tensors of the relative-L2 error of the heads, and of the parameter gradients, is for 'hip' at most twice that of 'torch'
    measured here -- both are float32 evaluations in another summation order than the recording's."""
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    herr, gerr = {}, {}
    for cf in ("torch", "hip"):
        assert not torch.backends.cudnn.deterministic      # the flag of the 'torch' run ends with its step
        _, _, herr[cf], gerr[cf], _ = T.recorded_step(dev, g, deterministic=cf == "torch", backend="hip", conv_backend="hip",
                                                      conv_forward=cf)
    print("%s: head error, rms over tensors: conv_forward hip %.3g  torch %.3g" % (fixture, T.rms(herr["hip"]), T.rms(herr["torch"])))
    print("%s: gradient error, rms over tensors: conv_forward hip %.3g  torch %.3g" % (fixture, T.rms(gerr["hip"]), T.rms(gerr["torch"])))
    assert T.rms(herr["hip"]) <= 2 * T.rms(herr["torch"])
    assert T.rms(gerr["hip"]) <= 2 * T.rms(gerr["torch"])


def test_one_trainer_step_repeats_its_bits_without_the_deterministic_flag(dev):
    """build_train_model with conv_backend and conv_forward 'hip' -> the HIP loss -> backward -> the HIP SGD step, twice from the
    same seed with torch.backends.cudnn.deterministic left False: the loss and every parameter are bit-identical."""
    assert not torch.backends.cudnn.deterministic
    runs = [T.trainer_steps(dev, dict(conv_backend="hip", conv_forward="hip"), 1) for _ in range(2)]
    for _, _, net in runs:
        assert net.backend == "hip" and net.conv_backend == "hip" and net.conv_forward == "hip"
        assert all(m.conv_forward == "hip" for m in net.modules() if isinstance(m, train.ConvBNLeaky))
    assert np.array_equal(runs[0][0][0], runs[1][0][0])
    differ = [n for (n, _), a, b in zip(runs[0][2].named_parameters(), runs[0][1][0], runs[1][1][0]) if not torch.equal(a, b)]
    assert not differ, differ[:5]
