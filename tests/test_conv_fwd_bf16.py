"""GPU tests of the bf16 forward convolution and frozen block (om_conv2d_bf16_forward, om_conv2d_bf16_frozen_forward,
csrc/conv_fwd_bf16.hip) through the C ABI and through orienmask_amd.train.conv2d_bf16 / conv_bn_leaky_frozen.

The arithmetic contract (include/orienmask_hip.h): x bf16 widened exactly, w the float32 master weight rounded to bf16 (nearest even)
by the kernel, exact products, one float32 sum whose order is a function of the geometry only, one float32 bias add, and the bf16
output the rounding of the float32 output.  Every output is pre-filled with NaN bits, so "finite" means "written".  Truth, S and the
torch-CPU yardstick are tests/conv_fwd_bf16_np.py; the rounding is tests/bf16_np.py.

Accuracy bar (test 4): per element |y - truth| <= k * 2^-23 * S, k = cin * ksize^2, S the sum of the |products|: at most k additions,
each committing at most one float32 ulp of a partial sum that S bounds, whatever the matrix instruction's internal rounding; the
products are exact.  It guards the precision class only (nothing accumulated in bf16); the integer test guards the indexing.  The
worst observed |y - truth| / (k * 2^-24 * S) per geometry class, beside torch-CPU float32's, is recorded in DESIGN.md 3.28."""
import numpy as np
import pytest
import torch

import bf16_np as Q
import conv_frozen_np as CF
import conv_fwd_bf16_np as C
import train_step as T
from orienmask_amd import lib as omlib, train
from test_conv_fwd import SPECIAL, _has_bias

pytestmark = pytest.mark.gpu

OM_EINVAL = -1
FULL_K = [(2, 512, 1024, 3, 1, 17, 17), (2, 1024, 512, 1, 1, 17, 17)]
NAN_BITS = 0x7fc0


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


_REFERENCES = {}      # computed once, never modified
WORST = {}            # geometry class -> (kernel, torch-CPU) worst error in units of k * 2^-24 * S


def _reference(case, seed, bias=None):
    bias = _has_bias(case) if bias is None else bias      # the head convolutions are the ones with a bias
    key = (case, seed, bias)
    if key not in _REFERENCES:
        d = C.inputs(*case, seed, bias)
        _REFERENCES[key] = (d, C.truth(d), C.scale(d), C.yardstick(d))
    return _REFERENCES[key]


def _bf16_dev(dev, bits, offset=0):
    """A device bf16 tensor with these bits; offset: a view that starts `offset` elements into a larger buffer."""
    flat = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).reshape(-1))
    buf = torch.zeros(flat.numel() + offset, dtype=torch.int16, device=dev)
    buf[offset:] = flat.to(dev)
    return buf[offset:].view(torch.bfloat16).view(bits.shape)


def _out(dev, shape, f32, offset=0):
    n = int(np.prod(shape))
    if f32:
        return torch.full((n,), float("nan"), device=dev).view(shape)
    buf = torch.full((n + offset,), NAN_BITS, dtype=torch.int16, device=dev)
    return buf[offset:].view(torch.bfloat16).view(shape)


def _np_out(y):
    """float32 array, or the uint16 bits of a bf16 tensor."""
    if y.dtype == torch.float32:
        return y.cpu().numpy()
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _call(dev, x, w, b, ks, stride, y):
    B, cin, H, W = x.shape
    return omlib.load().om_conv2d_bf16_forward(T.vp(x), T.vp(w), T.vp(b), B, cin, H, W, w.shape[0], ks, stride, T.vp(y),
                                               1 if y.dtype == torch.float32 else 0, omlib.current_stream_ptr(dev))


def _hip(dev, d, f32=True, w=None, x_offset=0, y_offset=0):
    """y through the C ABI, pre-filled with NaN.  -> float32 array, or uint16 bits."""
    x = _bf16_dev(dev, d["x_bits"], x_offset)
    wt = torch.from_numpy(d["w"] if w is None else w).to(dev)
    b = torch.from_numpy(d["bias"]).to(dev) if d["bias"] is not None else None
    Ho, Wo = C.out_hw(x.shape[2], x.shape[3], d["ksize"], d["stride"])
    y = _out(dev, (x.shape[0], wt.shape[0], Ho, Wo), f32, y_offset)
    omlib.check(_call(dev, x, wt, b, d["ksize"], d["stride"], y), "om_conv2d_bf16_forward")
    torch.cuda.synchronize(dev)
    return _np_out(y)


def _written(bits):
    return bool((bits != NAN_BITS).all())


# ---------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("case", T.SWEEP + SPECIAL + FULL_K, ids=T.case_id)
def test_exact_on_integer_data(dev, case):
    """x, w in -4 ... 4, bias in -8 ... 8: every partial sum in any order is an integer below 2^24, so the float32 output equals
    the float64 truth exactly and the bf16 output its rounding: any dropped, doubled or misplaced tap at any k shows."""
    d = C.integer_inputs(*case, seed=sum(case) + 11)
    t = C.truth(d)
    assert np.abs(t).max() < 2 ** 24 and np.array_equal(t.astype(np.float32).astype(np.float64), t)
    got = _hip(dev, d, True)
    assert got.shape == t.shape and np.isfinite(got).all(), (case, "an element was not written")
    assert np.array_equal(got.astype(np.float64), t), (case, int((got != t).sum()))
    bits = _hip(dev, d, False)
    assert np.array_equal(bits, Q.round_bits(t.astype(np.float32))), case


# ---------------------------------------------------------------------------------------------------------------- 2. weight rounding
def _tie_weights(shape):
    """Exact bf16 ties m * 2^-8 with the kept bit even and odd, both signs, one ulp either side of them, and the largest finite
    float32 (which rounds to inf) in one place."""
    words = np.array([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,
                      0x40008000, 0xc0018000, 0x3e828000, 0xbe838000], dtype=np.uint32)
    w = np.resize(words, int(np.prod(shape))).view(np.float32).reshape(shape).copy()
    w.reshape(-1)[5] = np.float32(3.4028234663852886e38)
    return w


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("case", [(3, 5, 7, 3, 1, 17, 17), (2, 64, 255, 1, 1, 17, 17)], ids=T.case_id)
def test_weight_is_rounded_to_nearest_even(dev, case, kind):
    """kernel(x, w) is bit-equal to kernel(x, quantise(w)): distinguishes round-to-nearest-even from truncation and from
    round-half-up (the ties) on the float32 master weight."""
    d = _reference(case, 61, bias=False)[0]
    w = d["w"] if kind == "random" else _tie_weights(d["w"].shape)
    wq = Q.quantise(w)
    assert not np.array_equal(w.view(np.uint32), wq.view(np.uint32))
    if kind == "ties":                       # truncation and round-half-up would each give other weights
        trunc = (w.view(np.uint32) & 0xffff0000).view(np.float32)
        half_up = ((w.view(np.uint32).astype(np.uint64) + 0x8000) >> 16 << 16).astype(np.uint32).view(np.float32)
        assert not np.array_equal(trunc, wq) and not np.array_equal(half_up.view(np.uint32), wq.view(np.uint32))
    a, b = _hip(dev, d, True, w=w), _hip(dev, d, True, w=wq)
    assert not np.isnan(a).any() or kind == "ties"
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (case, kind)
    if kind == "ties":                       # and the other two roundings are told apart by the output itself
        for other in (trunc, half_up):
            assert not np.array_equal(_hip(dev, d, True, w=other).view(np.uint32), a.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 3. one rounding
@pytest.mark.parametrize("case", SPECIAL, ids=T.case_id)
def test_bf16_output_is_the_rounded_float32_output(dev, case):
    d = _reference(case, sum(case) * 3 + 2)[0]
    y32, bits = _hip(dev, d, True), _hip(dev, d, False)
    assert np.isfinite(y32).all() and _written(bits)
    assert np.array_equal(bits, Q.round_bits(y32)), case


# ---------------------------------------------------------------------------------------------------------------- 4. accuracy
def _klass(case):
    return "%dx%d s%d" % (case[3], case[3], case[4])


@pytest.mark.parametrize("case", T.SWEEP + SPECIAL + FULL_K, ids=T.case_id)
def test_accuracy_on_random_data(dev, case):
    d, truth, S, ref = _reference(case, sum(case) * 5 + 1)
    got = _hip(dev, d, True)
    assert got.shape == truth.shape and np.isfinite(got).all(), (case, "an element was not written")
    k = C.k_of(d)
    unit = k * 2.0 ** -24 * np.maximum(S, np.finfo(np.float64).tiny)
    mine, theirs = float((np.abs(got - truth) / unit).max()), float((np.abs(ref - truth) / unit).max())
    kl = _klass(case)
    WORST[kl] = (max(WORST.get(kl, (0, 0))[0], mine), max(WORST.get(kl, (0, 0))[1], theirs))
    print("%-34s k %5d  |y-truth| / (k 2^-24 S): hip %.4f  torch-cpu-f32 %.4f   worst of %s so far: hip %.4f torch %.4f"
          % (case, k, mine, theirs, kl, WORST[kl][0], WORST[kl][1]))
    assert (np.abs(got - truth) <= k * 2.0 ** -23 * S).all(), (case, mine)


# ---------------------------------------------------------------------------------------------------------------- 5. batch, neighbours
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(5, 16, 32, 3, 1, 3, 5), (3, 5, 7, 3, 1, 17, 17), (5, 32, 64, 3, 2, 8, 8), (4, 64, 32, 1, 1, 17, 17)],
                         ids=T.case_id)
def test_batch_independence(dev, case, f32):
    """The batch equals, bit for bit, every image run alone, and the reversed batch reversed back."""
    d = _reference(case, 41, bias=True)[0]
    view = (lambda a: a.view(np.uint32)) if f32 else (lambda a: a)
    whole = _hip(dev, d, f32)
    assert np.isfinite(whole).all() if f32 else _written(whole)
    for i in range(case[0]):
        alone = _hip(dev, dict(d, x_bits=np.ascontiguousarray(d["x_bits"][i:i + 1])), f32)
        assert np.array_equal(view(alone[0]), view(whole[i])), (case, i)
    back = _hip(dev, dict(d, x_bits=np.ascontiguousarray(d["x_bits"][::-1])), f32)[::-1]
    assert np.array_equal(view(np.ascontiguousarray(back)), view(whole)), case


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(3, 5, 7, 3, 2, 17, 17), (2, 64, 255, 1, 1, 17, 17)], ids=T.case_id)
def test_neighbours_untouched(dev, case, f32):
    """y is a view in the middle of a larger buffer: the sentinel on both sides is intact after the call."""
    d, truth, _, _ = _reference(case, 43)
    x, w = _bf16_dev(dev, d["x_bits"]), torch.from_numpy(d["w"]).to(dev)
    b = torch.from_numpy(d["bias"]).to(dev) if d["bias"] is not None else None
    n, guard, sentinel = truth.size, 4099, -12288.0
    buf = torch.full((n + 2 * guard,), sentinel, device=dev, dtype=torch.float32 if f32 else torch.bfloat16)
    y = buf[guard:guard + n]
    y.fill_(float("nan"))
    omlib.check(_call(dev, x, w, b, d["ksize"], d["stride"], y), "om_conv2d_bf16_forward")
    torch.cuda.synchronize(dev)
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + n:] == sentinel).all())
    got = y.float().cpu().numpy().reshape(truth.shape)
    assert np.isfinite(got).all()
    assert np.abs(got - truth).max() <= (1e-5 if f32 else 2.0 ** -8) * np.abs(truth).max()


@pytest.mark.parametrize("case", [(3, 5, 7, 3, 2, 17, 17), (1, 3, 32, 3, 2, 33, 31)], ids=T.case_id)
def test_views_at_odd_element_offsets(dev, case):
    """A bf16 tensor is only guaranteed 2-byte alignment: an x view and a bf16 y view that start at an odd element give the bits
    of the aligned call."""
    d = _reference(case, 47, bias=True)[0]
    y32, bits = _hip(dev, d, True), _hip(dev, d, False)
    assert np.isfinite(y32).all() and _written(bits)
    assert np.array_equal(_hip(dev, d, True, x_offset=1).view(np.uint32), y32.view(np.uint32))
    assert np.array_equal(_hip(dev, d, False, x_offset=1), bits)
    assert np.array_equal(_hip(dev, d, False, y_offset=1), bits)
    assert np.array_equal(_hip(dev, d, False, x_offset=3, y_offset=5), bits)


# ---------------------------------------------------------------------------------------------------------------- 6. frozen
FROZEN = [(3, 5, 7, 1, 1, 17, 17), (3, 5, 7, 3, 1, 17, 17), (3, 5, 7, 3, 2, 17, 17), (2, 64, 255, 1, 1, 17, 17),
          (2, 512, 1024, 3, 1, 3, 5), (7, 16, 32, 3, 1, 1, 1)]


def _frozen_inputs(case, residual):
    d = dict(CF.inputs(*case, sum(case) * 3 + 2, residual))
    d["x_bits"] = Q.round_bits(d["x"])
    d["bias"] = None
    if residual:
        d["res_bits"] = Q.round_bits(d["residual"])
    return d


def _frozen_call(dev, x, w, stats, res, ks, stride, y):
    B, cin, H, W = x.shape
    return omlib.load().om_conv2d_bf16_frozen_forward(T.vp(x), T.vp(w), B, cin, H, W, w.shape[0], ks, stride, *[T.vp(s) for s in stats],
                                                      CF.EPS, CF.SLOPE, T.vp(res), T.vp(y), omlib.current_stream_ptr(dev))


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("case", FROZEN, ids=T.case_id)
def test_frozen_entry_equals_the_composition(dev, case, residual):
    """om_conv2d_bf16_frozen_forward == round_bits(om_bn_act_forward(eval, float32)(om_conv2d_bf16_forward(y_is_f32 = 1))) with
    the residual widened, bit for bit; conv_frozen_np's statistics (about half the gammas negative)."""
    L = omlib.load()
    d = _frozen_inputs(case, residual)
    assert (d["gamma"] < 0).any() and (d["gamma"] > 0).any()
    h = _hip(dev, d, True)
    assert np.isfinite(h).all()
    B, cout, Ho, Wo = h.shape
    stats = [torch.from_numpy(d[k]).to(dev) for k in CF.STATS]
    st = omlib.current_stream_ptr(dev)
    hd = torch.from_numpy(h).to(dev)
    res32 = torch.from_numpy(Q.widen(d["res_bits"])).to(dev) if residual else None
    want32 = torch.full_like(hd, float("nan"))
    save = torch.empty(4 * cout, device=dev)
    omlib.check(L.om_bn_act_forward(T.vp(hd), B, cout, Ho, Wo, *[T.vp(s) for s in stats], None, 0, 0.1, CF.EPS, CF.SLOPE, T.vp(res32),
                                    T.vp(want32), save.data_ptr(), save.data_ptr() + 8 * cout, None, 0, st), "om_bn_act_forward")
    torch.cuda.synchronize(dev)
    want32 = want32.cpu().numpy()
    assert np.isfinite(want32).all()
    x, w = _bf16_dev(dev, d["x_bits"]), torch.from_numpy(d["w"]).to(dev)
    res = _bf16_dev(dev, d["res_bits"]) if residual else None
    y = _out(dev, h.shape, False)
    omlib.check(_frozen_call(dev, x, w, stats, res, d["ksize"], d["stride"], y), "om_conv2d_bf16_frozen_forward")
    torch.cuda.synchronize(dev)
    got = _np_out(y)
    assert _written(got)
    assert np.array_equal(got, Q.round_bits(want32)), (case, int((got != Q.round_bits(want32)).sum()))


def test_frozen_entry_refuses_aliasing(dev):
    L = omlib.load()
    d = _frozen_inputs((3, 8, 8, 3, 1, 9, 9), True)
    x, w, res = _bf16_dev(dev, d["x_bits"]), torch.from_numpy(d["w"]).to(dev), _bf16_dev(dev, d["res_bits"])
    stats = [torch.from_numpy(d[k]).to(dev) for k in CF.STATS]
    keep_x, keep_r = x.clone(), res.clone()
    assert _frozen_call(dev, x, w, stats, res, 3, 1, x) == OM_EINVAL and b"om_conv2d_bf16_frozen_forward" in L.om_last_error()
    assert _frozen_call(dev, x, w, stats, res, 3, 1, res) == OM_EINVAL and b"alias" in L.om_last_error()
    torch.cuda.synchronize(dev)
    assert torch.equal(x, keep_x) and torch.equal(res, keep_r)


def test_frozen_module_function_on_bf16(dev):
    """conv_bn_leaky_frozen on a bf16 x: the C-ABI call's bits, bf16, no grad_fn; a mixed pair and anything that requires grad
    raise."""
    case = (3, 5, 7, 3, 1, 17, 17)
    d = _frozen_inputs(case, True)
    x, res = _bf16_dev(dev, d["x_bits"]), _bf16_dev(dev, d["res_bits"])
    conv = torch.nn.Conv2d(5, 7, 3, padding=1, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(7, eps=CF.EPS).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(d["w"]))
        for p, k in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "running_mean"), (bn.running_var, "running_var")):
            p.copy_(torch.from_numpy(d[k]))
    with torch.no_grad():
        y = train.conv_bn_leaky_frozen(x, conv.weight, bn, residual=res, stride=1, padding=1, slope=CF.SLOPE)
    assert y.dtype == torch.bfloat16 and y.grad_fn is None and not y.requires_grad
    want = _out(dev, y.shape, False)
    stats = [bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var]
    omlib.check(_frozen_call(dev, x, conv.weight.detach(), stats, res, 3, 1, want), "om_conv2d_bf16_frozen_forward")
    assert np.array_equal(_np_out(y), _np_out(want)) and _written(_np_out(y))
    with pytest.raises(omlib.OrienMaskHipError, match="residual"):
        train.conv_bn_leaky_frozen(x, conv.weight.detach(), bn, residual=res.float(), stride=1, padding=1)
    with pytest.raises(omlib.OrienMaskHipError, match="requires grad"):
        train.conv_bn_leaky_frozen(x, conv.weight, bn, stride=1, padding=1)
    for p in list(conv.parameters()) + list(bn.parameters()):
        p.requires_grad_(False)
    with pytest.raises(omlib.OrienMaskHipError, match="requires grad"):
        train.conv_bn_leaky_frozen(x.clone().requires_grad_(True), conv.weight, bn, stride=1, padding=1)
    assert train.conv_bn_leaky_frozen(x, conv.weight, bn, stride=1, padding=1).grad_fn is None


# ---------------------------------------------------------------------------------------------------------------- 7. autograd
@pytest.mark.parametrize("case,bias", [((2, 16, 32, 3, 2, 9, 9), True), ((2, 8, 8, 1, 1, 5, 5), False)], ids=["3x3s2-bias", "1x1"])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_autograd_function(dev, case, bias, out_dtype):
    """conv2d_bf16: the forward is the C-ABI call; dx, dw, db are bit-equal to aten.convolution_backward on the same tensors, of
    dtypes bf16, float32, float32; a frozen weight gets no dw."""
    B, cin, cout, ks, stride, H, W = case
    d = _reference(case, 71, bias=bias)[0]
    x = _bf16_dev(dev, d["x_bits"]).clone().requires_grad_(True)
    w = torch.from_numpy(d["w"]).to(dev).requires_grad_(True)
    b = torch.from_numpy(d["bias"]).to(dev).requires_grad_(True) if bias else None
    y = train.conv2d_bf16(x, w, b, stride, ks // 2, out_dtype=out_dtype)
    assert y.dtype == out_dtype and y.grad_fn is not None
    want = _hip(dev, d, out_dtype == torch.float32)
    assert np.array_equal(_np_out(y.detach()), want)
    dy = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(y.shape)).astype(np.float32)).to(dev).to(out_dtype)
    y.backward(dy)
    rdx, rdw, rdb = torch.ops.aten.convolution_backward(dy.to(torch.bfloat16), x.detach(), w.detach().to(torch.bfloat16),
                                                        [cout] if bias else None, [stride] * 2, [ks // 2] * 2, [1, 1], False, [0, 0], 1,
                                                        [True, True, bias])
    assert x.grad.dtype == torch.bfloat16 and w.grad.dtype == torch.float32
    assert torch.equal(x.grad, rdx) and torch.equal(w.grad, rdw.float())
    if bias:
        assert b.grad.dtype == torch.float32 and torch.equal(b.grad, rdb.float())
    # a frozen weight: no dw is computed, dx is the same
    seen = []
    orig = train.conv2d_bf16_backward

    def spy(*a):
        out = orig(*a)
        seen.append(out)
        return out
    x2, w2 = x.detach().clone().requires_grad_(True), w.detach().clone()
    train.conv2d_bf16_backward = spy
    try:
        train.conv2d_bf16(x2, w2, b.detach() if bias else None, stride, ks // 2, out_dtype=out_dtype).backward(dy)
    finally:
        train.conv2d_bf16_backward = orig
    assert len(seen) == 1 and seen[0][1] is None and seen[0][2] is None
    assert torch.equal(x2.grad, rdx) and w2.grad is None


def test_module_function_refusals(dev):
    x = torch.randn(2, 8, 10, 12, device=dev).to(torch.bfloat16)
    w = torch.randn(16, 8, 3, 3, device=dev)
    with pytest.raises(omlib.OrienMaskHipError, match="contiguous"):
        train.conv2d_bf16(x.to(memory_format=torch.channels_last), w, None, 1, 1)
    with pytest.raises(omlib.OrienMaskHipError, match="bfloat16"):
        train.conv2d_bf16(x.float(), w, None, 1, 1)
    with pytest.raises(omlib.OrienMaskHipError, match="float32"):
        train.conv2d_bf16(x, w.to(torch.bfloat16), None, 1, 1)
    with pytest.raises(omlib.OrienMaskHipError, match="geometries"):
        train.conv2d_bf16(x, w, None, 3, 1)
    with pytest.raises(ValueError, match="out_dtype"):
        train.conv2d_bf16(x, w, None, 1, 1, out_dtype=torch.float16)
