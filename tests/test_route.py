"""GPU tests of the up-sampling / concat / split kernels (om_route_concat_forward, om_route_concat_backward, csrc/route.hip) through
the C ABI, through orienmask_amd.train.upsample_concat / split_channels and through the training models built with
route_backend='hip'.

The reference is tests/route_np.py, which tests/test_route_cpu.py pins to torch's own composition on the CPU: the forward is copies
and must match it bit for bit; the backward is a sequential float32 block sum in a stated order and must match it bit for bit too,
and be within the sequential-sum bound of the float64 sum.  Every output is pre-filled with NaN, so "finite" means "written".

Figures measured on an MI355X are recorded in DESIGN.md 3.22."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
import bn_act_np as N
import route_np as R
import train_step as T
from orienmask_amd import lib as omlib, synth, train

pytestmark = pytest.mark.gpu

OM_EINVAL = -1
BOTH_FORMS = [R.CASES[4], R.CASES[6], R.CASES[9]]      # cases 5, 7 and 10 of the table
_REFERENCES = {}      # case -> (sources, dy, y, gradients): computed once, never modified


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _reference(case):
    key = R.case_id(case)
    if key not in _REFERENCES:
        srcs, dy = R.inputs(case, 5 + sum(case[:3]))
        chans, scales = R.chans_scales(case)
        _REFERENCES[key] = (srcs, dy, R.forward(srcs, chans, scales, *case[:3]), R.backward(dy, chans, scales))
    return _REFERENCES[key]


def _carve(dev, shape, offset, fill=float("nan")):
    """A contiguous tensor of `shape` that starts `offset` floats into a fresh (256-byte aligned) buffer."""
    n = int(np.prod(shape))
    buf = torch.full((n + 8,), fill, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf[offset:offset + n].view(*shape)


def _put(dev, a, offset):
    t = _carve(dev, a.shape, offset)
    t.copy_(torch.from_numpy(a))
    return t


def _arrays(chans, scales):
    n = len(chans)
    return ((ctypes.c_int * 4)(*list(chans) + [0] * (4 - n)), (ctypes.c_int * 4)(*list(scales) + [0] * (4 - n)))


def _ptrs(ts):
    return (ctypes.c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in ts] + [None] * (4 - len(ts)))


def _call_fwd(dev, srcs, chans, scales, B, H, W, y, n=None):
    c, s = _arrays(chans, scales)
    return omlib.load().om_route_concat_forward(_ptrs(srcs), c, s, len(chans) if n is None else n, B, H, W, T.vp(y),
                                                omlib.current_stream_ptr(dev))


def _call_bwd(dev, dy, chans, scales, B, H, W, dsrc, n=None):
    c, s = _arrays(chans, scales)
    return omlib.load().om_route_concat_backward(T.vp(dy), c, s, len(chans) if n is None else n, B, H, W, _ptrs(dsrc),
                                                 omlib.current_stream_ptr(dev))


def _forward(dev, case, srcs, offset=0):
    """y through the C ABI -> numpy; srcs numpy arrays or None."""
    B, H, W, _ = case
    chans, scales = R.chans_scales(case)
    ts = [_put(dev, a, offset) if a is not None else None for a in srcs]
    y = _carve(dev, (B, sum(chans), H, W), offset)
    omlib.check(_call_fwd(dev, ts, chans, scales, B, H, W, y), "om_route_concat_forward")
    torch.cuda.synchronize(dev)
    return y.cpu().numpy()


def _backward(dev, case, dy, want=None, offset=0):
    """The gradients through the C ABI -> numpy arrays; want[i] False: dsrc[i] is passed as null and its NaN-filled tensor comes
    back as it was."""
    B, H, W, _ = case
    chans, scales = R.chans_scales(case)
    want = [True] * len(chans) if want is None else want
    d = _put(dev, dy, offset)
    outs = [_carve(dev, (B, c, H // s, W // s), offset) for c, s in zip(chans, scales)]
    omlib.check(_call_bwd(dev, d, chans, scales, B, H, W, [o if w else None for o, w in zip(outs, want)]), "om_route_concat_backward")
    torch.cuda.synchronize(dev)
    return [o.cpu().numpy() for o in outs]


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_forward_equals_the_restatement(dev, case):
    srcs, _, want, _ = _reference(case)
    got = _forward(dev, case, srcs)
    assert got.shape == want.shape and np.isfinite(got).all()
    assert np.array_equal(R.bits(got), R.bits(want))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_backward_equals_the_restatement_and_is_within_the_bound(dev, case):
    _, dy, _, want = _reference(case)
    chans, scales = R.chans_scales(case)
    got = _backward(dev, case, dy)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.isfinite(g).all(), (case, i)
        assert np.array_equal(R.bits(g), R.bits(w)), (case, i)
    worst = R.within_bound(got, dy, chans, scales)
    print("%s: worst error / bound %.3f" % (R.case_id(case), worst))


@pytest.mark.parametrize("case", BOTH_FORMS, ids=R.case_id)
def test_both_forms_give_the_same_bits(dev, case):
    """Every tensor 16-byte aligned, then every tensor one float into its buffer (the scalar form, whatever W is)."""
    srcs, dy, y, grads = _reference(case)
    for offset in (0, 1):
        got = _forward(dev, case, srcs, offset)
        assert np.array_equal(R.bits(got), R.bits(y)), (case, offset)
        back = _backward(dev, case, dy, offset=offset)
        for i, (g, w) in enumerate(zip(back, grads)):
            assert np.array_equal(R.bits(g), R.bits(w)), (case, offset, i)


@pytest.mark.parametrize("guard", [4099, 4100], ids=["guard4099", "guard4100"])
@pytest.mark.parametrize("case", [R.CASES[4], R.CASES[9]], ids=R.case_id)
def test_neighbours_untouched(dev, case, guard):
    """y, and each dsrc, is a view in the middle of a sentinel-filled buffer; guard 4099 puts it at an odd float, 4100 on a
    16-byte boundary."""
    B, H, W, _ = case
    chans, scales = R.chans_scales(case)
    srcs, dy, y_want, grads = _reference(case)
    sentinel = -12345.5

    def framed(shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * guard,), sentinel, device=dev)
        view = buf[guard:guard + n]
        view.fill_(float("nan"))
        return buf, view.view(*shape)

    ybuf, y = framed(y_want.shape)
    omlib.check(_call_fwd(dev, [torch.from_numpy(a).to(dev) for a in srcs], chans, scales, B, H, W, y), "om_route_concat_forward")
    frames = [framed(g.shape) for g in grads]
    omlib.check(_call_bwd(dev, torch.from_numpy(dy).to(dev), chans, scales, B, H, W, [v for _, v in frames]), "om_route_concat_backward")
    torch.cuda.synchronize(dev)
    for buf, view, want in [(ybuf, y, y_want)] + [(b, v, g) for (b, v), g in zip(frames, grads)]:
        n = want.size
        assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + n:] == sentinel).all())
        assert np.array_equal(R.bits(view.cpu().numpy()), R.bits(want))


@pytest.mark.parametrize("case", [R.CASES[9], R.CASES[6]], ids=R.case_id)
def test_null_gradients_are_skipped_and_null_sources_are_zeros(dev, case):
    srcs, dy, y, grads = _reference(case)
    for want in ([True, False, True, False], [False, True, False, False], [False, False, False, True]):
        got = _backward(dev, case, dy, want)
        for i, (g, w, keep) in enumerate(zip(got, grads, want)):
            if keep:
                assert np.array_equal(R.bits(g), R.bits(w)), (want, i)
            else:
                assert np.isnan(g).all(), (want, i)
    chans, scales = R.chans_scales(case)
    for missing in range(4):
        part = [None if i == missing else a for i, a in enumerate(srcs)]
        got = _forward(dev, case, part)
        assert np.array_equal(R.bits(got), R.bits(R.forward(part, chans, scales, *case[:3]))), missing
        off = sum(chans[:missing])
        assert not got[:, off:off + chans[missing]].any()


@pytest.mark.parametrize("case", [R.CASES[6], R.CASES[9]], ids=R.case_id)
def test_batch_independence(dev, case):
    """Each image run alone, and the reversed batch reversed back, have the whole batch's bits."""
    srcs, dy, _, _ = _reference(case)
    y = _forward(dev, case, srcs)
    grads = _backward(dev, case, dy)
    one = (1,) + case[1:]
    for i in range(case[0]):
        alone = _forward(dev, one, [np.ascontiguousarray(a[i:i + 1]) for a in srcs])
        assert np.array_equal(R.bits(alone[0]), R.bits(y[i])), (case, i)
        galone = _backward(dev, one, np.ascontiguousarray(dy[i:i + 1]))
        for g, w in zip(galone, grads):
            assert np.array_equal(R.bits(g[0]), R.bits(w[i])), (case, i)
    back = _forward(dev, case, [np.ascontiguousarray(a[::-1]) for a in srcs])[::-1]
    assert np.array_equal(R.bits(back), R.bits(y))
    gback = _backward(dev, case, np.ascontiguousarray(dy[::-1]))
    for g, w in zip(gback, grads):
        assert np.array_equal(R.bits(g[::-1]), R.bits(w))


def test_rerun_and_a_non_default_stream_give_the_same_bits(dev):
    case = R.CASES[7]
    srcs, dy, y, grads = _reference(case)
    runs = [(_forward(dev, case, srcs), _backward(dev, case, dy)) for _ in range(2)]
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        runs.append((_forward(dev, case, srcs), _backward(dev, case, dy)))
    for got, back in runs:
        assert np.array_equal(R.bits(got), R.bits(y))
        for g, w in zip(back, grads):
            assert np.array_equal(R.bits(g), R.bits(w))


def test_refusals_on_the_device(dev):
    """Each returns OM_EINVAL with a message, launches nothing and leaves the NaN fill; a valid call afterwards works."""
    L = omlib.load()
    B, H, W, chans, scales = 2, 8, 16, [3, 2], [2, 1]
    srcs = [torch.randn(B, c, H // s, W // s, device=dev) for c, s in zip(chans, scales)]
    dy = torch.randn(B, sum(chans), H, W, device=dev)
    y = torch.full((B, sum(chans), H, W), float("nan"), device=dev)
    dsrc = [torch.full_like(t, float("nan")) for t in srcs]

    def both(chans_, scales_, B_, H_, W_, n=None):
        for rc in (_call_fwd(dev, srcs, chans_, scales_, B_, H_, W_, y, n), _call_bwd(dev, dy, chans_, scales_, B_, H_, W_, dsrc, n)):
            assert rc == OM_EINVAL, (chans_, scales_, B_, H_, W_, n)
            assert L.om_last_error()

    both(chans, scales, B, H, W, n=0)
    both(chans + [1, 1], scales + [1, 1], B, H, W, n=5)
    both(chans, [3, 1], B, 6, 6)
    both(chans, [16, 1], B, 16, 16)
    both(chans, [2, 1], B, 7, 16)                # H not divisible by a scale
    both(chans, [2, 1], B, 8, 15)
    both(chans, scales, 0, H, W)
    both([0, 2], scales, B, H, W)
    both([1024, 1024], [1, 1], 1, 1024, 1024)     # 2^31 elements, as numbers only
    both([1 << 30, 1 << 30], [1, 1], 4, 8, 8)
    assert _call_fwd(dev, srcs, chans, scales, B, H, W, None) == OM_EINVAL
    assert _call_bwd(dev, None, chans, scales, B, H, W, dsrc) == OM_EINVAL
    assert _call_bwd(dev, dy, chans, scales, B, H, W, [None, None]) == OM_EINVAL
    assert b"dsrc" in L.om_last_error()
    torch.cuda.synchronize(dev)
    assert torch.isnan(y).all() and all(torch.isnan(t).all() for t in dsrc)
    omlib.check(_call_fwd(dev, srcs, chans, scales, B, H, W, y), "om_route_concat_forward")
    omlib.check(_call_bwd(dev, dy, chans, scales, B, H, W, dsrc), "om_route_concat_backward")
    torch.cuda.synchronize(dev)
    assert torch.isfinite(y).all() and all(torch.isfinite(t).all() for t in dsrc)


# ---------------------------------------------------------------------------------------------------------------- the functions
def _compose(ts, scales):
    return torch.cat([F.interpolate(t, scale_factor=s, mode="nearest") if s > 1 else t for t, s in zip(ts, scales)], dim=1)


@pytest.mark.parametrize("case", BOTH_FORMS, ids=R.case_id)
def test_upsample_concat_under_autograd(dev, case):
    srcs, dy, _, grads = _reference(case)
    _, scales = R.chans_scales(case)
    ts = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in srcs]
    y = train.upsample_concat(ts, scales)
    assert torch.equal(y, _compose([t.detach() for t in ts], scales))
    y.backward(torch.from_numpy(dy).to(dev))
    for t, w in zip(ts, grads):
        assert np.array_equal(R.bits(t.grad.cpu().numpy()), R.bits(w))


@pytest.mark.parametrize("case", BOTH_FORMS + [(2, 24, 24, [(6, 1), (6, 1), (6, 1)])], ids=R.case_id)
def test_split_channels_under_autograd(dev, case):
    chans, _ = R.chans_scales(case)
    rng = np.random.Generator(np.random.PCG64(19))
    x = torch.from_numpy(rng.standard_normal((case[0], sum(chans), case[1], case[2])).astype(np.float32)).to(dev).requires_grad_(True)
    cots = [torch.from_numpy(rng.standard_normal((case[0], c, case[1], case[2])).astype(np.float32)).to(dev) for c in chans]
    outs = train.split_channels(x, chans)
    assert len(outs) == len(chans)
    for o, t in zip(outs, torch.split(x.detach(), chans, dim=1)):
        assert o.is_contiguous() and torch.equal(o, t)
    torch.autograd.backward(list(outs), cots)
    want = R.forward([c.cpu().numpy() for c in cots], chans, [1] * len(chans), *case[:3])
    assert np.array_equal(R.bits(x.grad.cpu().numpy()), R.bits(want))


def test_a_source_without_requires_grad_gets_no_gradient(dev):
    case = R.CASES[9]
    srcs, dy, _, grads = _reference(case)
    _, scales = R.chans_scales(case)
    ts = [torch.from_numpy(a).to(dev).requires_grad_(i in (0, 3)) for i, a in enumerate(srcs)]
    train.upsample_concat(ts, scales).backward(torch.from_numpy(dy).to(dev))
    for i, (t, w) in enumerate(zip(ts, grads)):
        if i in (0, 3):
            assert np.array_equal(R.bits(t.grad.cpu().numpy()), R.bits(w))
        else:
            assert t.grad is None
    frozen = [t.detach() for t in ts]
    assert train.upsample_concat(frozen, scales).grad_fn is None


def test_a_split_output_left_out_of_the_loss_contributes_zeros(dev):
    x = torch.randn(2, 18, 24, 24, device=dev, requires_grad=True)
    a, b, c = train.split_channels(x, [6, 6, 6])
    cot = torch.randn(2, 6, 24, 24, device=dev)
    torch.autograd.backward([a, c], [cot, 2 * cot])
    assert torch.equal(x.grad[:, :6], cot) and torch.equal(x.grad[:, 12:], 2 * cot)
    assert not x.grad[:, 6:12].any()
    del b


def test_a_non_contiguous_cotangent_works(dev):
    case = R.CASES[9]
    srcs, dy, _, grads = _reference(case)
    _, scales = R.chans_scales(case)
    ts = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in srcs]
    cot = torch.from_numpy(np.ascontiguousarray(dy.transpose(0, 1, 3, 2))).to(dev).transpose(2, 3)
    assert not cot.is_contiguous()
    train.upsample_concat(ts, scales).backward(cot)
    for t, w in zip(ts, grads):
        assert np.array_equal(R.bits(t.grad.cpu().numpy()), R.bits(w))
    x = torch.randn(2, 8, 6, 6, device=dev, requires_grad=True)
    outs = train.split_channels(x, [3, 5])
    cots = [torch.randn(2, c, 6, 6, device=dev).transpose(2, 3) for c in (3, 5)]
    torch.autograd.backward(list(outs), cots)
    assert torch.equal(x.grad, torch.cat(cots, dim=1))


def test_function_refusals(dev):
    t = torch.randn(2, 4, 6, 8, device=dev)
    half = torch.randn(2, 4, 3, 4, device=dev)
    E = omlib.OrienMaskHipError
    assert train.upsample_concat([half, t], [2, 1]).shape == (2, 8, 6, 8)
    with pytest.raises(E, match="no CPU fallback"):
        train.upsample_concat([half.cpu(), t], [2, 1])
    with pytest.raises(E, match="float32"):
        train.upsample_concat([half.double(), t], [2, 1])
    with pytest.raises(E, match="contiguous"):
        train.upsample_concat([half, t.to(memory_format=torch.channels_last)], [2, 1])
    with pytest.raises(E, match="do not give one"):
        train.upsample_concat([half, t], [1, 1])
    with pytest.raises(E, match="do not give one"):
        train.upsample_concat([half[:1], t], [2, 1])
    for bad in (3, 16, 0, 2.0):
        with pytest.raises(E, match="scale"):
            train.upsample_concat([half, t], [bad, 1])
    with pytest.raises(ValueError, match="1 to 4"):
        train.upsample_concat([t] * 5, [1] * 5)
    with pytest.raises(ValueError, match="as many scales"):
        train.upsample_concat([t], [1, 1])
    with pytest.raises(E, match="no CPU fallback"):
        train.split_channels(t.cpu(), [2, 2])
    with pytest.raises(E, match="float32"):
        train.split_channels(t.half(), [2, 2])
    with pytest.raises(E, match="contiguous"):
        train.split_channels(t.transpose(2, 3), [2, 2])
    with pytest.raises(E, match="do not split"):
        train.split_channels(t, [2, 3])
    with pytest.raises(ValueError, match="1 to 4"):
        train.split_channels(t, [1, 1, 1, 1, 0])


# ---------------------------------------------------------------------------------------------------------------- the models
ALL_HIP = dict(backend="hip", conv_backend="hip", conv_forward="hip")


@pytest.mark.parametrize("fixture", ["train_step_f96_b2", "train_step_bneval_f96_b2"])
def test_model_against_the_torch_routes_and_the_reference_step(dev, fixture):
    """route_backend 'hip' against 'torch', everything else HIP in both so that it repeats its bits.  The forward is copies: the six
    heads are equal.  The backward sums an up-sampled route's gradient in another order than torch's GPU kernel, so against the
    reference's recorded step (CPU float32) the rms over tensors of the parameter gradients' relative-L2 error is for 'hip' at
    most twice that of 'torch' measured here."""
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    heads, grads, gerr = {}, {}, {}
    for rb in ("torch", "hip"):
        heads[rb], grads[rb], _, gerr[rb], _ = T.recorded_step(dev, g, route_backend=rb, **ALL_HIP)
    for k, a, b in zip(N.HEAD_KEYS, heads["hip"], heads["torch"]):
        assert torch.equal(a, b), k
    same = sum(torch.equal(grads["hip"][n], grads["torch"][n]) for n in grads["hip"])
    print("%s: gradient error, rms over tensors: route_backend hip %.6g  torch %.6g; %d of %d gradients bit-equal"
          % (fixture, T.rms(gerr["hip"]), T.rms(gerr["torch"]), same, len(grads["hip"])))
    assert T.rms(gerr["hip"]) <= 2 * T.rms(gerr["torch"])


def test_the_non_plus_model_has_the_torch_routes_heads(dev):
    x = synth.synth_image_batch(8, 2, 96, 96).to(dev)
    torch.manual_seed(5)
    ref = train.OrienMaskYOLO(3, 80, route_backend="torch", **ALL_HIP)
    net = train.OrienMaskYOLO(3, 80, route_backend="hip", **ALL_HIP)
    net.load_state_dict(ref.state_dict(), strict=True)
    outs = []
    for m in (ref, net):
        m = m.to(dev).train()
        heads = [t for pair in m(x) for t in pair]
        torch.autograd.backward(heads, [torch.ones_like(h) for h in heads])
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
        outs.append([h.detach() for h in heads])
    for k, a, b in zip(N.HEAD_KEYS, outs[1], outs[0]):
        assert torch.isfinite(a).all() and torch.equal(a, b), k


def test_one_trainer_step_repeats_its_bits(dev):
    """build_train_model with all four options 'hip' -> the HIP loss -> backward -> the HIP SGD step, twice from one seed: the loss
    and every parameter are bit-identical, and no parameter is left unchanged."""
    def dense(out):
        assert all(o.is_contiguous() for _, o in out)      # the split's outputs are dense: the loss reads them as they are

    runs = [T.trainer_steps(dev, dict(conv_backend="hip", conv_forward="hip", route_backend="hip"), 1, on_output=dense) for _ in range(2)]
    for _, _, net in runs:
        assert (net.backend, net.conv_backend, net.conv_forward, net.route_backend) == ("hip",) * 4
    assert np.array_equal(runs[0][0][0], runs[1][0][0])
    differ = [n for (n, _), a, b in zip(runs[0][2].named_parameters(), runs[0][1][0], runs[1][1][0]) if not torch.equal(a, b)]
    assert not differ, differ[:5]
