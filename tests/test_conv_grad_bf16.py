"""GPU tests of the bf16 convolution gradients (om_conv2d_bf16_grad_input / om_conv2d_bf16_grad_weight; csrc/conv_grad_bf16.hip, csrc/conv_dw.hip)
through the C ABI and through orienmask_amd.train.conv2d_bf16(..., backward='hip').

The arithmetic contract (include/orienmask_hip.h): dy and x bf16 widened exactly, w the float32 master weight rounded to bf16 (nearest
even) by the kernel, exact products, float32-or-wider sums in an order that is a function of the geometry (dx) or of the shape and
the device (dw) only, and the bf16 dx the rounding of the float32 dx.  Every output is pre-filled with NaN (bits), so "finite" means
"written".  Truth, S and the torch-CPU yardstick are tests/conv_grad_bf16_np.py; the rounding is tests/bf16_np.py.

Accuracy bars (test 4).  Per element |g - truth| <= K * 2^-23 * S, K = cout * ksize^2 for dx and B * Ho * Wo for dw and db, S the sum
of the |products|: at most K additions, each committing at most one float32 ulp of a partial sum that S bounds (DESIGN 3.28's bound).
For dw and db additionally the project's standing gradient bar (tests/test_conv_grad.py): rel_max(kernel) <= max(2 x rel_max(torch
CPU float32 on the same operands), 2e-7).  The worst observed figures per geometry class are recorded in DESIGN.md 3.29."""
import numpy as np
import pytest
import torch

import bf16_np as Q
import conv_grad_bf16_np as C
import train_step as T
from orienmask_amd import lib as omlib, train
from test_conv_fwd import SPECIAL
from test_conv_fwd_bf16 import _tie_weights

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7fc0
MULTI_SPLIT, SINGLE_SPLIT = (2, 3, 32, 3, 1, 96, 96), (5, 32, 64, 3, 2, 8, 8)
CASES = T.SWEEP + SPECIAL + [c for c in (MULTI_SPLIT, SINGLE_SPLIT) if c not in T.SWEEP + SPECIAL]


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


_REFERENCES = {}      # computed once, never modified
WORST = {}            # (geometry class, which) -> worst kernel / yardstick figures


def _reference(case, seed):
    key = (case, seed)
    if key not in _REFERENCES:
        d = C.inputs(*case, seed)
        _REFERENCES[key] = (d, C.truth(d), C.scale(d), C.yardstick(d))
    return _REFERENCES[key]


def _geom(d):
    B, cin, H, W = d["x"].shape
    return (B, cin, H, W, d["w"].shape[0], d["ksize"], d["stride"])


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


def _ws(dev, geom):
    return torch.full((max(omlib.load().om_conv2d_bf16_grad_workspace_bytes(*geom), 16),), 255, dtype=torch.uint8, device=dev)


def _dx(dev, d, f32=True, w=None, dy_offset=0, dx_offset=0):
    """dx through the C ABI, pre-filled with NaN.  -> float32 array, or uint16 bits."""
    geom = _geom(d)
    dy = _bf16_dev(dev, d["dy_bits"], dy_offset)
    wt = torch.from_numpy(d["w"] if w is None else w).to(dev)
    dx = _out(dev, d["x"].shape, f32, dx_offset)
    ws = _ws(dev, geom)
    omlib.check(omlib.load().om_conv2d_bf16_grad_input(T.vp(dy), T.vp(wt), *geom, T.vp(dx), 1 if f32 else 0, T.vp(ws), ws.numel(),
                                                       omlib.current_stream_ptr(dev)), "om_conv2d_bf16_grad_input")
    torch.cuda.synchronize(dev)
    return _np_out(dx)


def _dw(dev, d, want_dw=True, want_db=True, x_offset=0, dy_offset=0):
    """(dw, db) through the C ABI, pre-filled with NaN; a gradient that is not wanted is passed as null and returned as it was."""
    geom = _geom(d)
    x, dy = _bf16_dev(dev, d["x_bits"], x_offset), _bf16_dev(dev, d["dy_bits"], dy_offset)
    dw, db = _out(dev, d["w"].shape, True), _out(dev, (d["w"].shape[0],), True)
    ws = _ws(dev, geom)
    omlib.check(omlib.load().om_conv2d_bf16_grad_weight(T.vp(x), T.vp(dy), *geom, T.vp(dw) if want_dw else None,
                                                        T.vp(db) if want_db else None, T.vp(ws), ws.numel(),
                                                        omlib.current_stream_ptr(dev)), "om_conv2d_bf16_grad_weight")
    torch.cuda.synchronize(dev)
    return dw.cpu().numpy(), db.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("case", T.SWEEP + SPECIAL, ids=T.case_id)
def test_exact_on_integer_data(dev, case):
    """x, dy, w in -4 ... 4: every product is an integer of magnitude at most 16, so every partial sum in any order is an integer of
    magnitude at most 16 K < 2^24 and float32 dx, dw, db equal the float64 truth exactly, the bf16 dx its rounding: any dropped,
    doubled or misplaced tap, parity class or split shows."""
    d = C.integer_inputs(*case, seed=sum(case) + 11)
    t = C.truth(d)
    assert 16 * max(C.k_of(d, "dx"), C.k_of(d, "dw")) < 2 ** 24
    assert all(np.array_equal(v.astype(np.float32).astype(np.float64), v) for v in t.values())
    dx = _dx(dev, d, True)
    assert dx.shape == t["dx"].shape and np.isfinite(dx).all(), (case, "an element of dx was not written")
    assert np.array_equal(dx.astype(np.float64), t["dx"]), (case, int((dx != t["dx"]).sum()))
    assert np.array_equal(_dx(dev, d, False), Q.round_bits(t["dx"].astype(np.float32))), case
    dw, db = _dw(dev, d)
    assert np.isfinite(dw).all() and np.isfinite(db).all(), (case, "an element of dw or db was not written")
    assert np.array_equal(dw.astype(np.float64), t["dw"]), (case, int((dw != t["dw"]).sum()))
    assert np.array_equal(db.astype(np.float64), t["db"]), case


# ---------------------------------------------------------------------------------------------------------------- 2. weight rounding
@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("case", [(3, 5, 7, 3, 1, 17, 17), (3, 5, 7, 3, 2, 17, 17), (2, 64, 255, 1, 1, 17, 17)], ids=T.case_id)
def test_weight_is_rounded_to_nearest_even_in_dx(dev, case, kind):
    """dx(dy, w) is bit-equal to dx(dy, quantise(w)): distinguishes round-to-nearest-even from truncation and from round-half-up
    (the ties) on the float32 master weight."""
    d = _reference(case, 61)[0]
    w = d["w"] if kind == "random" else _tie_weights(d["w"].shape)
    wq = Q.quantise(w)
    assert not np.array_equal(w.view(np.uint32), wq.view(np.uint32))
    if kind == "ties":                       # truncation and round-half-up would each give other weights
        trunc = (w.view(np.uint32) & 0xffff0000).view(np.float32)
        half_up = ((w.view(np.uint32).astype(np.uint64) + 0x8000) >> 16 << 16).astype(np.uint32).view(np.float32)
        assert not np.array_equal(trunc, wq) and not np.array_equal(half_up.view(np.uint32), wq.view(np.uint32))
    a, b = _dx(dev, d, True, w=w), _dx(dev, d, True, w=wq)
    assert not np.isnan(a).any() or kind == "ties"
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (case, kind)
    if kind == "ties":                       # and the other two roundings are told apart by the output itself
        for other in (trunc, half_up):
            assert not np.array_equal(_dx(dev, d, True, w=other).view(np.uint32), a.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 3. one rounding
@pytest.mark.parametrize("case", SPECIAL, ids=T.case_id)
def test_bf16_dx_is_the_rounded_float32_dx(dev, case):
    d = _reference(case, sum(case) * 3 + 2)[0]
    dx32, bits = _dx(dev, d, True), _dx(dev, d, False)
    assert np.isfinite(dx32).all() and bool((bits != NAN_BITS).all())
    assert np.array_equal(bits, Q.round_bits(dx32)), case


# ---------------------------------------------------------------------------------------------------------------- 4. accuracy
def _klass(case):
    return "%dx%d s%d" % (case[3], case[3], case[4])


def test_case_list_has_a_multi_split_and_a_single_split_dw(dev):
    L = omlib.load()
    assert MULTI_SPLIT in CASES and SINGLE_SPLIT in CASES
    for case, multi in ((MULTI_SPLIT, True), (SINGLE_SPLIT, False)):
        B, cin, cout, ks, stride, H, W = case
        assert (L.om_conv2d_bf16_grad_workspace_bytes(B, cin, H, W, cout, ks, stride) > 0) == multi, case


@pytest.mark.parametrize("case", CASES, ids=T.case_id)
def test_accuracy_on_random_data(dev, case):
    d, truth, S, ref = _reference(case, sum(case) * 5 + 1)
    dw, db = _dw(dev, d)
    got = dict(dx=_dx(dev, d, True), dw=dw, db=db)
    kl, failed = _klass(case), []
    for which in ("dx", "dw", "db"):
        g, t = got[which], truth[which]
        assert g.shape == t.shape and np.isfinite(g).all(), (case, which, "an element was not written")
        K = C.k_of(d, which)
        unit = K * 2.0 ** -24 * np.maximum(S[which], np.finfo(np.float64).tiny)
        mine, theirs = float((np.abs(g - t) / unit).max()), float((np.abs(ref[which] - t) / unit).max())
        rel, rel_ref = C.G.rel_max(g, t), C.G.rel_max(ref[which], t)
        w = WORST.get((kl, which), (0, 0, 0))
        WORST[(kl, which)] = (max(w[0], mine), max(w[1], theirs), max(w[2], rel / max(rel_ref, 1e-30)))
        print("%-34s %s K %7d  |g-truth| / (K 2^-24 S): hip %.4f torch-cpu-f32 %.4f   rel_max: hip %.3g torch-cpu-f32 %.3g ratio %.2f"
              "   worst of %s so far: %.4f %.4f ratio %.2f" % ((case, which, K, mine, theirs, rel, rel_ref, rel / max(rel_ref, 1e-30), kl)
                                                             + WORST[(kl, which)]))
        if not (np.abs(g - t) <= K * 2.0 ** -23 * S[which]).all():
            failed.append((which, "K 2^-23 S", mine))
        if which != "dx" and not rel <= max(2 * rel_ref, 2e-7):
            failed.append((which, "2 x torch-cpu", rel, rel_ref))
    assert not failed, (case, failed)


# ---------------------------------------------------------------------------------------------------------------- 5. batch
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(5, 16, 32, 3, 1, 3, 5), (3, 5, 7, 3, 1, 17, 17), (5, 32, 64, 3, 2, 8, 8), (4, 64, 32, 1, 1, 17, 17)],
                         ids=T.case_id)
def test_batch_independence_of_dx(dev, case, f32):
    """The batch equals, bit for bit, every image run alone, and the reversed batch reversed back."""
    d = _reference(case, 41)[0]
    sub = lambda sl: dict(d, x=d["x"][sl], dy_bits=np.ascontiguousarray(d["dy_bits"][sl]))      # noqa: E731
    whole = _dx(dev, d, f32)
    assert np.isfinite(whole).all() if f32 else bool((whole != NAN_BITS).all())
    for i in range(case[0]):
        alone = _dx(dev, sub(slice(i, i + 1)), f32)
        assert np.array_equal(_bits(alone[0]), _bits(whole[i])), (case, i)
    back = _dx(dev, sub(slice(None, None, -1)), f32)[::-1]
    assert np.array_equal(_bits(np.ascontiguousarray(back)), _bits(whole)), case


# ---------------------------------------------------------------------------------------------------------------- 6. repeat
def test_two_calls_give_the_same_bits(dev):
    d = _reference(MULTI_SPLIT, 53)[0]
    assert omlib.load().om_conv2d_bf16_grad_workspace_bytes(*_geom(d)) > 0
    a, b = _dw(dev, d), _dw(dev, d)
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    for f32 in (True, False):
        p, q = _dx(dev, d, f32), _dx(dev, d, f32)
        assert np.array_equal(_bits(p), _bits(q))


# ---------------------------------------------------------------------------------------------------------------- 7. neighbours
@pytest.mark.parametrize("case", [(3, 5, 7, 3, 2, 17, 17), (2, 64, 255, 1, 1, 17, 17), MULTI_SPLIT], ids=T.case_id)
def test_neighbours_untouched(dev, case):
    """dx (both types), dw and db are views in the middle of sentinel-filled buffers, and the workspace is handed over with exactly
    the advertised size inside a guarded buffer: the sentinels on both sides are intact after the calls."""
    d, truth, _, _ = _reference(case, 43)
    L, geom, st = omlib.load(), _geom(d), omlib.current_stream_ptr(dev)
    dy, x, w = _bf16_dev(dev, d["dy_bits"]), _bf16_dev(dev, d["x_bits"]), torch.from_numpy(d["w"]).to(dev)
    guard, sentinel = 4099, -12288.0
    need = L.om_conv2d_bf16_grad_workspace_bytes(*geom)
    wsbuf = torch.full((need + 2 * guard,), 0x5a, dtype=torch.uint8, device=dev)
    ws = wsbuf[guard:guard + need]

    def guarded(n, dtype):
        buf = torch.full((n + 2 * guard,), sentinel, device=dev, dtype=dtype)
        view = buf[guard:guard + n]
        view.fill_(float("nan"))
        return buf, view

    bufs = {k: guarded(truth["dx"].size, dt) for k, dt in (("dx32", torch.float32), ("dx16", torch.bfloat16))}
    bufs["dw"], bufs["db"] = guarded(truth["dw"].size, torch.float32), guarded(truth["db"].size, torch.float32)
    for key, f32 in (("dx32", 1), ("dx16", 0)):
        omlib.check(L.om_conv2d_bf16_grad_input(T.vp(dy), T.vp(w), *geom, T.vp(bufs[key][1]), f32, T.vp(ws) if need else None, need, st),
                    "om_conv2d_bf16_grad_input")
    omlib.check(L.om_conv2d_bf16_grad_weight(T.vp(x), T.vp(dy), *geom, T.vp(bufs["dw"][1]), T.vp(bufs["db"][1]),
                                             T.vp(ws) if need else None, need, st), "om_conv2d_bf16_grad_weight")
    torch.cuda.synchronize(dev)
    assert bool((wsbuf[:guard] == 0x5a).all()) and bool((wsbuf[guard + need:] == 0x5a).all())
    for key, (buf, view) in bufs.items():
        assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + view.numel():] == sentinel).all()), key
        t = truth[key[:2]]
        got = view.float().cpu().numpy().reshape(t.shape)
        assert np.isfinite(got).all(), key
        assert np.abs(got - t).max() <= (2.0 ** -8 if key == "dx16" else 1e-5) * np.abs(t).max(), key


# ---------------------------------------------------------------------------------------------------------------- 8. odd offsets
@pytest.mark.parametrize("case", [(3, 5, 7, 3, 2, 17, 17), (1, 3, 32, 3, 2, 33, 31)], ids=T.case_id)
def test_views_at_odd_element_offsets(dev, case):
    """A bf16 tensor is only guaranteed 2-byte alignment: dy, x and a bf16 dx views that start 1, 3 and 5 elements into a buffer give
    the bits of the aligned call."""
    d = _reference(case, 47)[0]
    dx32, bits = _dx(dev, d, True), _dx(dev, d, False)
    dw, db = _dw(dev, d)
    assert np.isfinite(dx32).all() and bool((bits != NAN_BITS).all()) and np.isfinite(dw).all() and np.isfinite(db).all()
    for off in (1, 3, 5):
        assert np.array_equal(_dx(dev, d, True, dy_offset=off).view(np.uint32), dx32.view(np.uint32)), off
        assert np.array_equal(_dx(dev, d, False, dy_offset=off), bits), off
        assert np.array_equal(_dx(dev, d, False, dx_offset=off), bits), off
        for kw in (dict(x_offset=off), dict(dy_offset=off), dict(x_offset=off, dy_offset=6 - off)):
            gw, gb = _dw(dev, d, **kw)
            assert np.array_equal(_bits(gw), _bits(dw)) and np.array_equal(_bits(gb), _bits(db)), (off, kw)
    assert np.array_equal(_dx(dev, d, False, dy_offset=3, dx_offset=5), bits)


# ---------------------------------------------------------------------------------------------------------------- 9. null outputs
@pytest.mark.parametrize("case", [(3, 5, 7, 3, 2, 17, 17), MULTI_SPLIT], ids=T.case_id)
def test_null_outputs(dev, case):
    d = _reference(case, 59)[0]
    dw, db = _dw(dev, d)
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    only_dw, no_db = _dw(dev, d, want_db=False)
    assert np.array_equal(_bits(only_dw), _bits(dw)) and np.isnan(no_db).all()
    no_dw, only_db = _dw(dev, d, want_dw=False)
    assert np.array_equal(_bits(only_db), _bits(db)) and np.isnan(no_dw).all()
    geom = _geom(d)
    x, dy = _bf16_dev(dev, d["x_bits"]), _bf16_dev(dev, d["dy_bits"])
    ws = _ws(dev, geom)
    L = omlib.load()
    assert L.om_conv2d_bf16_grad_weight(T.vp(x), T.vp(dy), *geom, None, None, T.vp(ws), ws.numel(), omlib.current_stream_ptr(dev)) == -1
    assert b"om_conv2d_bf16_grad_weight" in L.om_last_error()


# ---------------------------------------------------------------------------------------------------------------- 10. autograd
@pytest.mark.parametrize("case,bias", [((2, 16, 32, 3, 2, 9, 9), True), ((2, 8, 8, 1, 1, 5, 5), False), ((2, 8, 40, 3, 1, 7, 6), True)],
                         ids=["3x3s2-bias", "1x1", "3x3-bias"])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_autograd_function(dev, case, bias, out_dtype, monkeypatch):
    """conv2d_bf16(..., backward='hip'): dx, dw, db are the C-ABI calls' bits on the bf16-rounded dy, of dtypes bf16, float32,
    float32; a weight that needs no gradient launches no om_conv2d_bf16_grad_weight, an input that needs none no ..._grad_input."""
    B, cin, cout, ks, stride, H, W = case
    d = _reference(case, 71)[0]
    x = _bf16_dev(dev, d["x_bits"]).clone().requires_grad_(True)
    w = torch.from_numpy(d["w"]).to(dev).requires_grad_(True)
    b = torch.zeros(cout, device=dev).requires_grad_(True) if bias else None
    calls = []
    launch = omlib.launch
    monkeypatch.setattr(omlib, "launch", lambda name, *a, **k: (calls.append(name), launch(name, *a, **k))[1])
    y = train.conv2d_bf16(x, w, b, stride, ks // 2, out_dtype=out_dtype, backward="hip")
    assert y.dtype == out_dtype and y.grad_fn is not None
    dy = torch.from_numpy(d["dy"]).to(dev).to(out_dtype)          # bf16 values either way: the rounding in backward is exact
    y.backward(dy)
    torch.cuda.synchronize(dev)
    assert calls == ["om_conv2d_bf16_forward", "om_conv2d_bf16_grad_input", "om_conv2d_bf16_grad_weight"]
    want_dw, want_db = _dw(dev, d)
    assert x.grad.dtype == torch.bfloat16 and w.grad.dtype == torch.float32
    assert np.array_equal(_np_out(x.grad), _dx(dev, d, False))
    assert np.array_equal(_bits(w.grad.cpu().numpy()), _bits(want_dw))
    if bias:
        assert b.grad.dtype == torch.float32 and np.array_equal(_bits(b.grad.cpu().numpy()), _bits(want_db))
    # a weight (and bias) that need no gradient: no weight-gradient launch
    del calls[:]
    x2 = x.detach().clone().requires_grad_(True)
    train.conv2d_bf16(x2, w.detach(), b.detach() if bias else None, stride, ks // 2, out_dtype=out_dtype, backward="hip").backward(dy)
    assert calls == ["om_conv2d_bf16_forward", "om_conv2d_bf16_grad_input"]
    assert np.array_equal(_np_out(x2.grad), _np_out(x.grad))
    # an input that needs no gradient: no input-gradient launch
    del calls[:]
    w2 = w.detach().clone().requires_grad_(True)
    train.conv2d_bf16(x.detach(), w2, None, stride, ks // 2, out_dtype=out_dtype, backward="hip").backward(dy)
    assert calls == ["om_conv2d_bf16_forward", "om_conv2d_bf16_grad_weight"]
    assert np.array_equal(_bits(w2.grad.cpu().numpy()), _bits(want_dw))
