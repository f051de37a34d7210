"""GPU tests of the bf16 entry points of the BatchNorm + LeakyReLU (+ residual) block (om_bn_act_*_bf16, om_bn_sync_*_bf16;
csrc/bn_act.hip) through the C ABI.

The contract is exact (include/orienmask_hip.h): on inputs X that are bf16 values, the bf16 entry point equals the float32 entry
point on the widened X with its float32 activations rounded to bf16 to nearest even, bit for bit; and its float32 and double outputs
(save vectors, running buffers, dgamma, dbeta, SyncBatchNorm records and sums) have the float32 entry point's bits.  So each case
draws its inputs, rounds them to bf16, runs both entry points on the same values and compares bits: the bf16 tensors as int16
against the CPU-side rounding of tests/bf16_np.py (which tests/test_amp_cpu.py holds to torch), everything else as raw words.  The
float32 entry points themselves are judged against float64 in tests/test_bn_act.py and tests/test_bn_sync.py."""
import ctypes

import numpy as np
import pytest
import torch

import bf16_np as Q
import bn_act_np as N
from orienmask_amd import lib as omlib

pytestmark = pytest.mark.gpu

# (B, C, H, W)
SHAPES = [
    (2, 64, 1, 1), (3, 5, 17, 17), (1, 1, 7, 9),        # odd planes: one element per lane
    (2, 3, 2, 2), (2, 5, 6, 6),                         # H*W a multiple of 4 but not of 8
    (2, 3, 4, 4), (2, 32, 8, 8),                        # H*W a multiple of 8
    (2, 1024, 3, 5),                                    # more channels than workgroups per channel
    (2, 4, 96, 96),                                     # above BN_FUSED_MAX: the STATS + APPLY launches
    (2, 64, 17, 17),
]
MISALIGNED = (2, 8, 8, 8)                               # a view one element into a larger buffer: one element per lane
IDS = ["x".join(map(str, s)) for s in SHAPES]
ACT = ("x", "dy", "res")                                # the activation tensors of the inputs
BF16_OUT = ("y", "dx")                                  # outputs whose type follows the entry point
F32_OUT = ("save_mean", "save_invstd", "rm", "rv", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _inputs(shape, seed):
    """float32 arrays; the activations hold bf16 values only."""
    rng = np.random.default_rng(seed)
    C = shape[1]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    d = dict(x=f(rng.standard_normal(shape) * 1.5 + 0.3), dy=f(rng.standard_normal(shape)), res=f(rng.standard_normal(shape)),
             gamma=f(rng.standard_normal(C) * 0.5 + 1.2), beta=f(rng.standard_normal(C) * 0.3), rm=f(rng.standard_normal(C)),
             rv=f(rng.random(C) + 0.5))
    for k in ACT:
        d[k] = Q.quantise(d[k])
    return d


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _act(dev, a, bf16, offset, fill=None):
    """The activation `a` (or a NaN-filled tensor of its shape) on the device in the entry point's type, `offset` elements into its
    buffer."""
    dtype = torch.bfloat16 if bf16 else torch.float32
    buf = torch.full((a.size + offset,), float("nan"), dtype=dtype, device=dev)
    t = buf[offset:].view(a.shape)
    if fill is None:
        t.copy_(torch.from_numpy(a).to(dev))          # bf16 values: the cast is exact
    return t


def _words(t):
    """A device tensor's bits as a numpy integer array."""
    view = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype]
    return t.contiguous().view(view).cpu().numpy()


def _block(dev, d, bf16, training, residual, want_dx, offset=0):
    """The unsynchronised block through the C ABI -> {name: bits}."""
    L = omlib.load()
    sfx = "_bf16" if bf16 else ""
    B, C, H, W = d["x"].shape
    st = omlib.current_stream_ptr(dev)
    x, dy = _act(dev, d["x"], bf16, offset), _act(dev, d["dy"], bf16, offset)
    res = _act(dev, d["res"], bf16, offset) if residual else None
    y = _act(dev, d["x"], bf16, offset, fill="nan")
    dx = _act(dev, d["x"], bf16, offset, fill="nan") if want_dx else None
    p = {k: torch.from_numpy(d[k]).to(dev) for k in ("gamma", "beta", "rm", "rv")}
    sm, si = torch.empty(2 * C, device=dev), torch.empty(2 * C, device=dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    nbt = torch.tensor(7, dtype=torch.long, device=dev)
    ws = torch.full((L.om_bn_act_workspace_bytes(B, C, H, W),), 255, dtype=torch.uint8, device=dev)
    omlib.check(getattr(L, "om_bn_act_forward" + sfx)(
        _vp(x), B, C, H, W, _vp(p["gamma"]), _vp(p["beta"]), _vp(p["rm"]), _vp(p["rv"]), _vp(nbt), int(training), N.MOMENTUM, N.EPS,
        N.SLOPE, _vp(res), _vp(y), _vp(sm), _vp(si), _vp(ws), ws.numel(), st), "om_bn_act_forward" + sfx)
    ws.fill_(255)
    omlib.check(getattr(L, "om_bn_act_backward" + sfx)(
        _vp(x), _vp(dy), B, C, H, W, _vp(p["gamma"]), _vp(p["beta"]), _vp(sm), _vp(si), int(training), N.SLOPE, _vp(dx), _vp(dg),
        _vp(db), _vp(ws), ws.numel(), st), "om_bn_act_backward" + sfx)
    torch.cuda.synchronize(dev)
    out = dict(y=y, save_mean=sm, save_invstd=si, rm=p["rm"], rv=p["rv"], dgamma=dg, dbeta=db, nbt=nbt)
    if want_dx:
        out["dx"] = dx
    return out


def _same_as_rounded(got, ref, what):
    """got: a bf16 device tensor, ref: the float32 entry point's tensor -> got's bits are the rounding of ref's."""
    assert got.dtype == torch.bfloat16 and ref.dtype == torch.float32
    want = Q.round_bits(ref.cpu().numpy())
    have = _words(got).view(np.uint16)
    bad = int((have != want).sum())
    assert bad == 0, (what, "%d of %d elements differ from the rounded float32 result" % (bad, want.size))


def _compare(got, ref, what):
    for k in BF16_OUT:
        if k in ref:
            _same_as_rounded(got[k], ref[k], what + (k,))
        else:
            assert k not in got
    for k in F32_OUT:
        assert got[k].dtype == ref[k].dtype == torch.float32
        assert np.array_equal(_words(got[k]), _words(ref[k])), what + (k,)
    assert int(got["nbt"]) == int(ref["nbt"]) == (8 if what[1] == "train" else 7), what


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bf16_block_is_the_rounded_float32_block(dev, shape, training, residual):
    d = _inputs(shape, 1000 + sum(shape) + 2 * training + residual)
    for want_dx in (True, False):
        what = (shape, "train" if training else "eval", "res" if residual else "nores", "dx" if want_dx else "nodx")
        ref = _block(dev, d, False, training, residual, want_dx)
        got = _block(dev, d, True, training, residual, want_dx)
        assert torch.isfinite(ref["y"]).all() and (not want_dx or torch.isfinite(ref["dx"]).all()), what
        _compare(got, ref, what)
        if want_dx:
            again = _block(dev, d, True, training, residual, want_dx)
            for k in BF16_OUT + F32_OUT:
                assert np.array_equal(_words(again[k]), _words(got[k])), what + (k, "rerun")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_a_misaligned_view_takes_the_single_element_path(dev, training):
    """Every activation starts one element into its buffer: 2 bytes off in bf16, 4 in float32, so neither entry point may use its
    unit loads.  The values equal the aligned call's, and nothing outside the view is written."""
    d = _inputs(MISALIGNED, 77 + training)
    what = (MISALIGNED, "train" if training else "eval", "res", "dx", "offset 1")
    ref = _block(dev, d, False, training, True, True, offset=1)
    got = _block(dev, d, True, training, True, True, offset=1)
    assert got["y"].data_ptr() % 4 == 2 and ref["y"].data_ptr() % 16 == 4
    _compare(got, ref, what)
    aligned = _block(dev, d, True, training, True, True)
    for k in BF16_OUT:
        assert np.array_equal(_words(got[k]), _words(aligned[k])), what + (k, "against the aligned call")
        # the element in front of the view keeps its NaN fill
        assert got[k].storage_offset() == 1
        front = got[k].as_strided((1,), (1,), 0)
        assert torch.isnan(front).all(), what + (k, "the element in front of the view")


def test_mixed_alignment_falls_back_as_a_whole(dev):
    """x aligned, the residual one element in: the call as a whole takes the single-element path and still gives the rounded bits."""
    L = omlib.load()
    shape = (2, 8, 8, 8)
    d = _inputs(shape, 5)
    B, C, H, W = shape
    st = omlib.current_stream_ptr(dev)
    outs = []
    for bf16 in (False, True):
        sfx = "_bf16" if bf16 else ""
        x, res, y = _act(dev, d["x"], bf16, 0), _act(dev, d["res"], bf16, 1), _act(dev, d["x"], bf16, 0, fill="nan")
        p = {k: torch.from_numpy(d[k]).to(dev) for k in ("gamma", "beta", "rm", "rv")}
        sm, si = torch.empty(2 * C, device=dev), torch.empty(2 * C, device=dev)
        ws = torch.empty(L.om_bn_act_workspace_bytes(B, C, H, W), dtype=torch.uint8, device=dev)
        omlib.check(getattr(L, "om_bn_act_forward" + sfx)(
            _vp(x), B, C, H, W, _vp(p["gamma"]), _vp(p["beta"]), _vp(p["rm"]), _vp(p["rv"]), None, 1, N.MOMENTUM, N.EPS, N.SLOPE,
            _vp(res), _vp(y), _vp(sm), _vp(si), _vp(ws), ws.numel(), st), "om_bn_act_forward" + sfx)
        torch.cuda.synchronize(dev)
        outs.append((y, sm, si))
    _same_as_rounded(outs[1][0], outs[0][0], (shape, "mixed alignment", "y"))
    assert np.array_equal(_words(outs[1][1]), _words(outs[0][1])) and np.array_equal(_words(outs[1][2]), _words(outs[0][2]))


# ---------------------------------------------------------------------------------------------------------------- several ranks
def _sync(dev, d, cuts, bf16, residual):
    """The four staged calls over the ranks `cuts` of the batch d, in one process -> per-rank {name: tensor}, and the gathered
    records and sums."""
    L = omlib.load()
    sfx = "_bf16" if bf16 else ""
    R = len(cuts)
    C, H, W = d["x"].shape[1:]
    st = omlib.current_stream_ptr(dev)
    edges = np.cumsum([0] + list(cuts))
    part = lambda k, r: np.ascontiguousarray(d[k][edges[r]:edges[r + 1]])      # noqa: E731
    xs = [_act(dev, part("x", r), bf16, 0) for r in range(R)]
    dys = [_act(dev, part("dy", r), bf16, 0) for r in range(R)]
    ress = [_act(dev, part("res", r), bf16, 0) if residual else None for r in range(R)]
    gamma, beta = torch.from_numpy(d["gamma"]).to(dev), torch.from_numpy(d["beta"]).to(dev)
    wss = [torch.full((L.om_bn_act_workspace_bytes(B, C, H, W),), 255, dtype=torch.uint8, device=dev) for B in cuts]
    records = torch.full((R, 3, C), float("nan"), dtype=torch.float64, device=dev)
    for r, B in enumerate(cuts):
        omlib.check(getattr(L, "om_bn_sync_stats" + sfx)(_vp(xs[r]), B, C, H, W, _vp(records[r]), _vp(wss[r]), wss[r].numel(), st),
                    "om_bn_sync_stats" + sfx)
    out = []
    for r, B in enumerate(cuts):
        rm, rv = torch.from_numpy(d["rm"]).to(dev), torch.from_numpy(d["rv"]).to(dev)
        nbt = torch.tensor(7, dtype=torch.long, device=dev)
        y = _act(dev, part("x", r), bf16, 0, fill="nan")
        sm, si = torch.empty(2 * C, device=dev), torch.empty(2 * C, device=dev)
        nt = torch.zeros(1, dtype=torch.float64, device=dev)
        omlib.check(getattr(L, "om_bn_sync_forward" + sfx)(
            _vp(xs[r]), B, C, H, W, _vp(records), R, _vp(gamma), _vp(beta), _vp(rm), _vp(rv), _vp(nbt), N.MOMENTUM, N.EPS, N.SLOPE,
            _vp(ress[r]), _vp(y), _vp(sm), _vp(si), _vp(nt), st), "om_bn_sync_forward" + sfx)
        out.append(dict(y=y, save_mean=sm, save_invstd=si, rm=rm, rv=rv, nbt=nbt, nt=nt))
    sums_all = torch.full((R, 2, C), float("nan"), dtype=torch.float64, device=dev)
    for r, B in enumerate(cuts):
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        wss[r].fill_(255)
        omlib.check(getattr(L, "om_bn_sync_backward_sums" + sfx)(
            _vp(xs[r]), _vp(dys[r]), B, C, H, W, _vp(gamma), _vp(beta), _vp(out[r]["save_mean"]), _vp(out[r]["save_invstd"]), N.SLOPE,
            _vp(sums_all[r]), _vp(dg), _vp(db), _vp(wss[r]), wss[r].numel(), st), "om_bn_sync_backward_sums" + sfx)
        out[r].update(dgamma=dg, dbeta=db)
    for r, B in enumerate(cuts):
        dx = _act(dev, part("x", r), bf16, 0, fill="nan")
        omlib.check(getattr(L, "om_bn_sync_backward_dx" + sfx)(
            _vp(xs[r]), _vp(dys[r]), B, C, H, W, _vp(gamma), _vp(beta), _vp(out[r]["save_mean"]), _vp(out[r]["save_invstd"]), N.SLOPE,
            _vp(sums_all), R, _vp(out[r]["nt"]), _vp(dx), st), "om_bn_sync_backward_dx" + sfx)
        out[r]["dx"] = dx
    torch.cuda.synchronize(dev)
    return out, records, sums_all


SYNC_CASES = [([2], (64, 17, 17)), ([2], (32, 8, 8)), ([2], (4, 96, 96)), ([1, 1], (64, 17, 17)), ([2, 2], (6, 6, 6)),
              ([2, 2], (4, 96, 96)), ([1, 2], (5, 7, 9))]


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("cuts,chw", SYNC_CASES, ids=["%s_%s" % ("-".join(map(str, c)), "x".join(map(str, s))) for c, s in SYNC_CASES])
def test_bf16_sync_phases_are_the_rounded_float32_phases(dev, cuts, chw, residual):
    """R = 1, and R = 2 from the records of two parts of one batch: every phase's bf16 tensors are the float32 phase's, rounded; the
    records, sums, save vectors, running buffers, dgamma and dbeta have its bits."""
    shape = (sum(cuts),) + chw
    d = _inputs(shape, 2000 + sum(shape) + len(cuts) + residual)
    ref, ref_records, ref_sums = _sync(dev, d, cuts, False, residual)
    got, records, sums = _sync(dev, d, cuts, True, residual)
    what = (shape, "train", "ranks %s" % cuts, "res" if residual else "nores")
    assert np.array_equal(_words(records), _words(ref_records)), what + ("records",)
    assert np.array_equal(_words(sums), _words(ref_sums)), what + ("sums",)
    for r in range(len(cuts)):
        _compare(got[r], ref[r], what + ("rank %d" % r,))
        assert np.array_equal(_words(got[r]["nt"]), _words(ref[r]["nt"])) and float(got[r]["nt"]) == float(np.prod(shape)) / shape[1]
    if len(cuts) == 1:
        # one rank: the staged calls have the unsynchronised block's bits, in bf16 as in float32
        plain = _block(dev, d, True, True, residual, True)
        for k in BF16_OUT + F32_OUT:
            assert np.array_equal(_words(got[0][k]), _words(plain[k])), what + (k, "against om_bn_act_*_bf16")
