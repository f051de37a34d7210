"""GPU tests of the synchronised BatchNorm + LeakyReLU block (om_bn_sync_stats / _forward / _backward_sums / _backward_dx of
csrc/bn_act.hip), of train.convert_sync_batchnorm and of builder.build_train_model(is_distributed=True).

One device: through the C ABI.  A "rank" is a slice of one batch along its first axis; the ranks are processed one after the other
and the test concatenates their records (and backward sums) in place of the all-gather.  Truth and yardstick are those of
tests/test_bn_act.py, whose helpers are used as they are: float64 on the float32 inputs of the CONCATENATED batch, and torch's own
float32 batch_norm + leaky_relu on the CPU on that batch -- the kernels' error may be at most twice torch's, floor 1e-7, with that
file's sign-flip band and share.  The rank sum of the float32 dgamma / dbeta is held to the same bar (adding R float32 roundings of
parts that are no larger than the whole keeps the sum within R * 2^-25 of scale, below the floor for the R used here).

Two devices: two fresh child processes of tests/bn_sync_worker.py with the nccl backend, one device each; skipped with a reason where
fewer than two devices are visible."""
import ctypes
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import bn_act_np as N
import bn_sync_np as S
import test_bn_act as T
from orienmask_amd import lib as omlib

pytestmark = pytest.mark.gpu

# per-rank batch sizes, (C, H, W)
SHAPES = [
    ([2, 2], (64, 17, 17)),        # V = 1, one workgroup per channel
    ([1, 2, 2], (5, 17, 17)),      # unequal counts, odd C
    ([2, 2], (32, 8, 8)),          # V = 4
    ([2, 2], (4, 96, 96)),         # 18432 elements per channel and rank: per-workgroup partials in the workspace
    ([1, 1], (8, 1, 1)),           # one value per channel and rank, N = 2
    ([1] * 8, (16, 4, 4)),         # R = 8
]
IDS = ["%s_%s" % ("-".join(map(str, c)), "x".join(map(str, s))) for c, s in SHAPES]


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _vp(a):
    return ctypes.c_void_p(a.data_ptr()) if a is not None else None


def _sync(dev, d, cuts, residual, want_dx=True):
    """The staged block over the ranks `cuts` of the batch d.  -> list of per-rank dicts of numpy arrays: y0 (no residual), y, save_mean
    and save_invstd (2C floats each: value | remainder), rm, rv, nbt, n_total, dx, dgamma, dbeta."""
    L = omlib.load()
    R = len(cuts)
    C, H, W = d["x"].shape[1:]
    st = omlib.current_stream_ptr(dev)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    gamma, beta = dv(d["gamma"]), dv(d["beta"])
    xs = [dv(a) for a in S.split(d["x"], cuts)]
    dys = [dv(a) for a in S.split(d["dy"], cuts)]
    ress = [dv(a) for a in S.split(d["res"], cuts)] if residual else [None] * R
    wss = []
    for B in cuts:
        nbytes = L.om_bn_act_workspace_bytes(B, C, H, W)
        assert nbytes > 0
        wss.append(torch.full((nbytes,), 255, dtype=torch.uint8, device=dev))
    records = torch.full((R, 3, C), float("nan"), dtype=torch.float64, device=dev)
    for r, B in enumerate(cuts):
        omlib.check(L.om_bn_sync_stats(_vp(xs[r]), B, C, H, W, _vp(records[r]), _vp(wss[r]), wss[r].numel(), st), "om_bn_sync_stats")
    out = []
    for r, B in enumerate(cuts):
        o = {}
        nbt = torch.tensor(7, dtype=torch.long, device=dev)
        for key, res in (("y0", None), ("y", ress[r])):
            rm, rv = dv(d["rm"]), dv(d["rv"])
            y = torch.full_like(xs[r], float("nan"))
            sm, si = torch.empty(2 * C, device=dev), torch.empty(2 * C, device=dev)
            nt = torch.zeros(1, dtype=torch.float64, device=dev)
            omlib.check(L.om_bn_sync_forward(_vp(xs[r]), B, C, H, W, _vp(records), R, _vp(gamma), _vp(beta), _vp(rm), _vp(rv), _vp(nbt),
                                             N.MOMENTUM, N.EPS, N.SLOPE, _vp(res), _vp(y), _vp(sm), _vp(si), _vp(nt), st),
                        "om_bn_sync_forward")
            o[key] = y.cpu().numpy()
        o.update(sm=sm, si=si, nt=nt, save_mean=sm.cpu().numpy(), save_invstd=si.cpu().numpy(), rm=rm.cpu().numpy(), rv=rv.cpu().numpy(),
                 nbt=int(nbt), n_total=float(nt))
        out.append(o)
    sums_all = torch.full((R, 2, C), float("nan"), dtype=torch.float64, device=dev)
    dgs = []
    for r, B in enumerate(cuts):
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        wss[r].fill_(255)
        omlib.check(L.om_bn_sync_backward_sums(_vp(xs[r]), _vp(dys[r]), B, C, H, W, _vp(gamma), _vp(beta), _vp(out[r]["sm"]), _vp(out[r]["si"]),
                                               N.SLOPE, _vp(sums_all[r]), _vp(dg), _vp(db), _vp(wss[r]), wss[r].numel(), st),
                    "om_bn_sync_backward_sums")
        dgs.append((dg, db))
    for r, B in enumerate(cuts):
        dx = None
        if want_dx:
            dx = torch.full_like(xs[r], float("nan"))
            omlib.check(L.om_bn_sync_backward_dx(_vp(xs[r]), _vp(dys[r]), B, C, H, W, _vp(gamma), _vp(beta), _vp(out[r]["sm"]),
                                                 _vp(out[r]["si"]), N.SLOPE, _vp(sums_all), R, _vp(out[r]["nt"]), _vp(dx), st),
                        "om_bn_sync_backward_dx")
        out[r].update(dx=dx.cpu().numpy() if want_dx else None, dgamma=dgs[r][0].cpu().numpy(), dbeta=dgs[r][1].cpu().numpy())
    torch.cuda.synchronize(dev)
    for o in out:
        del o["sm"], o["si"], o["nt"]
    return out


def _whole(ranks, C):
    """The ranks' outputs as one batch, in the form tests/test_bn_act.py judges: rank 0's statistics and buffers, the rank sum of
    dgamma / dbeta (float64 sum of the float32 values)."""
    r0 = ranks[0]
    cat = lambda k: np.concatenate([o[k] for o in ranks])      # noqa: E731
    return dict(y=cat("y"), y0=cat("y0"), save_mean=r0["save_mean"][:C], save_invstd=r0["save_invstd"][:C], rm=r0["rm"], rv=r0["rv"],
                dx=cat("dx") if r0["dx"] is not None else None,
                dgamma=np.sum([o["dgamma"].astype(np.float64) for o in ranks], axis=0),
                dbeta=np.sum([o["dbeta"].astype(np.float64) for o in ranks], axis=0))


def _judge(dev, cuts, chw, seed, residual, want_dx, mean=0.0, std=1.0):
    shape = (sum(cuts),) + chw
    d = T._inputs(shape, seed, mean, std, residual)
    ranks = _sync(dev, d, cuts, residual, want_dx)
    got = _whole(ranks, chw[0])
    ref = T._torch_cpu(d, True, residual)
    truth = N.forward(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], True, d["res"] if residual else None)
    what = (tuple(cuts), chw, "res" if residual else "nores", "dx" if want_dx else "nodx")
    flips = T._check_mask(got, d, truth, what)
    mine, theirs = T._errors(got, d, True, residual, truth), T._errors(ref, d, True, residual, truth)
    if want_dx:
        # every rank's dx on its own, against that slice of the float64 gradient
        dx64 = N.backward(d["x"], d["dy"], d["gamma"], truth["mean"], truth["invstd"], got["y0"] > 0, True)[0]
        rdx64 = N.backward(d["x"], d["dy"], d["gamma"], truth["mean"], truth["invstd"], ref["y0"] > 0, True)[0]
        for r, (mine_r, want_r, ref_r, refwant_r) in enumerate(zip(S.split(got["dx"], cuts), S.split(dx64, cuts), S.split(ref["dx"], cuts),
                                                                   S.split(rdx64, cuts))):
            mine["dx_rank%d" % r], theirs["dx_rank%d" % r] = N.rel_max(mine_r, want_r), N.rel_max(ref_r, refwant_r)
    else:
        assert all(o["dx"] is None for o in ranks)
    for o in ranks:
        assert o["nbt"] == 9, what                                 # two forward calls on every rank
        assert o["n_total"] == shape[0] * chw[1] * chw[2], what
    for k, e in mine.items():
        print("%-52s %-12s hip %.3g  torch-cpu %.3g  ratio %.2f  flips %d" % (what, k, e, theirs[k], e / max(theirs[k], 1e-30), flips))
        assert e <= max(2 * theirs[k], T.FLOOR), (what, k, e, theirs[k])
    return ranks


# ---------------------------------------------------------------------------------------------------------------- one device
@pytest.mark.parametrize("cuts,chw", SHAPES, ids=IDS)
def test_ranks_of_one_batch_against_float64(dev, cuts, chw):
    """Every shape with and without residual, with and without dx, on N(0,1) and N(3,2) inputs; and (test 3) the save vectors, value
    and remainder, and the running buffers are byte-equal on every rank."""
    seed = sum(cuts) * 11 + sum(chw) * 7
    runs = [_judge(dev, cuts, chw, seed, True, True),
            _judge(dev, cuts, chw, seed + 1, False, False, mean=3.0, std=2.0),
            _judge(dev, cuts, chw, seed + 2, True, False, mean=3.0, std=2.0),
            _judge(dev, cuts, chw, seed + 3, False, True)]
    for ranks in runs:
        for o in ranks[1:]:
            for k in ("save_mean", "save_invstd", "rm", "rv"):
                assert np.array_equal(o[k].view(np.uint32), ranks[0][k].view(np.uint32)), (k, cuts, chw)


def _plain(dev, d, residual):
    """om_bn_act_forward / om_bn_act_backward on the batch, with the whole save vectors."""
    L = omlib.load()
    t = {k: (torch.from_numpy(v).to(dev) if v is not None else None) for k, v in d.items()}
    B, C, H, W = d["x"].shape
    ws = torch.full((L.om_bn_act_workspace_bytes(B, C, H, W),), 255, dtype=torch.uint8, device=dev)
    st = omlib.current_stream_ptr(dev)
    rm, rv = t["rm"].clone(), t["rv"].clone()
    y, dx = torch.empty_like(t["x"]), torch.empty_like(t["x"])
    sm, si, dg, db = torch.empty(2 * C, device=dev), torch.empty(2 * C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
    omlib.check(L.om_bn_act_forward(_vp(t["x"]), B, C, H, W, _vp(t["gamma"]), _vp(t["beta"]), _vp(rm), _vp(rv), None, 1, N.MOMENTUM, N.EPS,
                                    N.SLOPE, _vp(t["res"]) if residual else None, _vp(y), _vp(sm), _vp(si), _vp(ws), ws.numel(), st),
                "om_bn_act_forward")
    omlib.check(L.om_bn_act_backward(_vp(t["x"]), _vp(t["dy"]), B, C, H, W, _vp(t["gamma"]), _vp(t["beta"]), _vp(sm), _vp(si), 1, N.SLOPE,
                                     _vp(dx), _vp(dg), _vp(db), _vp(ws), ws.numel(), st), "om_bn_act_backward")
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in dict(y=y, save_mean=sm, save_invstd=si, rm=rm, rv=rv, dx=dx, dgamma=dg, dbeta=db).items()}


BITS = ("y", "save_mean", "save_invstd", "rm", "rv", "dx", "dgamma", "dbeta")


@pytest.mark.parametrize("shape", [(2, 64, 17, 17), (2, 32, 8, 8), (2, 4, 96, 96)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("residual", [False, True])
def test_one_rank_equals_the_unsynchronised_block_bit_for_bit(dev, shape, residual):
    d = T._inputs(shape, 21 + sum(shape), mean=1.5, std=2.0, residual=residual)
    want = _plain(dev, d, residual)
    got = _sync(dev, d, [shape[0]], residual)[0]
    for k in BITS:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


def test_ranks_that_see_different_data(dev):
    """Rank 0 from N(1000,1), rank 1 from N(-1000,1): the batch variance is 10^6, every rank's own is 1.  The statistics and the
    running buffers are held to the 2x bar; averaging per-rank variances, or E[x^2] - E[x]^2 in float32, misses by orders."""
    cuts, chw = [2, 2], (8, 17, 17)
    d = T._inputs((4,) + chw, 31, residual=False)
    rng = np.random.default_rng(32)
    d["x"] = np.concatenate([rng.standard_normal((2,) + chw) + 1000.0, rng.standard_normal((2,) + chw) - 1000.0]).astype(np.float32)
    ranks = _sync(dev, d, cuts, False)
    got = _whole(ranks, chw[0])
    ref = T._torch_cpu(d, True, False)
    truth = N.forward(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], True)
    mine, theirs = T._errors(got, d, True, False, truth, skip_grads=True), T._errors(ref, d, True, False, truth, skip_grads=True)
    assert abs(truth["invstd"] - 1e-3).max() < 1e-5
    for k in ("save_mean", "save_invstd", "running_mean", "running_var"):
        print("different data %-12s hip %.3g  torch-cpu %.3g" % (k, mine[k], theirs[k]))
        assert mine[k] <= max(2 * theirs[k], T.FLOOR), (k, mine[k], theirs[k])
    for k in ("save_mean", "save_invstd", "rm", "rv"):
        assert np.array_equal(ranks[0][k].view(np.uint32), ranks[1][k].view(np.uint32)), k


@pytest.mark.parametrize("cuts,chw", [([2, 2], (64, 17, 17)), ([2, 2], (4, 96, 96)), ([1, 2, 2], (5, 17, 17))],
                         ids=["2-2_64x17x17", "2-2_4x96x96", "1-2-2_5x17x17"])
def test_rerun_and_another_stream_give_the_same_bits(dev, cuts, chw):
    d = T._inputs((sum(cuts),) + chw, 9)
    a, b = _sync(dev, d, cuts, True), _sync(dev, d, cuts, True)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        c = _sync(dev, d, cuts, True)
    for other in (b, c):
        for ra, ro in zip(a, other):
            for k in BITS:
                assert np.array_equal(ra[k].view(np.uint32), ro[k].view(np.uint32)), k


def test_refusals_on_the_device(dev):
    L = omlib.load()
    c = torch.ones(64, device=dev)
    rec = torch.zeros(3 * 8 * 2, dtype=torch.float64, device=dev)
    one = torch.ones(1, dtype=torch.float64, device=dev)
    x1 = torch.rand(1, 8, 1, 1, device=dev)
    y1 = torch.empty_like(x1)
    # N < 2: one rank with one value per channel (with a second rank the same call is test 1's [1,1] x (8,1,1))
    rc = L.om_bn_sync_forward(_vp(x1), 1, 8, 1, 1, _vp(rec), 1, _vp(c), _vp(c), None, None, None, 0.1, 1e-5, 0.1, None, _vp(y1), _vp(c), _vp(c),
                              _vp(one), None)
    assert rc != 0 and b"more than 1 value per channel" in L.om_last_error()
    x = torch.rand(2, 8, 4, 4, device=dev)
    y = torch.empty_like(x)
    for R in (0, -1):
        rc = L.om_bn_sync_forward(_vp(x), 2, 8, 4, 4, _vp(rec), R, _vp(c), _vp(c), None, None, None, 0.1, 1e-5, 0.1, None, _vp(y), _vp(c),
                                  _vp(c), _vp(one), None)
        assert rc != 0 and b"ranks" in L.om_last_error()
        rc = L.om_bn_sync_backward_dx(_vp(x), _vp(x), 2, 8, 4, 4, _vp(c), _vp(c), _vp(c), _vp(c), 0.1, _vp(rec), R, _vp(one), _vp(y), None)
        assert rc != 0 and b"ranks" in L.om_last_error()
    big = (2, 32, 272, 272)
    xb = torch.rand(big, device=dev)
    need = L.om_bn_act_workspace_bytes(*big)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    recb = torch.zeros(3 * 32, dtype=torch.float64, device=dev)
    for wsp, nbytes in ((None, 0), (ws.data_ptr(), 16), (ws.data_ptr() + 8, need)):          # none, too small, misaligned
        rc = L.om_bn_sync_stats(_vp(xb), *big, _vp(recb), wsp, nbytes, None)
        assert rc != 0 and b"workspace" in L.om_last_error()
        rc = L.om_bn_sync_backward_sums(_vp(xb), _vp(xb), *big, _vp(c), _vp(c), _vp(c), _vp(c), 0.1, _vp(recb), _vp(c), _vp(c), wsp, nbytes, None)
        assert rc != 0 and b"workspace" in L.om_last_error()
    torch.cuda.synchronize(dev)


# ---------------------------------------------------------------------------------------------------------------- two devices
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 120


def _two_ranks(task, tmp_path):
    """Two fresh child processes of tests/bn_sync_worker.py, one device each, each with CHILD_TIMEOUT seconds.  If one fails or times
    out the other is terminated and the test fails; nothing is retried.  -> the two .npz files the children wrote."""
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs two MI355X devices, %d visible" % (torch.cuda.device_count() if torch.cuda.is_available() else 0))
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    children, logs = [], []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        logs.append(open(os.path.join(str(tmp_path), "%s_rank%d.log" % (task, rank)), "w+"))
        children.append(subprocess.Popen([sys.executable, os.path.join(HERE, "bn_sync_worker.py"), task, str(tmp_path)], env=env,
                                         stdout=logs[-1], stderr=subprocess.STDOUT))
    failed, running, deadline = None, list(range(2)), time.monotonic() + CHILD_TIMEOUT
    while running and failed is None:
        for rank in list(running):
            try:
                rc = children[rank].wait(timeout=0.25)             # returns as soon as this child ends
            except subprocess.TimeoutExpired:
                continue
            running.remove(rank)
            if rc != 0:
                failed = "rank %d exited with %s" % (rank, rc)
        if running and failed is None and time.monotonic() > deadline:
            failed = "rank(s) %s did not finish within %d s" % (running, CHILD_TIMEOUT)
    for rank in running:                                           # the other rank waits in a collective that will not complete
        children[rank].terminate()
        try:
            children[rank].wait(timeout=10)
        except subprocess.TimeoutExpired:
            children[rank].kill()
            children[rank].wait()
    outputs = []
    for f in logs:
        f.seek(0)
        outputs.append(f.read()[-3000:])
        f.close()
    assert failed is None, (failed, outputs)
    return [np.load(os.path.join(str(tmp_path), "%s_rank%d.npz" % (task, r))) for r in range(2)]


def test_two_ranks_block_against_torch_sync_batchnorm(dev, tmp_path):
    """A converted ConvBNLeaky(16, 32, 3), 2 images per rank at 12 x 12, beside nn.Sequential(conv, SyncBatchNorm, LeakyReLU) with the
    same weights in the same children.  Output and every gradient against the float64 truth of the concatenated batch: the hip error
    at most twice torch's; running buffers byte-equal on the two ranks; no collective in eval()."""
    import torch.nn.functional as F
    g = _two_ranks("block", tmp_path)
    x = np.concatenate([g[0]["x"], g[1]["x"]]).astype(np.float64)
    gy = np.concatenate([g[0]["gy"], g[1]["gy"]]).astype(np.float64)
    tw, tg, tb = (torch.tensor(g[0][k].astype(np.float64), requires_grad=True) for k in ("weight", "gamma", "beta"))
    tx = torch.tensor(x, requires_grad=True)
    rm, rv = torch.tensor(g[0]["rm0"].astype(np.float64)), torch.tensor(g[0]["rv0"].astype(np.float64))
    ty = F.leaky_relu(F.batch_norm(F.conv2d(tx, tw, None, 1, 1), rm, rv, tg, tb, True, N.MOMENTUM, N.EPS), N.SLOPE)
    ty.backward(torch.tensor(gy))
    want = dict(y=ty.detach().numpy(), dx=tx.grad.numpy(), rm=rm.numpy(), rv=rv.numpy())
    # the parameters' gradients stay local on each rank: their rank sum is the whole batch's
    want_params = dict(dweight=tw.grad.numpy(), dgamma=tg.grad.numpy(), dbeta=tb.grad.numpy())
    for side in ("hip", "torch"):
        for k in ("rm", "rv"):
            assert np.array_equal(g[0]["%s_%s" % (side, k)].view(np.uint32), g[1]["%s_%s" % (side, k)].view(np.uint32)), (side, k)
        assert int(g[0][side + "_nbt"]) == int(g[1][side + "_nbt"]) == 1
    err = {}
    for side in ("hip", "torch"):
        e = {k: N.rel_max(np.concatenate([g[0]["%s_%s" % (side, k)], g[1]["%s_%s" % (side, k)]]), want[k]) for k in ("y", "dx")}
        e.update({k: N.rel_max(g[0]["%s_%s" % (side, k)], want[k]) for k in ("rm", "rv")})
        e.update({k: N.rel_max(g[0]["%s_%s" % (side, k)].astype(np.float64) + g[1]["%s_%s" % (side, k)], w) for k, w in want_params.items()})
        err[side] = e
    for k, e in err["hip"].items():
        print("block %-8s hip %.3g  torch SyncBatchNorm %.3g" % (k, e, err["torch"][k]))
        assert e <= max(2 * err["torch"][k], T.FLOOR), (k, e, err["torch"][k])
    for r in range(2):
        assert int(g[r]["train_gathers"]) == 2 and int(g[r]["eval_gathers"]) == 0
        assert int(g[r]["nograd_gathers"]) == 1           # an input without gradient: the backward's all-gather is skipped


def test_two_ranks_model_against_the_single_process_model(dev, tmp_path):
    """build_train_model(cfg, is_distributed=True) at 96 x 96, 2 images per rank, against the single-process 'hip' model on the
    4-image batch: heads within 1e-4 of scale; every gradient identical on both ranks; DistributedDataParallel's averaged gradient
    times 2 within twice the 'torch'-against-'hip' error of the single-process batch (relative L2 per tensor, root mean square over
    the tensors: both are float32 reorderings of one computation); after one SGD step the two state_dicts are byte-equal."""
    from orienmask_amd import synth, train
    g = _two_ranks("model", tmp_path)
    names = [str(k) for k in g[0]["param_names"]]
    assert g[0]["grad_digest"].tolist() == g[1]["grad_digest"].tolist()          # sha256 of every gradient's bytes
    assert g[0]["state_keys"].tolist() == g[1]["state_keys"].tolist() and g[0]["state_digest"].tolist() == g[1]["state_digest"].tolist()
    assert all(np.array_equal(g[r]["nbt"], g[r]["nbt_before"] + 1) and len(g[r]["nbt"]) == 86 for r in range(2))
    # the single-process models on the whole batch, here
    sd = synth.synth_state_dict(int(g[0]["sd_seed"]))
    x = torch.from_numpy(np.concatenate([g[0]["x"], g[1]["x"]])).to(dev)
    cot = [torch.from_numpy(np.concatenate([g[0]["cot%d" % i], g[1]["cot%d" % i]])).to(dev) for i in range(6)]
    grads, heads = {}, {}
    for backend in ("hip", "torch"):
        net = train.OrienMaskYOLOFPNPlus(3, 80, backend=backend)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).train()
        heads[backend] = [t.detach().cpu().numpy() for t in T._step(net, x, cot)]
        grads[backend] = {n: p.grad.cpu().numpy() for n, p in net.named_parameters()}
        del net
    for i, k in enumerate(N.HEAD_KEYS):
        got = np.concatenate([g[0]["head%d" % i], g[1]["head%d" % i]])
        assert np.abs(got - heads["hip"][i]).max() <= 1e-4 * np.abs(heads["hip"][i]).max(), k
    assert names == list(grads["hip"])
    ddp = [N.rel_l2(2.0 * g[0]["grad." + n].astype(np.float64), grads["hip"][n]) for n in names]
    yard = [N.rel_l2(grads["torch"][n], grads["hip"][n]) for n in names]
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))      # noqa: E731
    print("gradient error, rms over %d tensors: 2 x DDP against single-process hip %.3g; torch against hip %.3g" % (len(names), rms(ddp), rms(yard)))
    assert rms(ddp) <= 2 * rms(yard)
