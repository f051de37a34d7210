"""GPU tests of the BatchNorm + LeakyReLU (+ residual) block (om_bn_act_forward / om_bn_act_backward, csrc/bn_act.hip) through the C ABI
and through orienmask_amd.train.ConvBNLeaky, and of the training model built on it.

Truth is tests/bn_act_np.py: float64 arithmetic on the float32 inputs.  The yardstick for an error is torch's OWN float32
batch_norm + leaky_relu on the CPU on the same input: both are float32 evaluations that differ in summation order and rounding
points, so the kernel's maximum error over the tensor's scale may be at most TWICE torch's, with a floor of 1e-7 (a wrong formula is
off by orders of magnitude).  Gradients are compared under the implementation's own sign mask; the mask itself may differ from the
float64 one only where |z| < 1e-5 |gamma|, on at most 1e-4 of the elements.

Ratios measured on an MI355X (kernel error / torch-CPU error, worst over the shape sweep) are recorded in DESIGN.md 3.17."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, fixture_weights_and_input
import bn_act_np as N
import train_step as T
from orienmask_amd import arch, lib as omlib, train

pytestmark = pytest.mark.gpu

FLOOR = 1e-7
BAND = 1e-5            # |z| < BAND * |gamma|: the float32 sign of z may differ from the float64 one
FLIP_SHARE = 1e-4


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _layer_shapes(size):
    """Every distinct (C, H, W) of the BatchNorm layers of the FPNPlus model at this image size."""
    out = []
    for spec in arch.fpnplus_convs():
        if spec.bn:
            d = arch.layer_div(spec)
            shp = (spec.cout, size[0] // d, size[1] // d)
            if shp not in out:
                out.append(shp)
    return out


SWEEP = [(2,) + s for s in _layer_shapes((96, 96))] + [(2,) + s for s in _layer_shapes((160, 128)) if (2,) + s not in
                                                        [(2,) + t for t in _layer_shapes((96, 96))]]
SPECIAL = [(2, 64, 1, 1), (1, 256, 1, 2), (2, 64, 17, 17), (3, 5, 17, 17), (1, 1, 7, 9), (2, 1024, 3, 5)]
LARGE = [(2, 32, 544, 544), (2, 64, 272, 272), (2, 128, 136, 136), (2, 1024, 17, 17)]


def _inputs(shape, seed, mean=0.0, std=1.0, residual=True):
    rng = np.random.default_rng(seed)
    C = shape[1]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    d = dict(x=f(rng.standard_normal(shape) * std + mean), gamma=f(rng.standard_normal(C) * 0.5 + 1.2), beta=f(rng.standard_normal(C) * 0.3),
             rm=f(rng.standard_normal(C)), rv=f(rng.random(C) + 0.5), dy=f(rng.standard_normal(shape)))
    d["res"] = f(rng.standard_normal(shape)) if residual else None
    return d


def _hip(dev, d, training, residual, want_dx=True, backward=True):
    """The block through the C ABI.  -> dict of numpy arrays (y, y0 = the output without residual: its sign is the mask, save_mean,
    save_invstd, rm, rv, nbt, dx, dgamma, dbeta)."""
    L = omlib.load()
    t = {k: (torch.from_numpy(v).to(dev) if v is not None else None) for k, v in d.items()}
    B, C, H, W = d["x"].shape
    vp = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None      # noqa: E731
    ws_bytes = L.om_bn_act_workspace_bytes(B, C, H, W)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    nbt = torch.tensor(7, dtype=torch.long, device=dev)
    out = {}
    st = omlib.current_stream_ptr(dev)
    for key, res in (("y0", None), ("y", t["res"] if residual else None)):
        rm, rv = t["rm"].clone(), t["rv"].clone()
        y = torch.full_like(t["x"], float("nan"))
        sm, si = torch.empty(2 * C, device=dev), torch.empty(2 * C, device=dev)      # value | remainder
        omlib.check(L.om_bn_act_forward(vp(t["x"]), B, C, H, W, vp(t["gamma"]), vp(t["beta"]), vp(rm), vp(rv), vp(nbt), int(training),
                                        N.MOMENTUM, N.EPS, N.SLOPE, vp(res), vp(y), vp(sm), vp(si), vp(ws), ws.numel(), st),
                    "om_bn_act_forward")
        out[key] = y.cpu().numpy()
    out.update(save_mean=sm[:C].cpu().numpy(), save_invstd=si[:C].cpu().numpy(), rm=rm.cpu().numpy(), rv=rv.cpu().numpy(), nbt=int(nbt))
    if backward:
        dx = torch.full_like(t["x"], float("nan")) if want_dx else None
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws.fill_(255)
        omlib.check(L.om_bn_act_backward(vp(t["x"]), vp(t["dy"]), B, C, H, W, vp(t["gamma"]), vp(t["beta"]), vp(sm), vp(si), int(training),
                                         N.SLOPE, vp(dx), vp(dg), vp(db), vp(ws), ws.numel(), st), "om_bn_act_backward")
        out.update(dx=dx.cpu().numpy() if want_dx else None, dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())
    torch.cuda.synchronize(dev)
    return out


def _torch_cpu(d, training, residual):
    """torch's float32 batch_norm + leaky_relu on the CPU, the same outputs."""
    x, g, b = (torch.from_numpy(d[k]).clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = torch.from_numpy(d["rm"]).clone(), torch.from_numpy(d["rv"]).clone()
    bn = F.batch_norm(x, rm, rv, g, b, training, N.MOMENTUM, N.EPS)
    y0 = F.leaky_relu(bn, N.SLOPE)
    y = y0 + torch.from_numpy(d["res"]) if residual else y0
    y.backward(torch.from_numpy(d["dy"]))
    # save_mean / save_invstd as torch's native op reports them
    sm, si = torch.native_batch_norm(x.detach(), g.detach(), b.detach(), torch.from_numpy(d["rm"]).clone(), torch.from_numpy(d["rv"]).clone(),
                                     training, N.MOMENTUM, N.EPS)[1:]
    if not training:
        sm, si = rm, (rv.double() + N.EPS).rsqrt().float()
    return dict(y=y.detach().numpy(), y0=y0.detach().numpy(), save_mean=sm.numpy(), save_invstd=si.numpy(), rm=rm.numpy(), rv=rv.numpy(),
                dx=x.grad.numpy(), dgamma=g.grad.numpy(), dbeta=b.grad.numpy())


def _errors(got, d, training, residual, truth, skip_grads=False, outside=None):
    """name -> maximum error over the tensor's scale, against the float64 restatement; gradients under `got`'s own sign mask."""
    sel = (lambda a: a[outside]) if outside is not None else (lambda a: a)
    err = dict(y=N.rel_max(sel(got["y"]), sel(truth["y"])), save_mean=N.rel_max(got["save_mean"], truth["mean"]),
               save_invstd=N.rel_max(got["save_invstd"], truth["invstd"]), running_mean=N.rel_max(got["rm"], truth["running_mean"]),
               running_var=N.rel_max(got["rv"], truth["running_var"]))
    if not skip_grads:
        dx, dgamma, dbeta = N.backward(d["x"], d["dy"], d["gamma"], truth["mean"], truth["invstd"], got["y0"] > 0, training)
        if got.get("dx") is not None:
            err["dx"] = N.rel_max(got["dx"], dx)
        err["dgamma"] = N.rel_max(got["dgamma"], dgamma)
        err["dbeta"] = N.rel_max(got["dbeta"], dbeta)
    return err


def _check_mask(got, d, truth, what):
    flips = (got["y0"] > 0) != (truth["z"] > 0)
    band = np.abs(truth["z"]) < BAND * np.abs(d["gamma"]).reshape(1, -1, 1, 1)
    assert not (flips & ~band).any(), (what, "a sign differs outside the band")
    assert flips.sum() <= FLIP_SHARE * flips.size, (what, int(flips.sum()))
    return int(flips.sum())


def _judge(dev, shape, seed, training, residual, want_dx, mean=0.0, std=1.0):
    d = _inputs(shape, seed, mean, std, residual)
    got = _hip(dev, d, training, residual, want_dx)
    ref = _torch_cpu(d, training, residual)
    truth = N.forward(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], training, d["res"] if residual else None)
    what = (shape, "train" if training else "eval", "res" if residual else "nores", "dx" if want_dx else "nodx")
    flips = _check_mask(got, d, truth, what)
    mine, theirs = _errors(got, d, training, residual, truth), _errors(ref, d, training, residual, truth)
    assert got["nbt"] == (9 if training else 7), what              # two forward calls
    if not want_dx:
        assert got["dx"] is None
    worst = 0.0
    for k, e in mine.items():
        bound = max(2 * theirs[k], FLOOR)
        print("%-44s %-12s hip %.3g  torch-cpu %.3g  ratio %.2f  flips %d" % (what, k, e, theirs[k], e / max(theirs[k], 1e-30), flips))
        assert e <= bound, (what, k, e, theirs[k])
        worst = max(worst, e / max(theirs[k], FLOOR / 2))
    return worst


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.mark.parametrize("shape", SWEEP + SPECIAL, ids=lambda s: "x".join(map(str, s)))
def test_every_layer_shape_against_float64(dev, shape):
    """Every distinct layer shape at 96 x 96 and 160 x 128 (B = 2), B*H*W = 2, H*W = 289 and odd planes: training and eval, with and
    without residual, with and without dx, N(0,1) and N(3,2) inputs."""
    seed = sum(shape) * 7
    per_channel = shape[0] * shape[2] * shape[3]
    _judge(dev, shape, seed, True, True, True)
    _judge(dev, shape, seed + 1, True, False, False, mean=3.0, std=2.0)
    _judge(dev, shape, seed + 2, False, True, True, mean=3.0, std=2.0)
    _judge(dev, shape, seed + 3, False, False, False)
    assert per_channel >= 2


@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "x".join(map(str, s)))
def test_full_size_shapes_against_float64(dev, shape):
    """544 x 544 layers: several workgroups per channel (the two-launch form), 1024 channels of 17 x 17 in one launch each."""
    _judge(dev, shape, 11, True, True, True, mean=3.0, std=2.0)
    _judge(dev, shape, 12, False, False, True)


def test_one_value_per_channel_in_eval_mode(dev):
    _judge(dev, (1, 8, 1, 1), 3, False, True, True)


def test_ill_conditioned_statistics(dev):
    """Channel mean 1000, std 1: the statistics and running buffers are held to the 2x bar (E[x^2] - E[x]^2 in float32 misses
    running_var by 0.3).  y is compared outside the band where float32 cannot know the sign of z: the mean rounded to float32 moves
    z by up to 2^-15 |gamma| invstd, so the band here is |z| < 4e-5 |gamma| invstd.  Gradients are not compared: torch's own float32
    gradients are off by 10 % on this input, from sign flips."""
    shape = (2, 16, 48, 48)
    d = _inputs(shape, 5, mean=1000.0, std=1.0, residual=False)
    got = _hip(dev, d, True, False, backward=False)
    ref = _torch_cpu(d, True, False)
    truth = N.forward(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], True)
    outside = np.abs(truth["z"]) >= 4e-5 * np.abs(d["gamma"] * truth["invstd"]).reshape(1, -1, 1, 1)
    assert outside.mean() > 0.999
    mine = _errors(got, d, True, False, truth, skip_grads=True, outside=outside)
    theirs = _errors(ref, d, True, False, truth, skip_grads=True, outside=outside)
    for k, e in mine.items():
        print("ill-conditioned %-12s hip %.3g  torch-cpu %.3g" % (k, e, theirs[k]))
        assert e <= max(2 * theirs[k], FLOOR), (k, e, theirs[k])


@pytest.mark.parametrize("shape", [(2, 64, 48, 48), (2, 32, 544, 544), (4, 512, 17, 17)], ids=lambda s: "x".join(map(str, s)))
def test_rerun_is_bit_identical(dev, shape):
    d = _inputs(shape, 9)
    a, b = _hip(dev, d, True, True), _hip(dev, d, True, True)
    for k in ("y", "save_mean", "save_invstd", "rm", "rv", "dx", "dgamma", "dbeta"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_non_default_stream(dev):
    d = _inputs((2, 32, 96, 96), 4)
    want = _hip(dev, d, True, True)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        got = _hip(dev, d, True, True)
    for k in ("y", "dx", "dgamma", "dbeta", "rv"):
        assert np.array_equal(got[k], want[k]), k


def test_refusals_on_the_device(dev):
    L = omlib.load()
    x = torch.rand(2, 8, 4, 4, device=dev)
    c = torch.ones(64, device=dev)
    vp = lambda a: ctypes.c_void_p(a.data_ptr())      # noqa: E731
    y = torch.empty_like(x)
    big = (2, 32, 272, 272)
    xb = torch.rand(big, device=dev)
    rc = L.om_bn_act_forward(vp(xb), *big, vp(c), vp(c), None, None, None, 1, 0.1, 1e-5, 0.1, None, vp(torch.empty_like(xb)), vp(c), vp(c),
                             None, 0, None)
    assert rc != 0 and b"workspace" in L.om_last_error()
    rc = L.om_bn_act_forward(vp(x), 2, 8, 4, 4, vp(c), vp(c), None, None, None, 0, 0.1, 1e-5, 0.1, None, vp(y), vp(c), vp(c), None, 0, None)
    assert rc != 0 and b"running statistics" in L.om_last_error()
    torch.cuda.synchronize(dev)


# ---------------------------------------------------------------------------------------------------------------- ConvBNLeaky
def _pair(dev, cin, cout, k, seed):
    torch.manual_seed(seed)
    hip = train.ConvBNLeaky(cin, cout, k, padding=k // 2).to(dev)
    ref = train.ConvBNLeaky(cin, cout, k, padding=k // 2, backend="torch").to(dev)
    with torch.no_grad():
        hip.conv_block[1].weight.uniform_(0.5, 1.5); hip.conv_block[1].bias.uniform_(-0.5, 0.5)
        hip.conv_block[1].running_mean.uniform_(-0.2, 0.2); hip.conv_block[1].running_var.uniform_(0.5, 1.5)
    ref.load_state_dict(hip.state_dict())
    return hip, ref


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("residual", [False, True])
def test_module_matches_the_torch_backend(dev, training, residual):
    hip, ref = _pair(dev, 16, 32, 3, 1)
    hip.train(training); ref.train(training)
    x = torch.randn(2, 16, 24, 20, device=dev)
    res = torch.randn(2, 32, 24, 20, device=dev) if residual else None
    gy = torch.randn(2, 32, 24, 20, device=dev)
    outs = []
    for m in (hip, ref):
        xi = x.clone().requires_grad_(True)
        ri = res.clone().requires_grad_(True) if residual else None
        y = m(xi, residual=ri)
        y.backward(gy)
        outs.append((y.detach(), xi.grad, ri.grad if residual else None, [p.grad for p in m.parameters()], m.state_dict()))
    (y, gx, gr, gp, sd), (ty, tgx, tgr, tgp, tsd) = outs
    close = lambda a, b: (a - b).abs().max().item() <= 1e-4 * max(b.abs().max().item(), 1e-6)      # noqa: E731
    assert close(y, ty) and close(gx, tgx) and all(close(a, b) for a, b in zip(gp, tgp))
    if residual:
        assert torch.equal(gr, gy) and torch.equal(tgr, gy)
    for k in sd:
        assert close(sd[k].float(), tsd[k].float()), k
    assert int(sd["conv_block.1.num_batches_tracked"]) == int(tsd["conv_block.1.num_batches_tracked"]) == (1 if training else 0)


def test_module_refusals(dev):
    blk = train.ConvBNLeaky(4, 8, 1).to(dev)
    with pytest.raises(omlib.OrienMaskHipError, match="float32"):
        blk.half()(torch.rand(2, 4, 5, 5, device=dev).half())
    blk = train.ConvBNLeaky(4, 8, 1).to(dev)
    bn = blk.conv_block[1]
    with pytest.raises(omlib.OrienMaskHipError, match="contiguous"):
        train.bn_leaky(torch.rand(2, 8, 5, 5, device=dev).to(memory_format=torch.channels_last), bn)
    with pytest.raises(omlib.OrienMaskHipError, match="contiguous"):
        train.bn_leaky(torch.rand(2, 8, 5, 10, device=dev)[..., ::2], bn)
    with pytest.raises(omlib.OrienMaskHipError, match="float32"):
        train.bn_leaky(torch.rand(2, 8, 5, 5, device=dev).double(), bn)
    with pytest.raises(omlib.OrienMaskHipError, match="residual"):
        blk(torch.rand(2, 4, 5, 5, device=dev), residual=torch.rand(2, 8, 5, 5, device=dev).to(memory_format=torch.channels_last))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        blk(torch.rand(1, 4, 1, 1, device=dev))
    blk.conv_block[1].momentum = None
    with pytest.raises(ValueError, match="momentum"):
        blk(torch.rand(2, 4, 5, 5, device=dev))


def test_saved_tensors_of_one_block(dev):
    """One 'hip' block keeps for its backward: the convolution's own inputs (x and the weight), the convolution's output once, and
    per-channel vectors -- at most 4 numel(conv output) + the convolution's saved inputs + 64 C bytes.  The 'torch' block keeps the
    normalised activation as well."""
    hip, ref = _pair(dev, 32, 64, 3, 2)
    hip.train(); ref.train()
    x = torch.randn(2, 32, 48, 48, device=dev, requires_grad=True)

    def saved_bytes(m):
        seen = {}

        def pack(t):
            seen[(t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape))] = t.numel() * t.element_size()
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            y = m(x)
        y.sum().backward()
        return sum(seen.values()), y

    got, y = saved_bytes(hip)
    conv_inputs = x.numel() * 4 + hip.conv_block[0].weight.numel() * 4
    bound = 4 * y.numel() + conv_inputs + 64 * 64
    print("saved bytes: hip %d (bound %d), torch %d" % (got, bound, saved_bytes(ref)[0]))
    assert got <= bound
    assert saved_bytes(ref)[0] >= got + 4 * y.numel() - 64 * 64        # the same, up to the per-channel vectors


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("fixture", ["train_step_f96_b2", "train_step_bneval_f96_b2"])
def test_model_against_the_torch_backend_and_the_reference_step(dev, fixture):
    """'hip' against 'torch' on the same GPU: heads within 1e-4 of scale.  Against the reference's recorded step (CPU): the 'hip'
    model's relative-L2 gradient error (root mean square over the recorded tensors, each relative to its own norm) is at most twice
    the 'torch' model's on this GPU -- the convolutions' error is common to both."""
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    errs, heads_of, nets = {}, {}, {}
    for backend in ("hip", "torch"):
        heads_of[backend], grads, _, errs[backend], nets[backend] = T.recorded_step(dev, g, backend=backend)
        l2 = np.array([v.double().norm().item() for v in grads.values()])
        errs[backend + "_l2"] = float(np.abs(l2 / g["grad_l2"] - 1).max())
    for k, a, b in zip(N.HEAD_KEYS, heads_of["hip"], heads_of["torch"]):
        assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item(), k
        print("%-8s against the reference's CPU heads: %.3g of scale" % (k, N.rel_max(a.cpu().numpy(), g[k])))
    for i, n in enumerate(N.GRAD_NAMES):
        print("%-50s hip %.3g  torch %.3g" % (n, errs["hip"][i], errs["torch"][i]))
    print("gradient error, rms over tensors: hip %.3g  torch %.3g; norms of all parameters: hip %.3g  torch %.3g"
          % (T.rms(errs["hip"]), T.rms(errs["torch"]), errs["hip_l2"], errs["torch_l2"]))
    assert T.rms(errs["hip"]) <= 2 * T.rms(errs["torch"])
    after = nets["hip"].state_dict()
    layers = [str(k) for k in g["bn_layers"]]
    assert N.rel_l2(np.concatenate([after[k + ".running_mean"].cpu().numpy() for k in layers]), g["running_mean"]) <= 1e-4
    assert N.rel_l2(np.concatenate([after[k + ".running_var"].cpu().numpy() for k in layers]), g["running_var"]) <= 1e-4
    assert [int(after[k + ".num_batches_tracked"]) for k in layers] == g["num_batches_tracked"].tolist()


def test_eval_forward_matches_the_inference_fixture(dev):
    g = np.load(os.path.join(GOLDEN, "fwd_f96_b2.npz"))
    sd, x = fixture_weights_and_input(g)
    net = train.OrienMaskYOLOFPNPlus(3, 80)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    with torch.no_grad():
        out = net(x.to(dev))
    got = dict(bbox32=out[0][0], bbox16=out[1][0], bbox8=out[2][0], oriens=torch.cat([out[0][1], out[1][1], out[2][1]], 1))
    for k, t in got.items():
        assert N.rel_max(t.cpu().numpy(), g[k]) <= 1e-4, k
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in net.state_dict().items())


def test_one_trainer_step_changes_every_parameter(dev):
    """trainer/trainer.py:42-55 with this package's pieces: build_train_model -> the HIP loss -> backward -> the HIP SGD step."""
    _, _, net = T.trainer_steps(dev, {}, 1)
    assert net.training and net.backend == "hip" and next(net.parameters()).device == dev
    assert all(int(v) == 1 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))
