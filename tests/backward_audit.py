"""Teacher-forced audit of one training step's backward: capture, truth, metrics and judge (tests/test_backward_audit.py on the GPU,
tests/test_backward_audit_cpu.py for the harness itself).

Capture.  ConvBNLeaky.forward and the models' _plain resolve `conv2d` and `bn_leaky` as globals of orienmask_amd.train, so a
recording wrapper installed there sees every HIP autograd node of a model built with backend='hip', conv_backend='hip'.  A wrapper
clones what the node was given (x, weight / h, gamma, beta, residual, the BatchNorm buffers before the call), hooks the node's output
for the dy that reaches it, and hands the real function an ALIAS of each input that requires grad (x.view_as(x)) with a hook on the
alias: that hook sees the node's OWN input gradient, where a hook on x would see the sum over all of x's consumers (the residual
path).  Parameter gradients are read from .grad afterwards: every parameter is used once.  The functions behind the wrappers are a
parameter: the real train.conv2d / train.bn_leaky on the GPU; torch's float32 ops of the same signatures on the CPU (the same
wiring without a GPU); and for a model built with backend='torch' the wrappers go on torch.nn.functional's conv2d, batch_norm and
leaky_relu instead (a block is then the batch_norm call and the leaky_relu call that follows it; the residual add is torch's).

Judge.  A node is re-run alone on its recorded tensors by a `rerun` function (the C ABI on the GPU, torch float32 on the CPU) and
  (a) tie: every gradient the model's own backward produced must equal the re-run's bit for bit (differing()), and
  (b) float64: truth is float64 on the CPU from the same float32 inputs, the yardstick torch's own float32 on the CPU:
      convolution   dx, dw, dbias: max |got - truth| / max |truth| ("scale"); dx, dw also per element,
                    max |got - truth| / (N + |truth|), N = the L2 norm of the products that make the element (torch.nn.grad's two
                    functions on the squared operands, then a square root): small where a channel is small, so a wrong low-scale
                    channel or a missing border tap shows.  Yardstick: the LARGER error of torch.nn.grad in float32 with oneDNN on
                    and off (in-network the two differ by up to 2.4x per layer; for dbias also F.conv2d's own backward, a third
                    valid float32 sum that is 3.6x further from float64 on the heads' dy).  Bar: 2 x yardstick, floor 2e-7.
      block         y, save_mean, save_invstd, running buffers, dgamma, dbeta, dh: scale, bar 2 x yardstick, floor 1e-7, gradients
                    under the implementation's own sign mask (tests/test_bn_act.py); dh also per channel (max error of channel c
                    over max |truth| of channel c, worst channel), bar 4 x yardstick: a plain numpy float32 evaluation of the
                    backward formula already reaches 2.34 x torch-CPU's there.  The mask may differ from the float64 one only
                    inside test_bn_act's BAND, on at most FLIP_SHARE of the elements.
"""
import collections
import contextlib
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import bn_act_np as N
import conv_grad_np as G
from test_bn_act import BAND, FLIP_SHARE, FLOOR as BLOCK_FLOOR
from test_conv_grad import FLOOR as CONV_FLOOR
from orienmask_amd import arch, lib as omlib, train

BAR = 2.0
BAR_DH_CHANNEL = 4.0
BLOCK_TIED = ("y", "rm", "rv", "nbt", "dx", "dgamma", "dbeta")


# ---------------------------------------------------------------------------------------------------------------- torch float32
def torch_conv2d(x, weight, bias=None, stride=1, padding=0):
    """train.conv2d's signature, torch's own float32 arithmetic."""
    return F.conv2d(x, weight, bias, stride, padding)


def torch_bn_leaky(x, bn, residual=None, slope=arch.LEAKY_SLOPE, sync=False, process_group=None):
    """train.bn_leaky's signature, torch's own float32 arithmetic (what ConvBNLeaky does with backend='torch')."""
    training = bn.training or bn.running_mean is None
    y = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, training, bn.momentum, bn.eps)
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    y = F.leaky_relu(y, slope)
    return y if residual is None else y + residual


# ---------------------------------------------------------------------------------------------------------------- capture
def _keep(rec, key):
    def hook(g):
        assert rec.get(key) is None, (rec["name"], key, "a second gradient arrived")
        rec[key] = g.detach().clone()
    return hook


def _alias(t, rec, key):
    """An alias of t whose hook records the gradient of this consumer alone; t itself when it takes no gradient."""
    if t is None or not t.requires_grad:
        return t
    a = t.view_as(t)
    a.register_hook(_keep(rec, key))
    return a


def _one(v):
    a, b = (v, v) if isinstance(v, int) else tuple(v)
    assert a == b, v
    return int(a)


class Capture:
    """Records every convolution and every BatchNorm + LeakyReLU block of one forward and backward of `net`.  After finish():
    convs / blocks are lists of dicts of numpy arrays in call order, keyed as the re-run functions' results."""

    def __init__(self, net):
        self.convs, self.blocks = [], []
        self._params = {id(p): n for n, p in net.named_parameters()}
        self._bn_of = {id(m.weight): m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)}
        self._live = []           # (record, parameters whose .grad finish() reads)
        self._open = None         # backend 'torch': the batch_norm call waiting for its leaky_relu

    def _name(self, weight, suffix):
        n = self._params[id(weight)]
        assert n.endswith(suffix), n
        return n[:-len(suffix)]

    # -- train.conv2d / F.conv2d
    def conv2d(self, real):
        def wrapper(x, weight, bias=None, stride=1, padding=0, *more, **kw):
            blockish = self._params[id(weight)].endswith(".conv_block.0.weight")
            rec = dict(name=self._name(weight, ".conv_block.0.weight" if blockish else ".weight"), x=x.detach().clone(),
                       w=weight.detach().clone(), bias=bias is not None, stride=_one(stride), ksize=int(weight.shape[2]),
                       x_requires_grad=bool(x.requires_grad), dx=None, dy=None)
            assert _one(padding) == rec["ksize"] // 2, (rec["name"], padding)
            y = real(_alias(x, rec, "dx"), weight, bias, stride, padding, *more, **kw)
            y.register_hook(_keep(rec, "dy"))
            self.convs.append(rec)
            self._live.append((rec, dict(dw=weight, db=bias)))
            return y
        return wrapper

    # -- train.bn_leaky
    def _block_before(self, h, bn, name):
        training = bool(bn.training or bn.running_mean is None)
        return dict(name=name, h=h.detach().clone(), gamma=bn.weight.detach().clone(), beta=bn.bias.detach().clone(), training=training,
                    rm0=bn.running_mean.clone(), rv0=bn.running_var.clone(), nbt0=int(bn.num_batches_tracked), momentum=float(bn.momentum),
                    eps=float(bn.eps), dx=None, dy=None, dres=None)

    def _block_after(self, rec, bn, y):
        rec.update(y=y.detach().clone(), rm=bn.running_mean.clone(), rv=bn.running_var.clone(), nbt=int(bn.num_batches_tracked))
        y.register_hook(_keep(rec, "dy"))
        self.blocks.append(rec)
        self._live.append((rec, dict(dgamma=bn.weight, dbeta=bn.bias)))

    def bn_leaky(self, real):
        def wrapper(x, bn, residual=None, slope=arch.LEAKY_SLOPE, **kw):
            rec = self._block_before(x, bn, self._name(bn.weight, ".conv_block.1.weight"))
            rec.update(slope=float(slope), res=residual.detach().clone() if residual is not None else None)
            y = real(_alias(x, rec, "dx"), bn, residual=_alias(residual, rec, "dres"), slope=slope, **kw)
            self._block_after(rec, bn, y)
            return y
        return wrapper

    # -- backend 'torch': F.batch_norm, then F.leaky_relu
    def batch_norm(self, real):
        def wrapper(x, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5):
            assert self._open is None
            bn = self._bn_of[id(weight)]
            assert running_mean is bn.running_mean and bias is bn.bias and momentum == bn.momentum and eps == bn.eps
            rec = self._block_before(x, bn, self._name(weight, ".conv_block.1.weight"))
            assert rec["training"] == bool(training)
            self._open = (rec, bn)
            return real(_alias(x, rec, "dx"), running_mean, running_var, weight, bias, training, momentum, eps)
        return wrapper

    def leaky_relu(self, real):
        def wrapper(x, negative_slope=0.01, inplace=False):
            (rec, bn), self._open = self._open, None
            y = real(x, negative_slope, inplace)
            rec.update(slope=float(negative_slope), res=None)       # the residual add is torch's own, after this call
            self._block_after(rec, bn, y)
            return y
        return wrapper

    @contextlib.contextmanager
    def installed(self, targets):
        """targets: (object, attribute, wrapper maker, function to wrap or None for the attribute's own value)."""
        old = []
        try:
            for obj, attr, make, real in targets:
                old.append((obj, attr, getattr(obj, attr)))
                setattr(obj, attr, make(real if real is not None else getattr(obj, attr)))
            yield self
        finally:
            for obj, attr, value in reversed(old):
                setattr(obj, attr, value)

    def finish(self):
        assert self._open is None
        for rec, params in self._live:
            for key, p in params.items():
                rec[key] = None if p is None or p.grad is None else p.grad.detach().clone()
        for rec in self.convs + self.blocks:
            for k, v in rec.items():
                if torch.is_tensor(v):
                    rec[k] = np.ascontiguousarray(v.detach().cpu().numpy())
        self._live = []
        return self


def hip_targets(capture, conv2d=None, bn_leaky=None, convs=True):
    """The wrappers on orienmask_amd.train's globals (a model with backend='hip'; conv_backend='hip' for the convolutions)."""
    t = [(train, "bn_leaky", capture.bn_leaky, bn_leaky)]
    return t + [(train, "conv2d", capture.conv2d, conv2d)] if convs else t


def torch_targets(capture):
    """The wrappers on torch.nn.functional (a model with backend='torch', conv_backend='torch')."""
    return [(F, "conv2d", capture.conv2d, None), (F, "batch_norm", capture.batch_norm, None), (F, "leaky_relu", capture.leaky_relu, None)]


def run_step(net, x, targets_of, backward):
    """One forward and backward of `net` on x under a Capture.  backward(heads): runs the backward from the six heads.  -> Capture."""
    cap = Capture(net)
    assert not x.requires_grad
    with cap.installed(targets_of(cap)), torch.backends.cudnn.flags(deterministic=True):
        heads = [t for pair in net(x) for t in pair]
        backward(heads)
    assert x.grad is None
    return cap.finish()


def cotangent_backward(seed):
    def backward(heads):
        cot = N.cotangents(seed, [t.shape for t in heads])
        torch.autograd.backward(heads, [torch.from_numpy(c).to(heads[0].device) for c in cot])
    return backward


def expected_nodes(model):
    """(names of the ConvBNLeaky blocks, names of all convolutions) in arch.model_convs order."""
    specs = list(arch.model_convs(model, 3, 80))
    return [s.name for s in specs if s.bn], [s.name for s in specs]


# ---------------------------------------------------------------------------------------------------------------- re-runs
def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def conv_inputs(rec):
    return dict(x=rec["x"], w=rec["w"], dy=rec["dy"], ksize=rec["ksize"], stride=rec["stride"])


def conv_wants(rec):
    return tuple(k for k, on in (("dx", rec["x_requires_grad"]), ("dw", True), ("db", rec["bias"])) if on)


def hip_conv_rerun(dev):
    """rec -> the gradients through the C ABI on a workspace of the call's own (pre-filled 0xFF; outputs pre-filled with NaN)."""
    def rerun(rec):
        L = omlib.load()
        x, w, dy = (torch.from_numpy(rec[k]).to(dev) for k in ("x", "w", "dy"))
        B, cin, H, W = x.shape
        geom = (B, cin, H, W, w.shape[0], rec["ksize"], rec["stride"])
        assert tuple(dy.shape) == (B, w.shape[0]) + G.out_hw(H, W, rec["ksize"], rec["stride"]), (rec["name"], tuple(dy.shape))
        ws = torch.full((max(L.om_conv2d_grad_workspace_bytes(*geom), 16),), 255, dtype=torch.uint8, device=dev)
        st = omlib.current_stream_ptr(dev)
        want = conv_wants(rec)
        dx = torch.full_like(x, float("nan")) if "dx" in want else None
        dw = torch.full_like(w, float("nan"))
        db = torch.full((w.shape[0],), float("nan"), device=dev) if "db" in want else None
        if dx is not None:
            omlib.check(L.om_conv2d_grad_input(_vp(dy), _vp(w), *geom, _vp(dx), _vp(ws), ws.numel(), st), "om_conv2d_grad_input")
        omlib.check(L.om_conv2d_grad_weight(_vp(x), _vp(dy), *geom, _vp(dw), _vp(db), _vp(ws), ws.numel(), st), "om_conv2d_grad_weight")
        torch.cuda.synchronize(dev)
        return {k: v.cpu().numpy() for k, v in (("dx", dx), ("dw", dw), ("db", db)) if v is not None}
    return rerun


def torch_conv_rerun(rec):
    """rec -> the gradients of F.conv2d under autograd in float32 on the CPU, as the model's own backward asks for them."""
    x, w, dy = (torch.from_numpy(rec[k]).clone() for k in ("x", "w", "dy"))
    x.requires_grad_(rec["x_requires_grad"])
    w.requires_grad_(True)
    b = torch.zeros(w.shape[0], requires_grad=True) if rec["bias"] else None
    F.conv2d(x, w, b, rec["stride"], rec["ksize"] // 2).backward(dy)
    return {k: v.grad.numpy() for k, v in (("dx", x), ("dw", w), ("db", b)) if v is not None and v.grad is not None}


def hip_block_rerun(dev):
    """rec -> the block through the C ABI (y0: the output without the residual, whose sign is the mask) on a workspace of the call's
    own, pre-filled 0xFF before each launch sequence."""
    def rerun(rec):
        L = omlib.load()
        t = {k: (torch.from_numpy(rec[k]).to(dev) if rec[k] is not None else None) for k in ("h", "gamma", "beta", "res", "dy", "rm0", "rv0")}
        B, C, H, W = rec["h"].shape
        training, track = rec["training"], rec["training"]
        ws = torch.empty(max(L.om_bn_act_workspace_bytes(B, C, H, W), 16), dtype=torch.uint8, device=dev)
        st = omlib.current_stream_ptr(dev)
        out = {}
        for key, res in (("y0", None), ("y", t["res"])):
            rm, rv = t["rm0"].clone(), t["rv0"].clone()
            nbt = torch.tensor(rec["nbt0"], dtype=torch.long, device=dev)
            y = torch.full_like(t["h"], float("nan"))
            sm, si = torch.empty(2 * C, device=dev), torch.empty(2 * C, device=dev)      # value | remainder
            ws.fill_(255)
            omlib.check(L.om_bn_act_forward(_vp(t["h"]), B, C, H, W, _vp(t["gamma"]), _vp(t["beta"]), _vp(rm), _vp(rv),
                                            _vp(nbt) if track else None, int(training), rec["momentum"], rec["eps"], rec["slope"], _vp(res),
                                            _vp(y), _vp(sm), _vp(si), _vp(ws), ws.numel(), st), "om_bn_act_forward")
            out[key] = y.cpu().numpy()
        dx = torch.full_like(t["h"], float("nan"))
        dg, db = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        ws.fill_(255)
        omlib.check(L.om_bn_act_backward(_vp(t["h"]), _vp(t["dy"]), B, C, H, W, _vp(t["gamma"]), _vp(t["beta"]), _vp(sm), _vp(si),
                                         int(training), rec["slope"], _vp(dx), _vp(dg), _vp(db), _vp(ws), ws.numel(), st), "om_bn_act_backward")
        torch.cuda.synchronize(dev)
        out.update(save_mean=sm[:C].cpu().numpy(), save_invstd=si[:C].cpu().numpy(), rm=rm.cpu().numpy(), rv=rv.cpu().numpy(), nbt=int(nbt),
                   dx=dx.cpu().numpy(), dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())
        return out
    return rerun


def torch_block_rerun(rec):
    """rec -> torch's float32 batch_norm + leaky_relu (+ residual) on the CPU, the same outputs: the yardstick of the block, and the
    implementation itself where the model ran on torch's ops."""
    h, g, b = (torch.from_numpy(rec[k]).clone().requires_grad_(True) for k in ("h", "gamma", "beta"))
    rm, rv = torch.from_numpy(rec["rm0"]).clone(), torch.from_numpy(rec["rv0"]).clone()
    training = rec["training"]
    y0 = F.leaky_relu(F.batch_norm(h, rm, rv, g, b, training, rec["momentum"], rec["eps"]), rec["slope"])
    y = y0 + torch.from_numpy(rec["res"]) if rec["res"] is not None else y0
    y.backward(torch.from_numpy(rec["dy"]))
    if training:          # save_mean / save_invstd as torch's native op reports them
        sm, si = torch.native_batch_norm(h.detach(), g.detach(), b.detach(), torch.from_numpy(rec["rm0"]).clone(),
                                         torch.from_numpy(rec["rv0"]).clone(), True, rec["momentum"], rec["eps"])[1:]
    else:
        sm, si = rm, (rv.double() + rec["eps"]).rsqrt().float()
    return dict(y=y.detach().numpy(), y0=y0.detach().numpy(), save_mean=sm.numpy(), save_invstd=si.numpy(), rm=rm.numpy(), rv=rv.numpy(),
                nbt=rec["nbt0"] + int(training), dx=h.grad.numpy(), dgamma=g.grad.numpy(), dbeta=b.grad.numpy())


# ---------------------------------------------------------------------------------------------------------------- (a) the tie
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(rec, again, keys):
    """The gradients (and outputs) among `keys` that the model's own step and the isolated re-run do not share bit for bit; a block's
    gradient for its residual must be the dy that reached the block."""
    out = [k for k in keys if not same_bits(rec[k], again[k])]
    if rec.get("res") is not None and not same_bits(rec["dres"], rec["dy"]):
        out.append("dres")
    return out


# ---------------------------------------------------------------------------------------------------------------- (b) float64
Score = collections.namedtuple("Score", "node grad metric err yard bar")     # passes when err <= bar


def over_bar(s):
    return s.err / s.bar


def _yardsticks_conv(d, want):
    """torch.nn.grad in float32 with oneDNN on and off; for dbias also what F.conv2d's own backward gives: on the heads' in-network dy
    that float32 sum is off by 3.9e-7 of scale where dy.sum is off by 1.1e-7 (bbox_head8.1, 96 x 96, B = 2), both valid."""
    out = []
    for on in (True, False):
        with torch.backends.mkldnn.flags(enabled=on):
            out.append(G.gradients(d, torch.float32, want))
    if "db" in want:
        x, w, dy = (torch.from_numpy(d[k]) for k in ("x", "w", "dy"))
        b = torch.zeros(w.shape[0], requires_grad=True)
        F.conv2d(x, w, b, d["stride"], d["ksize"] // 2).backward(dy)
        out.append(dict(db=b.grad.numpy()))
    return out


def per_element(got, truth, norm):
    """max |got - truth| / (norm + |truth|); an element whose products are all zero must be zero."""
    diff = np.abs(np.asarray(got, np.float64) - truth)
    den = norm + np.abs(truth)
    if (diff[den == 0] != 0).any() or not np.isfinite(diff).all():
        return float("inf")
    return float(np.divide(diff, den, out=np.zeros_like(diff), where=den > 0).max())


def scale_error(got, truth):
    got = np.asarray(got, np.float64)
    return N.rel_max(got, truth) if got.shape == truth.shape and np.isfinite(got).all() else float("inf")


def conv_reference(rec):
    """(truth, product norms, the two yardsticks) of a recorded convolution; computed once per record."""
    if "_ref" not in rec:
        d, want = conv_inputs(rec), conv_wants(rec)
        x, w, dy = (torch.from_numpy(d[k]).double() for k in ("x", "w", "dy"))
        s, p = rec["stride"], rec["ksize"] // 2
        norm = dict(dw=torch.nn.grad.conv2d_weight(x * x, w.shape, dy * dy, stride=s, padding=p).sqrt().numpy())
        if "dx" in want:
            norm["dx"] = torch.nn.grad.conv2d_input(x.shape, w * w, dy * dy, stride=s, padding=p).sqrt().numpy()
        rec["_ref"] = (G.truth(d, want), norm, _yardsticks_conv(d, want))
    return rec["_ref"]


def judge_conv(rec, got):
    """-> [Score]: dx, dw, db by scale; dx, dw per element.  The yardstick is the larger error of the two float32 evaluations."""
    truth, norm, yards = conv_reference(rec)
    assert sorted(got) == sorted(truth), (rec["name"], sorted(got), sorted(truth))
    out = []
    for k in conv_wants(rec):
        y = max(scale_error(r[k], truth[k]) for r in yards if k in r)
        out.append(Score(rec["name"], k, "scale", scale_error(got[k], truth[k]), y, max(BAR * y, CONV_FLOOR)))
        if k in norm:
            y = max(per_element(r[k], truth[k], norm[k]) for r in yards if k in r)
            e = per_element(got[k], truth[k], norm[k]) if got[k].shape == truth[k].shape else float("inf")
            out.append(Score(rec["name"], k, "element", e, y, max(BAR * y, CONV_FLOOR)))
    return out


def per_channel(got, truth):
    """Worst over the channels of: max error of channel c over max |truth| of channel c."""
    d = np.abs(np.asarray(got, np.float64) - truth).max(axis=(0, 2, 3))
    return float((d / np.maximum(np.abs(truth).max(axis=(0, 2, 3)), 1e-30)).max())


def block_reference(rec):
    if "_ref" not in rec:
        rec["_ref"] = (N.forward(rec["h"], rec["gamma"], rec["beta"], rec["rm0"], rec["rv0"], rec["training"], rec["res"], rec["eps"],
                                 rec["momentum"], rec["slope"]), torch_block_rerun(rec))
    return rec["_ref"]


def _block_errors(rec, got, truth):
    """{(gradient, metric): error} against the float64 restatement; gradients under `got`'s own sign mask."""
    dx, dgamma, dbeta = N.backward(rec["h"], rec["dy"], rec["gamma"], truth["mean"], truth["invstd"], got["y0"] > 0, rec["training"], rec["slope"])
    flips = (got["y0"] > 0) != (truth["z"] > 0)
    band = np.abs(truth["z"]) < BAND * np.abs(rec["gamma"]).reshape(1, -1, 1, 1)
    return {("y", "scale"): scale_error(got["y"], truth["y"]), ("save_mean", "scale"): scale_error(got["save_mean"], truth["mean"]),
            ("save_invstd", "scale"): scale_error(got["save_invstd"], truth["invstd"]),
            ("running_mean", "scale"): scale_error(got["rm"], truth["running_mean"]),
            ("running_var", "scale"): scale_error(got["rv"], truth["running_var"]),
            ("dgamma", "scale"): scale_error(got["dgamma"], dgamma), ("dbeta", "scale"): scale_error(got["dbeta"], dbeta),
            ("dh", "scale"): scale_error(got["dx"], dx), ("dh", "channel"): per_channel(got["dx"], dx),
            ("mask", "flips"): float("inf") if (flips & ~band).any() else float(flips.sum()) / flips.size,
            ("nbt", "count"): float(abs(int(got["nbt"]) - (rec["nbt0"] + int(rec["training"]))))}


def judge_block(rec, got):
    """-> [Score]: the block's outputs, statistics and gradients against float64, each with torch-CPU float32's error beside it; the
    sign mask (no flip outside the band, at most FLIP_SHARE of the elements); num_batches_tracked exactly."""
    truth, yard = block_reference(rec)
    mine, theirs = _block_errors(rec, got, truth), _block_errors(rec, yard, truth)
    out = []
    for (k, metric), e in mine.items():
        y = theirs[(k, metric)]
        if metric == "flips":
            bar = FLIP_SHARE
        elif metric == "count":
            bar = 0.5
        else:
            bar = max((BAR_DH_CHANNEL if metric == "channel" else BAR) * y, BLOCK_FLOOR)
        out.append(Score(rec["name"], k, metric, e, y, bar))
    return out


def geometry(rec):
    if "w" in rec:
        B, cin, H, W = rec["x"].shape
        return "%dx%d->%d k%d s%d %dx%d" % (B, cin, rec["w"].shape[0], rec["ksize"], rec["stride"], H, W)
    return "%s %s%s" % ("x".join(map(str, rec["h"].shape)), "train" if rec["training"] else "eval", " +res" if rec["res"] is not None else "")


def line(cid, rec, s, tie=""):
    return "%-18s %-30s %-30s %-12s %-8s impl %.3g  torch-cpu %.3g  ratio %.2f  of bar %.2f%s" % (
        cid, s.node, geometry(rec), s.grad, s.metric, s.err, s.yard, s.err / max(s.yard, 1e-30), over_bar(s), tie)
