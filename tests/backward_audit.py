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

The forward convolution and the route nodes (a model built with conv_forward='hip', route_backend='hip' as well: the step
orienmask_amd.trainer runs).  A convolution record also holds the node's output y, the bias values and the `forward` keyword of the
call; train.upsample_concat and train.split_channels, globals of orienmask_amd.train like the other two, are recorded as nodes of
their own: a concat with its sources, scales, y, the dy that reaches y and each source's own gradient (through an alias, as above:
neck32 feeds the neck, a head, route32.0 and skip32.0); the split with x, the sizes, the outputs, each output's dy and dx through
the alias.  A route node is named by what it feeds (cat.neck16, cat.neck8, cat.neck4, split.orien) and remembers which node made
each of its inputs.
  (a) tie: where the call asked for forward='hip' the model's own y equals om_conv2d_forward alone on the recorded x, w, bias bit
      for bit; a route node's y / outputs and every gradient equal om_route_concat_forward / _backward alone on the recorded tensors.
  (b) convolution y against F.conv2d in float64 (tests/conv_fwd_np.py): over the scale and per element with N = sqrt(conv2d(x^2,
      w^2)); yardstick the larger error of torch-CPU float32 F.conv2d with oneDNN on and off; bar 2 x yardstick, floor
      test_conv_fwd.FLOOR.  Routes against tests/route_np.py without a tolerance: y equals forward() and every source gradient
      equals backward() bit for bit, and is within within_bound() of backward64(); the split's outputs are x's channel slices and
      its dx the concatenation of the recorded dys, exact zeros where an output received none.
  chaining: a block's h has the bits of its convolution's y, and a route node's input the bits of the output of the node that
      made it: a difference is a wiring or aliasing fault, not a rounding one.
A node that takes no gradient (a frozen backbone) is recorded with its forward results only: no hook goes on a tensor that does not
require grad, and the re-runs and the judges then cover the forward quantities alone.
"""
import collections
import contextlib
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import bn_act_np as N
import conv_fwd_np as C
import conv_grad_np as G
import route_np as R
from test_bn_act import BAND, FLIP_SHARE, FLOOR as BLOCK_FLOOR
from test_conv_fwd import FLOOR as FWD_FLOOR
from test_conv_grad import FLOOR as CONV_FLOOR
from orienmask_amd import arch, lib as omlib, train

BAR = 2.0
BAR_DH_CHANNEL = 4.0
BLOCK_TIED = ("y", "rm", "rv", "nbt", "dx", "dgamma", "dbeta")


# ---------------------------------------------------------------------------------------------------------------- torch float32
def torch_conv2d(x, weight, bias=None, stride=1, padding=0, forward="torch"):
    """train.conv2d's signature, torch's own float32 arithmetic (whichever forward the call asks for)."""
    return F.conv2d(x, weight, bias, stride, padding)


def torch_upsample_concat(tensors, scales):
    """train.upsample_concat's signature, torch's own ops (what the models do with route_backend='torch')."""
    return torch.cat([F.interpolate(t, scale_factor=s, mode="nearest") if s > 1 else t for t, s in zip(tensors, scales)], dim=1)


def torch_split_channels(x, sizes):
    """train.split_channels' signature, torch.split."""
    return torch.split(x, [int(c) for c in sizes], dim=1)


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
        if g is not None:         # autograd hands an unused output of a several-output node an undefined gradient
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
    """Records every convolution, every BatchNorm + LeakyReLU block and every route node of one forward and backward of `net`.
    After finish(): convs / blocks / cats / splits are lists of dicts of numpy arrays in call order, keyed as the re-run functions'
    results (a concat's srcs and dsrc, a split's outs and dys are lists with one entry per tensor, None where there is none)."""

    def __init__(self, net):
        self.convs, self.blocks, self.cats, self.splits = [], [], [], []
        self._params = {id(p): n for n, p in net.named_parameters()}
        self._bn_of = {id(m.weight): m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)}
        self._live = []           # (record, parameters whose .grad finish() reads)
        self._open = None         # backend 'torch': the batch_norm call waiting for its leaky_relu
        self._made = {}           # id(a node's output) -> (the node's name, the output: held, so that no id is used twice)
        self._unfed = {}          # id(a concat's output) -> its record, until the convolution it feeds names it

    def _name(self, weight, suffix):
        n = self._params[id(weight)]
        assert n.endswith(suffix), n
        return n[:-len(suffix)]

    def _output(self, rec, y):
        """Hooks the node's output for its dy, unless nothing behind it takes a gradient; remembers who made it."""
        if y.requires_grad:
            y.register_hook(_keep(rec, "dy"))
        self._made[id(y)] = (rec["name"], y)

    def _maker(self, t):
        return self._made.get(id(t), (None, None))[0]

    # -- train.conv2d / F.conv2d
    def conv2d(self, real):
        def wrapper(x, weight, bias=None, stride=1, padding=0, *more, **kw):
            blockish = self._params[id(weight)].endswith(".conv_block.0.weight")
            rec = dict(name=self._name(weight, ".conv_block.0.weight" if blockish else ".weight"), x=x.detach().clone(),
                       w=weight.detach().clone(), bias=bias is not None, b=bias.detach().clone() if bias is not None else None,
                       forward=str(kw.get("forward", "torch")), stride=_one(stride), ksize=int(weight.shape[2]),
                       x_requires_grad=bool(x.requires_grad), w_requires_grad=bool(weight.requires_grad),
                       b_requires_grad=bool(bias is not None and bias.requires_grad), dx=None, dy=None)
            assert _one(padding) == rec["ksize"] // 2, (rec["name"], padding)
            fed = self._unfed.pop(id(x), None)
            if fed is not None:
                fed["name"] = "cat." + rec["name"].rsplit(".", 1)[0]
            y = real(_alias(x, rec, "dx"), weight, bias, stride, padding, *more, **kw)
            rec["y"] = y.detach().clone()
            self._output(rec, y)
            self.convs.append(rec)
            self._live.append((rec, dict(dw=weight, db=bias)))
            return y
        return wrapper

    # -- train.upsample_concat
    def upsample_concat(self, real):
        def wrapper(tensors, scales):
            tensors, scales = list(tensors), [int(s) for s in scales]
            rec = dict(name="cat.?", srcs=[t.detach().clone() for t in tensors], scales=scales, src_names=[self._maker(t) for t in tensors],
                       src_requires_grad=[bool(t.requires_grad) for t in tensors], dy=None)
            rec.update(("dsrc%d" % i, None) for i in range(len(tensors)))
            y = real([_alias(t, rec, "dsrc%d" % i) for i, t in enumerate(tensors)], scales)
            rec["y"] = y.detach().clone()
            self._output(rec, y)
            self._unfed[id(y)] = rec
            self.cats.append(rec)
            return y
        return wrapper

    # -- train.split_channels
    def split_channels(self, real):
        def wrapper(x, sizes):
            sizes = [int(c) for c in sizes]
            maker = self._maker(x)
            rec = dict(name="split." + (maker.split("_")[0] if maker else "?"), x=x.detach().clone(), x_name=maker, sizes=sizes,
                       x_requires_grad=bool(x.requires_grad), dx=None)
            outs = real(_alias(x, rec, "dx"), sizes)
            rec["outs"] = [o.detach().clone() for o in outs]
            for i, o in enumerate(outs):
                rec["dy%d" % i] = None
                if o.requires_grad:
                    o.register_hook(_keep(rec, "dy%d" % i))
            self.splits.append(rec)
            return outs
        return wrapper

    # -- train.bn_leaky
    def _block_before(self, h, bn, name):
        training = bool(bn.training or bn.running_mean is None)
        return dict(name=name, h=h.detach().clone(), gamma=bn.weight.detach().clone(), beta=bn.bias.detach().clone(), training=training,
                    rm0=bn.running_mean.clone(), rv0=bn.running_var.clone(), nbt0=int(bn.num_batches_tracked), momentum=float(bn.momentum),
                    eps=float(bn.eps), dx=None, dy=None, dres=None)

    def _block_after(self, rec, bn, y):
        rec.update(y=y.detach().clone(), rm=bn.running_mean.clone(), rv=bn.running_var.clone(), nbt=int(bn.num_batches_tracked))
        self._output(rec, y)
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
        assert not self._unfed, "a concat's output fed no convolution"
        for rec, params in self._live:
            for key, p in params.items():
                rec[key] = None if p is None or p.grad is None else p.grad.detach().clone()
        for rec in self.cats:
            rec["dsrc"] = [rec.pop("dsrc%d" % i) for i in range(len(rec["srcs"]))]
        for rec in self.splits:
            rec["dys"] = [rec.pop("dy%d" % i) for i in range(len(rec["sizes"]))]
        as_numpy = lambda v: np.ascontiguousarray(v.detach().cpu().numpy()) if torch.is_tensor(v) else v      # noqa: E731
        for rec in self.convs + self.blocks + self.cats + self.splits:
            for k, v in rec.items():
                rec[k] = [as_numpy(t) for t in v] if isinstance(v, list) else as_numpy(v)
        self._live, self._made = [], {}
        return self


def hip_targets(capture, conv2d=None, bn_leaky=None, convs=True, routes=False, upsample_concat=None, split_channels=None):
    """The wrappers on orienmask_amd.train's globals (a model with backend='hip'; conv_backend='hip' for the convolutions;
    route_backend='hip' for the route nodes)."""
    t = [(train, "bn_leaky", capture.bn_leaky, bn_leaky)]
    if convs:
        t.append((train, "conv2d", capture.conv2d, conv2d))
    if routes:
        t += [(train, "upsample_concat", capture.upsample_concat, upsample_concat),
              (train, "split_channels", capture.split_channels, split_channels)]
    return t


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


Route = collections.namedtuple("Route", "name inputs scales sizes")     # inputs: the nodes that make them; sizes: channels per part


def expected_nodes(model, num_anchors=3):
    """(names of the ConvBNLeaky blocks, names of all convolutions, the route nodes of a model with route_backend='hip') in
    arch.model_convs / call order."""
    specs = list(arch.model_convs(model, num_anchors, 80))
    cout = {s.name: s.cout for s in specs}
    feat = {idx: "backbone.conv%d.%d.conv.1" % (idx, nblocks) for idx, _, nblocks in arch.DARKNET_STAGES}
    cat4 = ((("skip32.0", "skip16.0", "skip8.0", "skip4"), (8, 4, 2, 1)) if model == "OrienMaskYOLOFPNPlus" else
            (("route8.0", feat[3]), (2, 1)))
    cats = [("cat.neck16", ("route32.0", feat[5]), (2, 1)), ("cat.neck8", ("route16.0", feat[4]), (2, 1)), ("cat.neck4",) + cat4]
    routes = [Route(n, tuple(i), tuple(s), tuple(cout[k] for k in i)) for n, i, s in cats]
    routes.append(Route("split.orien", ("orien_head.5",), None, (2 * num_anchors,) * 3))
    return [s.name for s in specs if s.bn], [s.name for s in specs], routes


def route_mismatches(cap, model):
    """What the recorded route nodes do not share with expected_nodes: names (each once), the nodes that made the inputs, scales and
    channels; a concat must fill the input channels of the convolution it feeds."""
    want = expected_nodes(model)[2]
    got = cap.cats + cap.splits
    out = []
    if [r["name"] for r in got] != [r.name for r in want]:
        return ["route nodes %s, expected %s" % ([r["name"] for r in got], [r.name for r in want])]
    cin = {r["name"]: r["x"].shape[1] for r in cap.convs}
    for rec, r in zip(got, want):
        if "srcs" in rec:
            seen = (tuple(rec["src_names"]), tuple(rec["scales"]), tuple(s.shape[1] for s in rec["srcs"]))
            if seen != (r.inputs, r.scales, r.sizes) or rec["y"].shape[1] != cin.get(r.name[4:] + ".0", sum(r.sizes)):
                out.append("%s: inputs, scales, channels %s, expected %s" % (r.name, seen, (r.inputs, r.scales, r.sizes)))
        else:
            seen = ((rec["x_name"],), tuple(rec["sizes"]), tuple(o.shape[1] for o in rec["outs"]))
            if seen != (r.inputs, r.sizes, r.sizes):
                out.append("%s: input, sizes, channels %s, expected %s" % (r.name, seen, (r.inputs, r.sizes, r.sizes)))
    return out


# ---------------------------------------------------------------------------------------------------------------- re-runs
def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def conv_inputs(rec):
    return dict(x=rec["x"], w=rec["w"], dy=rec["dy"], ksize=rec["ksize"], stride=rec["stride"])


def conv_grad_wants(rec):
    """The gradients the model's own backward produced at this node: none where no dy reached it (a frozen backbone)."""
    if rec["dy"] is None:
        return ()
    return tuple(k for k, on in (("dx", rec["x_requires_grad"]), ("dw", rec["w_requires_grad"]), ("db", rec["b_requires_grad"])) if on)


def conv_wants(rec):
    """What is tied and judged at this node: y where the call asked for forward='hip', and the gradients."""
    return (("y",) if rec["forward"] == "hip" else ()) + conv_grad_wants(rec)


def _to(dev, a):
    return torch.from_numpy(a).to(dev) if a is not None else None


def hip_conv_rerun(dev):
    """rec -> y through om_conv2d_forward (tests/test_conv_fwd.py's _hip) where the record's forward was HIP, and the gradients
    through the C ABI on a workspace of the call's own (pre-filled 0xFF); outputs pre-filled with NaN."""
    def rerun(rec):
        L = omlib.load()
        x, w, b, dy = (_to(dev, rec[k]) for k in ("x", "w", "b", "dy"))
        B, cin, H, W = x.shape
        geom = (B, cin, H, W, w.shape[0], rec["ksize"], rec["stride"])
        shape = (B, w.shape[0]) + G.out_hw(H, W, rec["ksize"], rec["stride"])
        assert dy is None or tuple(dy.shape) == shape, (rec["name"], tuple(dy.shape))
        st = omlib.current_stream_ptr(dev)
        want = conv_wants(rec)
        y = torch.full(shape, float("nan"), device=dev) if "y" in want else None
        if y is not None:
            omlib.check(L.om_conv2d_forward(_vp(x), _vp(w), _vp(b), *geom, _vp(y), st), "om_conv2d_forward")
        ws = torch.full((max(L.om_conv2d_grad_workspace_bytes(*geom), 16),), 255, dtype=torch.uint8, device=dev)
        dx = torch.full_like(x, float("nan")) if "dx" in want else None
        dw = torch.full_like(w, float("nan")) if "dw" in want else None
        db = torch.full((w.shape[0],), float("nan"), device=dev) if "db" in want else None
        if dx is not None:
            omlib.check(L.om_conv2d_grad_input(_vp(dy), _vp(w), *geom, _vp(dx), _vp(ws), ws.numel(), st), "om_conv2d_grad_input")
        if dw is not None or db is not None:
            omlib.check(L.om_conv2d_grad_weight(_vp(x), _vp(dy), *geom, _vp(dw), _vp(db), _vp(ws), ws.numel(), st), "om_conv2d_grad_weight")
        torch.cuda.synchronize(dev)
        return {k: v.cpu().numpy() for k, v in (("y", y), ("dx", dx), ("dw", dw), ("db", db)) if v is not None}
    return rerun


def torch_conv_rerun(rec):
    """rec -> F.conv2d in float32 on the CPU: y where the record's forward was HIP, and the gradients under autograd as the model's
    own backward asks for them."""
    x, w = (torch.from_numpy(rec[k]).clone() for k in ("x", "w"))
    want = conv_grad_wants(rec)
    x.requires_grad_("dx" in want)
    w.requires_grad_("dw" in want)
    b = torch.from_numpy(rec["b"]).clone().requires_grad_("db" in want) if rec["bias"] else None
    y = F.conv2d(x, w, b, rec["stride"], rec["ksize"] // 2)
    if want:
        y.backward(torch.from_numpy(rec["dy"]))
    out = {k: v.grad.numpy() for k, v in (("dx", x), ("dw", w), ("db", b)) if v is not None and v.grad is not None}
    if "y" in conv_wants(rec):
        out["y"] = y.detach().numpy()
    return out


def hip_route_rerun(dev):
    """rec -> a concat's y and source gradients, or the split's outputs and dx, through om_route_concat_forward / _backward on the
    recorded tensors; outputs pre-filled with NaN; a null pointer where the model's node received no gradient or a source takes none."""
    def call(fn, ptrs, chans, scales, B, H, W, whole):
        n = len(chans)
        table = (ctypes.c_void_p * train.ROUTE_MAX)(*[t.data_ptr() if t is not None else None for t in ptrs] + [None] * (train.ROUTE_MAX - n))
        c = (ctypes.c_int * train.ROUTE_MAX)(*list(chans) + [0] * (train.ROUTE_MAX - n))
        s = (ctypes.c_int * train.ROUTE_MAX)(*list(scales) + [0] * (train.ROUTE_MAX - n))
        L, st = omlib.load(), omlib.current_stream_ptr(dev)
        if fn == "forward":
            omlib.check(L.om_route_concat_forward(table, c, s, n, B, H, W, _vp(whole), st), "om_route_concat_forward")
        else:
            omlib.check(L.om_route_concat_backward(_vp(whole), c, s, n, B, H, W, table, st), "om_route_concat_backward")

    def nan(shape):
        return torch.full(tuple(shape), float("nan"), device=dev)

    def rerun(rec):
        if "srcs" in rec:
            srcs, dy = [_to(dev, a) for a in rec["srcs"]], _to(dev, rec["dy"])
            chans, scales = [a.shape[1] for a in rec["srcs"]], rec["scales"]
            B, H, W = rec["srcs"][0].shape[0], rec["srcs"][0].shape[2] * scales[0], rec["srcs"][0].shape[3] * scales[0]
            y = nan((B, sum(chans), H, W))
            call("forward", srcs, chans, scales, B, H, W, y)
            dsrc = [nan(a.shape) if dy is not None and g is not None else None for a, g in zip(rec["srcs"], rec["dsrc"])]
            if any(g is not None for g in dsrc):
                call("backward", dsrc, chans, scales, B, H, W, dy)
            torch.cuda.synchronize(dev)
            return dict(y=y.cpu().numpy(), dsrc=[g.cpu().numpy() if g is not None else None for g in dsrc])
        x, dys = _to(dev, rec["x"]), [_to(dev, a) for a in rec["dys"]]
        B, _, H, W = x.shape
        ones = [1] * len(rec["sizes"])
        outs = [nan((B, c, H, W)) for c in rec["sizes"]]
        call("backward", outs, rec["sizes"], ones, B, H, W, x)
        dx = nan(x.shape) if rec["dx"] is not None and any(d is not None for d in dys) else None
        if dx is not None:
            call("forward", dys, rec["sizes"], ones, B, H, W, dx)
        torch.cuda.synchronize(dev)
        return dict(outs=[o.cpu().numpy() for o in outs], dx=dx.cpu().numpy() if dx is not None else None)
    return rerun


def torch_route_rerun(rec):
    """rec -> the same results from torch's own float32 ops on the CPU."""
    if "srcs" in rec:
        srcs = [torch.from_numpy(a).clone().requires_grad_(g is not None) for a, g in zip(rec["srcs"], rec["dsrc"])]
        y = torch_upsample_concat(srcs, rec["scales"])
        if rec["dy"] is not None and y.requires_grad:
            y.backward(torch.from_numpy(rec["dy"]))
        return dict(y=y.detach().numpy(), dsrc=[t.grad.numpy() if t.grad is not None else None for t in srcs])
    x = torch.from_numpy(rec["x"]).clone().requires_grad_(rec["dx"] is not None)
    outs = torch_split_channels(x, rec["sizes"])
    used = [i for i, d in enumerate(rec["dys"]) if d is not None]
    if used and x.requires_grad:
        torch.autograd.backward([outs[i] for i in used], [torch.from_numpy(rec["dys"][i]) for i in used])
    return dict(outs=[np.ascontiguousarray(o.detach().numpy()) for o in outs], dx=x.grad.numpy() if x.grad is not None else None)


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
        out.update(save_mean=sm[:C].cpu().numpy(), save_invstd=si[:C].cpu().numpy(), rm=rm.cpu().numpy(), rv=rv.cpu().numpy(), nbt=int(nbt))
        if t["dy"] is None:          # no gradient reached the block: the forward alone
            return out
        dx = torch.full_like(t["h"], float("nan"))
        dg, db = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        ws.fill_(255)
        omlib.check(L.om_bn_act_backward(_vp(t["h"]), _vp(t["dy"]), B, C, H, W, _vp(t["gamma"]), _vp(t["beta"]), _vp(sm), _vp(si),
                                         int(training), rec["slope"], _vp(dx), _vp(dg), _vp(db), _vp(ws), ws.numel(), st), "om_bn_act_backward")
        torch.cuda.synchronize(dev)
        out.update(dx=dx.cpu().numpy(), dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())
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
    if rec["dy"] is not None:
        y.backward(torch.from_numpy(rec["dy"]))
    if training:          # save_mean / save_invstd as torch's native op reports them
        sm, si = torch.native_batch_norm(h.detach(), g.detach(), b.detach(), torch.from_numpy(rec["rm0"]).clone(),
                                         torch.from_numpy(rec["rv0"]).clone(), True, rec["momentum"], rec["eps"])[1:]
    else:
        sm, si = rm, (rv.double() + rec["eps"]).rsqrt().float()
    out = dict(y=y.detach().numpy(), y0=y0.detach().numpy(), save_mean=sm.numpy(), save_invstd=si.numpy(), rm=rm.numpy(), rv=rv.numpy(),
               nbt=rec["nbt0"] + int(training))
    if rec["dy"] is not None:
        out.update(dx=h.grad.numpy(), dgamma=g.grad.numpy(), dbeta=b.grad.numpy())
    return out


# ---------------------------------------------------------------------------------------------------------------- (a) the tie
def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(rec, again, keys):
    """The gradients (and outputs) among `keys` that the model's own step and the isolated re-run do not share bit for bit; a block's
    gradient for its residual must be the dy that reached the block."""
    out = [k for k in keys if not same_bits(rec[k], again.get(k))]
    if rec.get("res") is not None and not same_bits(rec["dres"], rec["dy"]):
        out.append("dres")
    return out


def block_tied(rec):
    """BLOCK_TIED; the forward results alone where no gradient reached the block."""
    return BLOCK_TIED if rec["dy"] is not None else ("y", "rm", "rv", "nbt")


def route_quantities(r):
    """A route record or re-run result as {quantity: array or None}: y, dsrc0 ...; out0 ..., dx."""
    if "y" in r:
        return dict([("y", r["y"])] + [("dsrc%d" % i, g) for i, g in enumerate(r["dsrc"])])
    return dict([("out%d" % i, o) for i, o in enumerate(r["outs"])] + [("dx", r["dx"])])


def route_differing(rec, again):
    """The quantities of a route node that the model's own step and the isolated re-run do not share bit for bit (a gradient that
    one of them does not have at all included)."""
    mine, theirs = route_quantities(rec), route_quantities(again)
    return [k for k in mine if not same_bits(mine[k], theirs.get(k))]


def chaining_faults(cap):
    """The nodes are chained by HIP code only, so what a node was handed has the bits of what the node before it returned: a block's
    h and its convolution's y; a concat's source and the block that made it; the split's x and orien_head.5's y."""
    convs, blocks = {r["name"]: r for r in cap.convs}, {r["name"]: r for r in cap.blocks}
    made = dict(convs, **blocks)          # a name that is both is a ConvBNLeaky: its output is the block's
    out = ["%s: h is not the convolution's y" % b["name"] for b in cap.blocks if b["name"] in convs and not same_bits(b["h"], convs[b["name"]]["y"])]
    for r in cap.cats:
        out += ["%s: source %d is not the output of %s" % (r["name"], i, n) for i, (s, n) in enumerate(zip(r["srcs"], r["src_names"]))
                if n not in made or not same_bits(s, made[n]["y"])]
    out += ["%s: x is not the output of %s" % (r["name"], r["x_name"]) for r in cap.splits
            if r["x_name"] not in made or not same_bits(r["x"], made[r["x_name"]]["y"])]
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
        d, want = conv_inputs(rec), conv_grad_wants(rec)
        x, w = (torch.from_numpy(d[k]).double() for k in ("x", "w"))
        s, p = rec["stride"], rec["ksize"] // 2
        truth, norm, yards = {}, {}, []
        if want:
            dy = torch.from_numpy(d["dy"]).double()
            if "dw" in want:
                norm["dw"] = torch.nn.grad.conv2d_weight(x * x, w.shape, dy * dy, stride=s, padding=p).sqrt().numpy()
            if "dx" in want:
                norm["dx"] = torch.nn.grad.conv2d_input(x.shape, w * w, dy * dy, stride=s, padding=p).sqrt().numpy()
            truth, yards = G.truth(d, want), _yardsticks_conv(d, want)
        if "y" in conv_wants(rec):
            f = dict(x=rec["x"], w=rec["w"], bias=rec["b"], ksize=rec["ksize"], stride=rec["stride"])
            truth["y"] = C.truth(f)
            norm["y"] = F.conv2d(x * x, w * w, None, s, p).sqrt().numpy()
            for on in (True, False):
                with torch.backends.mkldnn.flags(enabled=on):
                    yards.append(dict(y=C.yardstick(f)))
        rec["_ref"] = (truth, norm, yards)
    return rec["_ref"]


def judge_conv(rec, got):
    """-> [Score]: y, dx, dw, db by scale; y, dx, dw per element.  The yardstick is the larger error of the float32 evaluations."""
    truth, norm, yards = conv_reference(rec)
    assert sorted(got) == sorted(truth), (rec["name"], sorted(got), sorted(truth))
    out = []
    for k in conv_wants(rec):
        floor = FWD_FLOOR if k == "y" else CONV_FLOOR
        y = max(scale_error(r[k], truth[k]) for r in yards if k in r)
        out.append(Score(rec["name"], k, "scale", scale_error(got[k], truth[k]), y, max(BAR * y, floor)))
        if k in norm:
            y = max(per_element(r[k], truth[k], norm[k]) for r in yards if k in r)
            e = per_element(got[k], truth[k], norm[k]) if got[k].shape == truth[k].shape else float("inf")
            out.append(Score(rec["name"], k, "element", e, y, max(BAR * y, floor)))
    return out


Exact = collections.namedtuple("Exact", "node what check ok detail")     # a check without a tolerance


def _bound(got, dy, chans, scales):
    try:
        return True, "worst error / bound %.3f" % R.within_bound(got, dy, chans, scales)
    except AssertionError as e:
        return False, "outside the sequential-sum bound %s" % (e.args,)


def judge_route(rec, got):
    """-> [Exact].  A concat: y equals route_np.forward and every source gradient route_np.backward bit for bit, and the gradients
    are within route_np.within_bound of the float64 block sums; a source has a gradient exactly where the model's node produced one.
    The split: the outputs are the channel slices of x, dx the concatenation of the recorded dys with exact zeros where an output
    received none (no dx at all where none received any, or x takes none)."""
    name, out = rec["name"], []
    if "srcs" in rec:
        chans, scales = [a.shape[1] for a in rec["srcs"]], rec["scales"]
        B, H, W = rec["srcs"][0].shape[0], rec["srcs"][0].shape[2] * scales[0], rec["srcs"][0].shape[3] * scales[0]
        out.append(Exact(name, "y", "bits", same_bits(got["y"], R.forward(rec["srcs"], chans, scales, B, H, W)), ""))
        want = R.backward(rec["dy"], chans, scales) if rec["dy"] is not None else [None] * len(chans)
        for i, (g, w, mine) in enumerate(zip(got["dsrc"], want, rec["dsrc"])):
            if mine is None or rec["dy"] is None:
                out.append(Exact(name, "dsrc%d" % i, "absent", g is None and mine is None, "a source that takes no gradient"))
            else:
                out.append(Exact(name, "dsrc%d" % i, "bits", same_bits(g, w), "scale %d" % scales[i]))
        if rec["dy"] is not None and any(g is not None for g in got["dsrc"]):
            fits = all(g is None or g.shape == w.shape for g, w in zip(got["dsrc"], want))
            ok, detail = _bound(got["dsrc"], rec["dy"], chans, scales) if fits else (False, "shape")
            out.append(Exact(name, "dsrc", "bound", ok, detail))
        return out
    off = 0
    for i, (o, c) in enumerate(zip(got["outs"], rec["sizes"])):
        out.append(Exact(name, "out%d" % i, "bits", same_bits(o, np.ascontiguousarray(rec["x"][:, off:off + c])), ""))
        off += c
    if rec["dx"] is None or all(d is None for d in rec["dys"]):
        out.append(Exact(name, "dx", "absent", got["dx"] is None and rec["dx"] is None, "no gradient reached the split"))
    else:
        B, _, H, W = rec["x"].shape
        parts = [d if d is not None else np.zeros((B, c, H, W), np.float32) for d, c in zip(rec["dys"], rec["sizes"])]
        out.append(Exact(name, "dx", "bits", same_bits(got["dx"], np.concatenate(parts, axis=1)),
                         "%d outputs without a gradient" % sum(d is None for d in rec["dys"])))
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
    flips = (got["y0"] > 0) != (truth["z"] > 0)
    band = np.abs(truth["z"]) < BAND * np.abs(rec["gamma"]).reshape(1, -1, 1, 1)
    out = {("y", "scale"): scale_error(got["y"], truth["y"]), ("save_mean", "scale"): scale_error(got["save_mean"], truth["mean"]),
           ("save_invstd", "scale"): scale_error(got["save_invstd"], truth["invstd"]),
           ("running_mean", "scale"): scale_error(got["rm"], truth["running_mean"]),
           ("running_var", "scale"): scale_error(got["rv"], truth["running_var"])}
    if rec["dy"] is not None:          # a block that no gradient reached has its forward alone
        dx, dgamma, dbeta = N.backward(rec["h"], rec["dy"], rec["gamma"], truth["mean"], truth["invstd"], got["y0"] > 0, rec["training"],
                                       rec["slope"])
        out.update({("dgamma", "scale"): scale_error(got["dgamma"], dgamma), ("dbeta", "scale"): scale_error(got["dbeta"], dbeta),
                    ("dh", "scale"): scale_error(got["dx"], dx), ("dh", "channel"): per_channel(got["dx"], dx)})
    out.update({("mask", "flips"): float("inf") if (flips & ~band).any() else float(flips.sum()) / flips.size,
                ("nbt", "count"): float(abs(int(got["nbt"]) - (rec["nbt0"] + int(rec["training"]))))})
    return out


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
    if "srcs" in rec:
        return "%dx(%s) %dx%d" % (rec["y"].shape[0], "+".join("%d^%d" % (a.shape[1], s) for a, s in zip(rec["srcs"], rec["scales"])),
                                  rec["y"].shape[2], rec["y"].shape[3])
    if "sizes" in rec:
        return "%dx%d->%s %dx%d" % (rec["x"].shape[:2] + ("+".join(map(str, rec["sizes"])),) + rec["x"].shape[2:])
    return "%s %s%s" % ("x".join(map(str, rec["h"].shape)), "train" if rec["training"] else "eval", " +res" if rec["res"] is not None else "")


def route_line(cid, rec, e, tie=""):
    return "%-18s %-30s %-30s %-12s %-8s %s%s%s" % (cid, e.node, geometry(rec), e.what, e.check, "exact" if e.ok else "DIFFERS",
                                                   "  (%s)" % e.detail if e.detail else "", tie)


def line(cid, rec, s, tie=""):
    return "%-18s %-30s %-30s %-12s %-8s impl %.3g  torch-cpu %.3g  ratio %.2f  of bar %.2f%s" % (
        cid, s.node, geometry(rec), s.grad, s.metric, s.err, s.yard, s.err / max(s.yard, 1e-30), over_bar(s), tie)
