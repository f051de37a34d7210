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

The amp step (a model built with amp='bf16', conv_forward='hip', conv_grad='hip', route_backend='hip'; tests/test_amp_audit.py on
the GPU, tests/test_amp_audit_cpu.py for the harness; the last part of this file).  The wrappers also go on train.conv2d_bf16 and
train.conv_bn_leaky_frozen (hip_targets(amp=True)); a frozen block is one node of its own (Capture.frozen).  A recorded bf16 tensor
is kept as its uint16 bits (rec["bf16"] names the keys that were bf16) and same_bits compares bits of like dtypes, so bf16 against
float32 is a difference, never a cast; tests/bf16_np.py is the only rounding on the CPU side.  No tolerance is added: a bf16
quantity is judged through the identities include/orienmask_hip.h states (amp_conv_findings, amp_block_findings, frozen_findings,
_judge_concat_bf16), and the float32 quantities behind them through judge_conv / judge_block / within_bound unchanged, on the
operands the kernels multiply: widen(x), widen(round_bits(dy)), quantise(w).  amp_chaining_faults adds what only this step has:
backbone.conv1's x is round_bits(image), every other convolution's and frozen block's x the output of the node that made it, and
the six heads leave the model as float32.  The CPU stand-ins (standin_*) have the train functions' signatures and the contracts'
arithmetic.
"""
import collections
import contextlib
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import bf16_np as Q
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


def _as_numpy(v):
    """A tensor as a contiguous numpy array on the host, a bf16 tensor as its uint16 bits (numpy has no bfloat16); anything else as
    it is."""
    if not torch.is_tensor(v):
        return v
    v = v.detach().cpu().contiguous()
    if v.dtype == torch.bfloat16:
        return np.ascontiguousarray(v.view(torch.int16).numpy()).view(np.uint16)
    return np.ascontiguousarray(v.numpy())


def _one(v):
    a, b = (v, v) if isinstance(v, int) else tuple(v)
    assert a == b, v
    return int(a)


class Capture:
    """Records every convolution, every BatchNorm + LeakyReLU block and every route node of one forward and backward of `net`.
    After finish(): convs / blocks / cats / splits are lists of dicts of numpy arrays in call order, keyed as the re-run functions'
    results (a concat's srcs and dsrc, a split's outs and dys are lists with one entry per tensor, None where there is none)."""

    def __init__(self, net):
        self.convs, self.blocks, self.cats, self.splits, self.frozen = [], [], [], [], []
        self.image, self.head_dtypes = None, None          # run_step: the model's input and the element types of the six heads
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

    # -- train.conv2d / F.conv2d / train.conv2d_bf16
    def _conv_before(self, x, weight, bias, stride, padding, forward):
        blockish = self._params[id(weight)].endswith(".conv_block.0.weight")
        rec = dict(name=self._name(weight, ".conv_block.0.weight" if blockish else ".weight"), x=x.detach().clone(),
                   w=weight.detach().clone(), bias=bias is not None, b=bias.detach().clone() if bias is not None else None,
                   forward=forward, stride=_one(stride), ksize=int(weight.shape[2]),
                   x_requires_grad=bool(x.requires_grad), w_requires_grad=bool(weight.requires_grad),
                   b_requires_grad=bool(bias is not None and bias.requires_grad), dx=None, dy=None)
        assert _one(padding) == rec["ksize"] // 2, (rec["name"], padding)
        fed = self._unfed.pop(id(x), None)
        if fed is not None:
            fed["name"] = "cat." + rec["name"].rsplit(".", 1)[0]
        return rec, fed

    def _conv_after(self, rec, weight, bias, y):
        rec["y"] = y.detach().clone()
        self._output(rec, y)
        self.convs.append(rec)
        self._live.append((rec, dict(dw=weight, db=bias)))
        return y

    def conv2d(self, real):
        def wrapper(x, weight, bias=None, stride=1, padding=0, *more, **kw):
            rec, _ = self._conv_before(x, weight, bias, stride, padding, str(kw.get("forward", "torch")))
            return self._conv_after(rec, weight, bias, real(_alias(x, rec, "dx"), weight, bias, stride, padding, *more, **kw))
        return wrapper

    def conv2d_bf16(self, real):
        """train.conv2d_bf16 (amp='bf16', conv_forward='hip'): a convolution record that also names the node that made x (None:
        the image, cast by the block), the output type and the `backward` keyword."""
        def wrapper(x, weight, bias=None, stride=1, padding=0, out_dtype=torch.bfloat16, backward="torch"):
            maker = self._maker(x)
            rec, fed = self._conv_before(x, weight, bias, stride, padding, "hip")
            rec.update(x_name=fed["name"] if fed is not None else maker, out_dtype=str(out_dtype).replace("torch.", ""),
                       backward=str(backward))
            y = real(_alias(x, rec, "dx"), weight, bias, stride, padding, out_dtype=out_dtype, backward=backward)
            assert y.dtype == out_dtype, (rec["name"], y.dtype)
            return self._conv_after(rec, weight, bias, y)
        return wrapper

    # -- train.conv_bn_leaky_frozen
    def conv_bn_leaky_frozen(self, real):
        """A frozen block is one node without a backward: x, w, the BatchNorm's parameters and running statistics, the residual and
        y; the running buffers and num_batches_tracked must be what they were before the call."""
        def wrapper(x, weight, bn, residual=None, stride=1, padding=0, slope=arch.LEAKY_SLOPE):
            rec = dict(name=self._name(weight, ".conv_block.0.weight"), x=x.detach().clone(), x_name=self._maker(x),
                       w=weight.detach().clone(), gamma=bn.weight.detach().clone(), beta=bn.bias.detach().clone(),
                       rm0=bn.running_mean.clone(), rv0=bn.running_var.clone(), nbt0=int(bn.num_batches_tracked), eps=float(bn.eps),
                       momentum=float(bn.momentum), slope=float(slope), res=residual.detach().clone() if residual is not None else None,
                       res_name=self._maker(residual) if residual is not None else None, stride=_one(stride),
                       ksize=int(weight.shape[2]), training=False)
            assert _one(padding) == rec["ksize"] // 2, (rec["name"], padding)
            y = real(x, weight, bn, residual=residual, stride=stride, padding=padding, slope=slope)
            assert torch.equal(bn.running_mean, rec["rm0"]) and torch.equal(bn.running_var, rec["rv0"]) \
                and int(bn.num_batches_tracked) == rec["nbt0"], (rec["name"], "a frozen block touched its BatchNorm's buffers")
            assert not y.requires_grad, rec["name"]
            rec["y"] = y.detach().clone()
            self._made[id(y)] = (rec["name"], y)
            self.frozen.append(rec)
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
        for rec in self.convs + self.blocks + self.cats + self.splits + self.frozen:
            # a bf16 tensor is kept as its uint16 bits; which of the record's tensors were bf16 is remembered here
            rec["bf16"] = tuple(sorted(k for k, v in rec.items() if any(torch.is_tensor(t) and t.dtype == torch.bfloat16
                                                                        for t in (v if isinstance(v, list) else [v]))))
            for k, v in list(rec.items()):
                rec[k] = [_as_numpy(t) for t in v] if isinstance(v, list) else _as_numpy(v)
            if "out_dtype" in rec:        # what the node's contract differentiates with: a float32 head's dy rounded to bf16 once
                rec["dy_bits"] = rec["dy"] if rec["dy"] is None or rec["dy"].dtype == np.uint16 else Q.round_bits(rec["dy"])
        self._live, self._made = [], {}
        return self


def hip_targets(capture, conv2d=None, bn_leaky=None, convs=True, routes=False, upsample_concat=None, split_channels=None, amp=False,
                conv2d_bf16=None, conv_bn_leaky_frozen=None):
    """The wrappers on orienmask_amd.train's globals (a model with backend='hip'; conv_backend='hip' for the convolutions;
    route_backend='hip' for the route nodes; amp: a model with amp='bf16', conv_forward='hip', whose convolutions are
    train.conv2d_bf16 and whose frozen blocks train.conv_bn_leaky_frozen)."""
    t = [(train, "bn_leaky", capture.bn_leaky, bn_leaky)]
    if convs:
        t.append((train, "conv2d", capture.conv2d, conv2d))
    if routes:
        t += [(train, "upsample_concat", capture.upsample_concat, upsample_concat),
              (train, "split_channels", capture.split_channels, split_channels)]
    if amp:
        t += [(train, "conv2d_bf16", capture.conv2d_bf16, conv2d_bf16),
              (train, "conv_bn_leaky_frozen", capture.conv_bn_leaky_frozen, conv_bn_leaky_frozen)]
    return t


def torch_targets(capture):
    """The wrappers on torch.nn.functional (a model with backend='torch', conv_backend='torch')."""
    return [(F, "conv2d", capture.conv2d, None), (F, "batch_norm", capture.batch_norm, None), (F, "leaky_relu", capture.leaky_relu, None)]


def run_step(net, x, targets_of, backward, deterministic=True):
    """One forward and backward of `net` on x under a Capture.  backward(heads): runs the backward from the six heads.  The step
    runs under torch's deterministic-convolution flag unless deterministic=False (a step whose every node is this package's: the
    flag must then be off).  -> Capture."""
    cap = Capture(net)
    assert not x.requires_grad
    with cap.installed(targets_of(cap)), torch.backends.cudnn.flags(deterministic=deterministic):
        assert torch.backends.cudnn.deterministic == deterministic
        heads = [t for pair in net(x) for t in pair]
        cap.image, cap.head_dtypes = _as_numpy(x), [str(t.dtype).replace("torch.", "") for t in heads]
        backward(heads)
        assert torch.backends.cudnn.deterministic == deterministic
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


NAN_BITS = 0x7fc0          # a bf16 NaN: what an output of the bf16 entries is pre-filled with


def bf16_tensor(bits, dev=None):
    """uint16 bits -> the bf16 tensor with those bits (on dev)."""
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16))
    return (t if dev is None else t.to(dev)).view(torch.bfloat16)


def _to(dev, a):
    """A recorded array on the device; uint16 bits as the bf16 tensor they are."""
    if a is None:
        return None
    return bf16_tensor(a, dev) if a.dtype == np.uint16 else torch.from_numpy(a).to(dev)


def _nan(shape, dev, bf16=False):
    if bf16:
        return torch.full(tuple(shape), NAN_BITS, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return torch.full(tuple(shape), float("nan"), device=dev)


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
        assert all(t is None or t.dtype == whole.dtype for t in ptrs)
        sfx = "_bf16" if whole.dtype == torch.bfloat16 else ""          # the entry of the tensors' element type
        if fn == "forward":
            omlib.check(getattr(L, "om_route_concat_forward" + sfx)(table, c, s, n, B, H, W, _vp(whole), st), "om_route_concat_forward" + sfx)
        else:
            omlib.check(getattr(L, "om_route_concat_backward" + sfx)(_vp(whole), c, s, n, B, H, W, table, st), "om_route_concat_backward" + sfx)

    def rerun(rec):
        bf16 = (rec["y"] if "srcs" in rec else rec["x"]).dtype == np.uint16

        def nan(shape):
            return _nan(shape, dev, bf16)

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
            return dict(y=_as_numpy(y), dsrc=[_as_numpy(g) for g in dsrc])
        x, dys = _to(dev, rec["x"]), [_to(dev, a) for a in rec["dys"]]
        B, _, H, W = x.shape
        ones = [1] * len(rec["sizes"])
        outs = [nan((B, c, H, W)) for c in rec["sizes"]]
        call("backward", outs, rec["sizes"], ones, B, H, W, x)
        dx = nan(x.shape) if rec["dx"] is not None and any(d is not None for d in dys) else None
        if dx is not None:
            call("forward", dys, rec["sizes"], ones, B, H, W, dx)
        torch.cuda.synchronize(dev)
        return dict(outs=[_as_numpy(o) for o in outs], dx=_as_numpy(dx))
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
    own, pre-filled 0xFF before each launch sequence.  A record whose h is bf16 bits goes through the _bf16 entries: y, y0 and dx are
    then bits as well, everything else float32."""
    def rerun(rec):
        L = omlib.load()
        t = {k: _to(dev, rec[k]) for k in ("h", "gamma", "beta", "res", "dy", "rm0", "rv0")}
        sfx = "_bf16" if rec["h"].dtype == np.uint16 else ""
        assert all(t[k] is None or t[k].dtype == t["h"].dtype for k in ("res", "dy")), (rec["name"], "activations of two types")
        forward, backward = getattr(L, "om_bn_act_forward" + sfx), getattr(L, "om_bn_act_backward" + sfx)
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
            omlib.check(forward(_vp(t["h"]), B, C, H, W, _vp(t["gamma"]), _vp(t["beta"]), _vp(rm), _vp(rv),
                                            _vp(nbt) if track else None, int(training), rec["momentum"], rec["eps"], rec["slope"], _vp(res),
                                            _vp(y), _vp(sm), _vp(si), _vp(ws), ws.numel(), st), "om_bn_act_forward" + sfx)
            out[key] = _as_numpy(y)
        out.update(save_mean=sm[:C].cpu().numpy(), save_invstd=si[:C].cpu().numpy(), rm=rm.cpu().numpy(), rv=rv.cpu().numpy(), nbt=int(nbt))
        if t["dy"] is None:          # no gradient reached the block: the forward alone
            return out
        dx = torch.full_like(t["h"], float("nan"))
        dg, db = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        ws.fill_(255)
        omlib.check(backward(_vp(t["h"]), _vp(t["dy"]), B, C, H, W, _vp(t["gamma"]), _vp(t["beta"]), _vp(sm), _vp(si),
                                         int(training), rec["slope"], _vp(dx), _vp(dg), _vp(db), _vp(ws), ws.numel(), st), "om_bn_act_backward" + sfx)
        torch.cuda.synchronize(dev)
        out.update(dx=_as_numpy(dx), dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())
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
    made.update((r["name"], r) for r in cap.frozen)
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
    if "srcs" in rec and rec["y"].dtype == np.uint16:
        return _judge_concat_bf16(rec, got)
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


def _judge_concat_bf16(rec, got):
    """A concat of bf16 tensors (om_route_concat_forward_bf16 / _backward_bf16): y is a bit copy of the sources; a source gradient
    equals round_bits of route_np.backward on the widened dy, and that unrounded float32 sum is inside route_np.within_bound."""
    name, out = rec["name"], []
    chans, scales = [a.shape[1] for a in rec["srcs"]], rec["scales"]
    B, H, W = rec["srcs"][0].shape[0], rec["srcs"][0].shape[2] * scales[0], rec["srcs"][0].shape[3] * scales[0]
    copy = R.forward([Q.widen(a) for a in rec["srcs"]], chans, scales, B, H, W)        # values of bf16: round_bits gives the bits back
    out.append(Exact(name, "y", "bits", same_bits(got["y"], Q.round_bits(copy)), "a copy of bf16 bits"))
    dy = Q.widen(rec["dy"]) if rec["dy"] is not None else None
    sums = R.backward(dy, chans, scales) if dy is not None else [None] * len(chans)
    for i, (g, w, mine) in enumerate(zip(got["dsrc"], sums, rec["dsrc"])):
        if mine is None or dy is None:
            out.append(Exact(name, "dsrc%d" % i, "absent", g is None and mine is None, "a source that takes no gradient"))
        else:
            out.append(Exact(name, "dsrc%d" % i, "bits", same_bits(g, Q.round_bits(w)), "scale %d, the float32 block sum rounded once" % scales[i]))
    if dy is not None and any(g is not None for g in got["dsrc"]):
        ok, detail = _bound([w if g is not None else None for g, w in zip(got["dsrc"], sums)], dy, chans, scales)
        out.append(Exact(name, "dsrc", "bound", ok, detail + " (the unrounded sums)"))
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


# ================================================================================================================ amp='bf16'
# The step with amp='bf16', conv_forward='hip', conv_grad='hip', route_backend='hip' (module docstring, last part).  No tolerance of
# its own: a bf16 quantity is judged through the identities include/orienmask_hip.h states (a bf16 output is round_bits of the
# float32 output of the same entry; a _bf16 entry is round_bits of the float32 entry on the widened input), and the float32
# quantities behind them go through judge_conv / judge_block / within_bound unchanged.
def bits_of(t):
    """A bf16 tensor's uint16 bits."""
    assert t.dtype == torch.bfloat16, t.dtype
    return _as_numpy(t)


def _wide(a):
    """A recorded activation as the float32 values the kernels compute with: uint16 bits widened exactly."""
    return Q.widen(a) if a is not None and a.dtype == np.uint16 else a


def amp_conv_as_f32(rec):
    """The float32 convolution record of the operands a bf16 convolution node multiplies (tests/conv_fwd_bf16_np.py,
    tests/conv_grad_bf16_np.py): widen(x), quantise(w), widen(round_bits(dy)); what judge_conv takes.  A frozen block's record gives
    its convolution: no bias, no gradient."""
    if "_f32" not in rec:
        rec["_f32"] = dict(name=rec["name"], x=Q.widen(rec["x"]), w=Q.quantise(rec["w"]), bias=rec.get("bias", False), b=rec.get("b"),
                           dy=_wide(rec.get("dy_bits")), forward="hip", stride=rec["stride"], ksize=rec["ksize"],
                           x_requires_grad=rec.get("x_requires_grad", False), w_requires_grad=rec.get("w_requires_grad", False),
                           b_requires_grad=rec.get("b_requires_grad", False))
    return rec["_f32"]


def block_as_f32(rec):
    """The float32 block record of a bf16 block: h, dy and the residual widened, everything else as recorded."""
    if "_f32" not in rec:
        rec["_f32"] = dict({k: v for k, v in rec.items() if k != "_ref"}, h=_wide(rec["h"]), dy=_wide(rec["dy"]), res=_wide(rec["res"]))
    return rec["_f32"]


def frozen_block_as_f32(rec, h32):
    """The float32 eval-mode block record behind a frozen block: h the float32 convolution output, the residual widened."""
    return dict(name=rec["name"], h=h32, gamma=rec["gamma"], beta=rec["beta"], rm0=rec["rm0"], rv0=rec["rv0"], nbt0=rec["nbt0"],
                training=False, momentum=rec["momentum"], eps=rec["eps"], slope=rec["slope"], res=_wide(rec["res"]), dy=None, dx=None,
                dres=None)


# ---------------------------------------------------------------------------------------------------------------- the contracts on the CPU
def _no_autocast():
    return torch.autocast("cpu", enabled=False)


def amp_conv_math(x_bits, w, b, dy_bits, stride, ksize, want):
    """The arithmetic contract of om_conv2d_bf16_forward / _grad_input / _grad_weight in torch-CPU float32: float32 accumulation on
    widen(x), widen(dy) and quantise(w); y16 / dx16 one round_bits of y32 / dx32; dw and db float32, not rounded.  want: of y, dx,
    dw, db.  -> dict(y32, y16, dx32, dx16, dw, db) of those wanted."""
    out = {}
    with _no_autocast(), torch.no_grad():
        x, wq = Q.widen(x_bits), Q.quantise(w)
        if "y" in want:
            out["y32"] = F.conv2d(torch.from_numpy(x), torch.from_numpy(wq), torch.from_numpy(b) if b is not None else None, stride,
                                  ksize // 2).numpy()
            out["y16"] = Q.round_bits(out["y32"])
        grads = tuple(k for k in ("dx", "dw", "db") if k in want)
        if grads:
            g = G.gradients(dict(x=x, w=wq, dy=Q.widen(dy_bits), stride=stride, ksize=ksize), torch.float32, grads)
            if "dx" in g:
                out["dx32"], out["dx16"] = g["dx"], Q.round_bits(g["dx"])
            out.update((k, g[k]) for k in ("dw", "db") if k in g)
    return out


def cpu_amp_conv_rerun(rec):
    f = amp_conv_as_f32(rec)
    return amp_conv_math(rec["x"], rec["w"], rec.get("b"), rec.get("dy_bits"), rec["stride"], rec["ksize"], conv_wants(f))


def cpu_amp_block_rerun(rec):
    """dict(bf16=, f32=): torch's float32 block on the widened record, and its activations rounded once (the _bf16 entries'
    contract); the float32 outputs are shared."""
    f32 = torch_block_rerun(block_as_f32(rec))
    return dict(f32=f32, bf16=dict(f32, **{k: Q.round_bits(f32[k]) for k in ("y", "y0", "dx") if k in f32}))


def cpu_frozen_rerun(rec, training=False):
    """dict(y, conv, block_rec, block): the float32 convolution of the frozen block, torch's float32 eval-mode block on it with the
    widened residual, and y = round_bits of that block's output (training=True: with batch statistics, which a frozen block must
    never use)."""
    conv = amp_conv_math(rec["x"], rec["w"], None, None, rec["stride"], rec["ksize"], ("y",))
    block_rec = frozen_block_as_f32(rec, conv["y32"])
    block = torch_block_rerun(dict(block_rec, training=training))
    return dict(y=Q.round_bits(block["y"]), conv=conv, block_rec=block_rec, block=block)


def cpu_amp_route_rerun(rec):
    """torch's float32 ops on the widened record, every bf16 quantity rounded once; a float32 record (the split) as it is."""
    bf16 = (rec["y"] if "srcs" in rec else rec["x"]).dtype == np.uint16
    if not bf16:
        return torch_route_rerun(rec)
    rnd = lambda a: Q.round_bits(a) if a is not None else None      # noqa: E731
    if "srcs" in rec:
        r = torch_route_rerun(dict(rec, srcs=[_wide(a) for a in rec["srcs"]], dy=_wide(rec["dy"])))
        return dict(y=rnd(r["y"]), dsrc=[rnd(g) for g in r["dsrc"]])
    r = torch_route_rerun(dict(rec, x=_wide(rec["x"]), dys=[_wide(a) for a in rec["dys"]]))
    return dict(outs=[rnd(o) for o in r["outs"]], dx=rnd(r["dx"]))


# ---------------------------------------------------------------------------------------------------------------- CPU stand-ins
def _rne(t):
    """float32 CPU tensor -> bf16 tensor, rounded by tests/bf16_np.py (the only rounding of the CPU side)."""
    return bf16_tensor(Q.round_bits(t.detach().numpy())).view(t.shape)


def _f32(t):
    """A bf16 CPU tensor widened exactly (bf16_np.widen); a float32 tensor as it is."""
    if t is None or t.dtype == torch.float32:
        return t
    return torch.from_numpy(Q.widen(bits_of(t))).view(t.shape)


class _StandinConv2dBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, f32_out):
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.has_bias = stride, bias is not None
        r = amp_conv_math(bits_of(x), weight.detach().numpy(), bias.detach().numpy() if bias is not None else None, None, stride,
                          int(weight.shape[2]), ("y",))
        return torch.from_numpy(r["y32"]) if f32_out else bf16_tensor(r["y16"])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        # a float32 output's gradient is rounded to bf16 once; a bf16 one is taken as it is
        dy_bits = bits_of(dy) if dy.dtype == torch.bfloat16 else Q.round_bits(dy.numpy())
        want = tuple(k for k, need in zip(("dx", "dw", "db"), ctx.needs_input_grad[:3]) if need and (k != "db" or ctx.has_bias))
        r = amp_conv_math(bits_of(x), weight.detach().numpy(), None, dy_bits, ctx.stride, int(weight.shape[2]), want)
        return (bf16_tensor(r["dx16"]) if "dx16" in r else None, torch.from_numpy(r["dw"]) if "dw" in r else None,
                torch.from_numpy(r["db"]) if "db" in r else None, None, None)


def standin_conv2d_bf16(x, weight, bias=None, stride=1, padding=0, out_dtype=torch.bfloat16, backward="torch"):
    """train.conv2d_bf16's signature and contract (amp_conv_math) on CPU tensors."""
    assert x.dtype == torch.bfloat16 and weight.dtype == torch.float32 and _one(padding) == weight.shape[2] // 2
    return _StandinConv2dBf16.apply(x, weight, bias, _one(stride), out_dtype == torch.float32)


def standin_conv_bn_leaky_frozen(x, weight, bn, residual=None, stride=1, padding=0, slope=arch.LEAKY_SLOPE):
    """train.conv_bn_leaky_frozen's signature and contract on CPU bf16 tensors: cpu_frozen_rerun's y, no autograd node."""
    assert x.dtype == torch.bfloat16 and not x.requires_grad and _one(padding) == weight.shape[2] // 2
    rec = dict(name="?", x=bits_of(x), w=weight.detach().numpy(), gamma=bn.weight.detach().numpy(), beta=bn.bias.detach().numpy(),
               rm0=bn.running_mean.numpy(), rv0=bn.running_var.numpy(), nbt0=int(bn.num_batches_tracked), momentum=float(bn.momentum),
               eps=float(bn.eps), slope=float(slope), res=bits_of(residual) if residual is not None else None, stride=_one(stride),
               ksize=int(weight.shape[2]))
    with _no_autocast():
        return bf16_tensor(cpu_frozen_rerun(rec)["y"])


class _StandinBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, bn, slope):
        training = bool(bn.training or bn.running_mean is None)
        ctx.stats = None if training else (bn.running_mean.clone(), bn.running_var.clone())
        ctx.training, ctx.eps, ctx.slope, ctx.has_residual = training, float(bn.eps), float(slope), residual is not None
        ctx.save_for_backward(x, gamma, beta)
        with _no_autocast():
            y = torch_bn_leaky(_f32(x), bn, _f32(residual), slope)
        return _rne(y) if x.dtype == torch.bfloat16 else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, gamma, beta = ctx.saved_tensors
        assert dy.dtype == x.dtype, (dy.dtype, x.dtype)
        h, g, b = (t.detach().clone().requires_grad_(True) for t in (_f32(x), gamma, beta))
        rm, rv = ctx.stats if ctx.stats is not None else (None, None)
        with _no_autocast(), torch.enable_grad():
            y = F.leaky_relu(F.batch_norm(h, rm, rv, g, b, ctx.training, 0.0, ctx.eps), ctx.slope)
        dh, dg, db = torch.autograd.grad(y, (h, g, b), _f32(dy))
        return _rne(dh) if x.dtype == torch.bfloat16 else dh, dg, db, dy if ctx.has_residual else None, None, None


def standin_bn_leaky(x, bn, residual=None, slope=arch.LEAKY_SLOPE, sync=False, process_group=None):
    """train.bn_leaky's signature with the _bf16 entries' contract on CPU tensors: torch's float32 block on the widened activations,
    y and dx rounded once, everything else float32."""
    assert residual is None or residual.dtype == x.dtype
    return _StandinBNAct.apply(x, bn.weight, bn.bias, residual, bn, slope)


class _StandinConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, *tensors):
        ctx.scales, ctx.shapes, ctx.bf16 = scales, [t.shape for t in tensors], tensors[0].dtype == torch.bfloat16
        with _no_autocast():
            y = torch_upsample_concat([_f32(t) for t in tensors], scales)
        return _rne(y) if ctx.bf16 else y          # a copy: rounding a widened bf16 value gives its bits back

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        srcs = [torch.zeros(s, requires_grad=True) for s in ctx.shapes]
        with _no_autocast(), torch.enable_grad():
            y = torch_upsample_concat(srcs, ctx.scales)
        grads = torch.autograd.grad(y, srcs, _f32(dy).contiguous())
        return (None,) + tuple((_rne(g) if ctx.bf16 else g) if need else None for g, need in zip(grads, ctx.needs_input_grad[1:]))


def standin_upsample_concat(tensors, scales):
    """train.upsample_concat's signature and contract on CPU tensors: a copy; a source gradient is torch-CPU's float32 block sum,
    rounded once where the tensors are bf16."""
    tensors = list(tensors)
    assert all(t.dtype == tensors[0].dtype for t in tensors)
    return _StandinConcat.apply(tuple(int(s) for s in scales), *tensors)


def standin_targets(capture):
    """The CPU stand-ins behind the wrappers of a model with amp='bf16' and all four options on the HIP side."""
    return hip_targets(capture, convs=False, bn_leaky=standin_bn_leaky, routes=True, upsample_concat=standin_upsample_concat,
                       split_channels=torch_split_channels, amp=True, conv2d_bf16=standin_conv2d_bf16,
                       conv_bn_leaky_frozen=standin_conv_bn_leaky_frozen)


# ---------------------------------------------------------------------------------------------------------------- re-runs through the C ABI
def hip_amp_conv_rerun(dev):
    """rec -> y (float32 and bf16 output) through om_conv2d_bf16_forward, dx (both) through om_conv2d_bf16_grad_input, dw and db
    through om_conv2d_bf16_grad_weight on the recorded bits and round_bits(dy); outputs pre-filled with NaN bits, the workspace the
    call's own, filled 0xFF before every launch.  A frozen block's record gives its convolution's y alone."""
    def rerun(rec):
        L = omlib.load()
        x, w, b, dy = (_to(dev, rec.get(k)) for k in ("x", "w", "b", "dy_bits"))
        assert x.dtype == torch.bfloat16 and w.dtype == torch.float32 and (dy is None or dy.dtype == torch.bfloat16)
        B, cin, H, W = x.shape
        geom = (B, cin, H, W, w.shape[0], rec["ksize"], rec["stride"])
        shape = (B, w.shape[0]) + G.out_hw(H, W, rec["ksize"], rec["stride"])
        assert dy is None or tuple(dy.shape) == shape, (rec["name"], tuple(dy.shape))
        st = omlib.current_stream_ptr(dev)
        want = conv_wants(amp_conv_as_f32(rec))
        out = {}
        for key, f32 in (("y32", 1), ("y16", 0)):
            out[key] = _nan(shape, dev, not f32)
            omlib.check(L.om_conv2d_bf16_forward(_vp(x), _vp(w), _vp(b), *geom, _vp(out[key]), f32, st), "om_conv2d_bf16_forward")
        ws = torch.empty((max(L.om_conv2d_bf16_grad_workspace_bytes(*geom), 16),), dtype=torch.uint8, device=dev)
        for key, f32 in (("dx32", 1), ("dx16", 0)) if "dx" in want else ():
            out[key] = _nan(x.shape, dev, not f32)
            ws.fill_(255)
            omlib.check(L.om_conv2d_bf16_grad_input(_vp(dy), _vp(w), *geom, _vp(out[key]), f32, _vp(ws), ws.numel(), st),
                        "om_conv2d_bf16_grad_input")
        if "dw" in want or "db" in want:
            out.update((k, _nan(s, dev)) for k, s in (("dw", w.shape), ("db", (w.shape[0],))) if k in want)
            ws.fill_(255)
            omlib.check(L.om_conv2d_bf16_grad_weight(_vp(x), _vp(dy), *geom, _vp(out.get("dw")), _vp(out.get("db")), _vp(ws), ws.numel(), st),
                        "om_conv2d_bf16_grad_weight")
        torch.cuda.synchronize(dev)
        return {k: _as_numpy(v) for k, v in out.items()}
    return rerun


def hip_amp_block_rerun(dev):
    """rec -> dict(bf16=, f32=): the block through om_bn_act_forward_bf16 / _backward_bf16 on the recorded bits, and through the
    float32 entries on the widened h, dy and residual."""
    rerun = hip_block_rerun(dev)
    return lambda rec: dict(bf16=rerun(rec), f32=rerun(block_as_f32(rec)))


def hip_frozen_rerun(dev):
    """rec -> dict(y, conv, block_rec, block): y through om_conv2d_bf16_frozen_forward alone (pre-filled with NaN bits); the float32
    output of om_conv2d_bf16_forward on the same x and w; om_bn_act_forward in eval mode on that tensor with the widened residual."""
    conv_rerun, block_rerun = hip_amp_conv_rerun(dev), hip_block_rerun(dev)

    def rerun(rec):
        L = omlib.load()
        x, w, res = (_to(dev, rec[k]) for k in ("x", "w", "res"))
        stats = [_to(dev, rec[k]) for k in ("gamma", "beta", "rm0", "rv0")]
        B, cin, H, W = x.shape
        geom = (B, cin, H, W, w.shape[0], rec["ksize"], rec["stride"])
        y = _nan((B, w.shape[0]) + G.out_hw(H, W, rec["ksize"], rec["stride"]), dev, True)
        assert res is None or (res.dtype == torch.bfloat16 and res.shape == y.shape)
        omlib.check(L.om_conv2d_bf16_frozen_forward(_vp(x), _vp(w), *geom, *[_vp(t) for t in stats], rec["eps"], rec["slope"], _vp(res),
                                                    _vp(y), omlib.current_stream_ptr(dev)), "om_conv2d_bf16_frozen_forward")
        torch.cuda.synchronize(dev)
        conv = conv_rerun(rec)
        block_rec = frozen_block_as_f32(rec, conv["y32"])
        return dict(y=_as_numpy(y), conv=conv, block_rec=block_rec, block=block_rerun(block_rec))
    return rerun


# ---------------------------------------------------------------------------------------------------------------- the judges
def _rounding(node, what, bits, f32):
    return Exact(node, what, "rounding", bits is not None and f32 is not None and same_bits(bits, Q.round_bits(f32)),
                 "the bf16 output is round_bits of the float32 output")


def amp_conv_findings(rec, again):
    """-> (the quantities whose tie is broken, [Exact], [Score]).  Tie: the model's own y, dx, dw, db equal the re-run's, the bf16
    variant where the model's tensor is bf16.  One rounding: y16 == round_bits(y32), dx16 == round_bits(dx32).  Float64: y32, dx32,
    dw, db through judge_conv on the operands the kernel multiplies."""
    f = amp_conv_as_f32(rec)
    want = conv_wants(f)
    pick = {k: again.get(("%s32" if rec[k] is not None and rec[k].dtype == np.float32 else "%s16") % k) for k in ("y", "dx")}
    untied = differing(rec, dict(again, **pick), want)
    exact = [_rounding(rec["name"], k, again.get(k + "16"), again.get(k + "32")) for k in ("y", "dx") if k in want]
    got = {k: again.get(k + "32", again.get(k)) for k in want}
    missing = [k for k in want if got[k] is None]
    assert not missing, (rec["name"], "the re-run lacks", missing)
    return untied, exact, judge_conv(f, got)


def amp_block_findings(rec, again):
    """-> (untied, [Exact], [Score]).  Tie to the _bf16 entries; their activations (y, the output without the residual, dx) equal
    round_bits of the float32 entries' on the widened tensors and every float32 output is bit-equal between the two; the float32
    entries' results go through judge_block."""
    lo, hi = again["bf16"], again["f32"]
    untied = differing(rec, lo, block_tied(rec))
    exact = [_rounding(rec["name"], k, lo[k], hi[k]) for k in ("y", "y0", "dx") if k in hi]
    exact += [Exact(rec["name"], k, "bits", same_bits(lo.get(k), hi[k]), "float32 outputs of the bf16 and the float32 entries")
              for k in ("save_mean", "save_invstd", "rm", "rv", "dgamma", "dbeta") if k in hi]
    exact.append(Exact(rec["name"], "nbt", "bits", lo["nbt"] == hi["nbt"], ""))
    return untied, exact, judge_block(block_as_f32(rec), hi)


def frozen_findings(rec, again):
    """-> (untied, [Exact], [Score]).  Tie: the model's y equals the fused entry alone.  Identity: that y equals round_bits of the
    float32 eval-mode block on the float32-output bf16 convolution of the same x and w, residual included.  That convolution and
    that block are judged as every other."""
    untied = [] if same_bits(rec["y"], again["y"]) else ["y"]
    exact = [Exact(rec["name"], "y", "identity", same_bits(again["y"], Q.round_bits(again["block"]["y"])),
                   "round_bits(bn_act eval(conv float32)) with the running statistics"),
             _rounding(rec["name"], "h", again["conv"]["y16"], again["conv"]["y32"])]
    return untied, exact, judge_conv(amp_conv_as_f32(rec), dict(y=again["conv"]["y32"])) + judge_block(again["block_rec"], again["block"])


def amp_chaining_faults(cap):
    """chaining_faults, and what only the amp step has: backbone.conv1's x has the bits of round_bits(image) (the block's cast); the
    x of every other convolution and frozen block the bits of the output of the node that made it (a block, a frozen block, a
    concat); a frozen block's residual those of its maker's output; the six heads that leave the model are float32."""
    out = chaining_faults(cap)
    made = {r["name"]: r for r in cap.convs}
    made.update((r["name"], r) for r in cap.blocks + cap.frozen + cap.cats)
    for r in cap.convs + cap.frozen:
        if r["x_name"] is None:
            if r["name"] != "backbone.conv1" or cap.image is None or not same_bits(r["x"], Q.round_bits(cap.image)):
                out.append("%s: x is not round_bits(image)" % r["name"])
        elif r["x_name"] not in made or not same_bits(r["x"], made[r["x_name"]]["y"]):
            out.append("%s: x is not the output of %s" % (r["name"], r["x_name"]))
    out += ["%s: the residual is not the output of %s" % (r["name"], r["res_name"]) for r in cap.frozen
            if r["res"] is not None and (r["res_name"] not in made or not same_bits(r["res"], made[r["res_name"]]["y"]))]
    if cap.head_dtypes != ["float32"] * 6:
        out.append("the heads leave the model as %s" % (cap.head_dtypes,))
    return out


def amp_audit(cid, cap, model, rerun_conv, rerun_block, rerun_frozen, rerun_route, emit=print):
    """Every node of a captured amp step re-run alone, tied and judged.  -> (failures, {(kind, quantity, metric): worst Score}); one
    line per node, quantity and metric goes to emit."""
    failures, worst = amp_chaining_faults(cap) + route_mismatches(cap, model), {}
    for kind, records in (("conv", cap.convs), ("block", cap.blocks), ("frozen", cap.frozen), ("cat", cap.cats), ("split", cap.splits)):
        for rec in records:
            if kind == "conv":
                untied, exact, scores = amp_conv_findings(rec, rerun_conv(rec))
            elif kind == "block":
                untied, exact, scores = amp_block_findings(rec, rerun_block(rec))
            elif kind == "frozen":
                untied, exact, scores = frozen_findings(rec, rerun_frozen(rec))
            else:
                again = rerun_route(rec)
                untied, exact, scores = route_differing(rec, again), judge_route(rec, again), []
            tie = "  tie " + ("ok" if not untied else "BROKEN: " + ",".join(untied))
            if untied:
                failures.append("%s %s: the model's own %s differ from the isolated re-run's" % (cid, rec["name"], ", ".join(untied)))
            for s in scores:
                text = line(cid, rec, s, tie)
                emit(text)
                if not over_bar(s) <= 1:
                    failures.append(text)
                key = (kind, s.grad, s.metric)
                if key not in worst or over_bar(s) > over_bar(worst[key]):
                    worst[key] = s
            for e in exact:
                text = route_line(cid, rec, e, tie)
                emit(text)
                if not e.ok:
                    failures.append(text)
    return failures, worst
