"""The reference's training loss on the HIP path: ``builder.build(config["loss"], orienmask_amd.train)``.

  OrienMaskYOLOMultiScaleLoss  orienmask_amd.loss's class with the same constructor; when a head requires grad, ``forward``
                               returns a ``loss_sum`` with a ``grad_fn`` whose backward is ``om_loss_backward`` (csrc/loss.hip);
                               ``enqueue`` is the same call without the host copy (the values go to a DeviceEvalCounter)

This is the one-line swap of the reference's trainer/builder.py:34 (``build(config['loss'], evaluation_module)``): the trainer
then does ``loss, loss_log, _ = self.loss(predict, label, training=True)`` and ``loss.backward()`` as before, without the
reference's per-image, per-instance Python target building.

The forward is the values-only path (om_loss plus the host aggregation): loss_log and metric_log are the same, bit for bit.  The
backward follows the reference's autograd chain in torch-CPU's float32 order (csrc/loss.hip) and is ``once_differentiable``.  It
enqueues two kernels on the current stream and never synchronises with the host: the upstream gradient is read on the device.
Each call that builds a graph owns its workspace (the match records om_loss_backward reads) and result vector until the graph is
freed, so several losses may be computed before one ``backward()``.

And the reference's model in training mode: ``builder.build(config["model"], orienmask_amd.train)`` (trainer/builder.py:84).

  ConvBNLeaky                  the reference's Conv -> BatchNorm2d -> LeakyReLU(0.1) block (model/base.py:104-137,278-279) with
                               trainable parameters: torch's convolution, then BatchNorm + LeakyReLU (+ the DarkNet residual add)
                               as om_bn_act_forward / om_bn_act_backward (csrc/bn_act.hip) under autograd
  OrienMaskYOLOFPNPlus         the reference's two models (model/orienmask_yolo_fpnplus.py, model/orienmask_yolo.py) built from
  OrienMaskYOLO                arch.model_convs, with the reference's state_dict keys and parameter order

  convert_sync_batchnorm       the reference's nn.SyncBatchNorm.convert_sync_batchnorm (trainer/builder.py:86) for these blocks: batch
                               statistics over every rank of a process group (om_bn_sync_*: an all-gather of per-channel double
                               records between the block's two phases, merged in rank order on every rank)

  conv2d                       F.conv2d whose input, weight and bias gradients are om_conv2d_grad_input / om_conv2d_grad_weight
                               (csrc/conv_grad.hip, conv_dw.hip); the models use it with conv_backend='hip'.  With forward='hip' the
                               forward is om_conv2d_forward (csrc/conv_fwd.hip) too; the models pass it with conv_forward='hip'

  conv2d_bf16                  the bf16 forward: om_conv2d_bf16_forward (csrc/conv_fwd_bf16.hip) on a bf16 x and the float32 master
                               weight, bf16 or float32 out; the backward is conv2d_bf16_backward: torch's bf16 gradient, or with
                               backward='hip' om_conv2d_bf16_grad_input / om_conv2d_bf16_grad_weight (conv_grad_bf16.hip, conv_dw.hip).
                               The models use it with amp='bf16', conv_forward='hip' (and conv_grad='hip' for the latter)

The forward convolution is torch's with conv_forward='torch' (the default) and om_conv2d_forward with conv_forward='hip', which
needs conv_backend='hip' -- or, under amp='bf16', om_conv2d_bf16_forward with conv_backend='torch'.  Its gradients are torch's with
conv_backend='torch' (the default) and the HIP kernels of csrc/conv_grad.hip and conv_dw.hip with conv_backend='hip' (float32 only).

  conv_bn_leaky_frozen         a frozen block (the models' frozen_stages) as one kernel: the convolution with the fixed affine of the
                               running statistics, LeakyReLU and the residual add in its epilogue (om_conv2d_frozen_forward; on a
                               bf16 x om_conv2d_bf16_frozen_forward); no autograd node, nothing saved

  upsample_concat              torch.cat of nearest-up-sampled tensors (the models' three cat sites) as om_route_concat_forward, with
                               om_route_concat_backward (csrc/route.hip) as its backward
  split_channels               torch.split along the channels into dense tensors: the same two kernels with the roles swapped

The up-sampling, cat and split are torch ops with route_backend='torch' (the default) and these two functions with
route_backend='hip', which is independent of the other three options.

Mixed precision: amp='bf16' on a model or a block (default None: float32 throughout).  The forward then runs under
torch.autocast(dtype=torch.bfloat16): torch's convolutions produce bf16, and bn_leaky, upsample_concat and split_channels take and
return bf16 through the _bf16 entry points of csrc/bn_act.hip and csrc/route.hip (the saved x, dy and dx are bf16 too).  Parameters,
their gradients, the BatchNorm statistics and buffers, the heads the model returns, the loss and the optimizer stay float32, so
state_dicts move freely between amp and float32 models.  With amp, conv_forward='hip' (and conv_backend='torch') makes every forward
convolution this package's: conv2d_bf16 in the blocks and the heads (the heads float32 straight from the accumulators), the fused
bf16 kernel in frozen blocks; the first layer's float32 image is cast to bf16 once, as autocast does.  The forward then repeats bit
for bit without cudnn.deterministic.  amp excludes conv_backend='hip': the float32 gradient kernels take float32 operands only.
conv_grad='hip' (default 'torch'; needs amp='bf16', conv_forward='hip', conv_backend='torch') makes the gradients of those
convolutions the bf16 kernels of csrc/conv_grad_bf16.hip and conv_dw.hip: every convolution node of a step is then this package's, and a
whole trainer step repeats bit for bit without cudnn.deterministic, as the float32 path (conv_backend='hip', conv_forward='hip') does.
"""
import contextlib
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable
from torch.nn.modules.batchnorm import _BatchNorm

from . import lib as _lib
from . import pack as _pack
from .arch import DARKNET_STAGES, LEAKY_SLOPE, model_convs
from .loss import DeviceEvalCounter, EvalCounter, OrienMaskYOLOMultiScaleLoss as _ValuesLoss

__all__ = ["OrienMaskYOLOMultiScaleLoss", "EvalCounter", "DeviceEvalCounter", "ConvBNLeaky", "bn_leaky", "conv2d", "OrienMaskYOLOFPNPlus", "OrienMaskYOLO",
           "convert_sync_batchnorm", "upsample_concat", "split_channels", "conv_bn_leaky_frozen", "conv2d_bf16"]

BACKENDS = ("hip", "torch")
CONV_BACKENDS = ("torch", "hip")
CONV_FORWARDS = ("torch", "hip")
CONV_GRADS = ("torch", "hip")
ROUTE_BACKENDS = ("torch", "hip")
ROUTE_SCALES = (1, 2, 4, 8)
ROUTE_MAX = 4
AMP = (None, "bf16")
ACT_DTYPES = (torch.float32, torch.bfloat16)       # what the BatchNorm block and the routes take


def _check_backends(backend, conv_backend, conv_forward, route_backend="torch", amp=None, conv_grad="torch"):
    """The option strings of a block and of a model (a block has no route_backend: the default passes).  conv_grad is a key of its
    own, not a meaning of conv_backend 'hip' under amp, because that combination is pinned to raise."""
    if amp not in AMP:
        raise ValueError("amp must be one of %s, got %r" % (AMP, amp))
    if amp is not None and conv_backend == "hip":
        raise ValueError("amp %r with conv_backend 'hip' (conv_forward %r): the gradient kernels take float32 operands only.  With "
                         "amp the available combinations are conv_backend 'torch' with conv_forward 'torch' (torch's bf16 "
                         "convolutions) or conv_forward 'hip' (the bf16 forward kernel, torch's bf16 gradients; with conv_grad "
                         "'hip' the bf16 gradient kernels)" % (amp, conv_forward))
    for name, value, known in (("backend", backend, BACKENDS), ("conv_backend", conv_backend, CONV_BACKENDS),
                               ("conv_forward", conv_forward, CONV_FORWARDS), ("route_backend", route_backend, ROUTE_BACKENDS),
                               ("conv_grad", conv_grad, CONV_GRADS)):
        if value not in known:
            raise ValueError("%s must be one of %s, got %r" % (name, known, value))
    if conv_forward == "hip" and conv_backend != "hip" and amp is None:
        raise ValueError("conv_forward 'hip' requires conv_backend 'hip' (float32) or amp 'bf16' with conv_backend 'torch' (the bf16 "
                         "forward kernel), got conv_backend %r without amp: torch's gradient node under the float32 HIP forward is "
                         "not supported" % (conv_backend,))
    if conv_grad == "hip" and not (amp == "bf16" and conv_forward == "hip" and conv_backend == "torch"):
        raise ValueError("conv_grad 'hip' (the bf16 gradient kernels) requires amp 'bf16' with conv_forward 'hip' and conv_backend "
                         "'torch', got amp %r, conv_forward %r, conv_backend %r" % (amp, conv_forward, conv_backend))


class _LossBackward(torch.autograd.Function):
    """forward(ctx, call, *heads) -> loss_sum; ``call`` holds what om_loss read and wrote (the values path's prepare)."""

    @staticmethod
    def forward(ctx, call, *heads):
        ctx.call = call
        ctx.save_for_backward(*heads)                  # autograd's version check: a head changed in place before backward raises
        out, call.loss_sum = call.loss_sum, None       # the graph holds the call, the call must not hold the graph's output
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        ctx.saved_tensors                              # raises if a head was modified in place since the forward
        call = ctx.call
        grads = call.backward(grad_out)
        return (None,) + tuple(grads)


class _Call:
    """One forward's inputs, workspace and result vector (what the values path's prepare bound), kept alive by the autograd graph."""

    def __init__(self, loss, wants, run):
        self.loss, self.wants = loss, wants
        self.read, self.target, self.B, self.N, self.ws, self.result = run.heads, run.target, run.B, run.N, run.ws, run.result
        self.sw = [float(v) for v in loss.scales_weight[:len(self.read)]]
        self.loss_sum = None

    def bind(self, grad_out):
        """The gradient tensors and a callable that enqueues om_loss_backward into them on the current stream."""
        dev = self.result.device
        g = grad_out.detach().to(device=dev, dtype=torch.float32).reshape(()).contiguous()
        # gradients with the heads' shapes and strides; every element is written by the kernels
        gb = [torch.empty_like(b) for b, _ in self.read]
        go = [torch.empty_like(o) for _, o in self.read]
        S = len(self.read)
        cfg = self.loss.cfg_struct(self.read)
        ptrs = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts] + [None] * (3 - S))      # noqa: E731
        _, _, gt_index, gt_mask = self.target
        args = (ctypes.byref(cfg), ptrs([b for b, _ in self.read]), ptrs([o for _, o in self.read]), self.B,
                gt_index.data_ptr(), gt_mask.data_ptr(), self.N, self.result.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                g.data_ptr(), (ctypes.c_float * 3)(*self.sw + [0.0] * (3 - S)), ptrs(gb), ptrs(go))

        def run():
            _lib.launch("om_loss_backward", dev, *args)
            run.keep = (cfg, g)
        return run, gb, go

    def backward(self, grad_out):
        run, gb, go = self.bind(grad_out)
        run()
        out = []
        for s, (wb, wo) in enumerate(self.wants):
            out.append(gb[s] if wb else None)
            out.append(go[s] if wo else None)
        return out


class OrienMaskYOLOMultiScaleLoss(_ValuesLoss):
    """orienmask_amd.loss.OrienMaskYOLOMultiScaleLoss with a backward.  Heads without grad take the values-only path."""

    def forward(self, predict, target, training=True):
        """Returns (loss_sum, loss_log, metric_log) as the values-only class does; loss_sum has a grad_fn when any head requires
        grad (and grad mode is on)."""
        flat = self._wants_graph(predict)
        if flat is None:
            # no graph to build (no head requires grad, or grad mode is off): the values-only path
            return super().forward([(b.detach(), o.detach()) for b, o in predict], target, training)
        run = self._bind_own(predict, target)
        loss_sum, loss_log, metric_log = self._finish(run(), training, run.result.device)
        return self._attach(predict, flat, run, loss_sum), loss_log, metric_log

    def enqueue(self, predict, target, counter, step, training=True):
        """The values-only class's deferred call (om_loss, om_loss_accumulate into `counter`, no host copy); the device scalar it
        returns has the same grad_fn as forward's loss_sum when any head requires grad, so ``enqueue(...).backward()`` is
        ``forward(...)[0].backward()``."""
        flat = self._wants_graph(predict)
        if flat is None:
            return super().enqueue([(b.detach(), o.detach()) for b, o in predict], target, counter, step, training)
        run = self._bind_own(predict, target)
        loss_sum = counter.accumulate(run(), step, with_metrics=training is not True)
        return self._attach(predict, flat, run, loss_sum)

    def _wants_graph(self, predict):
        """The heads as a flat list when a graph is to be built (a head requires grad and grad mode is on), else None."""
        if len(predict) != self.num_scales:
            raise ValueError("predict has %d scales, the loss was built for %d" % (len(predict), self.num_scales))
        flat = [t for pair in predict for t in pair]
        if not (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in flat)):
            return None
        for t in flat:
            if isinstance(t, torch.Tensor) and t.requires_grad and t.dtype != torch.float32:
                raise _lib.OrienMaskHipError("the HIP loss takes float32 heads, got %s" % t.dtype)
        return flat

    def _bind_own(self, predict, target):
        """prepare() on dense detached heads with a workspace of this call's own."""
        dense = []
        for b, o in predict:
            # the gradient is written through the strides the kernels read: heads that are not dense are read from a copy
            b, o = b.detach(), o.detach()
            if torch.empty_like(b, device="meta").stride() != b.stride():
                b = b.contiguous()
            if torch.empty_like(o, device="meta").stride() != o.stride():
                o = o.contiguous()
            dense.append((b, o))
        B, dev = dense[0][0].shape[0], dense[0][0].device
        N = int(target[0].shape[0])
        # a workspace of this call's own: a later call must not overwrite the match records this graph's backward reads
        ws = torch.empty(self.workspace_bytes(B, N), dtype=torch.uint8, device=dev)
        return self.prepare(dense, target, workspace=ws)

    def _attach(self, predict, flat, run, loss_sum):
        call = _Call(self, [(b.requires_grad, o.requires_grad) for b, o in predict], run)
        call.loss_sum = loss_sum
        return _LossBackward.apply(call, *flat)


# ---------------------------------------------------------------------------------------------------------------- the model
_WORKSPACES = {}
_NO_SWITCH = contextlib.nullcontext()


def _workspace(dev, stream, nbytes):
    """The partial-sum workspace of (device, stream): the second launch of a call consumes what the first wrote, and calls on one
    stream are ordered, so a stream's calls share one grow-only buffer; another stream has its own."""
    key = (dev, stream.value)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
        _WORKSPACES[key] = ws
    return ws


def _sfx(t):
    """The entry points' suffix for t's element type: the float32 ones have none."""
    return "_bf16" if t.dtype == torch.bfloat16 else ""


def _autocast(amp, x):
    """The context a forward with `amp` runs under: torch.autocast to bf16 on x's device type, nothing without amp or inside one."""
    kind = x.device.type
    if amp is None or (torch.is_autocast_enabled(kind) and torch.get_autocast_dtype(kind) == torch.bfloat16):
        return _NO_SWITCH
    return torch.autocast(kind, dtype=torch.bfloat16)


def _bn_scratch(x):
    """(stream, workspace) of an om_bn_act_* / om_bn_sync_* call on x's device and current stream."""
    stream = _lib.current_stream_ptr(x.device)
    return stream, _workspace(x.device, stream, _lib.load().om_bn_act_workspace_bytes(*x.shape))


def _bn_forward_buffers(x):
    """y, and save_mean | save_invstd (include/orienmask_hip.h) as one buffer of 4C floats."""
    return torch.empty_like(x), torch.empty(4 * x.shape[1], dtype=torch.float32, device=x.device)


def _bn_backward_buffers(ctx, x, dy):
    """dy contiguous, dx where the input needs a gradient, and dgamma | dbeta as one [2, C] buffer."""
    if dy.dtype != x.dtype:
        raise _lib.OrienMaskHipError("the BatchNorm block's output gradient is %s, its input %s: there is no cast" % (dy.dtype, x.dtype))
    dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    return dy.contiguous(), dx, torch.empty((2, x.shape[1]), dtype=torch.float32, device=x.device)


def _bn_grads(ctx, dx, dgb, dy):
    """The gradients of (x, gamma, beta, residual) and None for the rest of forward's arguments."""
    return (dx, dgb[0] if ctx.needs_input_grad[1] else None, dgb[1] if ctx.needs_input_grad[2] else None,
            dy if ctx.has_residual and ctx.needs_input_grad[3] else None) + (None,) * (len(ctx.needs_input_grad) - 4)


class _BNAct(torch.autograd.Function):
    """forward(ctx, x, gamma, beta, residual, bn, slope) -> leaky(batch_norm(x)) (+ residual): om_bn_act_forward.  `bn` is the
    nn.BatchNorm2d whose buffers the kernel updates in training mode and reads in eval mode.  x (and residual) float32, or bf16
    through the _bf16 entry points: y, dy and dx then are bf16, everything else stays float32.  Saved for the backward: x, gamma, beta
    and one per-channel buffer the forward wrote (save_mean and save_invstd, 2C floats each); the LeakyReLU mask is recomputed from
    x (om_bn_act_backward)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, bn, slope):
        B, C, H, W = x.shape
        training = bool(bn.training or bn.running_mean is None)
        y, save = _bn_forward_buffers(x)
        track = training and bn.running_mean is not None
        stream, ws = _bn_scratch(x)
        _lib.launch("om_bn_act_forward" + _sfx(x), x.device, x, B, C, H, W, gamma, beta, bn.running_mean, bn.running_var,
                    bn.num_batches_tracked if track else None, 1 if training else 0, float(bn.momentum), float(bn.eps),
                    float(slope), residual, y, save.data_ptr(), save.data_ptr() + 8 * C, ws, ws.numel(), stream=stream)
        ctx.save_for_backward(x, gamma, beta, save)
        ctx.training, ctx.slope, ctx.has_residual = training, float(slope), residual is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma, beta, save = ctx.saved_tensors
        B, C, H, W = x.shape
        dy, dx, dgb = _bn_backward_buffers(ctx, x, dy)
        stream, ws = _bn_scratch(x)
        _lib.launch("om_bn_act_backward" + _sfx(x), x.device, x, dy, B, C, H, W, gamma, beta, save.data_ptr(), save.data_ptr() + 8 * C,
                    1 if ctx.training else 0, ctx.slope, dx, dgb.data_ptr(), dgb.data_ptr() + 4 * C, ws, ws.numel(), stream=stream)
        return _bn_grads(ctx, dx, dgb, dy)


def _conv_grads_hip(dy, x, weight, stride, need_x, need_w, need_b):
    """(dx, dw, db) of a convolution of x (float32 or bf16: the entry points of _sfx(x)) with the float32 weight, on the current
    stream, into torch.empty outputs, with the grow-only workspace of the device and stream; None for a gradient that is not
    needed: no input-gradient launch for an input that needs none, no weight-gradient launch where neither dw nor db is needed.
    dx has x's type, dw and db are float32."""
    B, cin, H, W = x.shape
    cout, ks = weight.shape[0], weight.shape[2]
    dev, sfx = x.device, _sfx(x)
    dx = torch.empty_like(x) if need_x else None
    dw = torch.empty_like(weight) if need_w else None
    db = torch.empty(cout, dtype=torch.float32, device=dev) if need_b else None
    stream = _lib.current_stream_ptr(dev)
    geom = (B, cin, H, W, cout, ks, stride)
    dx_is_f32 = (0,) if sfx else ()                 # the bf16 entry's extra argument: dx is bf16
    with _lib.on_device(dev):
        ws = _workspace(dev, stream, getattr(_lib.load(), "om_conv2d%s_grad_workspace_bytes" % sfx)(*geom))
        if need_x:
            _lib.launch("om_conv2d%s_grad_input" % sfx, dev, dy, weight, *geom, dx, *dx_is_f32, ws, ws.numel(), stream=stream)
        if need_w or need_b:
            _lib.launch("om_conv2d%s_grad_weight" % sfx, dev, x, dy, *geom, dw, db, ws, ws.numel(), stream=stream)
    return dx, dw, db


class _Conv2d(torch.autograd.Function):
    """forward(ctx, x, weight, bias, stride, hip_forward) -> F.conv2d(x, weight, bias, stride, ksize // 2), or with hip_forward
    the same convolution as om_conv2d_forward (csrc/conv_fwd.hip) into a torch.empty output.  Saved for the backward either way: x
    and the weight, what torch's own node saves.  The backward enqueues om_conv2d_grad_input and om_conv2d_grad_weight (csrc/conv_grad.hip,
    conv_dw.hip) on the current stream for the gradients that are needed: no input gradient for an input that needs none, no weight gradient for
    a frozen weight; the bias gradient comes from the weight-gradient call."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, hip_forward=False):
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.has_bias = stride, bias is not None
        if not hip_forward:
            return F.conv2d(x, weight, bias, stride, weight.shape[2] // 2)
        B, cin, H, W = x.shape
        cout, ks = weight.shape[0], weight.shape[2]
        pad = ks // 2
        dev = x.device
        y = torch.empty((B, cout, (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1), dtype=torch.float32, device=dev)
        _lib.launch("om_conv2d_forward", dev, x, weight, bias, B, cin, H, W, cout, ks, stride, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        return _conv_grads_hip(dy.contiguous(), x, weight, ctx.stride, need_x, need_w, need_b) + (None, None)


def _require_nchw(t, who, what, dtypes=(torch.float32,)):
    """`what` (as lib.require_cuda_tensor names it) is a CUDA NCHW-contiguous [B,C,H,W] tensor of one of `dtypes`, or `who` refuses
    it."""
    _lib.require_cuda_tensor(t, what, t.dtype if isinstance(t, torch.Tensor) and t.dtype in dtypes else dtypes[0])
    if t.dim() != 4 or not t.is_contiguous():
        raise _lib.OrienMaskHipError("%s takes NCHW-contiguous [B,C,H,W] activations, got strides %s for shape %s"
                                     % (who, t.stride(), tuple(t.shape)))


def _require_residual(residual, shape, dev, dtype=torch.float32):
    """None, or a CUDA NCHW-contiguous tensor of the block's element type and output shape on the block's device."""
    if residual is None:
        return
    _lib.require_cuda_tensor(residual, "residual", dtype)
    if tuple(residual.shape) != tuple(shape) or not residual.is_contiguous() or residual.device != dev:
        raise _lib.OrienMaskHipError("residual must be NCHW-contiguous with the block's output shape %s on %s, got %s strides %s on %s"
                                     % (tuple(shape), dev, tuple(residual.shape), residual.stride(), residual.device))


def _pair_of(v, what):
    a, b = (v, v) if isinstance(v, int) else tuple(v)
    if a != b:
        raise _lib.OrienMaskHipError("conv2d: %s %r must be the same along both axes" % (what, v))
    return int(a)


def _conv_geometry(who, x, weight, stride, padding):
    """(ksize, stride, padding) of a convolution of x with a contiguous [cout,cin,k,k] weight, one of the three geometries."""
    if weight.dim() != 4 or not weight.is_contiguous() or weight.shape[1] != x.shape[1] or weight.shape[2] != weight.shape[3]:
        raise _lib.OrienMaskHipError("%s: weight must be contiguous [cout,%d,k,k], got %s strides %s"
                                     % (who, x.shape[1], tuple(weight.shape), weight.stride()))
    ks, s, p = int(weight.shape[2]), _pair_of(stride, "stride"), _pair_of(padding, "padding")
    if (ks, s, p) not in ((1, 1, 0), (3, 1, 1), (3, 2, 1)):
        raise _lib.OrienMaskHipError("%s: kernel %d stride %d padding %d; the geometries are 1x1 stride 1 padding 0, 3x3 stride 1 "
                                     "padding 1 and 3x3 stride 2 padding 1" % (who, ks, s, p))
    return ks, s, p


def conv2d(x, weight, bias=None, stride=1, padding=0, forward="torch"):
    """F.conv2d(x, weight, bias, stride, padding) with the gradients as HIP kernels (csrc/conv_grad.hip, conv_dw.hip).  x, weight and bias
    CUDA float32, x NCHW-contiguous [B,cin,H,W], weight contiguous [cout,cin,k,k]; the geometry one of 1x1 stride 1 padding 0, 3x3
    stride 1 padding 1, 3x3 stride 2 padding 1, without dilation or groups.  Anything else raises: there is no fallback.
    forward 'torch' (default): the forward is F.conv2d.  forward 'hip': it is om_conv2d_forward (csrc/conv_fwd.hip), enqueued on
    the current stream and bit-identical from run to run; the backward and what it reads are the same, so for the same (x, weight,
    dy) the gradients have the same bits under either forward."""
    if forward not in CONV_FORWARDS:
        raise ValueError("forward must be one of %s, got %r" % (CONV_FORWARDS, forward))
    _require_nchw(x, "conv_backend 'hip'", "the convolution input (conv_backend 'hip')")
    _lib.require_cuda_tensor(weight, "the convolution weight (conv_backend 'hip')", torch.float32)
    if bias is not None:
        _lib.require_cuda_tensor(bias, "the convolution bias (conv_backend 'hip')", torch.float32)
    ks, s, p = _conv_geometry("conv2d", x, weight, stride, padding)
    if bias is not None and (tuple(bias.shape) != (weight.shape[0],) or not bias.is_contiguous()):
        raise _lib.OrienMaskHipError("conv2d: bias must be contiguous [%d], got %s" % (weight.shape[0], tuple(bias.shape)))
    return _Conv2d.apply(x, weight, bias, s, forward == "hip")


def _out_shape(x, cout, ks, s, p):
    B, _, H, W = x.shape
    return (B, cout, (H + 2 * p - ks) // s + 1, (W + 2 * p - ks) // s + 1)


def conv2d_bf16_backward(dy, x, weight, stride, padding, has_bias, needs, backend="torch"):
    """The gradients of conv2d_bf16.  dy and x bf16, weight the float32 master weight; `needs` = (x, weight, bias) as
    ctx.needs_input_grad gives them.  Returns (dx bf16, dw float32, db float32), None for a gradient that is not needed (or a bias
    that does not exist): it is not computed.
    backend 'torch' (default): torch's bf16 convolution gradient, aten.convolution_backward(dy, x, weight.to(bfloat16)), which is
    what F.conv2d under torch.autocast(dtype=bfloat16) leaves behind its weight cast.  Runs on CPU tensors too.
    backend 'hip': om_conv2d_bf16_grad_input / om_conv2d_bf16_grad_weight (csrc/conv_grad_bf16.hip, conv_dw.hip) on the current stream,
    into torch.empty outputs, with the grow-only workspace of the device and stream; CUDA NCHW-contiguous tensors only.  The weight is
    rounded to bf16 inside the kernel, as the forward rounds it; the same bits on every run."""
    if backend not in CONV_GRADS:
        raise ValueError("backend must be one of %s, got %r" % (CONV_GRADS, backend))
    need_x, need_w, need_b = bool(needs[0]), bool(needs[1]), bool(has_bias and needs[2])
    if not (need_x or need_w or need_b):
        return None, None, None
    cout = weight.shape[0]
    if backend == "hip":
        _require_nchw(dy, "conv2d_bf16_backward", "the output gradient (conv2d_bf16_backward)", (torch.bfloat16,))
        _require_nchw(x, "conv2d_bf16_backward", "the convolution input (conv2d_bf16_backward)", (torch.bfloat16,))
        _lib.require_cuda_tensor(weight, "the convolution weight (conv2d_bf16_backward)", torch.float32)
        ks, s, p = _conv_geometry("conv2d_bf16_backward", x, weight, stride, padding)
        dev = x.device
        if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or tuple(dy.shape) != _out_shape(x, cout, ks, s, p) \
                or dy.device != dev or weight.device != dev:
            raise _lib.OrienMaskHipError("conv2d_bf16_backward: dy %s %s on %s for x %s %s on %s, weight %s on %s"
                                         % (tuple(dy.shape), dy.dtype, dy.device, tuple(x.shape), x.dtype, dev, tuple(weight.shape),
                                            weight.device))
        return _conv_grads_hip(dy, x, weight, s, need_x, need_w, need_b)
    dx, dw, db = torch.ops.aten.convolution_backward(dy, x, weight.to(torch.bfloat16), [cout] if has_bias else None, [stride, stride],
                                                     [padding, padding], [1, 1], False, [0, 0], 1, [need_x, need_w, need_b])
    return (dx if need_x else None, dw.float() if need_w else None, db.float() if need_b else None)


class _Conv2dBf16(torch.autograd.Function):
    """forward(ctx, x, weight, bias, stride, padding, f32_out, backward) -> om_conv2d_bf16_forward (csrc/conv_fwd_bf16.hip) into a
    torch.empty output of bf16 or float32.  Saved: x and the float32 weight (the kernel rounds it while staging; nothing else exists
    to save).  The backward is conv2d_bf16_backward (backend `backward`) on a bf16 dy (a float32 output's gradient is rounded to bf16 once, as
    autocast's cast node does behind a .float())."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, f32_out, backward="torch"):
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.padding, ctx.has_bias, ctx.backward_backend = stride, padding, bias is not None, backward
        cout, ks = int(weight.shape[0]), int(weight.shape[2])
        B, cin, H, W = x.shape
        y = torch.empty(_out_shape(x, cout, ks, stride, padding), dtype=torch.float32 if f32_out else torch.bfloat16, device=x.device)
        _lib.launch("om_conv2d_bf16_forward", x.device, x, weight, bias, B, cin, H, W, cout, ks, stride, y, 1 if f32_out else 0)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        if ctx.backward_backend == "torch":         # positional only: unchanged for callers that wrap the function with (*args)
            grads = conv2d_bf16_backward(dy, x, weight, ctx.stride, ctx.padding, ctx.has_bias, ctx.needs_input_grad[:3])
        else:
            grads = conv2d_bf16_backward(dy, x, weight, ctx.stride, ctx.padding, ctx.has_bias, ctx.needs_input_grad[:3],
                                         backend=ctx.backward_backend)
        return grads + (None, None, None, None)


def conv2d_bf16(x, weight, bias=None, stride=1, padding=0, out_dtype=torch.bfloat16, backward="torch"):
    """F.conv2d(x, weight.to(bfloat16), bias, stride, padding) with float32 accumulation as om_conv2d_bf16_forward
    (csrc/conv_fwd_bf16.hip): x CUDA bf16 NCHW-contiguous, weight (contiguous [cout,cin,k,k]) and bias CUDA float32 -- the master
    parameters, which the kernel rounds to bf16 (nearest even) while staging, as autocast's cast does; the geometries of conv2d.
    out_dtype torch.bfloat16 (default) or torch.float32: both are the same float32 accumulators plus the bias, the bf16 output
    rounded once.  Bit-identical from run to run and independent of the batch.  The backward is conv2d_bf16_backward with backend
    `backward`: 'torch' (default) torch's bf16 gradient, 'hip' the kernels of csrc/conv_grad_bf16.hip (bit-identical from run to
    run); dx bf16, dw and db float32, only those that are needed.  Anything else raises: there is no fallback."""
    if backward not in CONV_GRADS:
        raise ValueError("backward must be one of %s, got %r" % (CONV_GRADS, backward))
    if out_dtype not in ACT_DTYPES:
        raise ValueError("out_dtype must be one of %s, got %r" % (ACT_DTYPES, out_dtype))
    _require_nchw(x, "conv2d_bf16", "the convolution input (conv2d_bf16)", (torch.bfloat16,))
    _lib.require_cuda_tensor(weight, "the convolution weight (conv2d_bf16)", torch.float32)
    if bias is not None:
        _lib.require_cuda_tensor(bias, "the convolution bias (conv2d_bf16)", torch.float32)
    ks, s, p = _conv_geometry("conv2d_bf16", x, weight, stride, padding)
    if bias is not None and (tuple(bias.shape) != (weight.shape[0],) or not bias.is_contiguous()):
        raise _lib.OrienMaskHipError("conv2d_bf16: bias must be contiguous [%d], got %s" % (weight.shape[0], tuple(bias.shape)))
    if weight.device != x.device or (bias is not None and bias.device != x.device):
        raise _lib.OrienMaskHipError("conv2d_bf16: x on %s, weight on %s" % (x.device, weight.device))
    return _Conv2dBf16.apply(x, weight, bias, s, p, out_dtype == torch.float32, backward)


def _require_no_grad(what, **tensors):
    """A frozen layer has no backward: under grad mode nothing it reads may require grad."""
    if not torch.is_grad_enabled():
        return
    for name, t in tensors.items():
        if t is not None and t.requires_grad:
            raise _lib.OrienMaskHipError("%s: %s requires grad, but a frozen layer has no backward (frozen layers are a prefix of the "
                                         "network: freeze what feeds them, or run under torch.no_grad())" % (what, name))


def conv_bn_leaky_frozen(x, weight, bn, residual=None, stride=1, padding=0, slope=LEAKY_SLOPE):
    """A frozen Conv -> BatchNorm -> LeakyReLU (+ residual) block as ONE kernel, om_conv2d_frozen_forward (csrc/conv_fwd.hip):
    leaky_relu(batch_norm(conv2d(x, weight), bn's running statistics), slope) + residual, where the convolution output is never
    stored.  x, weight and the geometries as conv2d; `bn` an nn.BatchNorm2d with affine parameters and running statistics, whose
    weight, bias, running_mean, running_var and eps are read (its mode is not asked: the running statistics are used, no buffer is
    touched); residual None or NCHW-contiguous with the output's shape.  x (and the residual) float32, or both bf16: then the kernel
    is om_conv2d_bf16_frozen_forward (csrc/conv_fwd_bf16.hip), the weight and bn stay float32 and the output is bf16; a mixed pair
    raises.  Returns a tensor without a grad_fn.  Under grad mode, x, residual, the weight or bn's parameters requiring grad raise;
    so does anything else that is off: there is no fallback."""
    what = "conv_bn_leaky_frozen"
    _require_nchw(x, what, "the frozen block's input", ACT_DTYPES)
    _lib.require_cuda_tensor(weight, "the frozen block's convolution weight", torch.float32)
    ks, s, p = _conv_geometry(what, x, weight, stride, padding)
    cout = int(weight.shape[0])
    if bn.running_mean is None or bn.running_var is None:
        raise _lib.OrienMaskHipError("%s: the BatchNorm has no running statistics (track_running_stats=False)" % what)
    if bn.weight is None or bn.bias is None:
        raise _lib.OrienMaskHipError("%s: the BatchNorm has no affine parameters" % what)
    for name, t in (("weight", bn.weight), ("bias", bn.bias), ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
        _lib.require_cuda_tensor(t, "the frozen block's BatchNorm " + name, torch.float32)
        if tuple(t.shape) != (cout,) or not t.is_contiguous() or t.device != x.device:
            raise _lib.OrienMaskHipError("%s: BatchNorm %s must be contiguous [%d] on %s, got %s on %s"
                                         % (what, name, cout, x.device, tuple(t.shape), t.device))
    if weight.device != x.device:
        raise _lib.OrienMaskHipError("%s: weight on %s, x on %s" % (what, weight.device, x.device))
    B, cin, H, W = x.shape
    shape = _out_shape(x, cout, ks, s, p)
    _require_residual(residual, shape, x.device, x.dtype)
    _require_no_grad(what, x=x, residual=residual, weight=weight, **{"bn.weight": bn.weight, "bn.bias": bn.bias})
    dev = x.device
    y = torch.empty(shape, dtype=x.dtype, device=dev)
    entry = "om_conv2d_bf16_frozen_forward" if x.dtype == torch.bfloat16 else "om_conv2d_frozen_forward"
    _lib.launch(entry, dev, x, weight, B, cin, H, W, cout, ks, s, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps),
                float(slope), residual, y)
    return y


def _route_call(fn, ptrs, chans, scales, B, H, W, whole, dev):
    """One om_route_concat_<fn> call on the current stream: `ptrs` the per-source tensors (None: null), `whole` y or dy; the entry
    point is the one of their element type."""
    n = len(chans)
    table = (ctypes.c_void_p * ROUTE_MAX)(*[t.data_ptr() if t is not None else None for t in ptrs] + [None] * (ROUTE_MAX - n))
    c = (ctypes.c_int * ROUTE_MAX)(*list(chans) + [0] * (ROUTE_MAX - n))
    s = (ctypes.c_int * ROUTE_MAX)(*list(scales) + [0] * (ROUTE_MAX - n))
    for t in ptrs:
        if t is not None and t.dtype != whole.dtype:
            raise _lib.OrienMaskHipError("om_route_concat_%s: tensors of %s and %s in one call: there is no cast" % (fn, t.dtype, whole.dtype))
    if fn == "forward":
        _lib.launch("om_route_concat_forward" + _sfx(whole), dev, table, c, s, n, B, H, W, whole)
    else:
        _lib.launch("om_route_concat_backward" + _sfx(whole), dev, whole, c, s, n, B, H, W, table)


class _UpsampleConcat(torch.autograd.Function):
    """forward(ctx, scales, *tensors) -> torch.cat([F.interpolate(t, scale_factor=s, mode='nearest')], 1): om_route_concat_forward
    into a torch.empty output.  Nothing is saved but the shapes.  The backward is om_route_concat_backward into a gradient per input
    that needs one; the others are passed as null and nothing is computed for them."""

    @staticmethod
    def forward(ctx, scales, *tensors):
        B = tensors[0].shape[0]
        H, W = tensors[0].shape[2] * scales[0], tensors[0].shape[3] * scales[0]
        chans = [int(t.shape[1]) for t in tensors]
        dev = tensors[0].device
        y = torch.empty((B, sum(chans), H, W), dtype=tensors[0].dtype, device=dev)
        _route_call("forward", tensors, chans, scales, B, H, W, y, dev)
        ctx.geom = (chans, tuple(scales), B, H, W)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        chans, scales, B, H, W = ctx.geom
        dev = dy.device
        dy = dy.contiguous()
        grads = [torch.empty((B, c, H // s, W // s), dtype=dy.dtype, device=dev) if need else None
                 for c, s, need in zip(chans, scales, ctx.needs_input_grad[1:])]
        if any(g is not None for g in grads):
            _route_call("backward", grads, chans, scales, B, H, W, dy, dev)
        return (None,) + tuple(grads)


class _SplitChannels(torch.autograd.Function):
    """forward(ctx, x, sizes) -> dense tensors with the values of torch.split(x, sizes, 1): om_route_concat_backward with x in the
    place of dy and every scale 1.  The backward is om_route_concat_forward into one [B,C,H,W] gradient; an output that received
    no gradient is passed as null and the kernel writes its zeros."""

    @staticmethod
    def forward(ctx, x, sizes):
        B, C, H, W = x.shape
        outs = [torch.empty((B, c, H, W), dtype=x.dtype, device=x.device) for c in sizes]
        _route_call("backward", outs, sizes, [1] * len(sizes), B, H, W, x, x.device)
        ctx.geom = (tuple(sizes), B, H, W, x.device, x.dtype)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        sizes, B, H, W, dev, dtype = ctx.geom
        if all(g is None for g in grads):
            return None, None
        grads = [g.contiguous() if g is not None else None for g in grads]
        dx = torch.empty((B, sum(sizes), H, W), dtype=dtype, device=dev)
        _route_call("forward", grads, sizes, [1] * len(sizes), B, H, W, dx, dev)
        return dx, None


def upsample_concat(tensors, scales):
    """torch.cat([F.interpolate(t, scale_factor=s, mode='nearest') for t, s in zip(tensors, scales)], dim=1) as one HIP kernel
    (csrc/route.hip), bit-identical to it, with the backward as one kernel too: the gradient of a source is the s x s block sum of
    its channels' dy in torch-CPU's order.  1 to 4 CUDA NCHW-contiguous tensors, all float32 or all bf16 (the output and the
    gradients have their type; a bf16 gradient is the float32 block sum rounded once), of one batch size whose up-sampled sizes
    agree, and their integer scales, each 1, 2, 4 or 8.  Anything else raises: there is no fallback and no cast."""
    tensors, scales = list(tensors), list(scales)
    if not 1 <= len(tensors) <= ROUTE_MAX or len(scales) != len(tensors):
        raise ValueError("upsample_concat takes 1 to %d tensors and as many scales, got %d and %d" % (ROUTE_MAX, len(tensors), len(scales)))
    for i, t in enumerate(tensors):
        _require_nchw(t, "route_backend 'hip'", "input %d of upsample_concat (route_backend 'hip')" % i, ACT_DTYPES)
    for s in scales:
        if isinstance(s, bool) or not isinstance(s, int) or s not in ROUTE_SCALES:
            raise _lib.OrienMaskHipError("upsample_concat: scale %r; the scales are the integers %s" % (s, ROUTE_SCALES))
    B, H, W = tensors[0].shape[0], tensors[0].shape[2] * scales[0], tensors[0].shape[3] * scales[0]
    for t, s in zip(tensors, scales):
        if t.dtype != tensors[0].dtype:
            raise _lib.OrienMaskHipError("upsample_concat: inputs of %s and %s: there is no cast" % (tensors[0].dtype, t.dtype))
        if t.device != tensors[0].device or t.shape[0] != B or t.shape[2] * s != H or t.shape[3] * s != W or min(t.shape) < 1:
            raise _lib.OrienMaskHipError("upsample_concat: shapes %s at scales %s do not give one [%d,*,%d,%d] tensor on one device"
                                         % ([tuple(t.shape) for t in tensors], scales, B, H, W))
    return _UpsampleConcat.apply(tuple(scales), *tensors)


def split_channels(x, sizes):
    """torch.split(x, sizes, dim=1) as dense tensors, one HIP kernel (csrc/route.hip); the backward is one kernel that writes the
    whole gradient of x, zeros for an output that took no part in the loss.  x CUDA float32 or bf16 NCHW-contiguous, 1 to 4 sizes >= 1
    that sum to its channels.  Anything else raises: there is no fallback."""
    sizes = [int(c) for c in sizes]
    if not 1 <= len(sizes) <= ROUTE_MAX:
        raise ValueError("split_channels takes 1 to %d sizes, got %d" % (ROUTE_MAX, len(sizes)))
    _require_nchw(x, "route_backend 'hip'", "the input of split_channels (route_backend 'hip')", ACT_DTYPES)
    if min(sizes) < 1 or sum(sizes) != x.shape[1] or min(x.shape) < 1:
        raise _lib.OrienMaskHipError("split_channels: sizes %s do not split the %d channels of shape %s" % (sizes, x.shape[1], tuple(x.shape)))
    return _SplitChannels.apply(x, tuple(sizes))


class _SyncBNAct(torch.autograd.Function):
    """forward(ctx, x, gamma, beta, residual, bn, slope, group) -> leaky(batch_norm(x)) (+ residual) with the batch statistics of
    every rank of `group` (torch.nn.SyncBatchNorm's): om_bn_sync_stats, an all-gather of the 3C-double record, om_bn_sync_forward;
    backward: om_bn_sync_backward_sums, an all-gather of the 2C-double sums, om_bn_sync_backward_dx.  Every rank merges the same
    gathered bytes in rank order, so the running buffers stay bit-identical across ranks.  The collectives are enqueued against the
    current stream; nothing synchronises with the host.  dgamma / dbeta are this rank's own (DistributedDataParallel averages them).
    Without an input gradient the second all-gather and the dx kernel are skipped."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, bn, slope, group):
        import torch.distributed as dist
        B, C, H, W = x.shape
        dev = x.device
        R = dist.get_world_size(group)
        y, save = _bn_forward_buffers(x)
        record = torch.empty(3 * C, dtype=torch.float64, device=dev)
        records = torch.empty(R * 3 * C, dtype=torch.float64, device=dev)
        n_total = torch.empty(1, dtype=torch.float64, device=dev)
        track = bn.running_mean is not None
        stream, ws = _bn_scratch(x)
        with _lib.on_device(dev):
            _lib.launch("om_bn_sync_stats" + _sfx(x), dev, x, B, C, H, W, record, ws, ws.numel(), stream=stream)
            dist.all_gather_into_tensor(records, record, group=group)
            _lib.launch("om_bn_sync_forward" + _sfx(x), dev, x, B, C, H, W, records, R, gamma, beta, bn.running_mean, bn.running_var,
                        bn.num_batches_tracked if track else None, float(bn.momentum), float(bn.eps), float(slope), residual,
                        y, save.data_ptr(), save.data_ptr() + 8 * C, n_total, stream=stream)
        ctx.save_for_backward(x, gamma, beta, save, n_total)
        ctx.slope, ctx.has_residual, ctx.group, ctx.R = float(slope), residual is not None, group, R
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        import torch.distributed as dist
        x, gamma, beta, save, n_total = ctx.saved_tensors
        B, C, H, W = x.shape
        dev = x.device
        R = ctx.R
        dy, dx, dgb = _bn_backward_buffers(ctx, x, dy)
        sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
        stream, ws = _bn_scratch(x)
        with _lib.on_device(dev):
            _lib.launch("om_bn_sync_backward_sums" + _sfx(x), dev, x, dy, B, C, H, W, gamma, beta, save.data_ptr(),
                        save.data_ptr() + 8 * C, ctx.slope, sums, dgb.data_ptr(), dgb.data_ptr() + 4 * C, ws, ws.numel(), stream=stream)
            if dx is not None:
                sums_all = torch.empty(R * 2 * C, dtype=torch.float64, device=dev)
                dist.all_gather_into_tensor(sums_all, sums, group=ctx.group)
                _lib.launch("om_bn_sync_backward_dx" + _sfx(x), dev, x, dy, B, C, H, W, gamma, beta, save.data_ptr(),
                            save.data_ptr() + 8 * C, ctx.slope, sums_all, R, n_total, dx, stream=stream)
        return _bn_grads(ctx, dx, dgb, dy)


def _sync_world_size(group):
    """Ranks the block's statistics span: 1 without an initialised process group (then nothing is exchanged)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


def _check_bn_batch(bn, h, synced):
    """What F.batch_norm refuses too: a cumulative moving average, and one value per channel in training mode on one rank."""
    if bn.momentum is None:
        raise ValueError("BatchNorm momentum=None (a cumulative moving average) is not supported")
    if (bn.training or bn.running_mean is None) and h.numel() // h.shape[1] <= 1 and not synced:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(h.shape),))


def bn_leaky(x, bn, residual=None, slope=LEAKY_SLOPE, sync=False, process_group=None):
    """leaky_relu(bn(x), slope) (+ residual) as the HIP block: `bn` is an nn.BatchNorm2d in training or eval mode, x (and residual)
    CUDA NCHW-contiguous, both float32 or both bf16 (the output has their type; bn's parameters and buffers are float32 either
    way); anything else raises.  sync=True: in training mode and with more than one rank in `process_group`
    (None: the default group) the batch statistics are those of every rank's batch (_SyncBNAct); otherwise nothing is exchanged."""
    synced = sync and bn.training and _sync_world_size(process_group) > 1
    _require_nchw(x, "backend 'hip'", "the BatchNorm input (backend 'hip')", ACT_DTYPES)
    _check_bn_batch(bn, x, synced)
    _require_residual(residual, x.shape, x.device, x.dtype)
    if synced:
        return _SyncBNAct.apply(x, bn.weight, bn.bias, residual, bn, slope, process_group)
    return _BNAct.apply(x, bn.weight, bn.bias, residual, bn, slope)


def _as_bf16(x):
    """The bf16 forward's input: a float32 tensor (the first layer's image) is cast once, as autocast casts it in front of a
    convolution; a bf16 tensor passes."""
    return x.to(torch.bfloat16) if x.dtype == torch.float32 else x


def _same_type(residual, y):
    """The residual of a backend-'torch' block, refused where torch's add would promote it or the block's output silently."""
    if residual.dtype != y.dtype:
        raise ValueError("residual is %s, the block's output %s: there is no cast" % (residual.dtype, y.dtype))
    return residual


class ConvBNLeaky(nn.Module):
    """The reference's conv_bn_leaky block (model/base.py:104-137,278-279) with its sub-structure and keys: conv_block.0 the
    bias-free nn.Conv2d, conv_block.1 the nn.BatchNorm2d, conv_block.2 the LeakyReLU(0.1).  forward(x, residual=None) returns
    leaky(bn(conv(x))) + residual.

    backend 'hip' (default): F.conv2d, then BatchNorm + LeakyReLU + residual as one HIP block under autograd (csrc/bn_act.hip);
    CUDA float32 tensors only -- anything else raises, there is no fallback.  backend 'torch': F.conv2d -> F.batch_norm ->
    F.leaky_relu, the comparator, and the only path that takes CPU tensors.  The block normalises with batch statistics while
    its BatchNorm module is in training mode and with the running statistics otherwise (model.eval(), backbone_batchnorm_eval).
    After convert_sync_batchnorm (`sync` True) the batch statistics are those of every rank of `process_group`.

    conv_backend 'torch' (default): the convolution is F.conv2d with torch's gradients.  conv_backend 'hip': the same forward
    through conv2d, whose gradients are the HIP kernels of csrc/conv_grad.hip; CUDA float32 NCHW-contiguous tensors only.

    conv_forward 'torch' (default): the forward convolution is F.conv2d.  conv_forward 'hip': without amp (needs conv_backend
    'hip') it is om_conv2d_forward (csrc/conv_fwd.hip); with amp 'bf16' (needs conv_backend 'torch') it is conv2d_bf16
    (csrc/conv_fwd_bf16.hip), whose gradients are torch's bf16 ones.

    frozen=True: the block's three parameters have requires_grad False; its BatchNorm normalises with the running statistics in
    every mode, never touches a buffer, stays in eval mode across train() calls and is left alone by convert_sync_batchnorm.  No
    autograd node is made, and an input that requires grad raises (frozen blocks are a prefix of the network).  The forward is
    F.conv2d -> F.batch_norm(training=False) -> leaky (+ residual) with backend 'torch'; F.conv2d -> bn_leaky's eval kernel with
    backend 'hip'; and with conv_forward 'hip' the single kernel of conv_bn_leaky_frozen.  The keys and buffers are an unfrozen
    block's; load_state_dict tolerates a missing num_batches_tracked (the reference's FrozenBatchNorm2d has none).

    amp None (default): float32.  amp 'bf16': the forward runs under torch.autocast(dtype=torch.bfloat16), so the convolution is
    torch's in bf16 and the output is bf16: from the _bf16 kernels with backend 'hip' (a frozen block: their eval phase), from
    torch's own bf16 batch_norm and leaky_relu with backend 'torch' (the comparator; CPU tensors too).  The parameters, their
    gradients and the buffers stay float32.  A residual must have the block's element type.  Needs conv_backend 'torch'.  With
    conv_forward 'hip' the convolution is conv2d_bf16 on the float32 master weight (a float32 x is cast to bf16 once, as autocast
    does), and a frozen block with backend 'hip' is the one bf16 kernel of conv_bn_leaky_frozen.

    conv_grad 'torch' (default): conv2d_bf16's gradients are torch's bf16 ones.  conv_grad 'hip' (needs amp 'bf16', conv_forward
    'hip', conv_backend 'torch'): they are om_conv2d_bf16_grad_input / om_conv2d_bf16_grad_weight (csrc/conv_grad_bf16.hip).  A key
    of its own because amp with conv_backend 'hip' is pinned to raise.  A frozen block has no backward and ignores it."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, backend="hip", conv_backend="torch",
                 conv_forward="torch", frozen=False, amp=None, conv_grad="torch"):
        super().__init__()
        _check_backends(backend, conv_backend, conv_forward, amp=amp, conv_grad=conv_grad)
        self.amp = amp
        self.conv_grad = conv_grad
        self.backend = backend
        self.conv_backend = conv_backend
        self.conv_forward = conv_forward
        self.sync, self.process_group = False, None          # set by convert_sync_batchnorm
        self.conv_block = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False),
            nn.BatchNorm2d(out_channels),
            nn.LeakyReLU(negative_slope=LEAKY_SLOPE, inplace=True))
        self.frozen = bool(frozen)
        if self.frozen:
            for p in self.parameters():
                p.requires_grad_(False)
            bn = self.conv_block[1]
            bn.eval()
            bn.register_load_state_dict_pre_hook(self._keep_num_batches_tracked)

    def _keep_num_batches_tracked(self, module, state_dict, prefix, *_):
        """A frozen block's counter is never read: where a checkpoint lacks it, the module keeps its own."""
        key = prefix + "num_batches_tracked"
        if key not in state_dict:
            state_dict[key] = self.conv_block[1].num_batches_tracked

    def train(self, mode=True):
        super().train(mode)
        if self.frozen:
            self.conv_block[1].eval()
        return self

    def _frozen_forward(self, x, residual):
        conv, bn, act = self.conv_block[0], self.conv_block[1], self.conv_block[2]
        if bn.training:
            bn.eval()                       # set by hand on the sub-module: .training tells what the block does
        if bn.running_mean is None or bn.running_var is None:
            raise ValueError("ConvBNLeaky: a frozen block needs the BatchNorm's running statistics")
        _require_no_grad("ConvBNLeaky(frozen=True)", x=x, residual=residual, **{n: p for n, p in self.named_parameters()})
        if self.amp and self.conv_forward == "hip":
            x = _as_bf16(x)
        if self.backend == "hip" and self.conv_forward == "hip":
            return conv_bn_leaky_frozen(x, conv.weight, bn, residual=residual, stride=conv.stride, padding=conv.padding,
                                        slope=act.negative_slope)
        if self.amp and self.conv_forward == "hip":
            h = conv2d_bf16(x, conv.weight, None, conv.stride, conv.padding)
        else:
            h = F.conv2d(x, conv.weight, None, conv.stride, conv.padding)
        if self.backend == "hip":
            return bn_leaky(h, bn, residual=residual, slope=act.negative_slope)
        y = F.batch_norm(h, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        y = F.leaky_relu(y, act.negative_slope, inplace=True)
        return y if residual is None else y + _same_type(residual, y)

    def forward(self, x, residual=None):
        with _autocast(self.amp, x):
            return self._forward(x, residual)

    def _forward(self, x, residual):
        if self.frozen:
            return self._frozen_forward(x, residual)
        conv, bn, act = self.conv_block[0], self.conv_block[1], self.conv_block[2]
        if self.conv_backend == "hip":
            h = conv2d(x, conv.weight, None, conv.stride, conv.padding, forward=self.conv_forward)
        elif self.amp and self.conv_forward == "hip":
            h = conv2d_bf16(_as_bf16(x), conv.weight, None, conv.stride, conv.padding, backward=self.conv_grad)
        else:
            h = F.conv2d(x, conv.weight, None, conv.stride, conv.padding)
        _check_bn_batch(bn, h, self.sync and bn.training and _sync_world_size(self.process_group) > 1)
        if self.backend == "torch":
            training = bn.training or bn.running_mean is None
            y = F.batch_norm(h, bn.running_mean, bn.running_var, bn.weight, bn.bias, training, bn.momentum, bn.eps)
            if training and bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)
            y = F.leaky_relu(y, act.negative_slope, inplace=True)
            return y if residual is None else y + _same_type(residual, y)
        return bn_leaky(h, bn, residual=residual, slope=act.negative_slope, sync=self.sync, process_group=self.process_group)


def convert_sync_batchnorm(model, process_group=None):
    """The reference's nn.SyncBatchNorm.convert_sync_batchnorm(model) (trainer/builder.py:86) for this module's models: marks every
    ConvBNLeaky so that, in training mode and with more than one rank in `process_group` (None: the default group), its batch
    statistics are taken over every rank's batch.  The module tree, the state_dict keys and the parameters() order are unchanged.
    Blocks in eval mode (model.eval(), backbone_batchnorm_eval) and a world of one rank exchange nothing, as torch's SyncBatchNorm.
    Frozen blocks (ConvBNLeaky(frozen=True), the models' frozen_stages) have no batch statistics and are left unsynchronised.
    Backend 'torch' is refused: F.batch_norm cannot synchronise.  Returns `model`."""
    blocks = [m for m in model.modules() if isinstance(m, ConvBNLeaky) and not m.frozen]
    for m in blocks:
        if m.backend != "hip":
            raise ValueError("convert_sync_batchnorm: backend %r cannot synchronise its batch statistics (F.batch_norm); build the "
                             "model with backend 'hip'" % (m.backend,))
    for m in blocks:
        m.sync, m.process_group = True, process_group
    return model


class _Container(nn.Module):
    """Holds sub-modules under the reference's names; the model's forward addresses them by name."""


class _Backbone(_Container):
    """BaseBackbone.train (model/base.py:71-77): with batchnorm_eval the BatchNorm modules stay in eval mode."""

    def __init__(self, batchnorm_eval):
        super().__init__()
        self.batchnorm_eval = batchnorm_eval

    def train(self, mode=True):
        super().train(mode)
        if mode and self.batchnorm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self


class OrienMaskYOLOFPNPlus(nn.Module):
    """The reference's OrienMaskYOLOFPNPlus (model/orienmask_yolo_fpnplus.py:9-90) for training: the same constructor arguments
    plus `backend` ('hip' / 'torch') and `conv_backend` ('torch' / 'hip': whose convolution gradients, see ConvBNLeaky; with 'hip'
    the plain head convolutions go through conv2d on the nn.Conv2d modules' parameters) and `conv_forward` ('torch' / 'hip': whose
    forward convolution, for the blocks and the four head convolutions; 'hip' needs conv_backend 'hip', or amp 'bf16') and `route_backend` ('torch'
    / 'hip': whose up-sampling, cat and split between the convolutions: torch's ops, or upsample_concat and split_channels
    (csrc/route.hip), CUDA float32 tensors only; independent of the other three), the same state_dict keys and parameters() order as the reference and as
    orienmask_amd.model (checkpoints and optimizer state move in both directions), trainable parameters, and a forward that
    returns the reference's ((bbox32, orien32), (bbox16, orien16), (bbox8, orien8)) with a graph behind it.

    frozen_stages (int 0...6, default 0): freezes backbone.conv1 ... backbone.conv{k} (conv1 the stem layer, conv2-conv6 a
    down-sampling layer plus its blocks each) as ConvBNLeaky(frozen=True): no gradients, running statistics in every mode, untouched
    buffers, and with conv_forward 'hip' one kernel per layer.  What the reference's freeze_backbone stage count means to do
    (model/backbone/darknet.py:31-38, model/base.py:210-266) under an unambiguous name: bools raise.  The keys, the parameters()
    order and the buffers are those of frozen_stages=0, which builds the model as before; independent of backbone_batchnorm_eval.

    amp (None / 'bf16', default None): mixed precision.  With 'bf16' the forward runs under torch.autocast(dtype=torch.bfloat16):
    every convolution is torch's in bf16 (conv_backend 'hip' raises) or, with conv_forward 'hip', this package's: conv2d_bf16 in the
    unfrozen blocks, one fused bf16 kernel per frozen block (backend 'hip'), and the four head convolutions as conv2d_bf16 with a
    float32 output; the first layer's image is cast to bf16 once.  The activations between them are bf16 through
    the blocks (ConvBNLeaky) and, with route_backend 'hip', through upsample_concat; the head convolutions' outputs are returned
    as float32, so the loss, the counters and the optimizer see what they see without amp.  Parameters, gradients, buffers and
    the state_dict (keys and dtypes) are those of amp=None: checkpoints move freely between the two and to the inference model.

    conv_grad ('torch' / 'hip', default 'torch'): whose gradients behind conv2d_bf16, in the blocks and the four head convolutions.
    'hip' needs amp 'bf16', conv_forward 'hip' and conv_backend 'torch' and makes them the bf16 kernels of csrc/conv_grad_bf16.hip:
    every convolution node of a step is then this package's and a step repeats bit for bit without cudnn.deterministic.  (A key
    of its own, because amp with conv_backend 'hip' is pinned to raise.)  Module tree, keys, parameter order and dtypes are unchanged."""

    def __init__(self, num_anchors, num_classes, pretrained=None, freeze_backbone=False, backbone_batchnorm_eval=False,
                 backend="hip", conv_backend="torch", conv_forward="torch", route_backend="torch", frozen_stages=0, amp=None,
                 conv_grad="torch"):
        super().__init__()
        if freeze_backbone is not False:
            # the reference's DarkNet53._freeze_network calls self._freeze_module, which does not exist (darknet.py:31-38)
            raise NotImplementedError("freeze_backbone=%r: the reference's own _freeze_network cannot run; not supported.  Use "
                                      "frozen_stages=k (0...6) to freeze backbone.conv1 ... backbone.conv{k}" % (freeze_backbone,))
        if isinstance(frozen_stages, bool) or not isinstance(frozen_stages, int) or not 0 <= frozen_stages <= len(DARKNET_STAGES) + 1:
            raise ValueError("frozen_stages must be an int from 0 to %d (the number of backbone stages conv1 ... conv%d to freeze), "
                             "got %r" % (len(DARKNET_STAGES) + 1, len(DARKNET_STAGES) + 1, frozen_stages))
        _check_backends(backend, conv_backend, conv_forward, route_backend, amp, conv_grad)
        self.amp = amp
        self.conv_grad = conv_grad
        self.num_anchors = num_anchors
        self.num_classes = num_classes
        self.pretrained = pretrained
        self.freeze_backbone = freeze_backbone
        self.backbone_batchnorm_eval = backbone_batchnorm_eval
        self.backend = backend
        self.conv_backend = conv_backend
        self.conv_forward = conv_forward
        self.route_backend = route_backend
        self.frozen_stages = frozen_stages
        self.backbone = _Backbone(backbone_batchnorm_eval)
        self._plus = type(self).__name__ == "OrienMaskYOLOFPNPlus"
        self._by_name = {}
        for spec in model_convs(type(self).__name__, num_anchors, num_classes):
            *path, leaf = spec.name.split(".")
            node = self
            for p in path:
                if p not in node._modules:
                    node.add_module(p, _Container())
                node = node._modules[p]
            pad = spec.ksize // 2
            if spec.bn:
                # backbone.conv{i}[...]: frozen where i <= frozen_stages
                frozen = spec.name.startswith("backbone.conv") and int(spec.name.split(".")[1][len("conv"):]) <= frozen_stages
                m = ConvBNLeaky(spec.cin, spec.cout, spec.ksize, stride=spec.stride, padding=pad, backend=backend,
                                conv_backend=conv_backend, conv_forward=conv_forward, frozen=frozen, amp=amp, conv_grad=conv_grad)
            else:
                m = nn.Conv2d(spec.cin, spec.cout, spec.ksize, stride=spec.stride, padding=pad)
            node.add_module(leaf, m)
            self._by_name[spec.name] = m
        if pretrained is not None:
            self._load_pretrained_backbone(pretrained)
        self._init_weights()

    def _init_weights(self):
        """model/base.py:26-32: BatchNorm outside the backbone starts at gamma 1, beta 0."""
        for name, module in self.named_modules():
            if "backbone" in name:
                continue
            if isinstance(module, _BatchNorm):
                nn.init.ones_(module.weight)
                nn.init.zeros_(module.bias)

    def _load_pretrained_backbone(self, path):
        """As orienmask_amd.model loads it (BaseBackbone._load_pretrained_weights, model/base.py:48-64): backbone-relative keys;
        keys that are missing or of another shape are ignored and reported.  Returns the ignored keys."""
        import warnings
        sd = _pack.unwrap_checkpoint(torch.load(path, map_location="cpu", weights_only=False))
        own = self.backbone.state_dict()
        picked = {k: v for k, v in sd.items() if k in own and tuple(v.shape) == tuple(own[k].shape)}
        ignored = [k for k in sd if k not in picked]
        if not picked:
            warnings.warn("pretrained file %s: none of its %d keys matches the backbone (expected backbone-relative keys such "
                          "as 'conv1.conv_block.0.weight'); the model keeps its initialisation" % (path, len(sd)))
        elif ignored:
            warnings.warn("pretrained file %s: ignored keys %s" % (path, ignored[:8] + (["..."] if len(ignored) > 8 else [])))
        own.update(picked)
        self.backbone.load_state_dict(own)
        return ignored

    # ------------------------------------------------------------------ forward
    def _run(self, prefix, x, n=5):
        for i in range(n):
            x = self._by_name["%s.%d" % (prefix, i)](x)
        return x

    def _route(self, name, x, up):
        x = self._by_name[name](x)
        if self.route_backend == "hip":
            return x, up                     # the up-sampling happens in _cat's kernel
        return F.interpolate(x, scale_factor=up, mode="nearest") if up > 1 else x

    def _cat(self, parts):
        """torch.cat along the channels; route_backend 'hip': upsample_concat of (tensor, scale) pairs, a bare tensor at scale 1."""
        if self.route_backend == "hip":
            pairs = [p if isinstance(p, tuple) else (p, 1) for p in parts]
            return upsample_concat([t for t, _ in pairs], [s for _, s in pairs])
        return torch.cat(parts, dim=1)

    def _split(self, x, size):
        if self.route_backend == "hip":
            return split_channels(x, [size] * (x.shape[1] // size))
        return torch.split(x, size, dim=1)

    def _backbone_forward(self, x):
        """model/backbone/darknet.py:47-54 with the blocks of :14-15."""
        m = self._by_name
        x = m["backbone.conv1"](x)
        feats = {}
        for idx, _, nblocks in DARKNET_STAGES:
            stage = "backbone.conv%d" % idx
            x = m[stage + ".0"](x)
            for j in range(1, nblocks + 1):
                h = m["%s.%d.conv.0" % (stage, j)](x)
                x = m["%s.%d.conv.1" % (stage, j)](h, residual=x)
            feats[idx] = x
        return feats[6], feats[5], feats[4], feats[3]

    def _plain(self, name, x):
        """A head's nn.Conv2d: the module itself, or conv2d on its parameters (conv_backend 'hip')."""
        m = self._by_name[name]
        if self.conv_backend == "hip":
            return conv2d(x, m.weight, m.bias, m.stride, m.padding, forward=self.conv_forward)
        if self.amp and self.conv_forward == "hip":      # float32 straight from the accumulators: no .float() pass
            return conv2d_bf16(_as_bf16(x), m.weight, m.bias, m.stride, m.padding, out_dtype=torch.float32, backward=self.conv_grad)
        return m(x).float() if self.amp else m(x)        # the heads leave the model as float32

    def _bbox_head(self, s, x):
        return self._plain("bbox_head%d.1" % s, self._by_name["bbox_head%d.0" % s](x))

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError("x must be [B,3,H,W] with H and W multiples of 32, got %s" % (tuple(x.shape),))
        with _autocast(self.amp, x):
            return self._forward(x)

    def _forward(self, x):
        x32, x16, x8, x4 = self._backbone_forward(x)
        neck32 = self._run("neck32", x32)
        neck16 = self._run("neck16", self._cat([self._route("route32.0", neck32, 2), x16]))
        neck8 = self._run("neck8", self._cat([self._route("route16.0", neck16, 2), x8]))
        bbox32 = self._bbox_head(32, neck32)
        bbox16 = self._bbox_head(16, neck16)
        bbox8 = self._bbox_head(8, neck8)
        if self._plus:
            cat4 = [self._route("skip32.0", neck32, 8), self._route("skip16.0", neck16, 4), self._route("skip8.0", neck8, 2),
                    self._route("skip4", x4, 1)]
        else:
            cat4 = [self._route("route8.0", neck8, 2), x4]
        oriens = self._run("neck4", self._cat(cat4))
        oriens = self._plain("orien_head.5", self._run("orien_head", oriens))
        orien32, orien16, orien8 = self._split(oriens, self.num_anchors * 2)
        return (bbox32, orien32), (bbox16, orien16), (bbox8, orien8)


class OrienMaskYOLO(OrienMaskYOLOFPNPlus):
    """The reference's non-Plus model (model/orienmask_yolo.py:8-86): route8 and x4 feed a 192-channel neck4."""
