"""The reference's training loss on the HIP path: ``builder.build(config["loss"], orienmask_amd.train)``.

  OrienMaskYOLOMultiScaleLoss  orienmask_amd.loss's class with the same constructor; when a head requires grad, ``forward``
                               returns a ``loss_sum`` with a ``grad_fn`` whose backward is ``om_loss_backward`` (csrc/loss.hip)

This is the one-line swap of the reference's trainer/builder.py:34 (``build(config['loss'], evaluation_module)``): the trainer
then does ``loss, loss_log, _ = self.loss(predict, label, training=True)`` and ``loss.backward()`` as before, without the
reference's per-image, per-instance Python target building.

The forward is the values-only path (om_loss plus the host aggregation): loss_log and metric_log are the same, bit for bit.  The
backward follows the reference's autograd chain in torch-CPU's float32 order (csrc/loss.hip) and is ``once_differentiable``.  It
enqueues two kernels on the current stream and never synchronises with the host: the upstream gradient is read on the device.
Each call that builds a graph owns its workspace (the match records om_loss_backward reads) and result vector until the graph is
freed, so several losses may be computed before one ``backward()``.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import lib as _lib
from .loss import EvalCounter, OrienMaskYOLOMultiScaleLoss as _ValuesLoss

__all__ = ["OrienMaskYOLOMultiScaleLoss", "EvalCounter"]


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
                ctypes.c_void_p(gt_index.data_ptr()), ctypes.c_void_p(gt_mask.data_ptr()), self.N,
                ctypes.c_void_p(self.result.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(),
                ctypes.c_void_p(g.data_ptr()), (ctypes.c_float * 3)(*self.sw + [0.0] * (3 - S)), ptrs(gb), ptrs(go))
        L = _lib.load()

        def run():
            with torch.cuda.device(dev):
                _lib.check(L.om_loss_backward(*args, _lib.current_stream_ptr(dev)), "om_loss_backward")
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
        if len(predict) != self.num_scales:
            raise ValueError("predict has %d scales, the loss was built for %d" % (len(predict), self.num_scales))
        flat = [t for pair in predict for t in pair]
        if not (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in flat)):
            # no graph to build (no head requires grad, or grad mode is off): the values-only path
            return super().forward([(b.detach(), o.detach()) for b, o in predict], target, training)
        for t in flat:
            if isinstance(t, torch.Tensor) and t.requires_grad and t.dtype != torch.float32:
                raise _lib.OrienMaskHipError("the HIP loss takes float32 heads, got %s" % t.dtype)
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
        run = self.prepare(dense, target, workspace=ws)
        loss_sum, loss_log, metric_log = self._finish(run(), training, dev)
        call = _Call(self, [(b.requires_grad, o.requires_grad) for b, o in predict], run)
        call.loss_sum = loss_sum
        out = _LossBackward.apply(call, *flat)
        return out, loss_log, metric_log
