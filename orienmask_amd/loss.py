"""The reference's validation loss and its counter on the HIP path.

  OrienMaskYOLOMultiScaleLoss  same constructor, attributes and call contract as
                               the reference's eval/orienmask_yolo_loss.py:259-325 with eval/base.py's aggregation
  EvalCounter                  the counter semantics of the reference's eval/counter.py
  DeviceEvalCounter            the same counter on a device block: ``enqueue`` (below) adds a call's values to it with
                               ``om_loss_accumulate`` (csrc/loss_counter.hip) and the host reads it when it wants the means

The values come from ``om_loss`` (csrc/loss.hip): four kernel launches for all scales and ONE device-to-host copy per call,
against the reference's per-image, per-instance Python loops over full-image tensors and dozens of ``.item()`` calls.  The
per-scale and cross-scale aggregation (eval/base.py:29-32,90-121) runs on the host in torch float32, the reference's own ops.

Deliberate departures from the reference:
  * no autograd: the values only (the validation epoch runs under no_grad).  A head that requires grad raises
    NotImplementedError: the class with a backward (om_loss_backward) is orienmask_amd.train.OrienMaskYOLOMultiScaleLoss;
  * a non-finite pred_wh raises FloatingPointError (the reference prints and calls exit());
  * loud limits: 1..3 scales of 1..3 anchors, at most 9 anchors, 2047 classes and OM_LOSS_MAX_GT (1024) GTs per image; the
    orientation maps are exactly image / 4 per side.  The GT limit is exercised: tests/test_loss_crowd.py checks values,
    targets and gradients of images with 63 .. 1024 GTs (1025 is refused, tests/test_loss.py);
  * scales_weight=None means ones (the reference reads num_scales before setting it and fails).
``enqueue(predict, target, counter, step)`` is the deferred form of a call, for a loop that must not stall: om_loss, then
om_loss_accumulate into a DeviceEvalCounter, and the device scalar loss_sum comes back; nothing is copied to the host.
Duplicate positives (two GTs on one cell) follow torch-CPU's answer: box targets from the highest GT index, tcls the union of
their classes (csrc/loss.hip).
"""
import ctypes

import torch

from . import lib as _lib


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


class EvalCounter:
    """Sums of values and item counts per key, for one stage (``counter`` / ``items``) and for the epoch (``*_epoch``).

    ``update(key, value)`` adds a plain value as one item, a ``(sum, count)`` pair as ``count`` items.  ``reset`` folds the
    stage into the epoch; ``average`` is the stage mean and ``average_epoch`` folds the stage in and returns the epoch mean;
    both return -1 when there are no items."""

    def __init__(self):
        self.keys = []
        self.items = {}
        self.counter = {}
        self.items_epoch = {}
        self.counter_epoch = {}

    def update(self, key, value):
        if isinstance(value, (tuple, dict)):
            value, item = value
        else:
            item = 1
        if key not in self.items:
            self.keys.append(key)
            self.items[key], self.counter[key] = item, value
            self.items_epoch[key], self.counter_epoch[key] = 0, 0.
            return
        self.items[key] += item
        self.counter[key] += value

    def _fold(self, key):
        self.items_epoch[key] += self.items[key]
        self.counter_epoch[key] += self.counter[key]
        self.items[key], self.counter[key] = 0, 0.

    def reset(self):
        for key in self.keys:
            self._fold(key)

    def reset_epoch(self):
        for key in self.keys:
            self.items[key], self.counter[key] = 0, 0.
            self.items_epoch[key], self.counter_epoch[key] = 0, 0.

    @staticmethod
    def _mean(total, n):
        try:
            return total / n
        except ZeroDivisionError:
            return -1

    def average(self, key):
        return self._mean(self.counter[key], self.items[key])

    def average_epoch(self, key):
        self._fold(key)
        return self._mean(self.counter_epoch[key], self.items_epoch[key])

    def save(self, filename):
        torch.save({"items": self.items, "counter": self.counter}, filename)

    def save_epoch(self, filename):
        torch.save({"items_epoch": self.items_epoch, "counter_epoch": self.counter_epoch}, filename)

    def merge(self, counter_dict):
        for key in self.keys:
            self.items[key] += counter_dict["items"][key]
            self.counter[key] += counter_dict["counter"][key]

    def merge_epoch(self, counter_dict):
        for key in self.keys:
            self.items_epoch[key] += counter_dict["items_epoch"][key]
            self.counter_epoch[key] += counter_dict["counter_epoch"][key]


def _accumulate_torch(block, result, num_scales, scales_weight, with_metrics, step, out):
    """om_loss_accumulate (include/orienmask_hip.h) in torch ops on the tensors' own device: the comparator of the kernel and
    what a counter on the CPU runs.  float32 throughout, one rounding per operation, sums left to right."""
    S, T, SF = num_scales, _lib.OM_LOSS_TERMS, _lib.OM_LOSS_SCALE_FLOATS
    r = result[:_lib.OM_LOSS_FLAG_OFF].view(_lib.OM_MAX_SCALES, SF)[:S]
    t = r[:, :T]
    ssum = t[:, 0]
    for j in range(1, T):
        ssum = ssum + t[:, j]
    v = torch.cat([t, ssum.unsqueeze(1)], 1)                               # [S, 8]: the terms and the scale sum
    w = torch.tensor(scales_weight[:S], dtype=torch.float32, device=result.device)
    wv = v * w.unsqueeze(1)
    cross = wv[0]
    for s in range(1, S):
        cross = cross + wv[s]
    loss_sum = cross[T]
    values = torch.cat([loss_sum.reshape(1), v.reshape(-1), cross]).double()
    n_loss = values.numel()
    pairs = block[_lib.OM_COUNTER_STAGE_OFF:_lib.OM_COUNTER_STAGE_OFF + 2 * n_loss].view(n_loss, 2)
    pairs[:, 0] += values
    pairs[:, 1] += 1.0
    if with_metrics:
        m = r[:, T:].reshape(S, _lib.OM_LOSS_METRICS, 2)
        cm = m[0]
        for s in range(1, S):
            cm = cm + m[s]
        mets = torch.cat([m.reshape(-1, 2), cm]).double()
        off = _lib.OM_COUNTER_STAGE_OFF + 2 * n_loss
        block[off:off + 2 * mets.shape[0]].view(-1, 2).add_(mets)
    status = block[_lib.OM_COUNTER_FLAG_OFF:_lib.OM_COUNTER_FLAG_OFF + 2].view(torch.int64)
    bits = result[_lib.OM_LOSS_FLAG_OFF:].view(torch.int32)[0].to(torch.int64)
    bits = bits | (~torch.isfinite(loss_sum)).to(torch.int64) * _lib.OM_COUNTER_FLAG_NONFINITE_LOSS
    first = (status[0] == 0) & (bits != 0)
    status[1] = torch.where(first, torch.full_like(bits, int(step)), status[1])
    status[0] |= bits
    out.copy_(loss_sum)
    return out


class DeviceEvalCounter:
    """EvalCounter (``average``, ``average_epoch``, ``reset``, ``reset_epoch``, ``keys``) for the keys of one loss, living in a
    block on `device` (include/orienmask_hip.h: OM_COUNTER_*).  ``accumulate`` -- what ``loss.enqueue`` calls -- adds a call's
    values on the device (om_loss_accumulate; on a CPU device the same arithmetic in torch ops); the keys are
    ['loss'] + loss.loss_id + loss.metric_id.

    Every reading method (``average``, ``average_epoch`` and their plural forms ``averages`` / ``averages_epoch``, which answer
    for many keys from the same copy) does ONE device-to-host copy of the block, calls ``check`` on it and answers with
    EvalCounter's arithmetic (-1 when there are no items).  ``reset`` / ``reset_epoch`` and the fold of ``average_epoch`` are
    asynchronous torch ops on the current stream.  The status words are sticky: ``check`` raises what the host path would have
    raised at the step that latched them, and names that step; ``reset_epoch`` clears them."""

    def __init__(self, loss, device):
        self.keys = ["loss"] + list(loss.loss_id) + list(loss.metric_id)
        self.num_scales = int(loss.num_scales)
        if len(self.keys) != 1 + 2 * (self.num_scales + 1) * _lib.OM_LOSS_METRICS:
            raise ValueError("a loss of %d scales has %d keys, not %d" % (self.num_scales, 1 + 2 * (self.num_scales + 1)
                                                                            * _lib.OM_LOSS_METRICS, len(self.keys)))
        self.num_classes = loss.num_classes
        self.scales_weight = [float(v) for v in loss.scales_weight]
        self._w = (ctypes.c_float * _lib.OM_MAX_SCALES)(*(self.scales_weight + [0.0] * (_lib.OM_MAX_SCALES - self.num_scales)))
        self._index = {k: i for i, k in enumerate(self.keys)}
        self.device = torch.device(device)
        self.block = torch.zeros(_lib.OM_COUNTER_BLOCK_DOUBLES, dtype=torch.float64, device=self.device)
        self.flags, self.first_bad_step = 0, None

    # -- the device side
    def accumulate(self, result, step, with_metrics=False, out=None):
        """Add one om_loss result vector (on the counter's device) as step `step`; returns loss_sum, a 0-dim float32 tensor on
        the device (`out` if given).  No host synchronisation."""
        if result.device != self.block.device or result.dtype != torch.float32 or result.numel() != _lib.OM_LOSS_RESULT_FLOATS \
                or not result.is_contiguous():
            raise ValueError("result must be om_loss's %d contiguous float32 on %s" % (_lib.OM_LOSS_RESULT_FLOATS, self.block.device))
        if out is None:
            out = torch.empty((), dtype=torch.float32, device=self.block.device)
        if not self.block.is_cuda:
            return _accumulate_torch(self.block, result, self.num_scales, self.scales_weight, with_metrics, step, out)
        _lib.launch("om_loss_accumulate", self.block.device, result, self.num_scales, self._w, int(bool(with_metrics)), int(step),
                    self.block, out)
        return out

    def _stage(self):
        return self.block[_lib.OM_COUNTER_STAGE_OFF:_lib.OM_COUNTER_STAGE_OFF + 2 * len(self.keys)]

    def _epoch(self):
        return self.block[_lib.OM_COUNTER_EPOCH_OFF:_lib.OM_COUNTER_EPOCH_OFF + 2 * len(self.keys)]

    def reset(self):
        self._epoch().add_(self._stage())
        self._stage().zero_()

    def reset_epoch(self):
        self.block.zero_()

    def gather(self, group=None):
        """All-gather the block and replace this rank's STAGE pairs by the sum of every rank's, added in rank order on every rank
        (the reference's _temp_counter_<rank>.pth merge, trainer/trainer.py:78-81,113-116,175-178, which merges the stage pairs:
        "not merge_epoch"); the status words become the OR of the ranks' flags and the smallest latched step.  The epoch pairs
        stay: a loop that gathers before every reset has the merged totals in them already.  No host synchronisation."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        blocks = [torch.empty_like(self.block) for _ in range(dist.get_world_size(group))]
        dist.all_gather(blocks, self.block, group=group)
        n = 2 * len(self.keys)
        total = blocks[0][:n].clone()
        for b in blocks[1:]:
            total += b[:n]
        status = torch.stack([b[_lib.OM_COUNTER_FLAG_OFF:].view(torch.int64) for b in blocks])        # [world, 2]
        flags = status[0, 0].clone()
        for f in status[1:, 0]:
            flags |= f
        big = torch.iinfo(torch.int64).max
        first = torch.where(status[:, 0] != 0, status[:, 1], torch.full_like(status[:, 1], big)).min()
        self._stage().copy_(total)
        mine = self.block[_lib.OM_COUNTER_FLAG_OFF:].view(torch.int64)
        mine[0] = flags
        mine[1] = torch.where(flags != 0, first, torch.zeros_like(first))
        return self

    # -- the host side
    def _host(self):
        host = self.block.cpu() if self.block.is_cuda else self.block.clone()            # the read's one device-to-host copy
        self.check(host)
        return host.tolist()

    def check(self, host=None):
        """Raise from the latched status words: FloatingPointError for a non-finite pred_wh or loss, ValueError for the GT flags
        (the errors of the host path's _finish); the message names the step that latched first.  `host`: a host copy of the
        block (one is made when it is not given)."""
        if host is None:
            host = self.block.cpu()
        flags, step = host[_lib.OM_COUNTER_FLAG_OFF:].view(torch.int64).tolist()
        self.flags, self.first_bad_step = flags, (step if flags else None)
        if not flags:
            return
        where = " (first at step %d)" % step
        if flags & _lib.OM_LOSS_FLAG_NONFINITE_WH:
            raise FloatingPointError("pred_wh not finite" + where)
        if flags & _lib.OM_LOSS_FLAG_TOO_MANY_GT:
            raise ValueError("gt_index is not a prefix of the GTs or an image has more than %d GTs (the HIP loss's limit)"
                             % _lib.OM_LOSS_MAX_GT + where)
        if flags & _lib.OM_LOSS_FLAG_BAD_CLASS:
            raise ValueError("a gt_cls value lies outside [0, %d)" % self.num_classes + where)
        if flags & _lib.OM_COUNTER_FLAG_NONFINITE_LOSS:
            raise FloatingPointError("loss not finite" + where)
        raise RuntimeError("unknown counter flags 0x%x" % flags + where)

    def averages(self, keys=None):
        """{key: stage mean} for `keys` (default: all) from one copy of the block."""
        host = self._host()
        out = {}
        for key in (self.keys if keys is None else keys):
            i = _lib.OM_COUNTER_STAGE_OFF + 2 * self._index[key]
            out[key] = EvalCounter._mean(host[i], host[i + 1])
        return out

    def averages_epoch(self, keys=None):
        """{key: epoch mean} for `keys` (default: all) from one copy of the block; like EvalCounter.average_epoch it folds the
        stage pairs of the keys it answers for into the epoch pairs (on the device, asynchronously)."""
        host = self._host()
        out = {}
        for key in (self.keys if keys is None else keys):
            s = _lib.OM_COUNTER_STAGE_OFF + 2 * self._index[key]
            e = _lib.OM_COUNTER_EPOCH_OFF + 2 * self._index[key]
            out[key] = EvalCounter._mean(host[e] + host[s], host[e + 1] + host[s + 1])
        if keys is None:
            self.reset()
        else:
            for key in keys:
                s = _lib.OM_COUNTER_STAGE_OFF + 2 * self._index[key]
                e = _lib.OM_COUNTER_EPOCH_OFF + 2 * self._index[key]
                self.block[e:e + 2] += self.block[s:s + 2]
                self.block[s:s + 2].zero_()
        return out

    def average(self, key):
        return self.averages([key])[key]

    def average_epoch(self, key):
        return self.averages_epoch([key])[key]


class OrienMaskYOLOMultiScaleLoss:
    def __init__(self, grid_size, image_size, anchors, anchor_mask, num_classes,
                 loss_id=("loss_xy", "loss_wh", "loss_obj", "loss_noobj",
                          "loss_cls", "loss_orien_pos", "loss_orien_neg"),
                 loss_sum_id="loss_sum", scales_id=("S32", "S16", "S08"),
                 metric_id=("cls_conf", "obj_pos", "obj_neg", "avg_iou",
                            "recall50", "recall75", "orien_pos_acc", "orien_neg_acc"),
                 center_region=0.6, valid_region=0.7, label_smooth=False,
                 obj_ignore_threshold=0.5, weight=None, scales_weight=None):
        assert len(grid_size) == len(anchor_mask) == len(scales_id)
        self.grid_size = grid_size
        self.image_size = image_size
        self.anchors = anchors
        self.anchor_mask = anchor_mask
        self.num_classes = num_classes
        self.center_region = center_region
        self.valid_region = valid_region
        self.label_smooth = label_smooth
        self.obj_ignore_threshold = obj_ignore_threshold
        self.weight = weight
        if len(loss_id) != _lib.OM_LOSS_TERMS or len(metric_id) != _lib.OM_LOSS_METRICS:
            raise ValueError("the loss has %d terms and %d metrics" % (_lib.OM_LOSS_TERMS, _lib.OM_LOSS_METRICS))
        # eval/base.py:66-98
        self.num_scales = len(scales_id)
        self.loss_suffix = list(loss_id) + [loss_sum_id]
        self.metric_suffix = list(metric_id)
        self.scales_prefix = list(scales_id)
        self.loss_sum_id = loss_sum_id
        self.loss_id, self.metric_id = [], []
        self.scales_loss_id, self.scales_loss_sum_id, self.scales_metric_id = [], [], []
        self.scales_weight = torch.tensor(scales_weight).float() if scales_weight is not None else torch.ones(self.num_scales)
        for sid in scales_id:
            sl = [sid + "_" + k for k in loss_id]
            self.loss_id += sl + [sid + "_" + loss_sum_id]
            self.metric_id += [sid + "_" + k for k in metric_id]
            self.scales_loss_id.append(sl)
            self.scales_loss_sum_id.append(sid + "_" + loss_sum_id)
            self.scales_metric_id.append([sid + "_" + k for k in metric_id])
        self.cross_scale_loss_id = ["cross_scale_" + k for k in self.loss_suffix]
        self.loss_id += self.cross_scale_loss_id
        self.cross_scale_metric_id = ["cross_scale_" + k for k in self.metric_suffix]
        self.metric_id += self.cross_scale_metric_id
        # per-scale item weights (orienmask_yolo_loss.py:311-315, base.py:24-25): float32(scales_weight[i] * weight[j]) or ones
        self.scale_item_weight = [torch.tensor([self.scales_weight[i] * w for w in weight]).float() if weight is not None
                                  else torch.ones(len(loss_id)) for i in range(self.num_scales)]
        self._check_limits()
        self._ws = None

    def _check_limits(self):
        S = self.num_scales
        self.grids = [_pair(g) for g in self.grid_size]
        self.image_h, self.image_w = _pair(self.image_size)
        nA = [len(m) for m in self.anchor_mask]
        if not 1 <= S <= _lib.OM_MAX_SCALES:
            raise ValueError("the HIP loss holds 1..%d scales, got %d" % (_lib.OM_MAX_SCALES, S))
        if any(not 1 <= n <= 3 for n in nA):
            raise ValueError("the HIP loss holds 1..3 anchors per scale, got %s" % (nA,))
        if not 1 <= len(self.anchors) <= _lib.OM_MAX_ANCHORS or any(not 0 <= a < len(self.anchors) for m in self.anchor_mask for a in m):
            raise ValueError("at most %d anchors, anchor_mask entries index them" % _lib.OM_MAX_ANCHORS)
        if not 1 <= int(self.num_classes) <= _lib.OM_LOSS_MAX_CLASSES:
            raise ValueError("the HIP loss holds 1..%d classes, got %d" % (_lib.OM_LOSS_MAX_CLASSES, self.num_classes))
        if self.image_h % 4 or self.image_w % 4:
            raise ValueError("image sides must be multiples of 4 (the orientation maps are image / 4), got %s" % (self.image_size,))

    def cfg_struct(self, predict=None):
        c = _lib.LossCfg()
        c.num_scales = self.num_scales
        for s, (gh, gw) in enumerate(self.grids):
            c.grid_h[s], c.grid_w[s] = gh, gw
            c.anchors_of_scale[s] = len(self.anchor_mask[s])
            for a, k in enumerate(self.anchor_mask[s]):
                c.anchor_mask[s][a] = int(k)
            for j in range(_lib.OM_LOSS_TERMS):
                c.weight[s][j] = float(self.scale_item_weight[s][j])
        c.image_h, c.image_w = self.image_h, self.image_w
        c.num_anchors_total = len(self.anchors)
        for k, (w, h) in enumerate(self.anchors):
            c.anchor_w[k], c.anchor_h[k] = float(w), float(h)
        c.num_classes = int(self.num_classes)
        c.center_region, c.valid_region = float(self.center_region), float(self.valid_region)
        ls = 1.0 / max(int(self.num_classes), 40) if self.label_smooth else 0
        c.label_smooth, c.label_on = float(ls), float(1 - ls)      # ctypes rounds the doubles to float32, as the tensor writes do
        c.obj_ignore_threshold = float(self.obj_ignore_threshold)
        if predict is not None:
            for s, (bbox, orien) in enumerate(predict):
                for i, v in enumerate(bbox.stride()):
                    c.bbox_stride[s][i] = v
                for i, v in enumerate(orien.stride()[:3]):
                    c.orien_stride[s][i] = v
        return c

    # -- inputs: the heads are read in place through their strides
    def _heads(self, predict):
        if len(predict) != self.num_scales:
            raise ValueError("predict has %d scales, the loss was built for %d" % (len(predict), self.num_scales))
        out = []
        for s, (bbox, orien) in enumerate(predict):
            for t, name in ((bbox, "bbox head"), (orien, "orientation head")):
                _lib.require_cuda_tensor(t, name, torch.float32)
                if t.requires_grad:
                    raise NotImplementedError("this HIP loss computes values only (call it under torch.no_grad() or on detached "
                                              "heads); orienmask_amd.train.OrienMaskYOLOMultiScaleLoss has the backward")
            nA = len(self.anchor_mask[s])
            gh, gw = self.grids[s]
            want = (nA * (5 + int(self.num_classes)), gh, gw)
            if bbox.dim() != 4 or tuple(bbox.shape[1:]) != want:
                raise ValueError("bbox head %d has shape %s, expected [B,%d,%d,%d]" % ((s, tuple(bbox.shape)) + want))
            wo = (2 * nA, self.image_h // 4, self.image_w // 4)
            if orien.dim() != 4 or tuple(orien.shape[1:]) != wo or orien.shape[0] != bbox.shape[0]:
                raise ValueError("orientation head %d has shape %s, expected [B,%d,%d,%d]" % ((s, tuple(orien.shape)) + wo))
            if orien.stride(3) != 1:
                orien = orien.contiguous()
            out.append((bbox, orien))
        return out

    def _targets(self, target, B, dev):
        gt_bbox, gt_cls, gt_index, gt_mask = target[:4]
        for t, name in ((gt_bbox, "gt_bbox"), (gt_cls, "gt_cls"), (gt_index, "gt_index"), (gt_mask, "gt_mask")):
            _lib.require_cuda_tensor(t, name)
            if t.device != dev:
                raise ValueError("%s is on %s, the heads on %s" % (name, t.device, dev))
        N = int(gt_bbox.shape[0])
        if gt_bbox.dtype != torch.float32 or tuple(gt_bbox.shape) != (N, 4):
            raise ValueError("gt_bbox must be float32 [N,4], got %s %s" % (gt_bbox.dtype, tuple(gt_bbox.shape)))
        if gt_cls.dtype != torch.int64 or tuple(gt_cls.shape) != (N,):
            raise ValueError("gt_cls must be int64 [N]")
        if gt_index.dtype != torch.int64 or tuple(gt_index.shape) != (B + 1,):
            raise ValueError("gt_index must be int64 [B+1] = [%d], got %s" % (B + 1, tuple(gt_index.shape)))
        if tuple(gt_mask.shape) != (N, self.image_h, self.image_w) or gt_mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("gt_mask must be bool [N,%d,%d], got %s %s" % (self.image_h, self.image_w, gt_mask.dtype,
                                                                          tuple(gt_mask.shape)))
        if N > B * _lib.OM_LOSS_MAX_GT:
            raise ValueError("%d GTs for %d images: the HIP loss holds at most %d GTs per image" % (N, B, _lib.OM_LOSS_MAX_GT))
        gt_mask = gt_mask.contiguous()
        if gt_mask.dtype == torch.bool:
            gt_mask = gt_mask.view(torch.uint8)
        return gt_bbox.contiguous(), gt_cls.contiguous(), gt_index.contiguous(), gt_mask, N

    def workspace_bytes(self, B, N):
        return _lib.workspace_bytes("om_loss_workspace_bytes", ctypes.byref(self.cfg_struct()), int(B), int(N))

    def _workspace(self, nbytes, dev):
        if self._ws is None or self._ws.device != dev or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws

    def prepare(self, predict, target, workspace=None):
        """Check the inputs and bind everything om_loss reads and writes; returns a callable that enqueues om_loss on the current
        stream (no host work but the C call itself) and returns the device result vector (OM_LOSS_RESULT_FLOATS floats).
        `workspace`: a uint8 device tensor of at least workspace_bytes(B, N) to use instead of the loss's own.  The callable's
        attributes `heads`, `target` (gt_bbox, gt_cls, gt_index, gt_mask), `B`, `N`, `ws` and `result` are what it binds."""
        heads = self._heads(predict)
        B, dev = heads[0][0].shape[0], heads[0][0].device
        gt_bbox, gt_cls, gt_index, gt_mask, N = self._targets(target, B, dev)
        cfg = self.cfg_struct(heads)
        if workspace is None:
            ws = self._workspace(self.workspace_bytes(B, N), dev)
        else:
            ws = workspace
            if ws.dtype != torch.uint8 or ws.device != dev or ws.numel() < self.workspace_bytes(B, N):
                raise ValueError("workspace must be uint8 on %s with at least %d bytes" % (dev, self.workspace_bytes(B, N)))
        result = torch.empty(_lib.OM_LOSS_RESULT_FLOATS, dtype=torch.float32, device=dev)
        bb = (ctypes.c_void_p * 3)(*[h[0].data_ptr() for h in heads] + [None] * (3 - len(heads)))
        oo = (ctypes.c_void_p * 3)(*[h[1].data_ptr() for h in heads] + [None] * (3 - len(heads)))
        args = (ctypes.byref(cfg), bb, oo, B, gt_bbox.data_ptr(), gt_cls.data_ptr(), gt_index.data_ptr(), gt_mask.data_ptr(), N,
                result.data_ptr(), ws.data_ptr(), ws.numel())
        keep = (cfg, heads, gt_bbox, gt_cls, gt_index, gt_mask, ws)        # alive as long as the callable

        def run():
            _lib.launch("om_loss", dev, *args)
            run.keep = keep
            return result
        run.heads, run.target, run.B, run.N, run.ws, run.result = heads, (gt_bbox, gt_cls, gt_index, gt_mask), B, N, ws, result
        return run

    def launch(self, predict, target):
        """Enqueue om_loss on the current stream; returns the device result vector (OM_LOSS_RESULT_FLOATS floats)."""
        return self.prepare(predict, target)()

    def __call__(self, predict, target, training=True):
        return self.forward(predict, target, training)

    def forward(self, predict, target, training=True):
        """Returns (loss_sum: 0-dim tensor on the heads' device, loss_log: {key: float}, metric_log: {key: (num, count)}) with
        eval/base.py:90-121's keys in its order; metric_log is empty when training is True (orienmask_yolo_loss.py:148)."""
        result = self.launch(predict, target)
        return self._finish(result, training, result.device)

    def enqueue(self, predict, target, counter, step, training=True):
        """The deferred call: om_loss, then om_loss_accumulate of its result into `counter` (a DeviceEvalCounter of this loss on
        the heads' device) as step `step`; with training=False the metric keys are counted too.  Returns loss_sum as a 0-dim
        device tensor.  Nothing is copied to the host: a bad input shows at the counter's next read (DeviceEvalCounter.check)."""
        return counter.accumulate(self.launch(predict, target), step, with_metrics=training is not True)

    def _finish(self, result, training, dev):
        """The host side of a call: the flag word, then aggregate."""
        host = result.cpu()                                  # the call's one device-to-host copy
        flags = int(host[_lib.OM_LOSS_FLAG_OFF:].view(torch.int32)[0])
        if flags & _lib.OM_LOSS_FLAG_NONFINITE_WH:
            raise FloatingPointError("pred_wh not finite")
        if flags & _lib.OM_LOSS_FLAG_TOO_MANY_GT:
            raise ValueError("gt_index is not a prefix of the GTs or an image has more than %d GTs (the HIP loss's limit)"
                             % _lib.OM_LOSS_MAX_GT)
        if flags & _lib.OM_LOSS_FLAG_BAD_CLASS:
            raise ValueError("a gt_cls value lies outside [0, %d)" % self.num_classes)
        return self.aggregate(host, training, dev)

    def aggregate(self, host, training=False, device=None):
        """eval/base.py:27-40 (per scale) and :90-121 (across scales) on the host result vector, in torch float32."""
        T, M, SF = _lib.OM_LOSS_TERMS, _lib.OM_LOSS_METRICS, _lib.OM_LOSS_SCALE_FLOATS
        loss_log, metric_log, scale_sums = {}, {}, []
        for s in range(self.num_scales):
            r = host[s * SF:(s + 1) * SF]
            loss_cat = r[:T].clone()
            for key, v in zip(self.scales_loss_id[s], loss_cat):
                loss_log[key] = v.item()
            scale_sum = loss_cat.sum()
            loss_log[self.scales_loss_sum_id[s]] = scale_sum.item()
            scale_sums.append(scale_sum)
            if training is not True:
                m = r[T:].tolist()
                for j, key in enumerate(self.scales_metric_id[s]):
                    num = int(m[2 * j]) if j in (4, 5) else m[2 * j]          # recall50 / recall75 are integer sums
                    metric_log[key] = (num, m[2 * j + 1])
        loss_sum = (torch.stack(scale_sums) * self.scales_weight).sum()
        loss_log[self.loss_sum_id] = loss_sum.item()
        cross = torch.tensor([[loss_log[k] for k in self.scales_loss_id[s]] + [loss_log[self.scales_loss_sum_id[s]]]
                              for s in range(self.num_scales)])
        cross = (cross * self.scales_weight.unsqueeze(-1)).sum(dim=0)
        for key, v in zip(self.cross_scale_loss_id, cross):
            loss_log[key] = v.item()
        if metric_log:
            cm = torch.tensor([[metric_log[k] for k in self.scales_metric_id[s]] for s in range(self.num_scales)]).sum(dim=0)
            for key, v in zip(self.cross_scale_metric_id, cm):
                metric_log[key] = (v[0].item(), v[1].item())
        if device is not None:
            loss_sum = loss_sum.to(device, non_blocking=True)
        return loss_sum, loss_log, metric_log

    def targets(self, predict_bbox, target, scale):
        """Test entry (om_loss_targets): scale `scale`'s built targets, as build_targets returns them
        (orienmask_yolo_loss.py:249-264) plus the raw orien_mask (int32: -1 positive, k > 0 negative count, 0 neither)."""
        if len(predict_bbox) != self.num_scales or not 0 <= scale < self.num_scales:
            raise ValueError("%d bbox heads and scale %d for a %d-scale loss" % (len(predict_bbox), scale, self.num_scales))
        for s, bbox in enumerate(predict_bbox):
            _lib.require_cuda_tensor(bbox, "bbox head", torch.float32)
            want = (len(self.anchor_mask[s]) * (5 + int(self.num_classes)),) + self.grids[s]
            if bbox.dim() != 4 or tuple(bbox.shape[1:]) != want or bbox.shape[0] != predict_bbox[0].shape[0]:
                raise ValueError("bbox head %d has shape %s, expected [B,%d,%d,%d]" % ((s, tuple(bbox.shape)) + want))
        B, dev = predict_bbox[0].shape[0], predict_bbox[0].device
        gt_bbox, gt_cls, gt_index, gt_mask, N = self._targets(target, B, dev)
        nA = len(self.anchor_mask[scale])
        gh, gw = self.grids[scale]
        H, W, C = self.image_h, self.image_w, int(self.num_classes)
        f = dict(device=dev, dtype=torch.float32)
        out = dict(bbox_pos_mask=torch.empty(B, nA, gh, gw, **f), bbox_neg_mask=torch.empty(B, nA, gh, gw, **f),
                   bbox_pos_scale=torch.empty(B, nA, gh, gw, **f), txy=torch.empty(B, nA, gh, gw, 2, **f),
                   twh=torch.empty(B, nA, gh, gw, 2, **f), tiou=torch.empty(B, nA, gh, gw, **f),
                   tcls=torch.empty(B, nA, gh, gw, C, **f),
                   orien_mask=torch.empty(B, nA, H, W, dtype=torch.int32, device=dev), torien=torch.empty(B, nA, H, W, 2, **f))
        cfg = self.cfg_struct()
        for s, b in enumerate(predict_bbox):
            for i, v in enumerate(b.stride()):
                cfg.bbox_stride[s][i] = v
        ws = torch.empty(self.workspace_bytes(B, N) + 512, dtype=torch.uint8, device=dev)
        bb = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in predict_bbox] + [None] * (3 - len(predict_bbox)))
        _lib.launch("om_loss_targets", dev, ctypes.byref(cfg), bb, B, gt_bbox, gt_cls, gt_index, gt_mask, N, scale,
                    *[out[k] for k in ("bbox_pos_mask", "bbox_neg_mask", "bbox_pos_scale", "txy", "twh", "tiou", "tcls", "orien_mask",
                                       "torien")], ws, ws.numel())
        return out
