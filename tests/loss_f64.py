"""A differentiable restatement of OrienMaskYOLOMultiScaleLoss's loss_sum (the reference's eval/orienmask_yolo_loss.py:62-145,
eval/base.py:27-40,102-119) as plain torch code over tensors of any floating dtype on any device, for tests that need the loss
as a float64 truth AND as a float32 yardstick (tests/step_audit.py).  torch autograd differentiates it.

Everything discrete is an INPUT: ``forced_targets`` evaluates loss_np.LossNP.build_targets once, on heads the caller names, and
``loss`` takes its result -- the positive / negative (ignore cells removed) masks, the box scale weights, txy / twh / tcls, the
orientation targets and the two ROI masks.  The only decision of the loss that depends on the predictions, an IoU against
obj_ignore_threshold, is therefore taken once and shared by every side of a comparison.

    term 0  sum(BCE(sigmoid(xy), txy) * pscale) / B               term 4  sum(BCE(sigmoid(cls), tcls) * pos) / B
    term 1  sum((wh - twh)^2 * pscale) / 2 / B                    term 5  sum(SmoothL1(up4(orien) - torien)[opos]) / npos * nbox / B
    term 2  sum(BCE(sigmoid(obj), pos) * pos) / B                 term 6  the same over oneg / nneg
    term 3  sum(BCE(sigmoid(obj), pos) * neg) / B
    loss_sum = sum_s scales_weight[s] * sum_j (scales_weight[s] * weight[j]) * term[s][j]      (the reference weighs a scale twice)

BCE is F.binary_cross_entropy: the logarithms clamped at -100 and, in the backward, (p - t) / max((1 - p) p, 1e-12), the
reference's nn.BCELoss.  SmoothL1 has beta 1; up4 is the x4 bilinear up-sample with align_corners=False.
"""
import numpy as np
import torch
import torch.nn.functional as F

import loss_grad_np
import loss_np

TARGET_KEYS = ("pos", "neg", "pscale", "txy", "twh", "tcls", "torien", "opos", "oneg")


def _loss_np(cfg):
    return loss_np.LossNP(**{k: v for k, v in cfg.items() if k != "type"})


def forced_targets(cfg, heads, target):
    """The discrete side of the loss from `heads` ([(bbox, orien)] per scale, float32 numpy or CPU tensors) and the collate
    tuple `target` (numpy): per scale a dict of TARGET_KEYS (numpy) plus "near_ignore", the number of cells with an IoU within
    4 ulp of obj_ignore_threshold (loss_grad_np.near_ulp): a decision another rounding of the same heads could take otherwise."""
    ln = _loss_np(cfg)
    out = []
    for s in range(len(ln.grids)):
        t = ln.build_targets(s, np.asarray(heads[s][0], np.float32), *target)
        f = {k: t[k] for k in TARGET_KEYS}
        f["near_ignore"] = int(sum(loss_grad_np.near_ulp(iou, ln.thr).any(1).sum() for iou in t["ious"] if iou.size))
        out.append(f)
    return out


def _bce(p, t):
    return F.binary_cross_entropy(p, t, reduction="none")


def loss(cfg, heads, forced):
    """(loss_sum, terms): loss_sum a 0-dim tensor with the heads' graph behind it, terms [scales, 7] the WEIGHTED terms (LossNP's
    `weighted`, detached).  `heads` [(bbox [B, A (5 + C), nH, nW], orien [B, 2 A, H / 4, W / 4])] per scale, any dtype and
    device; `forced` from forced_targets."""
    ln = _loss_np(cfg)
    total, rows = None, []
    for s, ((bbox, orien), f) in enumerate(zip(heads, forced)):
        dt, dev = bbox.dtype, bbox.device
        t = {k: torch.as_tensor(np.ascontiguousarray(f[k])).to(device=dev) for k in TARGET_KEYS}
        t = {k: (v if v.dtype == torch.bool else v.to(dt)) for k, v in t.items()}
        nH, nW = ln.grids[s]
        A, C = len(ln.mask[s]), ln.C
        B = bbox.shape[0]
        p = bbox.reshape(B, A, 5 + C, nH, nW).permute(0, 1, 3, 4, 2)
        pos, neg, ps = t["pos"], t["neg"], t["pscale"].unsqueeze(-1)
        terms = [(_bce(torch.sigmoid(p[..., 0:2]), t["txy"]) * ps).sum() / B,
                 (((p[..., 2:4] - t["twh"]) ** 2) * ps).sum() / 2 / B]
        bo = _bce(torch.sigmoid(p[..., 4]), pos)
        terms += [(bo * pos).sum() / B, (bo * neg).sum() / B,
                  (_bce(torch.sigmoid(p[..., 5:]), t["tcls"]) * pos.unsqueeze(-1)).sum() / B]
        up = F.interpolate(orien, scale_factor=4, mode="bilinear", align_corners=False)
        up = up.reshape(B, A, 2, ln.H, ln.W).permute(0, 1, 3, 4, 2)
        sl1 = F.smooth_l1_loss(up, t["torien"], reduction="none", beta=1.0)
        nbox = pos.sum()
        for m in (t["opos"], t["oneg"]):
            n = int(m.sum())
            terms.append(sl1[m].sum() / n * nbox / B if n else sl1.sum() * 0)
        weight = torch.as_tensor(ln.weight[s].astype(np.float64)).to(device=dev, dtype=dt)
        weighted = torch.stack(terms) * weight
        rows.append(weighted.detach())
        part = weighted.sum() * float(ln.scales_weight[s])
        total = part if total is None else total + part
    return total, torch.stack(rows)
