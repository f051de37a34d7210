"""Loop-form numpy restatement of OrienMaskYOLOMultiScaleLoss (the reference's eval/orienmask_yolo_loss.py, eval/base.py) in
float32 with float64 sums, for tests that cannot run the reference (it is not on the GPU machine).

Element-wise arithmetic is float32 in the reference's operation order; loops go over images and, in collate order, over the
matched instances, updating only their ROI (the rest of the image is untouched by the reference's full-image ops).  Elementary
functions are the correctly rounded ones (float64, one rounding): the reference's sigmoid / exp / log differ from them by one ulp
on a few percent of inputs, so loss terms agree to ~1e-7 relative and the targets that use only + - * / and round bit for bit.
Duplicate positive cells follow torch-CPU: box targets from the highest GT index, tcls the union of the classes.
"""
import numpy as np

f32 = np.float32


def _sig(x):
    e = np.exp(-np.asarray(x, np.float64)).astype(f32)
    return f32(1) / (f32(1) + e)


def _log(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(x, np.float64)).astype(f32)


def _bce(p, t):
    p = np.asarray(p, f32)
    t = np.asarray(t, f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        l1 = np.maximum(np.log1p(-p.astype(np.float64)).astype(f32), f32(-100))
        l0 = np.maximum(_log(p), f32(-100))
    return (t - f32(1)) * l1 - t * l0


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _taps(n_out, n_in):
    d = np.arange(n_out)
    src = _fma(f32(0.25), d.astype(f32) + f32(0.5), f32(-0.5))
    src = np.where(src < 0, f32(0), src)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = src - i0.astype(f32)
    return i0, i1, f32(1) - w1, w1


def upsample4(o):
    """F.interpolate(o, scale_factor=4, mode='bilinear', align_corners=False) on [..., h, w], torch-CPU's placement
    (csrc/bilinear.h): rows blended along x with fma(a0, w0, a1 * w1), then along y the same way."""
    h, w = o.shape[-2:]
    yi0, yi1, wy0, wy1 = _taps(4 * h, h)
    xi0, xi1, wx0, wx1 = _taps(4 * w, w)
    a = o[..., yi0, :]
    b = o[..., yi1, :]
    top = _fma(a[..., xi0], wx0, a[..., xi1] * wx1)
    bot = _fma(b[..., xi0], wx0, b[..., xi1] * wx1)
    return _fma(top, wy0[:, None], bot * wy1[:, None])


class LossNP:
    def __init__(self, grid_size, image_size, anchors, anchor_mask, num_classes, center_region=0.6, valid_region=0.7,
                 label_smooth=False, obj_ignore_threshold=0.5, weight=None, scales_weight=None, **_):
        self.grids = [(int(g[0]), int(g[1])) for g in grid_size]
        self.H, self.W = int(image_size[0]), int(image_size[1])
        self.anchors = np.asarray(anchors, f32)
        self.mask = [list(m) for m in anchor_mask]
        self.C = int(num_classes)
        self.cr, self.vr = f32(center_region), f32(valid_region)
        ls = 1.0 / max(self.C, 40) if label_smooth else 0
        self.ls_off, self.ls_on = f32(ls), f32(1 - ls)
        self.thr = f32(obj_ignore_threshold)
        S = len(self.grids)
        sw = np.asarray(scales_weight if scales_weight is not None else [1] * S, f32)
        self.scales_weight = sw
        self.weight = [np.asarray([sw[i] * f32(w) for w in weight], f32) if weight is not None else np.ones(7, f32)
                       for i in range(S)]

    # ---- one scale: orienmask_yolo_loss.py:62-264
    def build_targets(self, s, bbox_head, gt_bbox, gt_cls, gt_index, gt_mask):
        nH, nW = self.grids[s]
        A = len(self.mask[s])
        C = self.C
        B = len(gt_index) - 1
        H, W = self.H, self.W
        p = np.asarray(bbox_head, f32).reshape(B, A, 5 + C, nH, nW).transpose(0, 1, 3, 4, 2)
        scale_wh = np.asarray([W, H], f32) / np.asarray([nW, nH], f32)
        grid_all = self.anchors / scale_wh
        gy, gx = np.meshgrid(np.arange(nH, dtype=f32), np.arange(nW, dtype=f32), indexing="ij")
        px = _sig(p[..., 0]) + gx
        py = _sig(p[..., 1]) + gy
        ga = grid_all[self.mask[s]]
        pw = np.exp(p[..., 2].astype(np.float64)).astype(f32) * ga[None, :, None, None, 0]
        ph = np.exp(p[..., 3].astype(np.float64)).astype(f32) * ga[None, :, None, None, 1]
        t = dict(pos=np.zeros((B, A, nH, nW), f32), neg=np.ones((B, A, nH, nW), f32), pscale=np.zeros((B, A, nH, nW), f32),
                 txy=np.zeros((B, A, nH, nW, 2), f32), twh=np.zeros((B, A, nH, nW, 2), f32), tiou=np.zeros((B, A, nH, nW), f32),
                 tcls=np.full((B, A, nH, nW, C), self.ls_off, f32), omask=np.zeros((B, A, H, W), np.int64),
                 torien=np.zeros((B, A, H, W, 2), f32), ious=[])
        gtg = np.asarray(gt_bbox, f32) * np.asarray([nW, nH, nW, nH], f32)
        mesh_x = np.arange(W, dtype=f32)[None, :]
        mesh_y = np.arange(H, dtype=f32)[:, None]
        for b in range(B):
            g0, g1 = int(gt_index[b]), int(gt_index[b + 1])
            if g0 == g1:
                t["ious"].append(np.zeros((A * nH * nW, 0), f32))
                continue
            g = gtg[g0:g1]
            b1x1 = (px[b] - pw[b] / f32(2)).reshape(-1, 1); b1x2 = (px[b] + pw[b] / f32(2)).reshape(-1, 1)
            b1y1 = (py[b] - ph[b] / f32(2)).reshape(-1, 1); b1y2 = (py[b] + ph[b] / f32(2)).reshape(-1, 1)
            b2x1 = (g[:, 0] - g[:, 2] / f32(2))[None]; b2x2 = (g[:, 0] + g[:, 2] / f32(2))[None]
            b2y1 = (g[:, 1] - g[:, 3] / f32(2))[None]; b2y2 = (g[:, 1] + g[:, 3] / f32(2))[None]
            dx = np.maximum(np.minimum(b1x2, b2x2) - np.maximum(b1x1, b2x1), f32(0))
            dy = np.maximum(np.minimum(b1y2, b2y2) - np.maximum(b1y1, b2y1), f32(0))
            inter = dx * dy
            union = ((b1x2 - b1x1) * (b1y2 - b1y1) + (b2x2 - b2x1) * (b2y2 - b2y1)) - inter
            iou = inter / union                                                  # [A*nH*nW, G]
            t["ious"].append(iou)
            t["neg"][b][(iou > self.thr).any(1).reshape(A, nH, nW)] = 0
            iou4 = iou.reshape(A, nH, nW, -1)
            for j in range(g1 - g0):
                w, h = g[j, 2], g[j, 3]
                inter_a = np.minimum(w, grid_all[:, 0]) * np.minimum(h, grid_all[:, 1])
                ai = inter_a / ((w * h + grid_all[:, 0] * grid_all[:, 1]) - inter_a)
                best = int(np.argmax(ai))
                if best not in self.mask[s]:
                    continue
                a = self.mask[s].index(best)
                cx = int(min(max(np.floor(g[j, 0]), f32(0)), f32(nW - 1)))
                cy = int(min(max(np.floor(g[j, 1]), f32(0)), f32(nH - 1)))
                t["pos"][b, a, cy, cx] = 1
                t["neg"][b, a, cy, cx] = 0
                t["pscale"][b, a, cy, cx] = f32(2) - (w * h) / f32(nW * nH)
                t["txy"][b, a, cy, cx] = [g[j, 0] - f32(cx), g[j, 1] - f32(cy)]
                t["twh"][b, a, cy, cx] = [_log(w / ga[a, 0]), _log(h / ga[a, 1])]
                t["tcls"][b, a, cy, cx, int(gt_cls[g0 + j])] = self.ls_on
                t["tiou"][b, a, cy, cx] = iou4[a, cy, cx, j]
                # orientation targets of this instance, in collate order
                x, y = g[j, 0] * scale_wh[0], g[j, 1] * scale_wh[1]
                vw = (w * self.vr + f32(0.5)) * scale_wh[0]
                vh = (h * self.vr + f32(0.5)) * scale_wh[1]
                cw, ch = vw / self.vr * self.cr, vh / self.vr * self.cr
                x1 = int(np.rint(min(max(x - vw, f32(0)), f32(W - 1))))
                x2 = int(np.rint(min(max(x + vw, f32(0)), f32(W - 1)))) + 1
                y1 = int(np.rint(min(max(y - vh, f32(0)), f32(H - 1))))
                y2 = int(np.rint(min(max(y + vh, f32(0)), f32(H - 1)))) + 1
                om = t["omask"][b, a, y1:y2, x1:x2]
                to = t["torien"][b, a, y1:y2, x1:x2]
                ox = np.broadcast_to(mesh_x[:, x1:x2] - x, om.shape)
                oy = np.broadcast_to(mesh_y[y1:y2, :] - y, om.shape)
                m = np.asarray(gt_mask[g0 + j][y1:y2, x1:x2], bool)
                om[m] = -1
                to[m, 0] = ox[m]
                to[m, 1] = oy[m]
                ni = ~m & (om >= 0)
                om[ni] += 1
                lx = np.maximum(np.abs(ox), f32(1e-8)); ly = np.maximum(np.abs(oy), f32(1e-8))
                q = np.minimum(np.maximum(cw / lx, f32(1)), np.maximum(ch / ly, f32(1))) - f32(1)
                to[ni, 0] = to[ni, 0] + (q * np.sign(ox) * lx)[ni]
                to[ni, 1] = to[ni, 1] + (q * np.sign(oy) * ly)[ni]
        t["opos"] = t["omask"] < 0
        t["oneg"] = t["omask"] > 0
        pa = self.anchors[self.mask[s]] / f32(2)
        tor = t["torien"] / pa[None, :, None, None, :]
        den = np.where(t["omask"] == 0, 1000, t["omask"]).astype(f32)
        t["torien"] = tor / den[..., None]
        t["pred"] = (p, px, py, pw, ph)
        return t

    def scale_loss(self, s, head, target):
        bbox_head, orien_head = head
        B = len(target[2]) - 1
        t = self.build_targets(s, bbox_head, *target)
        p = t["pred"][0]
        A = len(self.mask[s])
        sxy = _sig(p[..., 0:2])
        so = _sig(p[..., 4])
        sc = _sig(p[..., 5:])
        pwh = p[..., 2:4]
        if not np.isfinite(pwh).all():
            raise FloatingPointError("pred_wh not finite")
        pos, neg, ps = t["pos"], t["neg"], t["pscale"]
        sum64 = lambda a: float(np.sum(np.asarray(a, np.float64)))          # noqa: E731
        terms = np.zeros(7, np.float64)
        nBf = f32(B)
        terms[0] = f32(sum64(_bce(sxy, t["txy"]) * ps[..., None])) / nBf
        terms[1] = f32(sum64(((pwh - t["twh"]) * (pwh - t["twh"])) * ps[..., None])) / f32(2) / nBf
        bo = _bce(so, pos)
        terms[2] = f32(sum64(bo * pos)) / nBf
        terms[3] = f32(sum64(bo * neg)) / nBf
        terms[4] = f32(sum64(_bce(sc, t["tcls"]) * pos[..., None])) / nBf
        po = upsample4(np.asarray(orien_head, f32)).reshape(B, A, 2, self.H, self.W).transpose(0, 1, 3, 4, 2)
        z = np.abs(po - t["torien"])
        sl1 = np.where(z < f32(1), f32(0.5) * z * z / f32(1), z - f32(0.5))
        npos, nneg = int(t["opos"].sum()), int(t["oneg"].sum())
        nbox = f32(pos.sum())
        terms[5] = f32(sum64(sl1[t["opos"]])) / f32(npos) * nbox / nBf if npos else 0.0
        terms[6] = f32(sum64(sl1[t["oneg"]])) / f32(nneg) * nbox / nBf if nneg else 0.0
        nposb, nnegb = float(pos.sum()), float(neg.sum())
        acc = z < f32(0.5)
        metrics = [(sum64(sc * (t["tcls"] > f32(0.5))), nposb), (sum64(so * pos), nposb), (sum64(so * neg), nnegb),
                   (sum64(t["tiou"]), nposb), (int((t["tiou"] > f32(0.5)).sum()), nposb), (int((t["tiou"] > f32(0.75)).sum()), nposb),
                   (float(acc[t["opos"]].sum()), float(npos * 2)), (float(acc[t["oneg"]].sum()), float(nneg * 2))]
        weighted = (terms.astype(f32) * self.weight[s]).astype(f32)
        return weighted, metrics, t

    def __call__(self, predict, target):
        """Per scale: (7 weighted terms float32, 8 (numerator, count) pairs, targets dict)."""
        return [self.scale_loss(s, predict[s], target) for s in range(len(self.grids))]


def load_fixture(path):
    """A tests/golden/loss_*.npz fixture -> (g, cfg dict, heads [(bbox, orien) torch CPU], target numpy tuple)."""
    import torch
    from orienmask_amd import synth
    g = np.load(path)
    cfg = {}
    for k in g["cfg_keys"]:
        v = g["cfg_" + str(k)]
        if k in ("label_smooth",):
            v = bool(v)
        elif k in ("num_classes",):
            v = int(v)
        elif k in ("center_region", "valid_region", "obj_ignore_threshold"):
            v = float(v)
        elif v.size == 0:
            v = None
        else:
            v = v.tolist()
        cfg[str(k)] = v
    B = int(g["B"])
    heads = [(b.clone(), o.clone()) for b, o in synth.synth_heads(int(g["hseed"]), B, cfg["grid_size"], regime="sparse")]
    if "planted" in g.files:
        for s, idx, v in g["planted"]:
            heads[int(s)][0].view(-1)[int(idx)] = float(v)
    H, W = [int(v) for v in g["size"]]
    n = len(g["gt_bbox"])
    mask = np.unpackbits(g["gt_mask_bits"], axis=1, count=H * W).reshape(n, H, W).astype(bool)
    return g, cfg, heads, (g["gt_bbox"], g["gt_cls"], g["gt_index"], mask)
