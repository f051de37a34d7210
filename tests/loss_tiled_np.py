"""A kernel-shaped variant of the restatements (tests/loss_np.py, tests/loss_grad_np.py), and the plausible kernel errors
("mutants") that the crowd tests must catch; not a test module.

TiledNP keeps the restatement's arithmetic and takes csrc/loss.hip's structure:
  * matching per GT (tests/loss_cases.py::match), then per cell the winner among the GTs on it and the union of their classes;
  * orientation targets per 16 x 64 pixel tile: the image's instances of the anchor whose ROI meets the tile are culled in
    rounds of 64 into a slot list that keeps collate order, and the tile's pixels walk that list;
  * orientation gradient per 64 x 64 pixel tile (16 x 16 quarter pixels): the cull against the tile plus a 2-pixel halo, the walk
    over that region, and per quarter pixel the adjoint of the x4 up-sample gathered from the region alone.
Unmutated it must equal LossNP / LossGradNP on every case.  `mutant` switches on one error of MUTANTS.
"""
import numpy as np

import loss_cases
import loss_grad_np
import loss_np

f32 = np.float32

MUTANTS = {
    1: "orientation instances beyond the first 64 of an image are dropped",
    2: "ballot rounds are emitted in reverse order",
    3: "base is not carried between rounds: every round writes its slots from 0",
    4: "the class union is capped at the first four matches",
    5: "the first GT on a cell supplies the box targets",
    6: "GTs beyond 256 are invisible to the ignore mask and to matching",
    7: "g0 is rounded down to a multiple of 64",
    8: "a ROI that overlaps a forward tile by one column is culled (x2 > tx0 + 1)",
    9: "the gradient cull has no halo",
    10: "the gradient cull's halo is 1 pixel",
    11: "an anchor tie resolves to the last maximum",
}
FWD_TILE_H, FWD_TILE_W, GRAD_Q = 16, 64, 16


class TiledNP(loss_grad_np.LossGradNP):
    def __init__(self, mutant=None, **cfg):
        super().__init__(**cfg)
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        self.cfg = cfg
        self._built = {}

    # ---- cull: rounds of 64 in collate order, the slot list (global GT indices)
    def _cull(self, m, g0, ng, a, x0, x1, y0, y1, forward):
        mu = self.mutant
        if mu == 7:
            g0 -= g0 % 64
        n = g0 + np.arange(ng)
        lo_x = x0 + 1 if (mu == 8 and forward) else x0
        mine = (m.key[n] >= 0) & (m.a[n] == a) & (m.x1[n] < x1) & (m.x2[n] > lo_x) & (m.y1[n] < y1) & (m.y2[n] > y0)
        rounds = [n[j0:j0 + 64][mine[j0:j0 + 64]] for j0 in range(0, ng, 64)]
        if mu == 1:
            rounds = rounds[:1]
        if mu == 2:
            rounds = rounds[::-1]
        if mu == 3:
            rounds = rounds[-1:]              # each round overwrote the one before; the count is the last round's
        return [int(j) for r in rounds for j in r]

    # ---- the per-pixel walk over a rectangle: loss_np.LossNP.build_targets' per-instance update, restricted to it
    def _walk(self, y0, y1, x0, x1, lst, m, gt_mask):
        om = np.zeros((y1 - y0, x1 - x0), np.int64)
        to = np.zeros((y1 - y0, x1 - x0, 2), f32)
        for j in lst:
            ry1, ry2, rx1, rx2 = max(int(m.y1[j]), y0), min(int(m.y2[j]), y1), max(int(m.x1[j]), x0), min(int(m.x2[j]), x1)
            if ry1 >= ry2 or rx1 >= rx2:
                continue
            o = om[ry1 - y0:ry2 - y0, rx1 - x0:rx2 - x0]
            t = to[ry1 - y0:ry2 - y0, rx1 - x0:rx2 - x0]
            ox = np.broadcast_to(np.arange(rx1, rx2, dtype=f32)[None, :] - m.px[j], o.shape)
            oy = np.broadcast_to(np.arange(ry1, ry2, dtype=f32)[:, None] - m.py[j], o.shape)
            k = np.asarray(gt_mask[j][ry1:ry2, rx1:rx2], bool)
            o[k] = -1
            t[k, 0] = ox[k]
            t[k, 1] = oy[k]
            ni = ~k & (o >= 0)
            o[ni] += 1
            lx = np.maximum(np.abs(ox), f32(1e-8)); ly = np.maximum(np.abs(oy), f32(1e-8))
            q = np.minimum(np.maximum(m.cw[j] / lx, f32(1)), np.maximum(m.ch[j] / ly, f32(1))) - f32(1)
            t[ni, 0] = t[ni, 0] + (q * np.sign(ox) * lx)[ni]
            t[ni, 1] = t[ni, 1] + (q * np.sign(oy) * ly)[ni]
        return om, to

    def _normalise(self, s, a, om, to):
        pa = self.anchors[self.mask[s]][a] / f32(2)
        den = np.where(om == 0, 1000, om).astype(f32)
        return (to / pa) / den[..., None]

    def build_targets(self, s, bbox_head, gt_bbox, gt_cls, gt_index, gt_mask):
        if s in self._built:
            return self._built[s]
        mu = self.mutant
        t = dict(super().build_targets(s, bbox_head, gt_bbox, gt_cls, gt_index, gt_mask))     # the decode and the IoUs
        nH, nW = self.grids[s]
        A, C, H, W = len(self.mask[s]), self.C, self.H, self.W
        B = len(gt_index) - 1
        m = loss_cases.match(self.cfg, gt_bbox, s, tie_last=(mu == 11))
        ga = (self.anchors / (np.asarray([W, H], f32) / np.asarray([nW, nH], f32)))[self.mask[s]]
        pos, neg, ps = np.zeros((B, A, nH, nW), f32), np.ones((B, A, nH, nW), f32), np.zeros((B, A, nH, nW), f32)
        txy, twh = np.zeros((B, A, nH, nW, 2), f32), np.zeros((B, A, nH, nW, 2), f32)
        tiou, tcls = np.zeros((B, A, nH, nW), f32), np.full((B, A, nH, nW, C), self.ls_off, f32)
        omask, torien = np.zeros((B, A, H, W), np.int64), np.zeros((B, A, H, W, 2), f32)
        for b in range(B):
            g0, ng = int(gt_index[b]), int(gt_index[b + 1]) - int(gt_index[b])
            if ng == 0:
                continue
            # box: one lane per cell, all the image's GTs
            vis = min(ng, 256) if mu == 6 else ng
            iou = t["ious"][b]
            neg[b][(iou[:, :vis] > self.thr).any(1).reshape(A, nH, nW)] = 0
            iou4 = iou.reshape(A, nH, nW, -1)
            keys = m.key[g0:g0 + vis]
            for key in np.unique(keys[keys >= 0]):
                js = np.flatnonzero(keys == key)
                win = int(js[0] if mu == 5 else js[-1])
                a, rem = divmod(int(key), nH * nW)
                cy, cx = divmod(rem, nW)
                g = m.g[g0 + win]
                pos[b, a, cy, cx], neg[b, a, cy, cx] = 1, 0
                ps[b, a, cy, cx] = f32(2) - (g[2] * g[3]) / f32(nW * nH)
                txy[b, a, cy, cx] = [g[0] - f32(cx), g[1] - f32(cy)]
                twh[b, a, cy, cx] = [loss_np._log(g[2] / ga[a, 0]), loss_np._log(g[3] / ga[a, 1])]
                tiou[b, a, cy, cx] = iou4[a, cy, cx, win]
                for j in (js[:4] if mu == 4 else js):
                    tcls[b, a, cy, cx, int(gt_cls[g0 + j])] = self.ls_on
            # orientation: one workgroup per (anchor, 16 x 64 tile)
            for a in range(A):
                for y0 in range(0, H, FWD_TILE_H):
                    for x0 in range(0, W, FWD_TILE_W):
                        y1, x1 = min(y0 + FWD_TILE_H, H), min(x0 + FWD_TILE_W, W)
                        lst = self._cull(m, g0, ng, a, x0, x0 + FWD_TILE_W, y0, y0 + FWD_TILE_H, True)
                        if lst:
                            omask[b, a, y0:y1, x0:x1], torien[b, a, y0:y1, x0:x1] = self._walk(y0, y1, x0, x1, lst, m, gt_mask)
        for a in range(A):
            torien[:, a] = self._normalise(s, a, omask[:, a], torien[:, a])
        t.update(pos=pos, neg=neg, pscale=ps, txy=txy, twh=twh, tiou=tiou, tcls=tcls, omask=omask, torien=torien,
                 opos=omask < 0, oneg=omask > 0, match=m)
        self._built[s] = t
        return t

    def scale_grad(self, s, head, target, gout=1.0):
        g_bbox, g_full, near = super().scale_grad(s, head, target, gout)
        t = self.build_targets(s, head[0], *target)
        m = t["match"]
        gt_index, gt_mask = target[2], target[3]
        B, A, H, W = len(gt_index) - 1, len(self.mask[s]), self.H, self.W
        oh, ow = H // 4, W // 4
        up = loss_np.upsample4(np.asarray(head[1], f32)).reshape(B, A, 2, H, W).transpose(0, 1, 3, 4, 2)
        G = [float(gout) * float(self.scales_weight[s]) * float(w) for w in self.weight[s]]
        npos, nneg, nbox = float(t["opos"].sum()), float(t["oneg"].sum()), float(t["pos"].sum())
        cp = G[5] / B * nbox / npos if npos else 0.0
        cn = G[6] / B * nbox / nneg if nneg else 0.0
        uy, ux = loss_grad_np._up_matrix(oh), loss_grad_np._up_matrix(ow)
        halo = {9: 0, 10: 1}.get(self.mutant, 2)
        g = np.zeros((B, 2 * A, oh, ow), np.float64)
        for b in range(B):
            g0, ng = int(gt_index[b]), int(gt_index[b + 1]) - int(gt_index[b])
            for a in range(A if ng else 0):
                for qy0 in range(0, oh, GRAD_Q):
                    for qx0 in range(0, ow, GRAD_Q):
                        qy1, qx1 = min(qy0 + GRAD_Q, oh), min(qx0 + GRAD_Q, ow)
                        lst = self._cull(m, g0, ng, a, max(4 * qx0 - halo, 0), min(4 * (qx0 + GRAD_Q) + halo, W),
                                         max(4 * qy0 - halo, 0), min(4 * (qy0 + GRAD_Q) + halo, H), False)
                        if not lst:
                            continue
                        fy0, fy1 = max(4 * qy0 - 2, 0), min(4 * (qy0 + GRAD_Q) + 2, H)
                        fx0, fx1 = max(4 * qx0 - 2, 0), min(4 * (qx0 + GRAD_Q) + 2, W)
                        om, to = self._walk(fy0, fy1, fx0, fx1, lst, m, gt_mask)
                        tor = self._normalise(s, a, om, to)
                        x = up[b, a, fy0:fy1, fx0:fx1].astype(np.float64) - tor.astype(np.float64)
                        d = cp * (om < 0) + cn * (om > 0)
                        gz = np.where(np.abs(x) < 1, x, np.sign(x)) * d[..., None]
                        for c in range(2):
                            g[b, 2 * a + c, qy0:qy1, qx0:qx1] = uy[fy0:fy1, qy0:qy1].T @ gz[..., c] @ ux[fx0:fx1, qx0:qx1]
        return g_bbox, g, near


def run(name, mutant=None):
    """loss_cases.run_restatement's record for a case under TiledNP"""
    cfg, heads, target = loss_cases.build(name)
    return loss_cases.run_restatement(TiledNP(mutant, **cfg), heads, target)
