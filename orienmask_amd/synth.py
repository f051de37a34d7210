"""Build-owned, platform-stable synthetic weights and inputs.

There is no checkpoint and no COCO on the build or GPU boxes, so every bench and
parity run uses seeded synthetic data. The generators use numpy's PCG64 stream
only (never ``torch.manual_seed``) so that this container and the GPU box
regenerate identical bytes.

Shapes follow the reference's 524-key state_dict
(/root/reference/model/orienmask_yolo_fpnplus.py:9-72); the value distributions are
ours, chosen so that activations stay O(1) through the 75-conv-deep path and BatchNorm
is far from identity (a folded-BN bug cannot hide).
"""
import numpy as np
import torch

from .arch import model_convs, state_dict_entries, is_residual_tail


def _rng(seed):
    return np.random.Generator(np.random.PCG64(int(seed)))


def synth_state_dict(seed=0, num_anchors=3, num_classes=80, obj_bias=0.0, head_gain=1.0,
                     coord_gain=0.3, orien_gain=0.2, model="OrienMaskYOLOFPNPlus"):
    """Seeded reference-format state_dict (CPU float32 tensors, 524 keys).

    A random-weight network's head outputs vary far more across channels than across
    positions, so the final 1x1 convs get per-role gains: head_gain on the objectness and
    class rows (spreads the logits over positions), coord_gain on the tx/ty/tw/th rows
    (keeps exp(tw) sane) and orien_gain on the orientation head (keeps masks non-empty).
    obj_bias shifts the objectness logits: with head_gain=4, about -10 passes tens of
    thousands of pairs, -18 a few hundred, -24 none.
    """
    rng = _rng(seed)
    sd = {}
    for spec in model_convs(model, num_anchors, num_classes):
        fan_in = spec.cin * spec.ksize * spec.ksize
        for key, shape, role in state_dict_entries(spec):
            if role == "conv_w":
                std = np.sqrt(2.0 / fan_in)
                v = rng.standard_normal(shape, dtype=np.float32) * np.float32(std)
                if not spec.bn:
                    gain = np.full((spec.cout, 1, 1, 1), orien_gain / np.sqrt(2.0), dtype=np.float32)
                    if spec.name.startswith("bbox_head"):
                        gain[:] = head_gain / np.sqrt(2.0)
                        for a in range(num_anchors):
                            gain[a * (5 + num_classes):a * (5 + num_classes) + 4] = coord_gain / np.sqrt(2.0)
                    v = v * gain
            elif role == "bn_gamma":
                lo, hi = (0.1, 0.25) if is_residual_tail(spec) else (0.7, 1.3)
                v = rng.uniform(lo, hi, shape).astype(np.float32)
            elif role == "bn_beta":
                v = (rng.standard_normal(shape) * 0.1).astype(np.float32)
            elif role == "bn_mean":
                v = (rng.standard_normal(shape) * 0.1).astype(np.float32)
            elif role == "bn_var":
                v = rng.uniform(0.6, 1.6, shape).astype(np.float32)
            elif role == "bn_count":
                sd[key] = torch.tensor(1, dtype=torch.long)
                continue
            elif role == "conv_b":
                v = (rng.standard_normal(shape) * 0.1).astype(np.float32)
                if spec.name.startswith("bbox_head") and obj_bias != 0.0:
                    per_anchor = 5 + num_classes
                    v[4::per_anchor] += np.float32(obj_bias)
            else:  # pragma: no cover
                raise AssertionError(role)
            sd[key] = torch.from_numpy(np.ascontiguousarray(v))
    return sd


def synth_state_dict_stress(seed, norms=None, num_anchors=3, num_classes=80, obj_bias=-3.0, head_gain=0.7,
                            coord_gain=0.3, orien_gain=0.2, model="OrienMaskYOLOFPNPlus"):
    """Heavy-tailed variant of synth_state_dict for the split-operand stress fixtures (tools/gen_golden.py: fwd_stress_*):

      * folded BatchNorm scale gamma / sqrt(var + eps) LOG-UNIFORM over [1e-2, 1e2] per output channel (x 0.2 on the
        residual tails so that the residual streams stay inside fp16's range), realised with running_var log-uniform over
        [1e-4, 1e2] and ~5 % of the channels at running_var = 1e-6;
      * ~2 % of the convolution rows scaled down to max |w| = 1e-20 and ~2 % exactly zero (their outputs are the BatchNorm
        shift alone): the per-output-channel power-of-two scaling of the split weights must survive both;
      * activations therefore span ~1e-6 ... 1e3 within one tensor.

    norms: one float32 per convolution (model_convs order) multiplying its weights, so that its pre-BatchNorm output has
    unit rms on the calibration input -- measured by tools/gen_golden.py through the reference model and STORED in the
    fixture, so that every machine regenerates the same bytes (None: all ones, the generator's first pass)."""
    rng = _rng(seed)
    specs = list(model_convs(model, num_anchors, num_classes))
    if norms is None:
        norms = np.ones(len(specs), dtype=np.float32)
    norms = np.asarray(norms, dtype=np.float32)
    assert norms.shape == (len(specs),)
    sd = {}
    for li, spec in enumerate(specs):
        fan_in = spec.cin * spec.ksize * spec.ksize
        cout = spec.cout
        w = rng.standard_normal((cout, spec.cin, spec.ksize, spec.ksize), dtype=np.float32) * np.float32(np.sqrt(1.0 / fan_in))
        w = w * norms[li]
        kind = rng.random(cout)
        if spec.bn:
            s = np.power(10.0, rng.uniform(-2.0, 2.0, cout))                     # folded scale, log-uniform
            if is_residual_tail(spec):
                s = s * 0.2
            var = np.power(10.0, rng.uniform(-4.0, 2.0, cout))
            var[rng.random(cout) < 0.05] = 1e-6
            gamma = s * np.sqrt(var + 1e-5)
            mean = rng.standard_normal(cout) * 0.3
            beta = rng.standard_normal(cout) * 0.1 * s
            tiny, zero = kind < 0.02, (kind >= 0.02) & (kind < 0.04)
            for c in np.nonzero(tiny)[0]:
                w[c] *= np.float32(1e-20) / np.abs(w[c]).max()
            w[zero] = 0.0
            p = spec.name + ".conv_block"
            sd[p + ".0.weight"] = torch.from_numpy(np.ascontiguousarray(w))
            sd[p + ".1.weight"] = torch.from_numpy(gamma.astype(np.float32))
            sd[p + ".1.bias"] = torch.from_numpy(beta.astype(np.float32))
            sd[p + ".1.running_mean"] = torch.from_numpy(mean.astype(np.float32))
            sd[p + ".1.running_var"] = torch.from_numpy(var.astype(np.float32))
            sd[p + ".1.num_batches_tracked"] = torch.tensor(1, dtype=torch.long)
        else:
            gain = np.full((cout, 1, 1, 1), orien_gain, dtype=np.float32)
            b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            if spec.name.startswith("bbox_head"):
                per_anchor = 5 + num_classes
                gain[:] = head_gain
                for a in range(num_anchors):
                    gain[a * per_anchor:a * per_anchor + 4] = coord_gain
                b[4::per_anchor] += np.float32(obj_bias)
            sd[spec.name + ".weight"] = torch.from_numpy(np.ascontiguousarray(w * gain))
            sd[spec.name + ".bias"] = torch.from_numpy(b)
    return sd


def synth_state_dict_trained(seed, stats=None, num_anchors=3, num_classes=80, obj_bias=-3.0, head_gain=0.7,
                             coord_gain=0.1, orien_gain=0.2, model="OrienMaskYOLOFPNPlus"):
    """Weights with the statistics of a CONVERGED network (tools/gen_golden.py: fwd_trained_*; VERDICT round 5, task 8) -- what
    stands in for the checkpoint that does not exist offline when the split representation's range guard (|activation| < 6550)
    is to meet realistic activations:

      * every BatchNorm's running_mean / running_var MATCH the statistics of its own input (as training leaves them), up to a
        dataset-vs-batch mismatch of ~20 %: measured by tools/gen_golden.py through the reference model on the fixture's input
        and STORED in the fixture (`stats` = (means, vars, head_norms): per BatchNorm channel in model_convs order, and one
        factor per bias-only head convolution), so that every machine regenerates the same bytes;
      * gamma heavy-tailed -- log-normal (sigma 0.5) around 1 with 0.5 % of the channels 20x larger -- and beta ~ N(0, 0.3) with
        the same outlier channels shifted by +-10: single channels of a tensor reach |x| in the hundreds while its bulk stays
        O(1), and the residual streams accumulate them block after block;
      * convolution weights He-initialised (their scale is irrelevant in front of a matched BatchNorm); the box-size logits kept
        small (coord_gain 0.1: the outlier channels give the head inputs heavy tails, and exp(t) of a logit of 5 is a box a
        hundred images wide).

    stats=None: placeholder statistics (mean 0, variance 1) for the generator's calibration pass."""
    rng = _rng(seed)
    specs = list(model_convs(model, num_anchors, num_classes))
    n_bn = sum(s_.cout for s_ in specs if s_.bn)
    n_head = sum(1 for s_ in specs if not s_.bn)
    if stats is None:
        means, vars_, head_norms = np.zeros(n_bn, np.float32), np.ones(n_bn, np.float32), np.ones(n_head, np.float32)
    else:
        means, vars_, head_norms = (np.asarray(v, dtype=np.float32) for v in stats)
    assert means.shape == (n_bn,) and vars_.shape == (n_bn,) and head_norms.shape == (n_head,)
    sd = {}
    off = hi = 0
    for spec in specs:
        fan_in = spec.cin * spec.ksize * spec.ksize
        cout = spec.cout
        w = rng.standard_normal((cout, spec.cin, spec.ksize, spec.ksize), dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_in))
        if spec.bn:
            gamma = np.exp(rng.standard_normal(cout) * 0.5)
            beta = rng.standard_normal(cout) * 0.3
            outlier = rng.random(cout) < 0.005
            gamma[outlier] *= 20.0
            beta[outlier] += np.where(rng.random(int(outlier.sum())) < 0.5, -10.0, 10.0)
            p = spec.name + ".conv_block"
            sd[p + ".0.weight"] = torch.from_numpy(np.ascontiguousarray(w))
            sd[p + ".1.weight"] = torch.from_numpy(gamma.astype(np.float32))
            sd[p + ".1.bias"] = torch.from_numpy(beta.astype(np.float32))
            sd[p + ".1.running_mean"] = torch.from_numpy(means[off:off + cout].copy())
            sd[p + ".1.running_var"] = torch.from_numpy(vars_[off:off + cout].copy())
            sd[p + ".1.num_batches_tracked"] = torch.tensor(1, dtype=torch.long)
            off += cout
        else:
            gain = np.full((cout, 1, 1, 1), orien_gain, dtype=np.float32)
            b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
            if spec.name.startswith("bbox_head"):
                per_anchor = 5 + num_classes
                gain[:] = head_gain
                for a in range(num_anchors):
                    gain[a * per_anchor:a * per_anchor + 4] = coord_gain
                b[4::per_anchor] += np.float32(obj_bias)
            sd[spec.name + ".weight"] = torch.from_numpy(np.ascontiguousarray(w * gain * head_norms[hi]))
            sd[spec.name + ".bias"] = torch.from_numpy(b)
            hi += 1
    return sd


def synth_image_batch_stress(seed, batch, height, width):
    """[B,3,H,W] float32 in [0,1] with SATURATED rectangles (exactly 1.0), NEAR-ZERO rectangles (~1e-6) and a smooth ramp over
    uniform noise: the input of the split-operand stress fixtures."""
    rng = _rng(seed)
    x = rng.random((batch, 3, height, width), dtype=np.float32)
    for b in range(batch):
        for k in range(8):
            h = int(rng.integers(height // 8, height // 2)); w = int(rng.integers(width // 8, width // 2))
            y0 = int(rng.integers(0, height - h)); x0 = int(rng.integers(0, width - w))
            if k % 3 == 0:
                x[b, :, y0:y0 + h, x0:x0 + w] = 1.0
            elif k % 3 == 1:
                x[b, :, y0:y0 + h, x0:x0 + w] = rng.random((3, h, w), dtype=np.float32) * np.float32(1e-6)
            else:
                ramp = np.linspace(0.0, 1.0, w, dtype=np.float32)[None, None, :]
                x[b, :, y0:y0 + h, x0:x0 + w] = ramp * x[b, :, y0:y0 + h, x0:x0 + w]
    return torch.from_numpy(x)


def synth_image_batch(seed, batch, height=544, width=544):
    """[B,3,H,W] float32 in [0,1): what FastCOCOTransform hands the model
    (/root/reference/config/base.py:158-164, Normalize std=255)."""
    rng = _rng(seed)
    x = rng.random((batch, 3, height, width), dtype=np.float32)
    return torch.from_numpy(x)


def synth_photo_batch(seed, batch, height, width):
    """[n,h,w,3] float32 with integer values 0..255: what infer.py builds from cv2.imread + cvtColor
    (/root/reference/infer.py:147-149) before FastCOCOTransform."""
    rng = _rng(seed)
    return torch.from_numpy(np.floor(rng.random((batch, height, width, 3)) * 256).astype(np.float32))


def _ulp_steps(x, k):
    """float32 x moved by k units in the last place (k may be negative)."""
    v = np.float32(x)
    i = v.view(np.int32)
    i = i + np.int32(k) if v >= 0 else i - np.int32(k)
    return i.view(np.float32)


def _plant_ties(rng, bbox, regime, nh, nw, grid_sizes, num_anchors, num_classes):
    """Near-tie structures of the 'ties_*' regimes (see synth_heads); all of them live on the finest scale."""
    if (nh, nw) != tuple(grid_sizes[-1]):
        return
    batch = bbox.shape[0]
    for b in range(batch):
        if regime == "ties_cut":
            # 39 clusters of 9 cells voting for one box each (the 'clustered' construction) ...
            cells = [(y, x) for y in range(2, nh - 2, 4) for x in range(2, nw - 2, 4)]
            order = rng.permutation(len(cells))
            n_clusters = min(39, len(cells) // 2)
            for ci in order[:n_clusters]:
                y, x = cells[ci]
                a = int(rng.integers(num_anchors)); c = int(rng.integers(num_classes))
                ob = 4.0 + rng.random(); cl = 4.0 + rng.random()
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        bbox[b, a, 0, y + dy, x + dx] = -3.0 * dx
                        bbox[b, a, 1, y + dy, x + dx] = -3.0 * dy
                        bbox[b, a, 2:4, y + dy, x + dx] = 1.2
                        bbox[b, a, 4, y + dy, x + dx] = ob - 0.2 * (abs(dy) + abs(dx)) - 0.1 * rng.random()
                        bbox[b, a, 5 + c, y + dy, x + dx] = cl
            # ... and the ladder: isolated small boxes on the remaining cluster sites, class logits 12 ulps apart
            # (confidence steps of 1-3 ulps, strictly monotone within one sigmoid implementation), visited in a shuffled order so that index order != score order
            sites = [cells[ci] for ci in order[n_clusters:]]
            n_lad = min(120, 4 * len(sites))
            ks = rng.permutation(n_lad)
            for j in range(n_lad):
                y, x = sites[j // 4]
                dy, dx = ((0, 0), (0, 2), (2, 0), (2, 2))[j % 4]       # 4 ladder boxes per site, two cells apart
                a = 0
                # one sigmoid implementation per image (torch evaluates classes below (C/32)*32 with Sleef, the rest with
                # glibc's expf, csrc/ref_math.h): a ladder that mixed them would contain exact ties, whose order inside
                # torch.topk is unspecified
                nvec = (num_classes // 32) * 32
                c = int(rng.integers(nvec)) if (b % 2 == 0 or nvec == num_classes) else nvec + int(rng.integers(num_classes - nvec))
                bbox[b, a, 0:2, y + dy, x + dx] = 0.0
                bbox[b, a, 2:4, y + dy, x + dx] = -1.0                   # small boxes: never overlap their neighbours
                bbox[b, a, 4, y + dy, x + dx] = 0.5
                bbox[b, a, 5 + c, y + dy, x + dx] = _ulp_steps(0.25, 12 * int(ks[j]))
        elif regime == "ties_thresh":
            # sigma(ob) * sigma(cl) = conf_thresh at the middle of the ladder (solved in float64)
            ob = np.float32(-2.9444389791664403)                          # logit(0.05)
            so = 1.0 / (1.0 + np.exp(-np.float64(ob)))
            target = 0.005 / so
            cl0 = np.float32(np.log(target / (1.0 - target)))
            cells = [(y, x) for y in range(1, nh - 1, 2) for x in range(1, nw - 1, 2)]
            order = rng.permutation(len(cells))
            n_lad = min(120, len(cells))
            ks = rng.permutation(n_lad) - n_lad // 2
            for j in range(n_lad):
                y, x = cells[order[j]]
                c = int(rng.integers(num_classes))
                bbox[b, 1, 0:2, y, x] = 0.0
                bbox[b, 1, 2:4, y, x] = -1.5
                bbox[b, 1, 4, y, x] = ob
                bbox[b, 1, 5 + c, y, x] = _ulp_steps(cl0, int(ks[j]))
        elif regime == "ties_iou":
            # anchor slot 2 of the finest scale; tw = th = 0 -> w, h = the anchor exactly.  Pair (x, x+1): IoU = 0.5 when the
            # centre distance is w / 3; the left box's tx walks through that point in steps of 8 ulps (~0.6 IoU ulps)
            from math import log
            a = num_anchors - 1
            w_cells = None
            k = 0
            for y in range(4, nh - 3, 8):
                for x in range(2, nw - 9, 8):
                    if k >= 64:
                        break
                    if w_cells is None:
                        w_cells = 40.0 / 8.0                              # ANCHORS_YOLOV4[2] = 40 px wide, 8 px cells
                    s2 = 1.0 / (1.0 + np.exp(-2.0))
                    s1 = s2 + 1.0 - w_cells / 3.0                         # (1 + s2 - s1) = w / 3 in cell units
                    t1 = np.float32(log(s1 / (1.0 - s1)))
                    for xx, tx, ob in ((x, _ulp_steps(t1, 8 * (k - 32)), 3.0), (x + 1, np.float32(2.0), 2.0)):
                        bbox[b, a, 0, y, xx] = tx
                        bbox[b, a, 1, y, xx] = 0.0
                        bbox[b, a, 2:4, y, xx] = 0.0
                        bbox[b, a, 4, y, xx] = ob
                        bbox[b, a, 5, y, xx] = 3.0                        # class 0: no class offset on the corners
                    k += 1


def synth_heads(seed, batch, grid_sizes, num_anchors=3, num_classes=80, regime="mixed",
                orien_scale=4):
    """Seeded head tensors in the model's output format, for postprocess-only tests.

    Returns ((bbox32, orien32), (bbox16, orien16), (bbox8, orien8)) with
    bbox_s [B, A*(5+C), nH_s, nW_s] and orien_s [B, A*2, H/4, W/4], shaped like
    /root/reference/model/orienmask_yolo_fpnplus.py:88-90.

    regime: 'dense'       - every (candidate, class) pair passes conf_thresh (worst case)
            'mixed'       - well over nms_pre pairs pass (top-k branch), NMS suppresses many
            'clustered'   - over nms_pre pairs pass but they sit in ~60 tight clusters, so fewer
                            than nms_post survive NMS
            'sparse'      - fewer than nms_pre pairs pass, fewer than nms_post survive NMS
            'sparse_many' - fewer than nms_pre pairs pass, more than nms_post survive NMS
            'empty'       - nothing passes (K = 0)
            'ties_cut'    - adversarial: ~39 tight clusters (351 strong pairs) plus a LADDER of 120 isolated boxes whose class
                            logits are 12 float32 ulps apart, so their confidences are 1-3 ulps apart and the
                            top-nms_pre cut falls inside the ladder; which ladder members survive is visible in the output
            'ties_thresh' - adversarial: ~40 clear detections plus a ladder of 120 pairs whose confidences step through
                            conf_thresh = 0.005 about two ulps at a time
            'ties_iou'    - adversarial: 64 isolated pairs of same-class boxes in neighbouring cells whose IoU steps through
                            0.5 a fraction of an ulp at a time (log-sizes 0, so the sizes are exact in any exp)
    The orientation maps are smooth fields pointing roughly at random centres so that
    masks are blobs rather than noise.
    """
    rng = _rng(seed)
    per_anchor = 5 + num_classes
    total = sum(num_anchors * nh * nw for nh, nw in grid_sizes)
    target_active = {"dense": 0, "mixed": 700, "clustered": 60, "sparse": 55, "sparse_many": 260,
                     "empty": 0, "ties_cut": 0, "ties_thresh": 22, "ties_iou": 0}[regime]
    target_active = min(target_active, total // 3)
    out = []
    oh = grid_sizes[-1][0] * 8 // orien_scale
    ow = grid_sizes[-1][1] * 8 // orien_scale
    for (nh, nw) in grid_sizes:
        bbox = rng.standard_normal((batch, num_anchors, per_anchor, nh, nw), dtype=np.float32)
        bbox[:, :, 2:4] *= 0.5
        if regime == "dense":
            bbox[:, :, 4] *= 2.0
            bbox[:, :, 5:] *= 1.5
        else:
            bbox[:, :, 4] = bbox[:, :, 4] * 0.5 - 14.0
            bbox[:, :, 5:] = bbox[:, :, 5:] * 0.5 - 10.0
            n_here = int(round(target_active * (num_anchors * nh * nw) / total))
            for b in range(batch):
                for _ in range(n_here):
                    a = int(rng.integers(num_anchors)); y = int(rng.integers(nh)); x = int(rng.integers(nw))
                    c = int(rng.integers(num_classes))
                    ob = 1.0 + 1.5 * rng.standard_normal(); cl = 1.0 + 1.5 * rng.standard_normal()
                    bbox[b, a, 4, y, x] = ob
                    bbox[b, a, 5 + c, y, x] = cl
                    if rng.random() < 0.3 and regime != "clustered":   # a second class on the same box
                        bbox[b, a, 5 + int(rng.integers(num_classes)), y, x] = cl - 1.0
                    if regime == "clustered":
                        # a 3x3 block of cells all voting for one box: centres pulled towards
                        # the middle cell, same class, same size -> NMS keeps about one each
                        bbox[b, a, 4, y, x] = ob = 2.0 + abs(ob)
                        bbox[b, a, 5 + c, y, x] = cl = 2.0 + abs(cl)
                        bbox[b, a, 2:4, y, x] = 1.2
                        for dy in (-1, 0, 1):
                            for dx in (-1, 0, 1):
                                yy, xx = y + dy, x + dx
                                if not (0 <= yy < nh and 0 <= xx < nw):
                                    continue
                                if dy or dx:
                                    bbox[b, a, :, yy, xx] = bbox[b, a, :, y, x]
                                    bbox[b, a, 4, yy, xx] = ob - 0.2 * (abs(dy) + abs(dx)) - 0.1 * rng.random()
                                bbox[b, a, 0, yy, xx] = -3.0 * dx
                                bbox[b, a, 1, yy, xx] = -3.0 * dy
                    if regime == "mixed" and rng.random() < 0.6 and x + 1 < nw:
                        # a near-duplicate in the neighbouring cell: same class, same size,
                        # centre pulled back towards the original so the IoU is high
                        bbox[b, a, :, y, x + 1] = bbox[b, a, :, y, x]
                        bbox[b, a, 0, y, x] = 2.0; bbox[b, a, 0, y, x + 1] = -2.0
                        bbox[b, a, 2:4, y, x] = 0.7; bbox[b, a, 2:4, y, x + 1] = 0.7
                        bbox[b, a, 4, y, x + 1] = ob - 0.5
        if regime.startswith("ties"):
            _plant_ties(rng, bbox, regime, nh, nw, grid_sizes, num_anchors, num_classes)
        ys = (np.arange(oh, dtype=np.float32) + 0.5) / oh
        xs = (np.arange(ow, dtype=np.float32) + 0.5) / ow
        orien = np.empty((batch, num_anchors, 2, oh, ow), dtype=np.float32)
        for b in range(batch):
            for a in range(num_anchors):
                cx, cy = rng.random(2)
                s = 2.0 + 6.0 * rng.random()
                orien[b, a, 0] = (cx - xs)[None, :] * s + 0.3 * rng.standard_normal((oh, ow), dtype=np.float32)
                orien[b, a, 1] = (cy - ys)[:, None] * s + 0.3 * rng.standard_normal((oh, ow), dtype=np.float32)
        out.append((torch.from_numpy(bbox.reshape(batch, num_anchors * per_anchor, nh, nw).copy()),
                    torch.from_numpy(orien.reshape(batch, num_anchors * 2, oh, ow).copy())))
    return tuple(out)


def _fill_polygon(vx, vy, H, W):
    """Even-odd fill of one polygon (float64 vertices, pixel units) sampled at pixel centres: bool [H, W]."""
    ys = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xs = np.arange(W, dtype=np.float64)[None, :] + 0.5
    inside = np.zeros((H, W), dtype=bool)
    n = len(vx)
    for i in range(n):
        x0, y0, x1, y1 = vx[i], vy[i], vx[(i + 1) % n], vy[(i + 1) % n]
        if y0 == y1:
            continue
        crosses = (ys >= min(y0, y1)) & (ys < max(y0, y1))
        xi = x0 + (ys - y0) * (x1 - x0) / (y1 - y0)
        inside ^= crosses & (xs < xi)
    return inside


def synth_targets(seed, batch, height, width, gts_per_image=7, num_classes=80, vertices=9):
    """Seeded targets in the reference's collate format (the reference's data/collate.py:13-30: gt_bbox [N,4] normalised cx, cy, w, h
    float32, gt_cls [N] int64, gt_index [B+1] int64, gt_mask [N,H,W] bool), as numpy arrays.

    Every instance is a filled star-shaped polygon inside its box; `gts_per_image` is an int or a list (one count per image).
    Box sizes span small to large so that every scale gets positives."""
    rng = _rng(seed)
    counts = [int(gts_per_image)] * batch if np.isscalar(gts_per_image) else [int(c) for c in gts_per_image]
    boxes, classes, masks = [], [], []
    for b in range(batch):
        for _ in range(counts[b]):
            w = float(np.exp(rng.uniform(np.log(8.0), np.log(0.8 * width))))
            h = float(np.clip(w * np.exp(rng.normal(0.0, 0.4)), 6.0, 0.9 * height))
            cx = float(rng.uniform(w / 4, width - w / 4))
            cy = float(rng.uniform(h / 4, height - h / 4))
            ang = np.sort(rng.uniform(0, 2 * np.pi, vertices))
            rad = rng.uniform(0.45, 1.0, vertices)
            vx = np.clip(cx + np.cos(ang) * rad * w / 2, 0, width)
            vy = np.clip(cy + np.sin(ang) * rad * h / 2, 0, height)
            boxes.append([cx / width, cy / height, w / width, h / height])
            classes.append(int(rng.integers(num_classes)))
            masks.append(_fill_polygon(vx, vy, height, width))
    index = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    gt_bbox = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    gt_mask = np.asarray(masks, dtype=bool).reshape(-1, height, width)
    return gt_bbox, np.asarray(classes, dtype=np.int64), index, gt_mask


def synth_coco_sample(seed, height, width, n_gt, border=False, with_info=True, image_id=0):
    """One sample as the reference's COCODataset._load_sample_data returns it (data/dataset.py:70-87): image [h,w,3] float32 RGB
    holding uint8 values, bbox [n,4] float32 (cx, cy, w, h normalised), cls [n] int64, mask = list of n uint8 [h,w] 0/1 arrays
    (elliptic blobs, each inside its box), info {id, height, width}.  border=True puts the first GT against the image's corner."""
    rng = _rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = rng.uniform(0, 255, 3)[None, None, :] + 60 * np.sin(xx[..., None] / (3 + 7 * rng.random(3)) + yy[..., None] / (4 + 9 * rng.random(3)))
    image = np.clip(np.rint(base + rng.normal(0, 25, (height, width, 3))), 0, 255).astype(np.float32)
    boxes, masks = [], []
    for k in range(n_gt):
        bw, bh = rng.integers(1, max(2, width // 2) + 1), rng.integers(1, max(2, height // 2) + 1)
        x0 = 0 if (border and k == 0) else int(rng.integers(0, width - bw + 1))
        y0 = 0 if (border and k == 0) else int(rng.integers(0, height - bh + 1))
        if border and k == 1:
            x0, y0 = width - bw, height - bh
        cx, cy = x0 + bw / 2.0, y0 + bh / 2.0
        m = (((xx + 0.5 - cx) / (bw / 2.0)) ** 2 + ((yy + 0.5 - cy) / (bh / 2.0)) ** 2 <= 1.0).astype(np.uint8)
        if border and k < 2:
            m[y0:y0 + bh, x0:x0 + bw] = 1           # the full box: the mask touches the image's edge
        masks.append(m)
        boxes.append([cx / width, cy / height, bw / width, bh / height])
    sample = {"image": image, "bbox": np.array(boxes, np.float32).reshape(-1, 4),
              "cls": rng.integers(0, 80, n_gt).astype(np.int64), "mask": masks}
    if with_info:
        sample["info"] = {"id": image_id, "height": height, "width": width}
    return sample


def synth_segm_sample(seed, height, width, n_gt, crowd=False, with_info=True, image_id=0):
    """synth_coco_sample's sample with its masks as the annotation json would hold them ('segm', no pixel): each GT is 1-3
    polygons of 20-200 vertices (wobbly ellipses, coordinates rounded to 2 decimals as COCO's are), except that with crowd=True
    the last GT is an uncompressed RLE ({'size', 'counts'}) of a few blobs, as COCO stores iscrowd annotations.  The image is
    uint8; bbox is the polygons' extent clipped to the image."""
    rng = _rng(seed)
    image = rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    boxes, segm = [], []
    for k in range(n_gt):
        cx, cy = rng.uniform(0.15, 0.85) * width, rng.uniform(0.15, 0.85) * height
        rx, ry = rng.uniform(0.05, 0.3) * width, rng.uniform(0.05, 0.3) * height
        if crowd and k == n_gt - 1:
            yy, xx = np.mgrid[0:height, 0:width]
            m = np.zeros((height, width), bool)
            for _ in range(4):
                ox, oy = rng.uniform(-rx, rx), rng.uniform(-ry, ry)
                m |= ((xx - cx - ox) / (rx / 2)) ** 2 + ((yy - cy - oy) / (ry / 2)) ** 2 <= 1.0
            flat = m.T.ravel()
            edges = np.flatnonzero(np.diff(flat)) + 1
            runs = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
            segm.append({"size": [height, width], "counts": ([0] if flat[0] else []) + [int(r) for r in runs]})
            ys, xs = np.nonzero(m)
            x0, x1, y0, y1 = (xs.min(), xs.max() + 1, ys.min(), ys.max() + 1) if len(xs) else (0, 1, 0, 1)
        else:
            polys = []
            for _ in range(int(rng.integers(1, 4))):
                n = int(rng.integers(20, 201))
                a = np.sort(rng.uniform(0, 2 * np.pi, n))
                r = 1 + 0.25 * np.sin(3 * a + rng.uniform(0, 6)) + rng.uniform(-0.1, 0.1, n)
                ox, oy = rng.uniform(-0.5, 0.5) * rx, rng.uniform(-0.5, 0.5) * ry
                x = np.clip(cx + ox + 0.6 * rx * r * np.cos(a), 0, width)
                y = np.clip(cy + oy + 0.6 * ry * r * np.sin(a), 0, height)
                polys.append(np.round(np.stack([x, y], 1).ravel(), 2).tolist())
            segm.append(polys)
            allx = np.concatenate([np.asarray(p)[0::2] for p in polys])
            ally = np.concatenate([np.asarray(p)[1::2] for p in polys])
            x0, x1, y0, y1 = allx.min(), allx.max(), ally.min(), ally.max()
        boxes.append([(x0 + x1) / 2 / width, (y0 + y1) / 2 / height, max(x1 - x0, 1) / width, max(y1 - y0, 1) / height])
    sample = {"image": image, "bbox": np.array(boxes, np.float32).reshape(-1, 4),
              "cls": rng.integers(0, 80, n_gt).astype(np.int64), "segm": segm}
    if with_info:
        sample["info"] = {"id": image_id, "height": height, "width": width}
    return sample


def synth_segm_batch(seed=0, batch=32, height=480, width=640, mean_gt=7, crowd_every=4):
    """A batch of COCO-like proportions for tools/bench_segm_decode.py: `batch` sources of height x width with about mean_gt GTs
    each (Poisson, at least 0) and one crowd RLE in every crowd_every-th image."""
    rng = _rng(seed)
    out = []
    for b in range(batch):
        n = int(rng.poisson(mean_gt))
        crowd = crowd_every > 0 and b % crowd_every == crowd_every - 1 and n > 0
        out.append(synth_segm_sample(1000 * seed + b, height, width, n, crowd=crowd, image_id=b))
    return out
