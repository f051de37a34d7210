"""Float64 restatement of the cv2 float code paths the reference's COCOTransform runs (DESIGN.md "Training augmentation"), and of
the whole device pipeline from a planned sample (orienmask_amd.augment).  Index arithmetic follows cv2 exactly (float32 linear
coefficients, double nearest indices); pixel arithmetic is float64.

  cvtColor RGB2GRAY / RGB2HSV / HSV2RGB   color_rgb RGB2Gray<float>, color_hsv RGB2HSV_f / HSV2RGB_f (hrange 360)
  resize_linear / resize_nearest          resize.cpp INTER_LINEAR (INTER_AREA at an exact 2x downscale), resizeNN
  copy_make_border                        BORDER_CONSTANT
  render(plan)                            the collated image and masks of one planned sample

Not checked against cv2 itself (cv2 is not a dependency of this project): this is what the kernels and the fixtures agree on.
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
GRAY = tuple(float(np.float32(c)) for c in (0.299, 0.587, 0.114))
INTER_NEAREST, INTER_LINEAR, INTER_AREA = 0, 1, 3
COLOR_RGB2GRAY, COLOR_RGB2HSV, COLOR_HSV2RGB = 7, 41, 55
BORDER_CONSTANT = 0
# cv2 HSV2RGB_f: sector -> (b, g, r) indices into tab = [v, v(1-s), v(1-sh), v(1-s(1-h))]
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def gray(img):
    img = np.asarray(img, np.float64)
    return img[..., 0] * GRAY[0] + img[..., 1] * GRAY[1] + img[..., 2] * GRAY[2]


def rgb2hsv(img):
    img = np.asarray(img, np.float64)
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = v - vmin
    s = diff / (np.abs(v) + FLT_EPSILON)
    k = 60.0 / (diff + FLT_EPSILON)
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + 120.0, (r - g) * k + 240.0))
    h = np.where(h < 0, h + 360.0, h)
    return np.stack([h, s, v], axis=-1)


def hsv2rgb(hsv):
    hsv = np.asarray(hsv, np.float64)
    h, s, v = hsv[..., 0] * (6.0 / 360.0), hsv[..., 1], hsv[..., 2]
    h = np.mod(h, 6.0)
    sector = np.floor(h).astype(np.int64)
    h = h - sector
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, 0.0, h)
    tab = np.stack([v, v * (1 - s), v * (1 - s * h), v * (1 - s * (1 - h))], axis=-1)
    idx = SECTOR[sector]
    b = np.take_along_axis(tab, idx[..., 0:1], -1)[..., 0]
    g = np.take_along_axis(tab, idx[..., 1:2], -1)[..., 0]
    r = np.take_along_axis(tab, idx[..., 2:3], -1)[..., 0]
    out = np.stack([r, g, b], axis=-1)
    return np.where((s == 0)[..., None], v[..., None], out)


def linear_coeffs(dst, src):
    """cv2 INTER_LINEAR along one axis: (s0, s1, w1) with w1 the float32 fraction; 1 - w1 weighs s0."""
    scale = 1.0 / (float(dst) / src)
    f = (((np.arange(dst, dtype=np.float64) + 0.5) * scale) - 0.5).astype(np.float32)
    s0 = np.floor(f).astype(np.int64)
    f = (f - s0.astype(np.float32)).astype(np.float32)
    lo = s0 < 0
    s0[lo], f[lo] = 0, 0
    hi = s0 >= src - 1
    s0[hi], f[hi] = src - 1, 0
    s1 = np.minimum(s0 + 1, src - 1)
    return s0, s1, f.astype(np.float64), (np.float32(1) - f.astype(np.float32)).astype(np.float64)


def is_area2x(src_hw, dst_hw):
    return src_hw[0] == 2 * dst_hw[0] and src_hw[1] == 2 * dst_hw[1]


def resize_linear(img, dsize):
    """img [h,w,c] -> [dh,dw,c] float64; dsize = (dw, dh) as cv2 takes it."""
    img = np.asarray(img, np.float64)
    dw, dh = dsize
    h, w = img.shape[:2]
    if is_area2x((h, w), (dh, dw)):
        return (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2]) * 0.25
    x0, x1, fx, ax = linear_coeffs(dw, w)
    y0, y1, fy, ay = linear_coeffs(dh, h)
    ex = (slice(None),) + (None,) * (img.ndim - 2)
    rows = img[:, x0] * ax[ex] + img[:, x1] * fx[ex]
    ey = (slice(None), None) + (None,) * (img.ndim - 2)
    return rows[y0] * ay[ey] + rows[y1] * fy[ey]


def nearest_index(dst, src):
    ifx = 1.0 / (float(dst) / src)
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * ifx).astype(np.int64), src - 1)


def resize_nearest(img, dsize):
    dw, dh = dsize
    return img[nearest_index(dh, img.shape[0])][:, nearest_index(dw, img.shape[1])]


def copy_make_border(img, top, bottom, left, right, value):
    h, w = img.shape[:2]
    out = np.empty((h + top + bottom, w + left + right) + img.shape[2:], img.dtype)
    if img.ndim == 3:
        out[...] = np.asarray(value, img.dtype)[:img.shape[2]]
    else:
        out[...] = np.asarray(value, img.dtype).reshape(-1)[0]
    out[top:top + h, left:left + w] = img
    return out


# ---- the jitter ops of BaseTransform (adjust_*), float64 ------------------------------------------------------------
def jitter(img, ops, mut=()):
    img = np.asarray(img, np.float64)
    for code, f in ops:
        if code == 0:
            img = np.clip(img * f, 0, 255)
        elif code == 1:
            img = np.clip(img * f + gray(img).mean() * (1 - f), 0, 255)
        elif code == 2:
            img = np.clip(img * f + gray(img)[..., None] * (1 - f), 0, 255)
        else:
            hsv = rgb2hsv(img)
            hsv[..., 0] = np.mod(hsv[..., 0] + f * 360, 360) if "hue_wrap" in mut else np.clip(hsv[..., 0] + f * 360, 0, 360)
            img = hsv2rgb(hsv)
    return img


def seam_hue(img, ops):
    """Float64 hue (before the shift) that the hue op sees at each source pixel, or None when the chain has no hue."""
    img = np.asarray(img, np.float64)
    for k, (code, _) in enumerate(ops):
        if code == 3:
            return rgb2hsv(jitter(img, ops[:k]))[..., 0]
    return None


def _geometry(plan, src):
    top, left, ch, cw = plan['crop']
    nh, nw, pt, pl = plan['resize']
    oh, ow = plan['out']
    return src[top:top + ch, left:left + cw], (nh, nw, pt, pl, oh, ow)


def _flip(a, plan):
    if plan['hflip']:
        a = np.flip(a, axis=-1 if a.ndim == 2 else 1)
    if plan['vflip']:
        a = np.flip(a, axis=0)
    return a


def _resize_image_edge(img, plan):
    """Mutation 'image_edge': INTER_LINEAR whose taps clamp at the SOURCE image's border instead of the crop window's."""
    top, left, ch, cw = plan['crop']
    nh, nw = plan['resize'][:2]

    def axis(dst, src, off, full):
        scale = 1.0 / (float(dst) / src)
        f = (((np.arange(dst, dtype=np.float64) + 0.5) * scale) - 0.5).astype(np.float32)
        s0 = np.floor(f).astype(np.int64)
        f = (f - s0.astype(np.float32)).astype(np.float64)
        g0 = s0 + off
        lo, hi = g0 < 0, g0 >= full - 1
        g0[lo], f[lo] = 0, 0
        g0[hi], f[hi] = full - 1, 0
        return g0, np.minimum(g0 + 1, full - 1), f

    x0, x1, fx = axis(nw, cw, left, img.shape[1])
    y0, y1, fy = axis(nh, ch, top, img.shape[0])
    rows = img[:, x0] * (1 - fx)[:, None] + img[:, x1] * fx[:, None]
    return rows[y0] * (1 - fy)[:, None, None] + rows[y1] * fy[:, None, None]


def render_image(image, plan, mut=()):
    """[3,H,W] float64: the collated, normalised image of one planned sample (image: the SOURCE [h,w,3]).  mut: deliberate bugs
    for the mutation tests ('image_edge', 'hue_wrap', 'flip_before_pad')."""
    img = jitter(image, plan['ops'], mut)
    win, (nh, nw, pt, pl, oh, ow) = _geometry(plan, img)
    res = _resize_image_edge(img, plan) if "image_edge" in mut else resize_linear(win, (nw, nh))
    pad = [float(np.float32(v)) for v in plan['pad_value']]
    if "flip_before_pad" in mut:
        out = copy_make_border(_flip(res, plan), pt, oh - nh - pt, pl, ow - nw - pl, pad)
    else:
        out = _flip(copy_make_border(res, pt, oh - nh - pt, pl, ow - nw - pl, pad), plan)
    mean = np.asarray(plan['mean'], np.float64)
    std = np.asarray(plan['std'], np.float64)
    return ((out - mean) / std).transpose(2, 0, 1)


def render_seam(image, plan, eps):
    """[H,W] bool: output pixels with a tap whose float64 hue lies within eps of the 0/360 seam (None when no hue op)."""
    h = seam_hue(image, plan['ops'])
    if h is None:
        return None
    near = ((h < eps) | (h > 360 - eps)).astype(np.float64)[..., None]
    win, (nh, nw, pt, pl, oh, ow) = _geometry(plan, near)
    if is_area2x(win.shape[:2], (nh, nw)):
        res = resize_linear(win, (nw, nh))
    else:       # any tap of the 2x2 footprint, weighted or not
        x0, x1, _, _ = linear_coeffs(nw, win.shape[1])
        y0, y1, _, _ = linear_coeffs(nh, win.shape[0])
        res = np.maximum(np.maximum(win[y0][:, x0], win[y0][:, x1]), np.maximum(win[y1][:, x0], win[y1][:, x1]))
    out = copy_make_border(res, pt, oh - nh - pt, pl, ow - nw - pl, [0, 0, 0])
    return _flip(out, plan)[..., 0] > 0


def nearest_index_f32(dst, src):
    """Mutation 'nearest_float': the nearest index computed in float32 and rounded, not floored in double."""
    ifx = np.float32(1.0 / (float(dst) / src))
    return np.minimum(np.rint(np.arange(dst, dtype=np.float32) * ifx).astype(np.int64), src - 1)


def render_masks(masks, plan, mut=()):
    """[n,H,W] bool: the collated masks of one planned sample, in ToTensor's permuted order (masks: the SOURCE [n,h,w]).
    mut: 'nearest_float', 'flip_before_pad', 'no_mask_perm'."""
    nh, nw, pt, pl = plan['resize']
    oh, ow = plan['out']
    out = []
    for m in masks:
        win, _ = _geometry(plan, np.asarray(m))
        if "nearest_float" in mut:
            r = win[nearest_index_f32(nh, win.shape[0])][:, nearest_index_f32(nw, win.shape[1])]
        else:
            r = resize_nearest(win, (nw, nh))
        if "flip_before_pad" in mut:
            r = copy_make_border(_flip(r, plan), pt, oh - nh - pt, pl, ow - nw - pl, 0)
        else:
            r = _flip(copy_make_border(r, pt, oh - nh - pt, pl, ow - nw - pl, 0), plan)
        out.append(r > 0)
    out = np.stack(out) if out else np.zeros((0, oh, ow), bool)
    if "no_mask_perm" in mut or not len(out):
        return out
    return out[np.asarray(plan['perm'], np.int64)]


def unpack_masks(packed, w):
    return np.unpackbits(packed, axis=2)[:, :, :w]


# ---- cv2 stand-in for the fixture generator (tools/gen_golden_augment.py) and the call-log test -----------------------
class CV2Restated:
    """The cv2 functions the reference's data/transform.py calls, computed by this restatement.  Every call is logged with its
    arguments (arrays as [dtype, shape])."""
    INTER_NEAREST, INTER_LINEAR, INTER_AREA, INTER_CUBIC, INTER_LANCZOS4 = 0, 1, 3, 2, 4
    COLOR_RGB2GRAY, COLOR_RGB2HSV, COLOR_HSV2RGB = COLOR_RGB2GRAY, COLOR_RGB2HSV, COLOR_HSV2RGB
    BORDER_CONSTANT = BORDER_CONSTANT

    def __init__(self):
        self.log = []

    @staticmethod
    def _desc(a):
        if isinstance(a, np.ndarray):
            return [str(a.dtype), list(a.shape)]
        if isinstance(a, (tuple, list)):
            return [float(v) if isinstance(v, (float, np.floating)) else v for v in a]
        if isinstance(a, (np.floating,)):
            return float(a)
        return a

    def _rec(self, name, args, kwargs):
        self.log.append([name, [self._desc(a) for a in args], {k: self._desc(v) for k, v in kwargs.items()}])

    def cvtColor(self, img, code):
        self._rec("cvtColor", (img, code), {})
        if code == COLOR_RGB2GRAY:
            return gray(img).astype(img.dtype)
        if code == COLOR_RGB2HSV:
            return rgb2hsv(img).astype(img.dtype)
        if code == COLOR_HSV2RGB:
            return hsv2rgb(img).astype(img.dtype)
        raise NotImplementedError(code)

    def resize(self, img, dsize, interpolation=INTER_LINEAR):
        self._rec("resize", (img, tuple(dsize)), {"interpolation": interpolation})
        if interpolation == INTER_NEAREST:
            return resize_nearest(img, dsize)
        if interpolation == INTER_LINEAR and img.dtype == np.float32:
            return resize_linear(img, dsize).astype(np.float32)
        raise NotImplementedError((interpolation, img.dtype))

    def copyMakeBorder(self, img, top, bottom, left, right, border_type, value=0):
        self._rec("copyMakeBorder", (img, top, bottom, left, right, border_type), {"value": value})
        assert border_type == BORDER_CONSTANT
        return copy_make_border(img, top, bottom, left, right, value)


# ---- draw recorders: the reference's `random` and `torch.randperm`, logged -------------------------------------------
def _num(v):
    return [type(v).__name__, float(v)] if isinstance(v, (float, np.floating)) else [type(v).__name__, v]


class RecordingRandom:
    """Stands in for the `random` module of the reference's data/transform.py (and of orienmask_amd.augment): forwards to the
    real module and logs every draw with its arguments' types (np.float32 bounds change random.uniform's arithmetic)."""

    def __init__(self, log):
        import random as _random
        self._r = _random
        self.log = log

    def random(self):
        v = self._r.random()
        self.log.append(["random", v])
        return v

    def uniform(self, a, b):
        v = self._r.uniform(a, b)
        self.log.append(["uniform", _num(a), _num(b), _num(v)])
        return v

    def shuffle(self, x):
        self._r.shuffle(x)
        self.log.append(["shuffle", len(x)])


class RecordingTorch:
    """Stands in for the `torch` module name of a transform module: forwards everything, logs randperm."""

    def __init__(self, log):
        import torch as _torch
        self._t = _torch
        self.log = log

    def __getattr__(self, name):
        return getattr(self._t, name)

    def randperm(self, n, *a, **kw):
        p = self._t.randperm(n, *a, **kw)
        self.log.append(["randperm", int(n), p.tolist()])
        return p


# ---- fixtures (tools/gen_golden_augment.py) --------------------------------------------------------------------------
def load_fixture(path):
    """(meta, samples, outputs): samples as COCODataset._load_sample_data returns them (float32 image, uint8 masks)."""
    import json
    g = np.load(path)
    meta = json.loads(bytes(g["meta"]).decode())
    samples = []
    for k in range(len(meta["specs"])):
        img = g["src_image_%d" % k]
        h, w = img.shape[:2]
        packed = g["src_mask_%d" % k]
        samples.append({"image": img.astype(np.float32), "bbox": g["src_bbox_%d" % k].copy(), "cls": g["src_cls_%d" % k].copy(),
                        "mask": list(unpack_masks(packed, w)), "info": dict(meta["src_info"][k])})
    out = {k[4:]: g[k] for k in g.files if k.startswith("out_")}
    out["mask"] = unpack_masks(out["mask"], meta["out_w"]).astype(bool)
    return meta, samples, out


def seeds_of(meta, n):
    """Per-sample `random` seeds (None: one seed for the batch, set before the first sample)."""
    return meta["rseed"] if isinstance(meta["rseed"], list) else None


def expected_cv2_log(plan, has_mask, n_gt):
    """The cv2 calls the reference makes for one planned sample, in order, arrays as [dtype, shape]."""
    h, w = plan['src_h'], plan['src_w']
    top, left, ch, cw = plan['crop']
    nh, nw, pt, pl = plan['resize']
    oh, ow = plan['out']
    img = ["float32", [h, w, 3]]
    log = []
    for code, _ in plan['ops']:
        if code in (1, 2):
            log.append(["cvtColor", [img, COLOR_RGB2GRAY], {}])
        elif code == 3:
            log.append(["cvtColor", [img, COLOR_RGB2HSV], {}])
            log.append(["cvtColor", [img, COLOR_HSV2RGB], {}])
    padded = plan['padded']
    log.append(["resize", [["float32", [ch, cw, 3]], [nw, nh]], {"interpolation": INTER_LINEAR}])
    if padded:
        log.append(["copyMakeBorder", [["float32", [nh, nw, 3]], pt, oh - nh - pt, pl, ow - nw - pl, BORDER_CONSTANT],
                    {"value": [float(v) for v in plan['pad_value']]}])
    if has_mask:
        log += [["resize", [["uint8", [ch, cw]], [nw, nh]], {"interpolation": INTER_NEAREST}]] * n_gt
        if padded:
            log += [["copyMakeBorder", [["uint8", [nh, nw]], pt, oh - nh - pt, pl, ow - nw - pl, BORDER_CONSTANT], {"value": 0}]] * n_gt
    return log


def plan_fixture(meta, samples, transport_uint8=True):
    """Run orienmask_amd's planner on a fixture's samples under the fixture's seeds, with the draws recorded.
    Returns (draws, planned samples, the planner object)."""
    import copy
    import random
    import torch
    from orienmask_amd import augment, transform
    draws = []
    saved = augment.random, augment.torch
    augment.random, augment.torch = RecordingRandom(draws), RecordingTorch(draws)
    try:
        tf = transform.build_transform(dict(type="COCOTransform", pipeline=copy.deepcopy(meta["pipeline"])))
        tf.transport_uint8 = transport_uint8
        seeds = seeds_of(meta, len(samples))
        if seeds is None:
            random.seed(meta["rseed"])
        torch.manual_seed(meta["tseed"])
        planned = []
        for k, s in enumerate(samples):
            if seeds is not None:
                random.seed(seeds[k])
            planned.append(tf(copy.deepcopy(s)))
    finally:
        augment.random, augment.torch = saved
    return draws, planned, tf
