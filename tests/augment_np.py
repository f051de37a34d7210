"""Float64 restatement of the cv2 float code paths the reference's COCOTransform runs (DESIGN.md "Training augmentation"), and of
the whole device pipeline from a planned sample (orienmask_amd.augment).  Index arithmetic follows cv2 exactly (float32 linear
coefficients, double nearest indices); pixel arithmetic is float64.

  cvtColor RGB2GRAY / RGB2HSV / HSV2RGB   color_rgb RGB2Gray<float>, color_hsv RGB2HSV_f / HSV2RGB_f (hrange 360)
  resize_linear / resize_nearest          resize.cpp INTER_LINEAR (INTER_AREA at an exact 2x downscale), resizeNN
  copy_make_border                        BORDER_CONSTANT
  render(plan)                            the collated image and masks of one planned sample
  jitter_branches                         the chain and its twin whose hue at the 0/360 seam is carried across it
  jitter32 / render_image32               the same composition in float32, in the kernels' operation order: a CPU stand-in for the
                                          device in tests/test_augment_directed_cpu.py, never an expected value

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


def gray(img, mut=()):
    img = np.asarray(img, np.float64)
    if "gray_bgr" in mut:
        return img[..., 2] * GRAY[0] + img[..., 1] * GRAY[1] + img[..., 0] * GRAY[2]
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


def sector_table(mut=()):
    """cv2's sector table, or mutation 'sector_swap': the g and r entries of sector 2 exchanged."""
    if "sector_swap" not in mut:
        return SECTOR
    tab = SECTOR.copy()
    tab[2, 1], tab[2, 2] = SECTOR[2, 2], SECTOR[2, 1]
    return tab


def hsv2rgb(hsv, mut=()):
    hsv = np.asarray(hsv, np.float64)
    h, s, v = hsv[..., 0] * (6.0 / 360.0), hsv[..., 1], hsv[..., 2]
    h = np.mod(h, 6.0)
    sector = np.floor(h).astype(np.int64)
    h = h - sector
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, 0.0, h)
    tab = np.stack([v, v * (1 - s), v * (1 - s * h), v * (1 - s * (1 - h))], axis=-1)
    idx = sector_table(mut)[sector]
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


def area2x_taps(src, dst):
    """Rows (or columns) 2d and 2d + 1 of the 2x2 mean, kept inside the window (they only leave it under 'area2x_one_axis')."""
    d = np.arange(dst)
    return np.minimum(2 * d, src - 1), np.minimum(2 * d + 1, src - 1)


def takes_area2x(src_hw, dst_hw, mut=()):
    """Mutation 'area2x_one_axis': the 2x2 mean taken as soon as ONE axis halves."""
    if "area2x_one_axis" in mut:
        return src_hw[0] == 2 * dst_hw[0] or src_hw[1] == 2 * dst_hw[1]
    return is_area2x(src_hw, dst_hw)


def resize_linear(img, dsize, mut=()):
    """img [h,w,c] -> [dh,dw,c] float64; dsize = (dw, dh) as cv2 takes it.  mut: 'area2x_one_axis'."""
    img = np.asarray(img, np.float64)
    dw, dh = dsize
    h, w = img.shape[:2]
    if "area2x_one_axis" in mut and takes_area2x((h, w), (dh, dw), mut):
        (ya, yb), (xa, xb) = area2x_taps(h, dh), area2x_taps(w, dw)
        return (img[ya][:, xa] + img[ya][:, xb] + img[yb][:, xa] + img[yb][:, xb]) * 0.25
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
GRAY_BLOCKS, GRAY_THREADS = 256, 256        # the grey-mean reduction's grid: workgroups per image, threads per workgroup


def contrast_mean(g, mut=(), crop=None):
    """Mean (a Python float) of the grey plane g [h,w] that adjust_contrast takes: over the FULL source.  Mutations:
    'mean_of_crop' (over the crop window), 'mean_first_pass' (a reduction loop that runs once: only the first 256 pixels of each of
    the 256 chunks are summed)."""
    if "mean_of_crop" in mut and crop is not None:
        top, left, ch, cw = crop
        g = g[top:top + ch, left:left + cw]
    if "mean_first_pass" in mut:
        flat = np.asarray(g, np.float64).reshape(-1)
        chunk = (flat.size + GRAY_BLOCKS - 1) // GRAY_BLOCKS
        return float(sum(flat[b * chunk:min(b * chunk + min(chunk, GRAY_THREADS), flat.size)].sum() for b in range(GRAY_BLOCKS))
                     / flat.size)
    if g.dtype == np.float64:
        return float(g.mean())
    return float(g.sum(dtype=np.float64) / g.size)


def _hue_op(img, f, mut=(), move=None):
    """adjust_hue in float64.  move: bool per pixel -- the hue is carried across the 0/360 seam before the shift and the clip."""
    hsv = rgb2hsv(img)
    h = hsv[..., 0]
    if move is not None:
        h = np.where(move, np.where(h > 180, h - 360, h + 360), h)
    hsv[..., 0] = np.mod(h + f * 360, 360) if "hue_wrap" in mut else np.clip(h + f * 360, 0, 360)
    out = hsv2rgb(hsv, mut)
    return np.clip(out, 0, 255) if "hue_clip_255" in mut else out


def _op(img, src, code, f, mut, crop, move=None, mean_of=None):
    if code == 0:
        return np.clip(img * f, 0, 255)
    if code == 1:
        mean = contrast_mean(gray(src if "mean_before_ops" in mut else img if mean_of is None else mean_of, mut), mut, crop)
        return np.clip(img * f + mean * (1 - f), 0, 255)
    if code == 2:
        return np.clip(img * f + gray(img, mut)[..., None] * (1 - f), 0, 255)
    return _hue_op(img, f, mut, move)


def jitter(img, ops, mut=(), crop=None):
    """mut: 'hue_wrap', 'sector_swap', 'gray_bgr', 'mean_of_crop' (needs crop = (top, left, h, w)), 'mean_before_ops',
    'hue_clip_255', 'mean_first_pass'."""
    src = img = np.asarray(img, np.float64)
    for code, f in ops:
        img = _op(img, src, code, f, mut, crop)
    return img


def near_seam(h, eps):
    return (h < eps) | (h > 360 - eps)


def jitter_branches(img, ops, eps):
    """(a, alt, seam): a is jitter(img, ops); alt is the same chain where, at every hue op, the pixels whose float64 hue before the
    shift lies within eps of the 0/360 seam have that hue carried across it (h - 360 if h > 180, else h + 360) before the shift
    and the clip; seam [h,w] bool is the union of those pixels.  A later contrast takes a's grey mean in both, so alt differs from
    a on seam pixels only.  A float32 hue that rounds to the other side of the seam lands on alt, so a seam pixel must match one
    of two stated values."""
    src = a = alt = np.asarray(img, np.float64)
    seam = np.zeros(a.shape[:-1], bool)
    for code, f in ops:
        move = None
        if code == 3:
            move = near_seam(rgb2hsv(alt)[..., 0], eps)
            seam = seam | move | near_seam(rgb2hsv(a)[..., 0], eps)
        a, alt = _op(a, src, code, f, (), None), _op(alt, src, code, f, (), None, move, a)
    return a, alt, seam


# ---- the same chain in float32, operation by operation as csrc/augment.hip's apply_ops runs it (no fused multiply-add: numpy
# rounds every product).  The CPU stand-in for the device in tests/test_augment_directed_cpu.py; never an expected value.
F32 = np.float32
EPS32 = F32(FLT_EPSILON)
GRAY32 = tuple(F32(c) for c in (0.299, 0.587, 0.114))


def gray32(img, mut=()):
    r, g, b = (img[..., 2], img[..., 1], img[..., 0]) if "gray_bgr" in mut else (img[..., 0], img[..., 1], img[..., 2])
    return r * GRAY32[0] + g * GRAY32[1] + b * GRAY32[2]


def rgb2hsv32(img):
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = v - vmin
    s = diff / (np.abs(v) + EPS32)
    k = (60.0 / (diff + EPS32).astype(np.float64)).astype(F32)
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + F32(120), (r - g) * k + F32(240)))
    h = np.where(h < 0, h + F32(360), h)
    return h, s, v


def hsv2rgb32(h, s, v, mut=()):
    h = h * (F32(6) / F32(360))
    while (h < 0).any():
        h = np.where(h < 0, h + F32(6), h)
    while (h >= 6).any():
        h = np.where(h >= 6, h - F32(6), h)
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(F32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, F32(0), h)
    one = F32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    idx = sector_table(mut)[sector]
    b = np.take_along_axis(tab, idx[..., 0:1], -1)[..., 0]
    g = np.take_along_axis(tab, idx[..., 1:2], -1)[..., 0]
    r = np.take_along_axis(tab, idx[..., 2:3], -1)[..., 0]
    out = np.stack([r, g, b], axis=-1)
    return np.where((s == 0)[..., None], v[..., None], out)


def jitter32(img, ops, mut=(), crop=None):
    """[h,w,3] float32.  fa = float32(f); fb = float32(1 - f), float32(360 f) for hue; the grey mean summed in double and rounded
    to float32, its product with fb in float32; 60 / (diff + eps) in double and rounded.  mut as jitter's."""
    src = img = np.asarray(img).astype(F32)
    lo, hi = F32(0), F32(255)
    for code, f in ops:
        fa = F32(f)
        fb = F32(f * 360) if code == 3 else F32(1 - f)
        if code == 0:
            img = np.clip(img * fa, lo, hi)
        elif code == 1:
            mean = F32(contrast_mean(gray32(src if "mean_before_ops" in mut else img, mut), mut, crop))
            img = np.clip(img * fa + mean * fb, lo, hi)
        elif code == 2:
            img = np.clip(img * fa + (gray32(img, mut) * fb)[..., None], lo, hi)
        else:
            h, s, v = rgb2hsv32(img)
            h = np.mod(h + fb, F32(360)) if "hue_wrap" in mut else np.clip(h + fb, lo, F32(360))
            img = hsv2rgb32(h, s, v, mut)
            if "hue_clip_255" in mut:
                img = np.clip(img, lo, hi)
        assert img.dtype == F32
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


def _edge_axis(dst, src, off, full):
    """Mutation 'image_edge' along one axis: (g0, g1, w1) as indices into the SOURCE, clamped at the source's border."""
    scale = 1.0 / (float(dst) / src)
    f = (((np.arange(dst, dtype=np.float64) + 0.5) * scale) - 0.5).astype(np.float32)
    s0 = np.floor(f).astype(np.int64)
    f = (f - s0.astype(np.float32)).astype(np.float64)
    g0 = s0 + off
    lo, hi = g0 < 0, g0 >= full - 1
    g0[lo], f[lo] = 0, 0
    g0[hi], f[hi] = full - 1, 0
    return g0, np.minimum(g0 + 1, full - 1), f


def _resize_image_edge(img, plan):
    """Mutation 'image_edge': INTER_LINEAR whose taps clamp at the SOURCE image's border instead of the crop window's."""
    top, left, ch, cw = plan['crop']
    nh, nw = plan['resize'][:2]
    x0, x1, fx = _edge_axis(nw, cw, left, img.shape[1])
    y0, y1, fy = _edge_axis(nh, ch, top, img.shape[0])
    rows = img[:, x0] * (1 - fx)[:, None] + img[:, x1] * fx[:, None]
    return rows[y0] * (1 - fy)[:, None, None] + rows[y1] * fy[:, None, None]


def place_image(img, plan, mut=()):
    """[3,H,W] float64: the geometry half of render_image -- crop, resize, pad, flips, Normalize -- of an already jittered SOURCE
    [h,w,3].  mut: 'image_edge', 'flip_before_pad', 'area2x_one_axis'."""
    win, (nh, nw, pt, pl, oh, ow) = _geometry(plan, img)
    res = _resize_image_edge(img, plan) if "image_edge" in mut else resize_linear(win, (nw, nh), mut)
    pad = [float(np.float32(v)) for v in plan['pad_value']]
    if "flip_before_pad" in mut:
        out = copy_make_border(_flip(res, plan), pt, oh - nh - pt, pl, ow - nw - pl, pad)
    else:
        out = _flip(copy_make_border(res, pt, oh - nh - pt, pl, ow - nw - pl, pad), plan)
    mean = np.asarray(plan['mean'], np.float64)
    std = np.asarray(plan['std'], np.float64)
    return ((out - mean) / std).transpose(2, 0, 1)


def render_image(image, plan, mut=()):
    """[3,H,W] float64: the collated, normalised image of one planned sample (image: the SOURCE [h,w,3]).  mut: deliberate bugs
    for the mutation tests (jitter's and place_image's)."""
    return place_image(jitter(image, plan['ops'], mut, plan['crop']), plan, mut)


def render_image32(image, plan, mut=()):
    """[3,H,W] float32: jitter32 on every tap, then the blend, the pad and Normalize in float32 in the image kernel's order -- the
    CPU stand-in for the device.  mut: jitter32's, 'image_edge', 'area2x_one_axis'."""
    img = jitter32(image, plan['ops'], mut, plan['crop'])
    top, left, ch, cw = plan['crop']
    nh, nw, pt, pl = plan['resize']
    oh, ow = plan['out']
    if takes_area2x((ch, cw), (nh, nw), mut):
        (ya, yb), (xa, xb) = area2x_taps(ch, nh), area2x_taps(cw, nw)
        ya, yb, xa, xb = ya + top, yb + top, xa + left, xb + left
        res = (img[ya][:, xa] + img[ya][:, xb] + img[yb][:, xa] + img[yb][:, xb]) * F32(0.25)
    else:
        if "image_edge" in mut:
            x0, x1, fx = _edge_axis(nw, cw, left, img.shape[1])
            y0, y1, fy = _edge_axis(nh, ch, top, img.shape[0])
        else:
            x0, x1, fx, _ = linear_coeffs(nw, cw)
            y0, y1, fy, _ = linear_coeffs(nh, ch)
            x0, x1, y0, y1 = x0 + left, x1 + left, y0 + top, y1 + top
        fx, fy = fx.astype(F32)[None, :, None], fy.astype(F32)[:, None, None]
        ax, ay = F32(1) - fx, F32(1) - fy
        res = (img[y0][:, x0] * ax + img[y0][:, x1] * fx) * ay + (img[y1][:, x0] * ax + img[y1][:, x1] * fx) * fy
    full = np.empty((oh, ow, 3), F32)
    full[...] = np.asarray(plan['pad_value'], F32)
    full[pt:pt + nh, pl:pl + nw] = res
    full = _flip(full, plan)
    res = (full - np.asarray(plan['mean'], F32)) / np.asarray(plan['std'], F32)
    assert res.dtype == F32
    return np.ascontiguousarray(res.transpose(2, 0, 1))


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
