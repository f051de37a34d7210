"""Float64 restatement of the three kernels that turn image geometry into pixels, and the geometry table that
tests/test_geometry_sweep.py iterates.

  preprocess.hip   FastCOCOTransform (permute, Resize / ShortEdgeResize, Normalize) + pad to a multiple of 32
  coco_format.hip  _recover_shape_bbox, _recover_shape_segm (crop collate_pad then pad, hflip, vflip, resize, round) + RLE
  visualize.hip    InferenceVisualizer's mask crop, resize, ascending-area sort and plot_all_mask composite

Written from the documented semantics of F.interpolate(mode='bilinear', align_corners=False), not from any implementation.

Bilinear along one axis of n_in source and n_out output samples: output d reads the source coordinate
    src = (d + 0.5) * n_in / n_out - 0.5,   clamped at 0,
taps i0 = min(floor(src), n_in - 1) and i1 = min(i0 + 1, n_in - 1), weights 1 - l and l with l = src - i0.  `axis64` evaluates
src from the exact rational ((2d + 1) n_in - n_out) / (2 n_out): i0 by integer floor division, l with one float64 rounding.

The kernels (and torch-CPU) evaluate the same formula in float32: scale32 = fl32(n_in / n_out), src32 = fmaf(scale32, d + 0.5,
-0.5).  `axis32` restates that exactly (the product of a float32 scale and d + 0.5 has at most 37 significant bits, so it and
the -0.5 are exact in float64 and the one rounding to float32 is the fma's), which gives the per-element float bound:

    FLOAT BOUND  |v32 - v64| <= e_y * D_y + e_x * D_x + 8 ulp32(max |tap|)

  * e = |src32 - src| along each axis, known exactly per output index;
  * D = the local tap difference: the largest difference between adjacent source samples from one sample before i0 to one
    after i1 (moving the sample point by e moves a piecewise-linear function by at most e times its steepest slope there,
    also when the point crosses a source sample);
  * 8 ulp of the largest tap magnitude cover the rounding of 1 - l and the three float32 operations of the blend.
  Normalize ((v - mean) / std) divides the bound by std and adds 2 ulp of the normalised value.

  MASK RULE  a rounded mask pixel must equal v64 > 0.5 wherever |v64 - 0.5| > max(1e-5, FLOAT BOUND).  The float bound, not
  1e-5 alone: at 544 source samples the float32 index itself is off by up to ~3e-5 (half an ulp of 544 plus the scale's
  rounding times d), which moves a 0/1 blend by as much when the taps differ.

  VISUALISER BOUND  out = img * prod_k (1 - a m_k) + sum_k a c_k m_k prod_{j<k} (1 - a m_j) moves by at most a * 510 per unit
  of any m_k (colours and image within [0, 255]), so |out32 - out64| <= sum_k 510 a e_k + (K + 4) * 4 ulp32(256), e_k being
  mask k's float bound at that pixel; a = float32(alpha), as the reference's float32 tensors see it.

The float32 restatements (`resize32`, `recover_segm32`, `rle_counts_bitmap`) exist for the teeth test: each takes a `variant`
that is a plausible bug, and the test asserts every bug disagrees with torch somewhere on the table.
"""
import collections
import math

import numpy as np

f32 = np.float32
f64 = np.float64
EPS32 = 2.0 ** -23
MI355X_LDS_PER_BLOCK = 160 * 1024      # hipDeviceAttributeMaxSharedMemoryPerBlock on MI355X; the GPU test reads the device's


# --------------------------------------------------------------------------------------------------------------- one axis
def axis64(n_in, n_out):
    """(i0, i1, w0, w1) of every output index, from the exact rational source coordinate."""
    d = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * d + 1) * n_in - n_out, 0)          # src = num / den, clamped at 0
    den = 2 * n_out
    i0 = np.minimum(num // den, n_in - 1)
    w1 = (num - i0 * den).astype(f64) / den
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, 1.0 - w1, w1


def src32(n_in, n_out, fused=True, scale=None, scale_double=False):
    """The float32 source coordinate (clamped at 0) as the kernels compute it; the keywords are the teeth test's variants."""
    d = np.arange(n_out, dtype=f32) + f32(0.5)
    if scale_double:                                         # the whole index in double, one rounding at the end
        s = (np.arange(n_out, dtype=f64) + 0.5) * (n_in / n_out) - 0.5
        s = s.astype(f32)
    else:
        sc = f32(n_in) / f32(n_out) if scale is None else f32(scale)
        if fused:
            s = (f64(sc) * d.astype(f64) - 0.5).astype(f32)
        else:
            s = (sc * d - f32(0.5)).astype(f32)
    return np.maximum(s, f32(0))


def axis32(n_in, n_out, i1_past=False, **kw):
    """(i0, i1, w0, w1) in float32 as bilinear.h's tap(); i1_past: the bug that clamps i1 at n_in instead of n_in - 1."""
    s = src32(n_in, n_out, **kw)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in if i1_past else n_in - 1)
    w1 = (s - i0.astype(f32)).astype(f32)
    return i0, i1, (f32(1) - w1).astype(f32), w1


def src_error(n_in, n_out):
    """e = |src32 - src| per output index (both clamped at 0)."""
    num = np.maximum((2 * np.arange(n_out, dtype=np.int64) + 1) * n_in - n_out, 0)
    return np.abs(src32(n_in, n_out).astype(f64) - num.astype(f64) / (2 * n_out))


def _slope(a, i0, i1, axis):
    """Largest |a[j+1] - a[j]| along `axis` for j in [i0 - 1, i1] (clamped): the local tap difference D."""
    n = a.shape[axis]
    if n == 1:
        shape = list(a.shape)
        shape[axis] = len(i0)
        return np.zeros(shape)
    diff = np.abs(np.diff(a, axis=axis))                      # n - 1 segments
    out = None
    for off in (-1, 0, 1):
        j = np.clip(i0 + off, 0, n - 2)
        t = np.take(diff, j, axis=axis)
        out = t if out is None else np.maximum(out, t)
    return out


# --------------------------------------------------------------------------------------------------------------- resize
def resize64(x, oh, ow, with_bound=False):
    """x [..., H, W] -> [..., oh, ow] float64; with_bound: also the per-element FLOAT BOUND."""
    x = np.asarray(x, dtype=f64)
    H, W = x.shape[-2:]
    y0, y1, wy0, wy1 = axis64(H, oh)
    x0, x1, wx0, wx1 = axis64(W, ow)
    r = x[..., y0, :] * wy0[:, None] + x[..., y1, :] * wy1[:, None]           # rows first: [..., oh, W]
    v = r[..., x0] * wx0 + r[..., x1] * wx1
    if not with_bound:
        return v
    ey, ex = src_error(H, oh), src_error(W, ow)
    # D_y: slope along the rows at the two column taps; D_x: slope along the columns at the two row taps
    dy = _slope(x, y0, y1, x.ndim - 2)                                        # [..., oh, W]
    dy = np.maximum(dy[..., x0], dy[..., x1])
    dx = _slope(x, x0, x1, x.ndim - 1)                                        # [..., H, ow]
    dx = np.maximum(dx[..., y0, :], dx[..., y1, :])
    big = np.maximum(np.abs(x[..., y0, :]), np.abs(x[..., y1, :]))
    big = np.maximum(big[..., x0], big[..., x1])
    bound = ey[:, None] * dy + ex[None, :] * dx + 8 * EPS32 * big
    return v, bound


# torch-CPU resizes outputs with height + width <= SMALL_OUT with another kernel (the channels-last loop it prefers for small
# outputs): the weights h_i * w_j rounded to float32 first, the four taps summed left to right with fma
SMALL_OUT = 128


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


RESIZE_VARIANTS = ("unfused", "scale_double", "i1_past", "swap_scales", "generic_blend", "small_lt", "small_129")


def resize32(x, oh, ow, variant=None):
    """x [..., H, W] float32 -> [..., oh, ow] float32 with torch-CPU's arithmetic: bilinear.h's blend, or the four-weight sum
    when oh + ow <= SMALL_OUT.  variant: None, 'unfused', 'scale_double', 'i1_past' (reads one sample past the edge: zero
    here), 'swap_scales', 'generic_blend' (bilinear.h's generic blend at every size), 'small_lt' / 'small_129' (the
    small-output threshold at < 128 / <= 129)."""
    x = np.asarray(x, dtype=f32)
    H, W = x.shape[-2:]
    kw = dict(fused=variant != "unfused", scale_double=variant == "scale_double")
    ky = dict(kw, scale=f32(W) / f32(ow)) if variant == "swap_scales" else kw
    kx = dict(kw, scale=f32(H) / f32(oh)) if variant == "swap_scales" else kw
    if variant == "i1_past":
        pad = [(0, 0)] * (x.ndim - 2) + [(0, 1), (0, 1)]
        x = np.pad(x, pad)
    y0, y1, wy0, wy1 = axis32(H, oh, i1_past=variant == "i1_past", **ky)
    x0, x1, wx0, wx1 = axis32(W, ow, i1_past=variant == "i1_past", **kx)
    if variant == "swap_scales":          # a swapped scale can point past the source: clamp as tap() does
        y0, y1, x0, x1 = (np.minimum(a, n - 1) for a, n in ((y0, H), (y1, H), (x0, W), (x1, W)))
    r0, r1 = x[..., y0, :], x[..., y1, :]
    small = {"generic_blend": False, "small_lt": oh + ow < SMALL_OUT, "small_129": oh + ow <= SMALL_OUT + 1}.get(
        variant, oh + ow <= SMALL_OUT)
    if small:
        w00, w01 = wy0[:, None] * wx0[None, :], wy0[:, None] * wx1[None, :]
        w10, w11 = wy1[:, None] * wx0[None, :], wy1[:, None] * wx1[None, :]
        v = _fma(r0[..., x0], w00, (r0[..., x1] * w01).astype(f32))
        return _fma(r1[..., x1], w11, _fma(r1[..., x0], w10, v))
    top = _fma(r0[..., x0], wx0, (r0[..., x1] * wx1).astype(f32))
    bot = _fma(r1[..., x0], wx0, (r1[..., x1] * wx1).astype(f32))
    return _fma(top, wy0[:, None], (bot * wy1[:, None]).astype(f32))


# --------------------------------------------------------------------------------------------------------------- COCO format
def crop_of(info):
    """(top, down, left, right) removed from the network mask: collate_pad is (left, right, top, down, h, w), pad is
    (top, down, left, right, h, w), and both add up."""
    top = down = left = right = 0
    if info.get("collate_pad") is not None:
        l, r, t, d = info["collate_pad"][:4]
        left += l; right += r; top += t; down += d
    if info.get("pad") is not None:
        t, d, l, r = info["pad"][:4]
        left += l; right += r; top += t; down += d
    return top, down, left, right


def crop_flip(mask, info, variant=None):
    """[K,H,W] -> the cropped and flipped [K,ch,cw] the resize reads.  variant: 'crop_top' / 'crop_down' / 'crop_left' /
    'crop_right' (that side cropped one pixel too many), 'flip_before_crop'."""
    top, down, left, right = crop_of(info)
    if variant in ("crop_top", "crop_down", "crop_left", "crop_right"):
        top, down, left, right = (v + (variant == n) for v, n in
                                  zip((top, down, left, right), ("crop_top", "crop_down", "crop_left", "crop_right")))
    m = np.asarray(mask)
    H, W = m.shape[-2:]
    if variant == "flip_before_crop":
        if info.get("hflip", False):
            m = m[..., :, ::-1]
        if info.get("vflip", False):
            m = m[..., ::-1, :]
    m = m[..., top:H - down, left:W - right]
    if variant != "flip_before_crop":
        if info.get("hflip", False):
            m = m[..., :, ::-1]
        if info.get("vflip", False):
            m = m[..., ::-1, :]
    return np.ascontiguousarray(m)


def recover_shape_segm64(mask, info):
    """_recover_shape_segm before round(): (v64 [K,oh,ow], FLOAT BOUND [K,oh,ow])."""
    m = crop_flip(mask, info).astype(f64)
    return resize64(m, int(info["height"]), int(info["width"]), with_bound=True)


def mask_rule(got_u8, v64, bound):
    """Indices where a rounded mask breaks the MASK RULE (empty when it holds)."""
    decided = np.abs(v64 - 0.5) > np.maximum(1e-5, bound)
    return np.argwhere(decided & ((np.asarray(got_u8) != 0) != (v64 > 0.5)))


def recover_segm32(mask, info, variant=None):
    """_recover_shape_segm in the kernels' float32 arithmetic, rounded: uint8 [K,oh,ow].  variant: one of crop_flip's,
    resize32's, or 'round_half_up'."""
    m = crop_flip(mask, info, variant).astype(f32)
    if m.shape[-1] == 0 or m.shape[-2] == 0:
        return None
    v = resize32(m, int(info["height"]), int(info["width"]), variant if variant in RESIZE_VARIANTS else None)
    r = np.floor(v + f32(0.5)) if variant == "round_half_up" else np.rint(v)
    return r.astype(np.uint8)


def recover_shape_bbox64(bbox, info):
    """_recover_shape_bbox in float64: [K,>=4] (cx,cy,w,h) normalised -> [K,4] x,y,w,h in original pixels."""
    b = np.asarray(bbox, dtype=f64)
    bx, by, bw, bh = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    for key, order in (("collate_pad", "lrtd"), ("pad", "tdlr")):
        p = info.get(key)
        if p is None:
            continue
        side = dict(zip(order, p[:4]))
        h, w = p[4], p[5]
        nh, nw = h - side["t"] - side["d"], w - side["l"] - side["r"]
        bx, by = (bx * w - side["l"]) / nw, (by * h - side["t"]) / nh
        bw, bh = bw * w / nw, bh * h / nh
    if info.get("hflip", False):
        bx = 1 - bx
    if info.get("vflip", False):
        by = 1 - by
    oh, ow = info["height"], info["width"]
    return np.stack([(bx - bw / 2) * ow, (by - bh / 2) * oh, bw * ow, bh * oh], axis=1)


def rle_counts_bitmap(mask_hw, variant=None):
    """pycocotools' run lengths of one [oh,ow] 0/1 mask through coco_format.hip's column-major bitmap: 32 rows of a column per
    word, value changes as w ^ ((w << 1) | prev) masked to the column's valid rows, prev the last valid row of the previous
    column.  variant 'tail_bit': the rows past oh in a column's last word read as 1 and are not masked off."""
    m = (np.asarray(mask_hw) != 0).astype(np.uint64)
    oh, ow = m.shape
    wpc = (oh + 31) // 32
    last = oh - 32 * (wpc - 1)
    rows = np.zeros((wpc * 32, ow), dtype=np.uint64)
    rows[:oh] = m
    if variant == "tail_bit":
        rows[oh:] = 1
    words = (rows.reshape(wpc, 32, ow) << np.arange(32, dtype=np.uint64)[None, :, None]).sum(axis=1).T.reshape(-1)   # [ow*wpc]
    yb = np.tile(np.arange(wpc), ow)
    x = np.repeat(np.arange(ow), wpc)
    prev_word = np.concatenate([[np.uint64(0)], words[:-1]])
    prev_bit = 31 if variant == "tail_bit" else last - 1
    prev = np.where(yb > 0, prev_word >> np.uint64(31), np.where(x > 0, (prev_word >> np.uint64(prev_bit)) & np.uint64(1), 0))
    full = np.uint64(0xFFFFFFFF)
    valid = np.where((yb == wpc - 1) & (last < 32) & (variant != "tail_bit"), (np.uint64(1) << np.uint64(last)) - np.uint64(1), full)
    changes = (words ^ (((words << np.uint64(1)) | prev.astype(np.uint64)) & full)) & valid
    bits = ((changes[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    wi, b = np.nonzero(bits)
    pos = x[wi].astype(np.int64) * oh + 32 * yb[wi] + b
    edges = np.concatenate([[0], pos, [oh * ow]])
    return np.diff(edges).tolist()


def rle_lds_bytes(h, w):
    """coco_format.hip: LDS of one mask in recover_rle_lds_kernel, 16 B of row taps per output row + the bitmap."""
    return 16 * h + 4 * w * ((h + 31) // 32)


def rle_lds_max(lds_per_block):
    """coco_format.hip: the per-block LDS less 10 KiB for the kernel's static arrays."""
    return max(lds_per_block, 64 * 1024) - 10 * 1024


# --------------------------------------------------------------------------------------------------------------- preprocess
def short_edge_target(h, w, short_length, max_size):
    """ShortEdgeResize: the scale that brings the short side to short_length unless the long side would pass max_size,
    each side rounded half up."""
    scale = min(short_length / min(h, w), max_size / max(h, w))
    return int(h * scale + 0.5), int(w * scale + 0.5)


def pad_info(rh, rw, divisor=32):
    """pad(): centred padding to a multiple of divisor, [left, right, top, down, H, W]."""
    H, W = int(math.ceil(rh / divisor) * divisor), int(math.ceil(rw / divisor) * divisor)
    left, top = (W - rw) // 2, (H - rh) // 2
    return [left, W - rw - left, top, H - rh - top, H, W]


def preprocess64(image_nhwc, size, mean, std, divisor=32, pad_value=0.0):
    """FastCOCOTransform + pad in float64: (out [N,3,H,W], FLOAT BOUND of it, pad info)."""
    x = np.asarray(image_nhwc, dtype=f64).transpose(0, 3, 1, 2)
    rh, rw = size
    v, b = resize64(x, rh, rw, with_bound=True)
    mean = np.asarray(mean, dtype=f32).astype(f64)[None, :, None, None]
    std = np.asarray(std, dtype=f32).astype(f64)[None, :, None, None]
    v = (v - mean) / std
    b = b / std + 2 * EPS32 * np.abs(v)
    info = pad_info(rh, rw, divisor)
    left, right, top, down = info[:4]
    pad = ((0, 0), (0, 0), (top, down), (left, right))
    return np.pad(v, pad, constant_values=pad_value), np.pad(b, pad), info


# --------------------------------------------------------------------------------------------------------------- visualiser
def plot_all_mask64(mask64, bound64, image, colors, alpha, order=None):
    """plot_all_mask after the ascending-area argsort, in float64: (out [h,w,3], VISUALISER BOUND [h,w,3], area order, areas).
    mask64 [K,h,w] resized mask values (unsorted), image [h,w,3], colors [K,3]; the k >= 1 colour terms enter only when the
    image is taller than one row (the reference tests image.shape[0] > 1, the image's height, not the number of masks).
    order: composite in this order instead of float64's (a kernel's, once it has been checked against float64's areas: masks
    of equal area, which the reference's unstable argsort leaves in any order, may come in another order than here)."""
    a = float(f32(alpha))
    img = np.asarray(image, dtype=f64)
    area = mask64.sum(axis=(1, 2))
    if order is None:
        order = np.argsort(area, kind="stable")
    cum = np.ones(img.shape[:2])
    terms = np.zeros_like(img)
    err = np.zeros(img.shape[:2])
    for r, k in enumerate(order):
        m = mask64[k]
        cm = m[:, :, None] * np.asarray(colors[k], dtype=f64)[None, None, :] * a
        if r == 0:
            first = cm
        elif img.shape[0] > 1:
            terms += cm * cum[:, :, None]
        cum = cum * (1 - a * m)
        err += 510 * a * bound64[k]
    out = img * cum[:, :, None] + first + terms
    bound = err[:, :, None] + (len(order) + 4) * 4 * 256 * EPS32
    return out, bound, order, area


# --------------------------------------------------------------------------------------------------------------- masks
MASK_FAMILIES = ("noise", "blobs", "empty", "full", "corner_tl", "corner_tr", "corner_bl", "corner_br", "row_first", "row_last",
                 "col_first", "col_last", "stripes", "checker")


def make_mask(family, H, W, seed):
    """One [H,W] bool mask of a family, at mask (network) resolution."""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), dtype=bool)
    if family == "noise":
        m = rng.random((H, W)) < 0.5
    elif family == "blobs":
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(4):
            cy, cx = rng.random() * H, rng.random() * W
            ry, rx = 1 + rng.random() * H / 3, 1 + rng.random() * W / 3
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    elif family == "full":
        m[:] = True
    elif family.startswith("corner_"):
        m[0 if family[7] == "t" else -1, 0 if family[8] == "l" else -1] = True
    elif family == "row_first":
        m[0, :] = True
    elif family == "row_last":
        m[-1, :] = True
    elif family == "col_first":
        m[:, 0] = True
    elif family == "col_last":
        m[:, -1] = True
    elif family == "stripes":                 # diagonal: the runs cross from the bottom of a column to the top of the next
        yy, xx = np.mgrid[0:H, 0:W]
        m = ((yy + xx) // 3) % 2 == 0
    elif family == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        m = (yy + xx) % 2 == 0
    return m


def mask_stack(H, W, seed, families=MASK_FAMILIES):
    return np.stack([make_mask(f, H, W, seed * 131 + i) for i, f in enumerate(families)])


# --------------------------------------------------------------------------------------------------------------- the table
Geometry = collections.namedtuple("Geometry", "name H W info")      # network mask [H,W] and the sample_info


def _g(name, oh, ow, H=544, W=544, collate_pad=None, pad=None, hflip=False, vflip=False):
    info = dict(height=oh, width=ow, hflip=hflip, vflip=vflip)
    if collate_pad is not None:
        info["collate_pad"] = list(collate_pad)
    if pad is not None:
        info["pad"] = list(pad)
    return Geometry(name, H, W, info)


def lds_boundary(lds_per_block=MI355X_LDS_PER_BLOCK, h=640):
    """(h, w) whose RLE bitmap fills recover_rle_lds_kernel's LDS exactly, and its two neighbours that go over."""
    cap = rle_lds_max(lds_per_block)
    w = (cap - 16 * h) // (4 * ((h + 31) // 32))
    assert rle_lds_bytes(h, w) <= cap < rle_lds_bytes(h, w + 1) and cap < rle_lds_bytes(h + 1, w)
    return (h, w), (h, w + 1), (h + 1, w)


def table(lds_per_block=MI355X_LDS_PER_BLOCK):
    """Every geometry the sweep runs, in a fixed order that interleaves LDS-path and over-capacity images."""
    (eh, ew), (ah, aw), (bh, bw) = lds_boundary(lds_per_block)
    flips = [(False, False), (True, False), (False, True), (True, True)]
    g = []
    # val2017-typical original sizes, squashed to 544 x 544 (Resize(544)); flips cycle through the four combinations
    for i, (oh, ow) in enumerate([(640, 480), (480, 640), (640, 427), (427, 640), (500, 375), (375, 500), (333, 500),
                                  (612, 612), (640, 359), (640, 640)]):
        hf, vf = flips[i % 4]
        g.append(_g("val_%dx%d%s%s" % (oh, ow, "_h" if hf else "", "_v" if vf else ""), oh, ow, hflip=hf, vflip=vf))
        if i == 1:                      # the over-capacity images come in two clusters (here and at the end), so that a
            g.append(_g("lds_exact_%dx%d" % (eh, ew), eh, ew))        # batch in table order fills whole RLE_BATCH launches
            g.append(_g("lds_over_w_%dx%d" % (ah, aw), ah, aw, hflip=True))
            g.append(_g("lds_over_h_%dx%d" % (bh, bw), bh, bw, vflip=True))
    # tiny originals
    g += [_g("tiny_1x1", 1, 1), _g("tiny_1x7", 1, 7, hflip=True), _g("tiny_7x1", 7, 1, vflip=True), _g("tiny_2x3", 2, 3),
          _g("tiny_31x33", 31, 33, H=96, W=128, hflip=True, vflip=True)]
    # heights around the 32-row words, from masks of several sizes
    for i, oh in enumerate((31, 32, 33, 63, 64, 65)):
        hf, vf = flips[i % 4]
        g.append(_g("word_h%d" % oh, oh, 45 + 14 * i, H=64 + 32 * (i % 3), W=96, hflip=hf, vflip=vf))
    # extreme aspect ratios, strong down- and upscale
    g += [_g("aspect_640x50", 640, 50, W=64, hflip=True), _g("aspect_50x640", 50, 640, H=64, vflip=True),
          _g("down_544_to_17", 17, 17), _g("down_544_to_7", 7, 7, hflip=True, vflip=True)]
    # crops: odd and asymmetric letterbox pads on each side, collate_pad with pad, 1-pixel crops
    g += [_g("pad_top3_down4", 333, 500, H=96, W=96, pad=[3, 4, 0, 0, 96, 96]),
          _g("pad_left5_right6", 500, 333, H=96, W=96, pad=[0, 0, 5, 6, 96, 96], hflip=True),
          _g("pad_top1", 101, 99, H=64, W=64, pad=[1, 0, 0, 0, 64, 64], vflip=True),
          _g("pad_down1", 99, 101, H=64, W=64, pad=[0, 1, 0, 0, 64, 64]),
          _g("pad_left1", 77, 130, H=64, W=64, pad=[0, 0, 1, 0, 64, 64], hflip=True, vflip=True),
          _g("pad_right1", 130, 77, H=64, W=64, pad=[0, 0, 0, 1, 64, 64]),
          _g("pad_all_odd", 427, 640, H=544, W=544, pad=[67, 68, 1, 2, 544, 544], hflip=True),
          _g("collate_and_pad", 375, 500, H=160, W=192, collate_pad=[0, 32, 0, 16, 160, 192],
             pad=[9, 10, 3, 0, 144, 160], vflip=True),
          _g("collate_and_pad_hv", 480, 640, H=128, W=160, collate_pad=[5, 27, 3, 13, 128, 160],
             pad=[1, 2, 2, 1, 112, 128], hflip=True, vflip=True),
          _g("crop_1row", 5, 40, H=33, W=40, pad=[16, 16, 0, 0, 33, 40]),
          _g("crop_1col", 40, 5, H=40, W=33, pad=[0, 0, 16, 16, 40, 33], hflip=True),
          _g("crop_1px_collate_and_pad", 3, 3, H=9, W=9, collate_pad=[2, 2, 2, 2, 9, 9], pad=[2, 2, 2, 2, 5, 5], vflip=True)]
    # small outputs of small crops, where torch blends with its small-output kernel (height + width <= 128): the generic blend
    # rounds a mask pixel differently at the first two; the last two sit on either side of the threshold
    g += [_g("small_crop_37x34_to_33x31", 33, 31, H=41, W=36, pad=[2, 2, 1, 1, 41, 36]),
          _g("small_crop_1x4_to_9x26", 9, 26, H=3, W=4, pad=[1, 1, 0, 0, 3, 4]),
          _g("small_out_128_37x34_to_60x68", 60, 68, H=41, W=36, pad=[2, 2, 1, 1, 41, 36], hflip=True),
          _g("small_out_129_37x34_to_60x69", 60, 69, H=41, W=36, pad=[2, 2, 1, 1, 41, 36], vflip=True)]
    g += [_g("full_1080x1920_letterbox", 1080, 1920, pad=[119, 119, 0, 0, 544, 544]),
          _g("up_136_to_1920", 1080, 1920, H=136, W=136)]
    names = [x.name for x in g]
    assert len(set(names)) == len(names)
    return g
