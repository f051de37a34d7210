"""Directed cases for the augmentation's image kernel and its two grey-mean kernels (csrc/augment.hip), written by hand as planned
samples -- no random draws -- and the checkers that tests/test_augment_directed.py (the device) and
tests/test_augment_directed_cpu.py (the float32 stand-in, augment_np.render_image32) share.  Not a test module.

A case is (id, source image, ops, plan geometry, masks); planned(case) makes the sample augment.collate takes.  Every jitter factor is
a multiple of 1/64, so float32(f) == f and the float64 restatement and the kernel work with the same factor.
"""
import collections
import itertools

import numpy as np
import torch

import augment_np as A
from test_augment_cpu import PIXEL_BOUND, SEAM_EPS
from orienmask_amd import augment

B, C, S, H = augment.BRIGHTNESS, augment.CONTRAST, augment.SATURATION, augment.HUE
Case = collections.namedtuple("Case", "id image ops geom masks")

# |device - float64| on the 0..255 scale.  Chains without a hue op: at most 4 float32 roundings on values <= 382.5, ulp/2 = 1.53e-5
# each, and the float64 restatement's (1 - f) at most 3e-5 from float32(1 - f)'s product.  Chains with hue: the project's bound.
BOUND_NO_HUE = 1e-4
BOUND_HUE = PIXEL_BOUND
PAD = [123.675, 116.28, 103.53]


def bound_of(case):
    if case.id.startswith("gray_"):     # the grey-mean group is held to 1e-4 throughout, its [hue, saturation, contrast] chain too
        return BOUND_NO_HUE
    return BOUND_HUE if any(code == H for code, _ in case.ops) else BOUND_NO_HUE


def geom(src_hw, crop=None, resize=None, out=None, hflip=False, vflip=False, pad_value=(0.0, 0.0, 0.0), mean=(0.0, 0.0, 0.0),
         std=(1.0, 1.0, 1.0)):
    """Plan geometry; the defaults are the identity: no crop, no resize, no pad, no flip, mean 0 and std 1."""
    h, w = src_hw
    crop = tuple(crop) if crop else (0, 0, h, w)
    resize = tuple(resize) if resize else (crop[2], crop[3], 0, 0)
    if len(resize) == 2:
        resize += (0, 0)
    out = tuple(out) if out else (resize[0] + resize[2], resize[1] + resize[3])
    return dict(crop=crop, resize=resize, out=out, hflip=hflip, vflip=vflip, pad_value=list(pad_value), mean=list(mean), std=list(std))


def plan_of(case):
    """The 'aug' record COCOTransform would have written for this case."""
    g = case.geom
    h, w = case.image.shape[:2]
    n = len(case.masks)
    return dict(src_h=h, src_w=w, crop=g['crop'], resize=g['resize'], out=g['out'], padded=g['out'] != g['resize'][:2],
                pad_value=list(g['pad_value']), ops=list(case.ops), hflip=g['hflip'], vflip=g['vflip'],
                perm=np.arange(n, dtype=np.int64)[::-1].copy(), mean=list(g['mean']), std=list(g['std']))


def planned(case, transport_uint8=True):
    n = len(case.masks)
    h, w = case.image.shape[:2]
    bbox = torch.tensor([[0.5, 0.5, 0.25 + 0.5 * k, 0.5] for k in range(n)], dtype=torch.float32).reshape(n, 4)
    # the dataset hands over float32; the planner sends it as uint8 where that is exact
    out = {'image': augment._transport_image(case.image.astype(np.float32), transport_uint8), 'bbox': bbox, 'cls': torch.arange(n, dtype=torch.int64),
           'aug': plan_of(case)}
    out['mask'] = np.packbits(np.stack(case.masks) > 0, axis=2) if n else np.zeros((0, h, (w + 7) // 8), np.uint8)
    return out


def factors(cases):
    return [f for c in cases for _, f in c.ops]


# ---- colour lattice --------------------------------------------------------------------------------------------------
LEVELS = (0, 1, 2, 63, 64, 127, 128, 129, 191, 254, 255)


def lattice_u8():
    """[1,1331,3] uint8: every RGB triple over LEVELS -- the greys, every two-channel tie, both ends of the range."""
    return np.array(list(itertools.product(LEVELS, repeat=3)), np.uint8).reshape(1, -1, 3)


def lattice_frac():
    """The lattice as float32 * 0.997 + 0.37: fractional, so it stays float32 in transport."""
    return (lattice_u8().astype(np.float32) * np.float32(0.997) + np.float32(0.37)).astype(np.float32)


def lattice_wide():
    """The lattice as float32 * 1.01 - 1.2: [-1.2, 256.35].  A float32 source may leave [0, 255], and only there does the hue op's
    result leave it too (s > 1): the case that tells 'hue_clip_255' from the reference, which does not clip after the hue op."""
    return (lattice_u8().astype(np.float32) * np.float32(1.01) - np.float32(1.2)).astype(np.float32)


# the configured ends (brightness 0.2, contrast 0.5, saturation 0.5, hue 0.1) at the nearest multiple of 1/64, one interior value
SINGLE = {B: (0.796875, 1.203125, 1.0625), C: (0.5, 1.5, 1.125), S: (0.5, 1.5, 0.875, 0.0),
          H: (-0.109375, 0.109375, 0.03125, -0.5, 0.5)}
FIXED = ({B: 1.203125, C: 1.5, S: 1.5, H: 0.109375}, {B: 0.796875, C: 0.5, S: 0.5, H: -0.109375},
         {B: 1.0625, C: 0.75, S: 1.25, H: 0.421875})
NAME = {B: "b", C: "c", S: "s", H: "h"}


def chains():
    """[(id, ops)]: each op alone; every 2- and 3-op subset in one order; all 24 orders of the four ops under three factor sets."""
    out = []
    for code in (B, C, S, H):
        out += [("%s%+g" % (NAME[code], f), [(code, f)]) for f in SINGLE[code]]
    for n in (2, 3):
        for k, sub in enumerate(itertools.combinations((H, S, C, B), n)):
            sub = sub[k % n:] + sub[:k % n]         # rotated, so hue and contrast each come first, in the middle and last
            out.append(("".join(NAME[c] for c in sub), [(c, FIXED[k % 2][c]) for c in sub]))
    for k, fx in enumerate(FIXED):
        out += [("".join(NAME[c] for c in order) + str(k), [(c, fx[c]) for c in order]) for order in itertools.permutations((B, C, S, H))]
    return out


def lattice_cases():
    """{source name: [Case]} at identity geometry, no masks."""
    srcs = {"u8": lattice_u8(), "frac": lattice_frac()}
    out = {k: [Case("lat_%s_%s" % (k, cid), img, ops, geom(img.shape[:2]), []) for cid, ops in chains()] for k, img in srcs.items()}
    wide = lattice_wide()
    out["wide"] = [Case("lat_wide_%s" % cid, wide, ops, geom(wide.shape[:2]), []) for cid, ops in
                   (("h+", [(H, 0.109375)]), ("h-", [(H, -0.5)]), ("hb", [(H, 0.03125), (B, 1.0625)]))]
    return out


def noop_cases():
    return [Case("noop_u8", lattice_u8(), [], geom((1, 1331)), []), Case("noop_frac", lattice_frac(), [], geom((1, 1331)), [])]


# ---- geometry --------------------------------------------------------------------------------------------------------
GEOM_OPS = [(S, 0.75), (B, 1.25)]       # two ops, so that a wrong tap shows; no hue


def seeded(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def two_masks(h, w):
    """A checkerboard and a 1-pixel frame."""
    yy, xx = np.mgrid[0:h, 0:w]
    frame = np.zeros((h, w), np.uint8)
    frame[[0, -1], :] = 1
    frame[:, [0, -1]] = 1
    return [((yy + xx) & 1).astype(np.uint8), frame]


def geometry_cases():
    def case(cid, hw, **kw):
        return Case("geo_" + cid, seeded(len(cid) * 131 + hw[0], *hw), GEOM_OPS, geom(hw, **kw), two_masks(*hw))

    pad4 = dict(resize=(10, 14, 3, 2), out=(16, 24), pad_value=PAD)
    out = [
        case("identity", (12, 20)),
        case("crop_w1", (12, 20), crop=(2, 7, 9, 1), resize=(9, 6)),
        case("crop_h1", (12, 20), crop=(5, 3, 1, 11), resize=(4, 11)),
        case("nw1", (12, 20), resize=(12, 1)),
        case("nh1", (12, 20), resize=(1, 20)),
        case("1x1_to_16", (1, 1), resize=(16, 16)),
        case("97x89_to_5x7", (97, 89), resize=(5, 7)),
        case("corner_up", (12, 20), crop=(7, 13, 5, 7), resize=(40, 56)),              # taps must clamp at the window
        case("area2x_odd_last", (13, 21), crop=(1, 1, 12, 20), resize=(6, 10)),        # 2x2 mean ending on the last row and column
        case("rows2x", (12, 20), resize=(6, 27)),                                      # one axis halves: stays INTER_LINEAR
        case("cols2x", (12, 20), resize=(17, 10)),
        case("pad_hflip", (12, 20), hflip=True, **pad4),
        case("pad_vflip", (12, 20), vflip=True, **pad4),
        case("pad_both", (12, 20), hflip=True, vflip=True, mean=(16.0, 32.0, 64.0), std=(2.0, 4.0, 0.5), **pad4),
        case("pad_bottom_flush", (12, 20), resize=(10, 14, 6, 2), out=(16, 24), pad_value=PAD),
        case("plane_15x17", (12, 20), resize=(11, 13, 2, 3), out=(15, 17), pad_value=PAD),
    ]
    out += [case("src_w%d" % w, (6, w), resize=(9, w + 3)) for w in (1, 7, 8, 9)]
    return out


ONE_AXIS = ("geo_rows2x", "geo_cols2x")


# ---- grey mean -------------------------------------------------------------------------------------------------------
def ramp(seed, h, w):
    """Seeded uint8 noise on a diagonal ramp: the mean of a corner differs from the mean of the whole."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = 200.0 * (yy * w + xx) / max(h * w - 1, 1)
    return np.clip(base[..., None] + np.random.RandomState(seed).randint(0, 56, (h, w, 3)), 0, 255).astype(np.uint8)


BIG = "gray_300x500"


def graymean_cases():
    """Contrast at f = 0.5 into a 32x32 output: x / 2 + mean / 2.  300x500 is the smallest listed source whose chunk (586) takes the
    reduction loop round more than twice; 1x257 leaves most workgroups empty; 16x16 is exactly one pixel per workgroup."""
    big = ramp(7, 300, 500)
    con = [(C, 0.5)]
    pad = dict(out=(32, 32), pad_value=PAD)
    return [
        Case(BIG, big, con, geom((300, 500), crop=(268, 468, 32, 32)), []),
        Case("gray_1x257", ramp(8, 1, 257), con, geom((1, 257), crop=(0, 225, 1, 32), resize=(1, 32, 31, 0), **pad), []),
        Case("gray_1x1", ramp(9, 1, 1) + np.uint8(77), con, geom((1, 1), resize=(1, 1, 5, 9), **pad), []),
        Case("gray_16x16", ramp(10, 16, 16), con, geom((16, 16), crop=(8, 8, 8, 8), resize=(8, 8, 8, 8), **pad), []),
        Case(BIG + "_hsc", big, [(H, 0.109375), (S, 1.5), (C, 0.5)], geom((300, 500), crop=(268, 468, 32, 32)), []),
    ]


# ---- batches ---------------------------------------------------------------------------------------------------------
def batch_cases():
    """One launch: the full chain, ops without contrast, no ops, contrast alone (a taller source, so the image offsets differ and
    the mean is not the crop's), and the fractional lattice, which makes the whole batch travel as float32."""
    u8, frac = lattice_u8(), lattice_frac()
    tall = np.concatenate([u8[:, ::-1], u8, 255 - u8], axis=0)
    fx = FIXED[0]
    return [
        Case("bat_full", u8, [(S, fx[S]), (H, fx[H]), (C, fx[C]), (B, fx[B])], geom((1, 1331)), []),
        Case("bat_hue_bright", u8, [(H, -0.109375), (B, 1.203125)], geom((1, 1331)), []),
        Case("bat_noop", u8, [], geom((1, 1331)), []),
        Case("bat_contrast", tall, [(C, 1.5)], geom((3, 1331), crop=(1, 0, 1, 1331)), []),
        Case("bat_frac", frac, [(B, fx[B]), (C, 0.5), (H, fx[H]), (S, fx[S])], geom((1, 1331)), []),
    ]


def all_cases():
    lat = lattice_cases()
    return lat["u8"] + lat["frac"] + lat["wide"] + noop_cases() + geometry_cases() + graymean_cases() + batch_cases()


# ---- the checkers: the same functions judge the device and the float32 stand-in ----------------------------------------
class Worst:
    """Worst errors seen by one group of checks, for `pytest -s` and DESIGN.md."""

    def __init__(self, name):
        self.name, self.err, self.where, self.seam, self.alt, self.n = name, 0.0, None, 0, 0, 0

    def add(self, stats, cid):
        self.n += 1
        self.seam += stats["seam"]
        self.alt += stats["alt"]
        if stats["err"] >= self.err:
            self.err, self.where = stats["err"], cid

    def __str__(self):
        return "%s: worst |got - float64| = %.3g (0..255 scale, %s) over %d cases; %d seam pixels, %d of them on the other branch" % (
            self.name, self.err, self.where, self.n, self.seam, self.alt)


def check_image(got, case, bound=None):
    """got [3,H,W] normalised.  Every pixel within `bound` (0..255 scale) of the float64 chain a; a pixel with a tap whose float64
    hue lies within SEAM_EPS of the 0/360 seam within `bound` of a OR of alt (the hue carried across the seam).  No allowance.
    Returns dict(err: the worst error against the nearer branch, seam: flagged pixels, alt: flagged pixels that needed alt)."""
    bound = bound_of(case) if bound is None else bound
    plan = plan_of(case)
    assert tuple(got.shape) == (3,) + tuple(plan['out']), "%s: shape %s" % (case.id, got.shape)
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: not finite" % case.id
    std = np.asarray(plan['std'], np.float64)[:, None, None]
    a, alt, seam = A.jitter_branches(case.image, case.ops, SEAM_EPS)
    err = (np.abs(got - A.place_image(a, plan)) * std).max(axis=0)
    stats = dict(seam=0, alt=0)
    if seam.any():
        flagged = A.render_seam(case.image, plan, SEAM_EPS)
        err_alt = (np.abs(got - A.place_image(alt, plan)) * std).max(axis=0)
        stats = dict(seam=int(flagged.sum()), alt=int((flagged & (err > bound) & (err_alt <= bound)).sum()))
        err = np.where(flagged, np.minimum(err, err_alt), err)
    stats["err"] = float(err.max())
    bad = err > bound
    assert not bad.any(), "%s: %d pixels off by up to %.3g (bound %g), first at %s" % (
        case.id, int(bad.sum()), stats["err"], bound, tuple(np.argwhere(bad)[0]))
    return stats


def check_pad(got, case):
    """Pad pixels equal (float32(pad) - mean) / std exactly."""
    plan = plan_of(case)
    nh, nw, pt, pl = plan['resize']
    inside = np.zeros(plan['out'], bool)
    inside[pt:pt + nh, pl:pl + nw] = True
    inside = A._flip(inside, plan)
    want = (np.asarray(plan['pad_value'], np.float32) - np.asarray(plan['mean'], np.float32)) / np.asarray(plan['std'], np.float32)
    for c in range(3):
        assert np.array_equal(np.asarray(got)[c][~inside].view(np.uint32), np.full(int((~inside).sum()), want[c], np.float32).view(np.uint32)), \
            "%s: pad pixels of channel %d" % (case.id, c)
    return int((~inside).sum())


def check_masks(got, case):
    """got [n,H,W] bool: bit-exact to the restatement."""
    want = A.render_masks(np.stack(case.masks), plan_of(case))
    assert got.shape == want.shape and np.array_equal(np.asarray(got, bool), want), "%s: masks" % case.id


def fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def standin(case, mut=()):
    """The float32 stand-in for the device: image [3,H,W] float32."""
    return A.render_image32(case.image, plan_of(case), mut)
