"""numpy restatement of the device stages of the JPEG decoder (csrc/jpeg.hip), fed by the library's own host entry
om_jpeg_entropy_decode through ctypes (the library loads without a GPU).  It is a second, independent statement of the
arithmetic the header documents -- dequantise, accurate-integer 8x8 IDCT, +128 and clamp, "fancy" chroma up-sampling, YCbCr -> RGB
-- pinned to PIL's decoder by tests/golden/jpeg_cases.npz (tests/test_jpeg_cpu.py).

Every function takes `mutant`: one named deviation of the arithmetic, each of which at least one fixture must catch
(MUTANTS).  islow_1d is written once over anything with + - * : numpy arrays for the decoder, LinForm for the proof that
int32 holds every intermediate (int32_bound).
"""
import ctypes

import numpy as np

from orienmask_amd import lib as omlib

MUTANTS = ("bias_h2v2", "bias_h2v1", "pad_edge", "no_narrow", "descale17", "split_g")

FIX = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137,
           f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)


# ------------------------------------------------------------------------------------------------ the host entries
class Rejected(ValueError):
    """The library returned an error for the stream."""


def info(data):
    """om_jpeg_info: the int32 record as a numpy array; raises Rejected with the library's message."""
    L = omlib.load()
    rec = np.zeros(omlib.OM_JPEG_INFO_WORDS, np.int32)
    buf = np.frombuffer(bytes(data), np.uint8)
    rc = L.om_jpeg_info(buf.ctypes.data if buf.size else None, buf.size, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != 0:
        raise Rejected(L.om_last_error().decode())
    return rec


def comp_rows(rec):
    """[(h, v, blocks per row, block rows, real width, real height)] per component of a supported stream's info record."""
    o, k = omlib.OM_JPEG_I_COMP, omlib.OM_JPEG_COMP_WORDS
    return [tuple(int(v) for v in rec[o + k * c:o + k * c + 6]) for c in range(int(rec[omlib.OM_JPEG_I_NCOMP]))]


def entropy_decode(data, slack=0):
    """om_jpeg_entropy_decode -> (info record, [coef [bh,bw,64] int16 per component], quant [ncomp,64] uint16); coef is None for
    a stream that is unsupported.  `slack` int16 elements of 0x5555 lie behind the buffer and must come back untouched."""
    L = omlib.load()
    rec = info(data)
    buf = np.frombuffer(bytes(data), np.uint8)
    blocks = int(rec[omlib.OM_JPEG_I_BLOCKS]) if rec[omlib.OM_JPEG_I_SUPPORTED] else 0
    coef = np.full(blocks * 64 + slack + 1, 0x5555, np.int16)
    quant = np.zeros((3, 64), np.uint16)
    rc = L.om_jpeg_entropy_decode(buf.ctypes.data, buf.size, coef.ctypes.data, blocks * 128, quant.ctypes.data,
                                  rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != 0:
        raise Rejected(L.om_last_error().decode())
    assert (coef[blocks * 64:] == 0x5555).all(), "om_jpeg_entropy_decode wrote behind its buffer"
    if not rec[omlib.OM_JPEG_I_SUPPORTED]:
        return rec, None, None
    planes, off = [], 0
    for (_, _, bw, bh, _, _) in comp_rows(rec):
        planes.append(coef[off:off + bw * bh * 64].reshape(bh, bw, 64))
        off += bw * bh * 64
    return rec, planes, quant[:len(planes)]


# ------------------------------------------------------------------------------------------------ stage 1
def islow_1d(x, shift, rec=None):
    """One pass of the accurate-integer IDCT over x[0..7] -> the 8 outputs BEFORE `>> shift`, rounding add included.  rec(v) is
    called with every intermediate (the proof's hook)."""
    r = rec if rec is not None else (lambda v: v)
    F = FIX
    z2, z3 = x[2], x[6]
    z1 = r(r(z2 + z3) * F["f0_541"])
    tmp2 = r(z1 + r(z3 * -F["f1_847"]))
    tmp3 = r(z1 + r(z2 * F["f0_765"]))
    z2, z3 = x[0], x[4]
    tmp0 = r(r(z2 + z3) * 8192)
    tmp1 = r(r(z2 - z3) * 8192)
    tmp10, tmp13, tmp11, tmp12 = r(tmp0 + tmp3), r(tmp0 - tmp3), r(tmp1 + tmp2), r(tmp1 - tmp2)
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = r(tmp0 + tmp3), r(tmp1 + tmp2), r(tmp0 + tmp2), r(tmp1 + tmp3)
    z5 = r(r(z3 + z4) * F["f1_175"])
    tmp0, tmp1, tmp2, tmp3 = r(tmp0 * F["f0_298"]), r(tmp1 * F["f2_053"]), r(tmp2 * F["f3_072"]), r(tmp3 * F["f1_501"])
    z1, z2, z3, z4 = r(z1 * -F["f0_899"]), r(z2 * -F["f2_562"]), r(z3 * -F["f1_961"]), r(z4 * -F["f0_390"])
    z3, z4 = r(z3 + z5), r(z4 + z5)
    tmp0 = r(r(tmp0 + z1) + z3)
    tmp1 = r(r(tmp1 + z2) + z4)
    tmp2 = r(r(tmp2 + z2) + z3)
    tmp3 = r(r(tmp3 + z1) + z4)
    rnd = 1 << (shift - 1)
    pairs = ((tmp10, tmp3), (tmp11, tmp2), (tmp12, tmp1), (tmp13, tmp0))
    out = [None] * 8
    for k, (a, b) in enumerate(pairs):
        out[k] = r(r(a + b) + rnd)
        out[7 - k] = r(r(a - b) + rnd)
    return out


def idct_plane(coef, quant, mutant=None):
    """coef [bh,bw,64] int16, quant [64] -> the uint8 plane [8 bh, 8 bw] of whole blocks."""
    bh, bw, _ = coef.shape
    x = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(bh, bw, 8, 8)
    ws = np.stack([v >> 11 for v in islow_1d([x[:, :, k, :] for k in range(8)], 11)], axis=2)        # columns: [bh,bw,k,c]
    shift2 = 17 if mutant == "descale17" else 18
    px = np.stack([v >> shift2 for v in islow_1d([ws[:, :, :, e] for e in range(8)], shift2)], axis=3)   # rows: [bh,bw,r,e]
    px = np.clip(px + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


# ------------------------------------------------------------------------------------------------ stage 2
def _shift(a, d, axis):
    """a moved by one along axis with the edge replicated: d = +1 gives a[i - 1], d = -1 gives a[i + 1]."""
    first, last = np.take(a, [0], axis), np.take(a, [-1], axis)
    n = a.shape[axis]
    if d > 0:
        return np.concatenate([first, np.take(a, range(0, n - 1), axis)], axis)
    return np.concatenate([np.take(a, range(1, n), axis), last], axis)


def upsample_h2v1(p, mutant=None):
    p = p.astype(np.int64)
    if p.shape[1] <= 2 and mutant != "no_narrow":
        return np.repeat(p, 2, axis=1)
    be, bo = (2, 1) if mutant == "bias_h2v1" else (1, 2)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + _shift(p, 1, 1) + be) >> 2
    out[:, 1::2] = (3 * p + _shift(p, -1, 1) + bo) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def upsample_h2v2(p, mutant=None):
    p = p.astype(np.int64)
    if p.shape[1] <= 2 and mutant != "no_narrow":
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    be, bo = (7, 8) if mutant == "bias_h2v2" else (8, 7)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for parity, far in ((0, _shift(p, 1, 0)), (1, _shift(p, -1, 0))):
        s = 3 * p + far
        out[parity::2, 0::2] = (3 * s + _shift(s, 1, 1) + be) >> 4         # at the ends s's neighbour is s itself: (4 s + bias) >> 4
        out[parity::2, 1::2] = (3 * s + _shift(s, -1, 1) + bo) >> 4
    return out


def ycc_to_rgb(y, cb, cr, mutant=None):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    if mutant == "split_g":
        g = y + ((-22554 * cb) >> 16) + ((-46802 * cr + 32768) >> 16)
    else:
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data, mutant=None):
    """The [h,w,3] uint8 RGB image of a SUPPORTED stream."""
    rec, coefs, quant = entropy_decode(data)
    assert coefs is not None, "unsupported stream (reason %d)" % rec[omlib.OM_JPEG_I_REASON]
    w, h = int(rec[omlib.OM_JPEG_I_WIDTH]), int(rec[omlib.OM_JPEG_I_HEIGHT])
    rows = comp_rows(rec)
    planes = [idct_plane(c, q, mutant) for c, q in zip(coefs, quant)]
    if len(planes) == 1:
        return np.repeat(planes[0][:h, :w, None], 3, axis=2)
    hmax, vmax = rows[0][0], rows[0][1]
    chroma = []
    for p, (_, _, _, _, cw, ch) in zip(planes[1:], rows[1:]):
        if mutant != "pad_edge":
            p = p[:ch, :cw]                       # the real plane: its last row and column are the up-sampler's edge
        if hmax == 2:
            p = upsample_h2v2(p, mutant) if vmax == 2 else upsample_h2v1(p, mutant)
        chroma.append(p[:h, :w])
    return ycc_to_rgb(planes[0][:h, :w], chroma[0], chroma[1], mutant)


# ------------------------------------------------------------------------------------------------ the int32 proof
class LinForm:
    """c . x + k over inputs |x_i| <= bound: the largest magnitude is |c|_1 * bound + |k| (the inputs are independent)."""

    def __init__(self, c, k=0):
        self.c, self.k = np.asarray(c, dtype=object), k

    def __add__(self, o):
        return LinForm(self.c + o.c, self.k + o.k) if isinstance(o, LinForm) else LinForm(self.c, self.k + o)

    def __sub__(self, o):
        return LinForm(self.c - o.c, self.k - o.k)

    def __mul__(self, m):
        return LinForm(self.c * m, self.k * m)

    def magnitude(self, bound):
        return int(sum(abs(int(v)) for v in self.c)) * bound + abs(int(self.k))


def int32_bound(B):
    """The largest magnitude any intermediate of the two IDCT passes can take when every |coefficient * quantiser| <= B:
    (pass 1, the bound W of a pass-1 output, pass 2).  Exact integers."""
    def run(bound, shift):
        seen = []
        outs = islow_1d([LinForm([int(i == k) for i in range(8)]) for k in range(8)], shift, rec=lambda v: (seen.append(v), v)[1])
        return max(v.magnitude(bound) for v in seen), max(v.magnitude(bound) for v in outs)
    m1, o1 = run(B, 11)
    W = (o1 >> 11) + 1                  # |(v + round) >> 11| <= |v + round| / 2048 rounded up
    m2, _ = run(W, 18)
    return m1, W, m2


# ------------------------------------------------------------------------------------------------ the fixtures
SUPPORTED, UNSUPPORTED, REJECTED = 0, 1, 2
_CASES = None


class Case:
    """One stream of tests/golden/jpeg_cases.npz: name, kind, reason, data (bytes), rgb ([h,w,3] uint8: PIL's pixels; None for a
    rejected stream)."""

    def __init__(self, name, kind, reason, data, rgb):
        self.name, self.kind, self.reason, self.data, self.rgb = name, kind, reason, data, rgb

    def __repr__(self):
        return "Case(%s)" % self.name


def load_cases():
    """The fixture table, read once and shared (nothing changes it)."""
    global _CASES
    if _CASES is None:
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
        jo, ro, out = z["jpeg_off"], z["rgb_off"], []
        for i, name in enumerate(z["name"]):
            kind = int(z["kind"][i])
            h, w = (int(v) for v in z["shape"][i])
            rgb = None if kind == REJECTED else z["rgb"][ro[i]:ro[i + 1]].reshape(h, w, 3)
            if rgb is not None:
                rgb.setflags(write=False)
            out.append(Case(str(name), kind, int(z["reason"][i]), z["jpeg"][jo[i]:jo[i + 1]].tobytes(), rgb))
        _CASES = out
    return _CASES
