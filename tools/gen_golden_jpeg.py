#!/usr/bin/env python3
"""Writes tests/golden/jpeg_cases.npz: JPEG byte strings and what PIL (libjpeg-turbo; Image.open(...).convert('RGB')) decodes
them to -- the pin of the JPEG decoder (csrc/om_jpeg.cpp + csrc/jpeg.hip).  Data only; needs PIL, which the GPU tests do not.

    python tools/gen_golden_jpeg.py [OUT.npz]

Arrays: name [n] str; kind [n] (0 supported, 1 unsupported, 2 rejected); reason [n] (OM_JPEG_R_* of an unsupported stream);
jpeg uint8 + jpeg_off [n+1]; rgb uint8 + rgb_off [n+1] + shape [n,2] (h, w): PIL's pixels of every stream PIL can read (kinds 0
and 1), nothing for a rejected one.  The file is written with fixed zip timestamps: the same PIL gives the same bytes
(tests/test_jpeg_cpu.py regenerates it).

The cases are the smallest at which each stage can go wrong: sizes from 1x1 over the narrow-chroma rule (width <= 4), single
and partial blocks and MCUs, to several MCU rows; every sampling; quality 1 and 10 (clamping), 75, 100 (unit tables); optimised
Huffman tables; restart intervals; noise, ramps, 0/255 checker, flat; streams re-muxed by byte surgery (fill bytes, COM / APPn
between tables, DHT / DQT split and merged); one stream of each unsupported kind PIL writes; broken streams derived from a
good one.
"""
import io
import os
import sys
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "jpeg_cases.npz")

SIZES = [(1, 1), (2, 3), (3, 4), (4, 5), (5, 3), (7, 9), (8, 8), (9, 17), (16, 16), (15, 31), (17, 33), (33, 65)]     # (h, w)
SAMPLINGS = ["444", "422", "420", "grey"]
SUPPORTED, UNSUPPORTED, REJECTED = 0, 1, 2
R_PROGRESSIVE, R_ORIENTATION, R_RANGE = 1, 12, 14          # include/orienmask_hip.h: OM_JPEG_R_*


def content(kind, h, w, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:h, 0:w]
        c = (((x + y) & 1) * 255).astype(np.uint8)
        return np.stack([c, 255 - c, c], -1)
    if kind == "flat":
        return np.full((h, w, 3), (200, 30, 90), np.uint8)
    raise ValueError(kind)


def encode(a, sampling, quality, **kw):
    from PIL import Image
    buf = io.BytesIO()
    if sampling == "grey":
        Image.fromarray(np.ascontiguousarray(a[:, :, 0])).save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[sampling], **kw)
    return buf.getvalue()


def pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


# ---- byte surgery: the segments in front of the scan ---------------------------------------------------------------
def segments(data):
    """([(marker, payload)], rest): the segments between SOI and SOS, and everything from the SOS marker on."""
    assert data[:2] == b"\xff\xd8"
    pos, segs = 2, []
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        if m == 0xDA:
            return segs, data[pos:]
        n = (data[pos + 2] << 8) | data[pos + 3]
        segs.append((m, data[pos + 4:pos + 2 + n]))
        pos += 2 + n


def join(segs, rest, fill=0):
    out = b"\xff\xd8"
    for m, payload in segs:
        out += b"\xff" * fill + bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, "big") + payload
    return out + b"\xff" * fill + rest


def tables(payload, marker):
    """The single tables of a DQT (0xDB) or DHT (0xC4) payload."""
    out, o = [], 0
    while o < len(payload):
        n = 65 + 64 * (payload[o] >> 4) if marker == 0xDB else 17 + sum(payload[o + 1:o + 17])
        out.append(payload[o:o + n])
        o += n
    return out


def remux(data, how):
    segs, rest = segments(data)
    if how == "fill":
        return join(segs, rest, fill=3)
    if how == "comments":
        out = []
        for k, s in enumerate(segs):
            out.append(s)
            out.append((0xFE, b"between the tables %d" % k))
            out.append((0xE5, b"APP5\0" + bytes(range(7))))
        return join(out, rest)
    if how == "split":
        out = []
        for m, p in segs:
            out.extend([(m, t) for t in tables(p, m)] if m in (0xDB, 0xC4) else [(m, p)])
        return join(out, rest)
    if how == "merged":
        dqt = b"".join(p for m, p in segs if m == 0xDB)
        dht = b"".join(p for m, p in segs if m == 0xC4)
        out = [(m, p) for m, p in segs if m not in (0xDB, 0xC4)]
        sof = [k for k, (m, _) in enumerate(out) if m == 0xC0][0]
        return join(out[:sof] + [(0xDB, dqt)] + out[sof:] + [(0xC4, dht)], rest)
    raise ValueError(how)


def patch_luma_quant0(data, q):
    """The stream with the first entry of quantisation table 0 set to q."""
    segs, rest = segments(data)
    out = []
    for m, p in segs:
        if m == 0xDB:
            p = b"".join((t[:1] + bytes([q]) + t[2:]) if (t[0] & 15) == 0 else t for t in tables(p, m))
        out.append((m, p))
    return join(out, rest)


def cases():
    """[(name, kind, reason, bytes)]"""
    from PIL import Image
    out = []

    def good(name, data):
        out.append((name, SUPPORTED, 0, data))

    seed = 0
    for h, w in SIZES:                                           # every size x every sampling
        for s in SAMPLINGS:
            seed += 1
            good("noise_%dx%d_%s_q75" % (h, w, s), encode(content("noise", h, w, seed), s, 75))
    for h, w in [(5, 3), (9, 17), (17, 33)]:                     # quality, tables, restart intervals, content
        for s in SAMPLINGS:
            for q in (1, 10, 100):
                seed += 1
                good("noise_%dx%d_%s_q%d" % (h, w, s, q), encode(content("noise", h, w, seed), s, q))
            seed += 1
            good("noise_%dx%d_%s_q75_opt" % (h, w, s), encode(content("noise", h, w, seed), s, 75, optimize=True))
            for rst in (1, 3):
                seed += 1
                good("noise_%dx%d_%s_q75_rst%d" % (h, w, s, rst), encode(content("noise", h, w, seed), s, 75, restart_marker_blocks=rst))
            for kind in ("ramp", "checker", "flat"):
                good("%s_%dx%d_%s_q75" % (kind, h, w, s), encode(content(kind, h, w, 0), s, 75))
            good("checker_%dx%d_%s_q1" % (h, w, s), encode(content("checker", h, w, 0), s, 1))
    for h, w in [(2, 3), (3, 4), (4, 5), (15, 31), (33, 65)]:    # the narrow-chroma rule and the plane edges on structured content
        for s in ("422", "420"):
            good("checker_%dx%d_%s_q100" % (h, w, s), encode(content("checker", h, w, 0), s, 100))
            good("ramp_%dx%d_%s_q100" % (h, w, s), encode(content("ramp", h, w, 0), s, 100))
    base = encode(content("noise", 17, 33, 901), "420", 75)
    base_grey = encode(content("noise", 9, 17, 902), "grey", 75, optimize=True)
    for how in ("fill", "comments", "split", "merged"):
        good("remux_%s_420" % how, remux(base, how))
        good("remux_%s_grey" % how, remux(base_grey, how))
    # |coefficient * quantiser| against OM_JPEG_COEF_BOUND = 1170: a flat grey 129 has DC coefficient 8 under unit tables
    flat = encode(np.full((8, 8, 3), 129, np.uint8), "grey", 100)
    good("range_inside_8x146", patch_luma_quant0(flat, 146))
    out.append(("range_beyond_8x147", UNSUPPORTED, R_RANGE, patch_luma_quant0(flat, 147)))
    # unsupported kinds PIL writes
    a = content("noise", 17, 33, 903)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=75, progressive=True)
    out.append(("progressive", UNSUPPORTED, R_PROGRESSIVE, buf.getvalue()))
    exif = Image.Exif()
    exif[0x0112] = 6
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=75, exif=exif.tobytes())
    out.append(("exif_orientation_6", UNSUPPORTED, R_ORIENTATION, buf.getvalue()))
    exif[0x0112] = 1
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=75, exif=exif.tobytes())
    good("exif_orientation_1", buf.getvalue())
    # broken streams, derived from good ones
    segs, rest = segments(base)
    scan = len(base) - len(rest) + 2 + ((rest[2] << 8) | rest[3])          # the first entropy-coded byte
    for k in (0, 1, 3, 20, scan - 5, scan, scan + 1, scan + (len(base) - scan) // 2, len(base) - 3, len(base) - 2):
        out.append(("truncated_%d" % k, REJECTED, 0, base[:k]))
    out.append(("undefined_code", REJECTED, 0, base[:scan] + b"\xff\x00\xff\x00" + base[scan + 4:]))      # sixteen 1 bits: no code
    rst = encode(content("noise", 17, 33, 904), "420", 75, restart_marker_blocks=1)
    k = rst.index(b"\xff\xd0", len(rst) - len(segments(rst)[1]))
    out.append(("bad_restart_number", REJECTED, 0, rst[:k] + b"\xff\xd3" + rst[k + 2:]))
    out.append(("missing_restart", REJECTED, 0, rst[:k] + rst[k + 2:]))
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def build():
    rows = cases()
    assert len({r[0] for r in rows}) == len(rows), "duplicate case names"
    jpeg, rgb, shape = [], [], []
    for name, kind, reason, data in rows:
        jpeg.append(np.frombuffer(data, np.uint8))
        if kind == REJECTED:
            rgb.append(np.zeros(0, np.uint8))
            shape.append((0, 0))
        else:
            px = pil_rgb(data)
            rgb.append(px.reshape(-1))
            shape.append(px.shape[:2])
    off = lambda parts: np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)      # noqa: E731
    return {"name": np.array([r[0] for r in rows]), "kind": np.array([r[1] for r in rows], np.int32),
            "reason": np.array([r[2] for r in rows], np.int32), "jpeg": np.concatenate(jpeg), "jpeg_off": off(jpeg),
            "rgb": np.concatenate(rgb), "rgb_off": off(rgb), "shape": np.array(shape, np.int32)}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    arrays = build()
    write_npz(path, arrays)
    kinds = arrays["kind"]
    print("%s: %d streams (%d supported, %d unsupported, %d rejected), %d bytes of JPEG, %d bytes in the file"
          % (path, len(kinds), (kinds == 0).sum(), (kinds == 1).sum(), (kinds == 2).sum(), arrays["jpeg"].size, os.path.getsize(path)))


if __name__ == "__main__":
    main()
