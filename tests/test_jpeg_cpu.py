"""CPU: the JPEG decoder's host entries (csrc/om_jpeg.cpp), the numpy restatement of its device stages (tests/jpeg_np.py) and
the planner and fallback logic of orienmask_amd.jpeg.JpegDecoder, against PIL's pixels in tests/golden/jpeg_cases.npz.

The pin is exact equality: libjpeg's arithmetic is integer.  The host memory-safety check is a stand-alone program
(tools/jpeg_host_check.cpp) built with -fsanitize=address,undefined and run as a child process; nothing is preloaded.
"""
import io
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_np as J
from conftest import REPO
from orienmask_amd import jpeg as omjpeg, lib as omlib

CASES = J.load_cases()
GOOD = [c for c in CASES if c.kind == J.SUPPORTED]


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


# ------------------------------------------------------------------------------------------------ the pin
def test_fixture_table_covers_the_issue():
    names = {c.name for c in CASES}
    assert len(GOOD) >= 150 and os.path.getsize(os.path.join(REPO, "tests", "golden", "jpeg_cases.npz")) < 300 * 1024
    for h, w in [(1, 1), (2, 3), (3, 4), (4, 5), (5, 3), (7, 9), (8, 8), (9, 17), (16, 16), (15, 31), (17, 33), (33, 65)]:
        for s in ("444", "422", "420", "grey"):
            assert "noise_%dx%d_%s_q75" % (h, w, s) in names
    assert {c.reason for c in CASES if c.kind == J.UNSUPPORTED} == {omlib.OM_JPEG_R_PROGRESSIVE, omlib.OM_JPEG_R_ORIENTATION,
                                                                    omlib.OM_JPEG_R_RANGE}
    assert sum(c.kind == J.REJECTED for c in CASES) >= 12


def test_restatement_equals_pil_on_every_fixture(built):
    bad = [c.name for c in GOOD if not np.array_equal(J.decode(c.data), c.rgb)]
    assert bad == []


def test_restatement_equals_pil_decoded_here_and_fixtures_regenerate(built, tmp_path):
    Image = _pil()
    if Image is None:
        pytest.skip("PIL is not importable: the fixtures cannot be re-decoded or regenerated here")
    for c in CASES:
        if c.kind != J.REJECTED:
            with Image.open(io.BytesIO(c.data)) as im:
                assert np.array_equal(np.asarray(im.convert("RGB")), c.rgb), c.name
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_golden_jpeg
    finally:
        sys.path.pop(0)
    out = str(tmp_path / "again.npz")
    gen_golden_jpeg.write_npz(out, gen_golden_jpeg.build())
    with open(out, "rb") as a, open(os.path.join(REPO, "tests", "golden", "jpeg_cases.npz"), "rb") as b:
        assert a.read() == b.read(), "tools/gen_golden_jpeg.py no longer writes the committed fixture file"


@pytest.mark.parametrize("mutant", J.MUTANTS)
def test_every_mutant_is_caught(built, mutant):
    """Each deviation of the arithmetic changes at least one fixture's pixels: the table can tell them apart."""
    caught = [c.name for c in GOOD if not np.array_equal(J.decode(c.data, mutant), c.rgb)]
    assert caught, "no fixture notices mutant %s" % mutant
    if mutant in ("bias_h2v2", "pad_edge", "no_narrow"):
        assert any("420" in n for n in caught)
    if mutant in ("bias_h2v1", "pad_edge", "no_narrow"):
        assert any("422" in n for n in caught)


# ------------------------------------------------------------------------------------------------ the host entries
def test_info_reports_geometry_support_and_reason(built):
    for c in CASES:
        if c.kind == J.REJECTED:
            continue
        rec = J.info(c.data)
        h, w = c.rgb.shape[:2]
        assert (rec[omlib.OM_JPEG_I_WIDTH], rec[omlib.OM_JPEG_I_HEIGHT]) == (w, h), c.name
        if c.kind == J.SUPPORTED or c.reason == omlib.OM_JPEG_R_RANGE:      # the range is found by the entropy decoder only
            assert rec[omlib.OM_JPEG_I_SUPPORTED] == 1 and rec[omlib.OM_JPEG_I_REASON] == omlib.OM_JPEG_R_NONE, c.name
            grey = "grey" in c.name or c.name.startswith("range_")
            assert rec[omlib.OM_JPEG_I_NCOMP] == (1 if grey else 3), c.name
            rows = J.comp_rows(rec)
            hmax, vmax = int(rec[omlib.OM_JPEG_I_HMAX]), int(rec[omlib.OM_JPEG_I_VMAX])
            for s, hv in (("444", (1, 1)), ("422", (2, 1)), ("420", (2, 2)), ("grey", (1, 1))):
                if "_%s" % s in c.name:
                    assert (hmax, vmax) == hv, c.name
            mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
            assert rows[0] == (hmax, vmax, mx * hmax, my * vmax, w, h), c.name
            for r in rows[1:]:
                assert r == (1, 1, mx, my, -(-w // hmax), -(-h // vmax)), c.name
            assert rec[omlib.OM_JPEG_I_BLOCKS] == sum(r[2] * r[3] for r in rows)
        else:
            assert rec[omlib.OM_JPEG_I_SUPPORTED] == 0 and rec[omlib.OM_JPEG_I_REASON] == c.reason, c.name
        rec2, coefs, _ = J.entropy_decode(c.data)
        assert (coefs is not None) == (c.kind == J.SUPPORTED), c.name
        if c.kind == J.UNSUPPORTED:
            assert rec2[omlib.OM_JPEG_I_SUPPORTED] == 0 and rec2[omlib.OM_JPEG_I_REASON] == c.reason, c.name


def test_restart_interval_and_tables_are_reported(built):
    by = {c.name: c for c in CASES}
    assert J.info(by["noise_17x33_420_q75_rst3"].data)[omlib.OM_JPEG_I_RESTART] == 3
    assert J.info(by["noise_17x33_420_q75"].data)[omlib.OM_JPEG_I_RESTART] == 0
    _, _, quant = J.entropy_decode(by["noise_17x33_444_q100"].data)
    assert quant.shape == (3, 64) and (quant == 1).all()                       # quality 100: unit tables
    _, coefs, quant = J.entropy_decode(by["range_inside_8x146"].data)
    assert quant[0, 0] == 146 and coefs[0][0, 0, 0] == 8 and not coefs[0][0, 0, 1:].any()


def test_every_rejected_stream_returns_an_error(built):
    for c in CASES:
        if c.kind != J.REJECTED:
            continue
        with pytest.raises(J.Rejected) as e:
            J.entropy_decode(c.data)
        assert str(e.value), c.name
    by = {c.name: c for c in CASES}
    for name, word in (("undefined_code", "undefined Huffman code"), ("bad_restart_number", "RST0 is due"),
                       ("missing_restart", "restart marker")):
        with pytest.raises(J.Rejected, match=word):
            J.entropy_decode(by[name].data)


def _generator():
    """tools/gen_golden_jpeg.py as a module: its byte-surgery helpers need no PIL."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_golden_jpeg
    finally:
        sys.path.pop(0)
    return gen_golden_jpeg


def test_directed_header_cases(built):
    """Stream kinds PIL does not write, made by byte surgery on a fixture: each is reported unsupported with its reason or
    rejected -- never decoded."""
    base = {c.name: c for c in CASES}["noise_17x33_420_q75"].data
    sof = base.index(b"\xff\xc0")

    def reason(data):
        rec = J.info(data)
        assert rec[omlib.OM_JPEG_I_SUPPORTED] == 0
        return int(rec[omlib.OM_JPEG_I_REASON])

    patched = lambda off, val: base[:off] + bytes([val]) + base[off + 1:]      # noqa: E731
    assert reason(patched(sof + 1, 0xC9)) == omlib.OM_JPEG_R_ARITHMETIC
    assert reason(patched(sof + 1, 0xC3)) == omlib.OM_JPEG_R_LOSSLESS
    assert reason(patched(sof + 1, 0xC1)) == omlib.OM_JPEG_R_FRAME
    assert reason(patched(sof + 4, 12)) == omlib.OM_JPEG_R_PRECISION
    assert reason(base[:sof + 5] + b"\0\0" + base[sof + 7:]) == omlib.OM_JPEG_R_DNL              # height 0
    assert reason(patched(sof + 11, 0x12)) == omlib.OM_JPEG_R_SAMPLING                           # luma 1x2: 4:4:0
    assert reason(patched(sof + 11, 0x41)) == omlib.OM_JPEG_R_SAMPLING                           # luma 4x1: 4:1:1
    assert reason(patched(sof + 10, 82)) == omlib.OM_JPEG_R_COMPONENTS                           # component id 'R'
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    assert reason(base[:2] + adobe + base[2:]) == omlib.OM_JPEG_R_ADOBE
    dqt = base.index(b"\xff\xdb")
    n = (base[dqt + 2] << 8) | base[dqt + 3]
    tabs = base[dqt + 4:dqt + 2 + n]
    wide = bytes([0x10 | tabs[0]]) + b"".join(b"\0" + bytes([v]) for v in tabs[1:65])
    assert reason(base[:dqt] + b"\xff\xdb" + struct.pack(">H", 2 + len(wide)) + wide + base[dqt:]) == omlib.OM_JPEG_R_QUANT16
    sos = base.index(b"\xff\xda")
    one = b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    assert reason(base[:sos] + one + base[sos + 14:]) == omlib.OM_JPEG_R_SCANS                  # a scan of one of three components
    # a second scan behind a complete one is found by the entropy decoder
    rec, coefs, _ = J.entropy_decode(base[:-2] + base[sos:])
    assert coefs is None and rec[omlib.OM_JPEG_I_REASON] == omlib.OM_JPEG_R_SCANS
    # rejected: tables that are referenced but not defined, a segment that runs past the end, garbage between segments
    for data in (base[:dqt] + base[dqt + 2 + n:] if base.count(b"\xff\xdb") == 1 else base[:2] + base[sos:],
                 base[:dqt + 2] + b"\xff\xff" + base[dqt + 4:], base[:2] + b"\x00" + base[2:], b"", b"\xff\xd8", base[:2] + b"\xff\xd9"):
        with pytest.raises(J.Rejected):
            J.info(data)


def test_dc_predictor_and_run_checks(built):
    """A stream whose every DC difference is the largest of category 11 walks the predictor out of int16: rejected."""
    gen = _generator()
    flat = {c.name: c for c in CASES}["range_inside_8x146"].data            # 8 x 8 grey, unit tables but one entry
    sof = flat.index(b"\xff\xc0")
    flat = flat[:sof + 7] + struct.pack(">H", 400) + flat[sof + 9:]           # ... declared 400 wide: 50 blocks
    segs, rest = gen.segments(flat)
    # one DC table with the single symbol 11 (code '0'), one AC table with the single symbol 0 = EOB (code '0'): a block is
    # '0' + 11 bits of DC difference + '0'
    dht = lambda cls: (0xC4, bytes([cls << 4]) + bytes([1] + [0] * 15) + (b"\x0b" if cls == 0 else b"\x00"))      # noqa: E731
    segs = [s for s in segs if s[0] != 0xC4] + [dht(0), dht(1)]
    bits = ("0" + "1" * 11 + "0") * 50
    bits += "1" * (-len(bits) % 8)
    scan = b"".join(bytes([int(bits[k:k + 8], 2)]) + (b"\0" if bits[k:k + 8] == "1" * 8 else b"") for k in range(0, len(bits), 8))
    data = gen.join(segs, rest[:10] + scan + b"\xff\xd9")
    with pytest.raises(J.Rejected, match="DC predictor"):
        J.entropy_decode(data)
    # and an AC table whose only symbol is a run of 15 with a value: the fifth such coefficient lies past 63
    segs = segs[:-1] + [(0xC4, bytes([0x10]) + bytes([1] + [0] * 15) + b"\xf1")]
    bits = "0" + "0" * 11 + "01" * 5
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8))
    with pytest.raises(J.Rejected, match="past coefficient 63"):
        J.entropy_decode(gen.join(segs, rest[:10] + scan + b"\xff\xd9"))


# ------------------------------------------------------------------------------------------------ the int32 bound
def test_int32_holds_every_intermediate_up_to_the_bound(built):
    """Interval arithmetic over the restatement's own IDCT: every intermediate is a linear form of its pass's inputs, its range
    over |input| <= b is b * |coefficients|_1 (+ the rounding constant)."""
    B = omlib.OM_JPEG_COEF_BOUND
    m1, W, m2 = J.int32_bound(B)
    assert max(m1, m2) <= 2 ** 31 - 1, (m1, W, m2)
    assert max(J.int32_bound(B + 10)) > 2 ** 31 - 1               # and the bound is not slack: ten more overflow
    # the forms are the restatement's: a random block through LinForm-free arithmetic agrees with the direct matrix product
    rng = np.random.default_rng(0)
    x = rng.integers(-B, B + 1, (1, 1, 64)).astype(np.int16)
    plane = J.idct_plane(x, np.ones(64, np.uint16))
    c = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * i + 1) * u * np.pi / 16) for u in range(8)] for i in range(8)])
    want = np.clip(np.rint(c @ x.reshape(8, 8).astype(np.float64) @ c.T) + 128, 0, 255)
    assert np.abs(plane.astype(np.float64) - want).max() <= 1
    # an 8-bit image's own coefficients: at most 1024 before quantisation, 1024 + 127 behind the coarsest table's rounding
    assert 1024 + 127 <= B


def test_a_stream_just_beyond_the_bound_is_routed_away(built):
    by = {c.name: c for c in CASES}
    inside, beyond = by["range_inside_8x146"], by["range_beyond_8x147"]
    assert 8 * 146 <= omlib.OM_JPEG_COEF_BOUND < 8 * 147
    assert np.array_equal(J.decode(inside.data), inside.rgb)
    rec, coefs, _ = J.entropy_decode(beyond.data)
    assert coefs is None and rec[omlib.OM_JPEG_I_SUPPORTED] == 0 and rec[omlib.OM_JPEG_I_REASON] == omlib.OM_JPEG_R_RANGE


# ------------------------------------------------------------------------------------------------ the planner and the fallback
class HostStandIn(omjpeg.JpegDecoder):
    """JpegDecoder with the device replaced: the staging buffer is ordinary memory, the copy a clone, and the launch the numpy
    restatement reading the staged bytes THROUGH the descriptor table -- so the planner's offsets are what is tested."""

    def __init__(self, **kw):
        super().__init__("cuda", **kw)
        self.launches, self.uploads = [], 0

    def _alloc_stage(self, size):
        return torch.empty(size, dtype=torch.uint8)

    def _new_event(self):
        class Event:
            def synchronize(self):
                pass

            def record(self, stream=None):
                pass
        return Event()

    def _guard(self):
        import contextlib
        return contextlib.nullcontext()

    def _to_device(self, image):
        return torch.from_numpy(image)

    def _upload(self, pinned, nbytes, event):
        self.uploads += 1
        return pinned[:nbytes].clone()

    def _launch(self, p, staged):
        self.launches.append(len(p.desc))
        raw = staged.numpy()
        coef = raw[:p.quant_stage_off].view(np.int16)
        quant = raw[p.quant_stage_off:p.stage_bytes].view(np.uint16)
        assert coef.size == p.coef_elems and quant.size == p.quant_elems
        out = np.full(p.out_bytes, 0xEE, np.uint8)
        for w, h, nc, hmax, vmax, co, qo, oo in p.desc:
            assert co % 64 == 0 and qo % 64 == 0 and oo % 16 == 0
            mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
            planes, chroma = [], []
            for c in range(nc):
                bw, bh = (mx * hmax, my * vmax) if c == 0 else (mx, my)
                planes.append(J.idct_plane(coef[co:co + bw * bh * 64].reshape(bh, bw, 64), quant[qo + 64 * c:qo + 64 * c + 64]))
                co += bw * bh * 64
            if nc == 1:
                rgb = np.repeat(planes[0][:h, :w, None], 3, axis=2)
            else:
                for pl in planes[1:]:
                    pl = pl[:-(-h // vmax), :-(-w // hmax)]
                    if hmax == 2:
                        pl = J.upsample_h2v2(pl) if vmax == 2 else J.upsample_h2v1(pl)
                    chroma.append(pl[:h, :w])
                rgb = J.ycc_to_rgb(planes[0][:h, :w], chroma[0], chroma[1])
            out[oo:oo + h * w * 3] = rgb.reshape(-1)
        return torch.from_numpy(out)


def _mixed(n):
    """n supported fixtures of mixed sizes and samplings"""
    pick = [c for c in GOOD if "_q75" in c.name and c.name.startswith("noise")]
    return (pick[::5] + pick)[:n]                  # a stride coprime to the four samplings the table cycles through


def test_planner_and_decode_with_a_stand_in_device(built, tmp_path):
    d = HostStandIn(threads=4)
    cases = _mixed(17)
    assert len({c.rgb.shape for c in cases}) > 5 and len({c.name.split("_")[2] for c in cases}) == 4
    path = tmp_path / "a.jpg"
    path.write_bytes(cases[3].data)
    items = [c.data for c in cases]
    items[3] = str(path)                                                          # a path among the bytes
    got = d.decode(items)
    assert d.uploads == 1 and d.launches == [17]                                 # one copy, one call (the library cuts it into sets)
    for g, c in zip(got, cases):
        assert g.dtype == torch.uint8 and np.array_equal(g.numpy(), c.rgb), c.name
    assert d.stats() == {"device": 17, "fallback": 0, "reasons": {}}
    p = omjpeg.plan([J.info(c.data) for c in cases])
    assert p.desc.shape == (17, omlib.OM_JPEG_DESC_WORDS) and p.desc.dtype == np.int64
    assert p.coef_off == sorted(p.coef_off) and p.stage_bytes == 2 * p.coef_elems + 2 * 192 * 17
    assert all(b - a >= c.rgb.size for a, b, c in zip(p.out_off, p.out_off[1:] + [p.out_bytes], cases))
    assert d.decode([]) == []


def test_fallback_raise_and_rejected_with_a_stand_in_device(built):
    by = {c.name: c for c in CASES}
    seen = []

    def reader(data):
        seen.append(len(data))
        return by["progressive"].rgb if data == by["progressive"].data else by["exif_orientation_6"].rgb

    d = HostStandIn(threads=2, imread=reader)
    items = [GOOD[5].data, by["progressive"].data, GOOD[40].data, by["exif_orientation_6"].data, by["range_beyond_8x147"].data]
    flat = by["range_beyond_8x147"].rgb
    d2 = HostStandIn(threads=2, imread=lambda data: flat if data == by["range_beyond_8x147"].data else reader(data))
    got = d2.decode(items)
    for g, want in zip(got, [GOOD[5].rgb, by["progressive"].rgb, GOOD[40].rgb, by["exif_orientation_6"].rgb, flat]):
        assert np.array_equal(g.numpy(), want)
    assert d2.stats() == {"device": 2, "fallback": 3, "reasons": {"progressive": 1, "orientation": 1, "range": 1}}
    assert d2.launches == [2] and d2.uploads == 1            # the stream found unsupported while decoding caused a second plan, no launch
    # 'raise': names the item and the reason, nothing launched
    d3 = HostStandIn(on_unsupported="raise")
    with pytest.raises(omjpeg.JpegError, match=r"item 1 .*progressive"):
        d3.decode(items[:2])
    with pytest.raises(omjpeg.JpegError, match=r"item 0 .*range"):
        d3.decode([by["range_beyond_8x147"].data])
    assert d3.launches == [] and d3.uploads == 0
    # a rejected stream raises before anything is launched, names the item, and the decoder stays usable
    for bad in ("truncated_20", "truncated_%d" % max(int(c.name.split("_")[1]) for c in CASES if c.name.startswith("truncated_")),
                "undefined_code", "bad_restart_number"):
        with pytest.raises(omjpeg.JpegError, match="item 2"):
            d.decode([GOOD[0].data, GOOD[1].data, by[bad].data, GOOD[2].data])
    assert d.launches == [] and d.uploads == 0
    assert np.array_equal(d.decode([GOOD[7].data])[0].numpy(), GOOD[7].rgb)
    with pytest.raises(ValueError):
        HostStandIn(on_unsupported="ignore")
    with pytest.raises(TypeError):
        d.decode([17])
    assert omjpeg.JpegDecoder("cuda", threads=1000).threads == omjpeg.MAX_THREADS


# ------------------------------------------------------------------------------------------------ host memory safety
def test_host_entries_under_address_and_undefined_sanitizers(built, tmp_path):
    """tools/jpeg_host_check.cpp + csrc/om_jpeg.cpp, built by the plain host compiler with -fsanitize=address,undefined, over
    every fixture stream, every prefix of a few and seeded single-byte corruptions of each: a child process that must exit
    clean.  Nothing runs under Python and nothing is preloaded."""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_host_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tools", "jpeg_host_check.cpp"),
           os.path.join(REPO, "orienmask_amd", "csrc", "om_jpeg.cpp"), "-o", exe]
    # the sanitizer runtimes linked INTO the program where the compiler has them as archives (gcc's flags; clang's default)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    # the streams the prefixes are taken of come first: one of each sampling with restart markers, one optimised grey
    by = {c.name: c for c in CASES}
    first = [by[n] for n in ("noise_17x33_420_q75_rst3", "noise_9x17_422_q75_rst1", "noise_9x17_grey_q75_opt", "noise_5x3_444_q1")]
    order = first + [c for c in CASES if c not in first]
    flat = tmp_path / "streams.bin"
    with open(flat, "wb") as f:
        f.write(struct.pack("<I", len(order)))
        for c in order:
            f.write(struct.pack("<I", len(c.data)) + c.data)
    run = subprocess.run([exe, str(flat), str(len(first)), "48"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-3000:]
    assert "FAILED" not in run.stdout and "%d streams" % len(order) in run.stdout, run.stdout[-500:]
