// Host side of the JPEG decoder (include/orienmask_hip.h: om_jpeg_info, om_jpeg_entropy_decode): the marker parser and the
// Huffman entropy decoder of baseline JPEG -- the inherently serial part.  What comes out are the UNDEQUANTISED coefficients,
// de-zigzagged, [block][64] per component in raster order of the component's block-padded plane, and the quantisation table of
// every component in natural order; csrc/jpeg.hip does the rest on the device (dequantise, IDCT, up-sampling, colour).
//
// Plain C++: no HIP call, no device memory, nothing that initialises the GPU -- a loader worker may call it -- and no include of
// the library's HIP headers, so that it compiles with a plain host compiler into a stand-alone program (tools/jpeg_host_check.cpp
// builds it with -fsanitize=address,undefined).  The only symbol it takes from the rest of the library is om::set_error.
//
// Three outcomes, never mixed:
//   supported      info[OM_JPEG_I_SUPPORTED] = 1: the device path decodes it bit for bit as libjpeg does
//   unsupported    a well-formed stream of a kind the device path does not do (progressive, Exif orientation, ...): status OM_OK,
//                  supported = 0 and a reason code; the caller hands the bytes to a host reader.  Never guessed at.
//   rejected       a broken stream (truncated, undefined Huffman code, run past coefficient 63, bad restart sequence, DC
//                  predictor outside int16, ...): status OM_EINVAL and a message.
// Every read is checked against the given length and every write against the given capacity, for any byte string whatever.
//
// OM_JPEG_COEF_BOUND.  The device IDCT works in int32 where libjpeg's C code works in `long` (64 bits on this platform).  Every
// intermediate of the accurate-integer IDCT is a linear form of the eight inputs of its pass, so its largest magnitude over
// |input| <= b is b times the form's L1 norm.  Pass 1 (columns, inputs |coef * quant| <= B): the largest L1 norm, rounding add
// included, is that of an output sum before the descale, 61 214 B + 1024; its descaled outputs are bounded by W = 29.9 B + 1.
// Pass 2 (rows, inputs <= W): 61 214 W + 2^17 <= 2^31 - 1 gives B <= 1173.  OM_JPEG_COEF_BOUND = 1170 is what the header states
// and tests/test_jpeg_cpu.py re-derives by interval arithmetic over the linear forms of tests/jpeg_np.py's restatement.  A
// stream with one |coef * quant| beyond it is reported unsupported (OM_JPEG_R_RANGE).  An 8-bit image's own coefficients are at
// most 1024 in magnitude before quantisation and 1024 + 127 after the coarsest table's rounding.
#include <cstdarg>
#include <cstdint>
#include <cstring>

#include "../../include/orienmask_hip.h"

namespace om {
void set_error(const char* fmt, ...);
}

namespace {

#define JP_FAIL(...)                                                                    \
    do {                                                                                \
        om::set_error(__VA_ARGS__);                                                     \
        return OM_EINVAL;                                                               \
    } while (0)

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK = 9;      // bits of the Huffman lookahead table

struct Huff {
    bool defined = false;
    uint8_t counts[17];      // codes of each length 1..16
    uint8_t vals[256];
    int nvals;
    int32_t maxcode[18];     // largest code of length l, -1 if none
    int32_t valoff[17];      // vals index of the first code of length l minus that code
    uint16_t look[1 << LOOK];   // (length << 8) | symbol for codes of at most LOOK bits, 0: longer or undefined
};

struct Comp {
    int id, h, v, tq, td, ta;
};

struct Header {
    int width = 0, height = 0, ncomp = 0, hmax = 1, vmax = 1, restart = 0;
    int reason = OM_JPEG_R_NONE;        // first reason the stream is unsupported
    Comp comp[4];
    bool have_sof = false;
    uint16_t quant[4][64];              // natural order
    bool quant_defined[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    size_t scan = 0;                    // offset of the first entropy-coded byte
    int mcus_x = 0, mcus_y = 0;
    int bw[3], bh[3], cw[3], ch[3];
};

inline void unsupported(Header& hd, int reason) {
    if (hd.reason == OM_JPEG_R_NONE) hd.reason = reason;
}

int build_huff(Huff& t, bool is_dc, int cls_id) {
    int code = 0, k = 0;
    memset(t.look, 0, sizeof(t.look));
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        if (t.counts[l]) {
            if (code + t.counts[l] > (1 << l)) JP_FAIL("jpeg: Huffman table %d: more codes of length %d than the code space holds", cls_id, l);
            for (int i = 0; i < t.counts[l]; ++i, ++k, ++code) {
                if (is_dc && t.vals[k] > 15) JP_FAIL("jpeg: DC Huffman table %d: symbol %d", cls_id, t.vals[k]);
                if (l <= LOOK) {
                    const int first = code << (LOOK - l);
                    for (int j = 0; j < (1 << (LOOK - l)); ++j) t.look[first + j] = (uint16_t)((l << 8) | t.vals[k]);
                }
            }
            t.maxcode[l] = code - 1;
        } else {
            t.maxcode[l] = -1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.defined = true;
    return OM_OK;
}

// Exif: the orientation tag (0x0112) of IFD0, or 0 when there is none that can be read.  body = the segment behind "Exif\0\0".
int exif_orientation(const uint8_t* b, size_t n) {
    if (n < 8) return 0;
    const bool le = b[0] == 'I' && b[1] == 'I';
    if (!le && !(b[0] == 'M' && b[1] == 'M')) return 0;
    auto u16 = [&](size_t o) { return le ? (unsigned)(b[o] | (b[o + 1] << 8)) : (unsigned)((b[o] << 8) | b[o + 1]); };
    auto u32 = [&](size_t o) {
        return le ? ((uint32_t)b[o] | ((uint32_t)b[o + 1] << 8) | ((uint32_t)b[o + 2] << 16) | ((uint32_t)b[o + 3] << 24))
                  : (((uint32_t)b[o] << 24) | ((uint32_t)b[o + 1] << 16) | ((uint32_t)b[o + 2] << 8) | (uint32_t)b[o + 3]);
    };
    if (u16(2) != 42) return 0;
    const size_t ifd = u32(4);
    if (ifd > n || n - ifd < 2) return 0;
    const size_t count = u16(ifd);
    for (size_t i = 0; i < count; ++i) {
        const size_t e = ifd + 2 + 12 * i;
        if (e > n || n - e < 12) return 0;
        if (u16(e) == 0x0112) return (int)u16(e + 8);
    }
    return 0;
}

// Everything up to the first entropy-coded byte.  OM_OK with hd.reason set for an unsupported stream (the geometry is filled as
// far as the frame header gives it), OM_EINVAL for a broken one.
int parse_header(const uint8_t* p, size_t len, Header& hd) {
    if (len < 4 || p[0] != 0xFF || p[1] != 0xD8) JP_FAIL("jpeg: no SOI marker");
    size_t pos = 2;
    for (;;) {
        if (pos >= len) JP_FAIL("jpeg: truncated in the header (at byte %zu)", pos);
        if (p[pos] != 0xFF) JP_FAIL("jpeg: byte 0x%02x where a marker should be (at byte %zu)", p[pos], pos);
        while (pos < len && p[pos] == 0xFF) ++pos;          // fill bytes
        if (pos >= len) JP_FAIL("jpeg: truncated in the header (at byte %zu)", pos);
        const int m = p[pos++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // stand-alone markers
        if (m == 0xD9) JP_FAIL("jpeg: EOI before any scan");
        if (m == 0x00) JP_FAIL("jpeg: stuffed byte in the header (at byte %zu)", pos);
        if (len - pos < 2) JP_FAIL("jpeg: truncated in the header (at byte %zu)", pos);
        const size_t seg = ((size_t)p[pos] << 8) | p[pos + 1];
        if (seg < 2 || seg > len - pos) JP_FAIL("jpeg: segment 0x%02x of %zu bytes runs past the end (at byte %zu)", m, seg, pos);
        const uint8_t* s = p + pos + 2;
        const size_t n = seg - 2;
        pos += seg;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {      // a frame header
            if (hd.have_sof) JP_FAIL("jpeg: a second frame header");
            if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) unsupported(hd, OM_JPEG_R_PROGRESSIVE);
            else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) unsupported(hd, OM_JPEG_R_LOSSLESS);
            else if (m >= 0xC9) unsupported(hd, OM_JPEG_R_ARITHMETIC);
            else if (m != 0xC0) unsupported(hd, OM_JPEG_R_FRAME);      // SOF1 (extended sequential) and SOF5: not the baseline process
            if (n < 6) JP_FAIL("jpeg: short frame header");
            const int prec = s[0];
            hd.height = (s[1] << 8) | s[2];
            hd.width = (s[3] << 8) | s[4];
            hd.ncomp = s[5];
            if (n != 6 + 3 * (size_t)hd.ncomp) JP_FAIL("jpeg: frame header of %zu bytes for %d components", n, hd.ncomp);
            if (hd.width == 0) JP_FAIL("jpeg: width 0");
            if (prec != 8) unsupported(hd, prec == 12 || prec == 16 ? OM_JPEG_R_PRECISION : OM_JPEG_R_FRAME);
            if (hd.height == 0) unsupported(hd, OM_JPEG_R_DNL);
            if (hd.ncomp == 4) unsupported(hd, OM_JPEG_R_COMPONENTS);
            else if (hd.ncomp != 1 && hd.ncomp != 3) unsupported(hd, OM_JPEG_R_COMPONENTS);
            for (int c = 0; c < hd.ncomp && c < 4; ++c) {
                Comp& q = hd.comp[c];
                q.id = s[6 + 3 * c]; q.h = s[7 + 3 * c] >> 4; q.v = s[7 + 3 * c] & 15; q.tq = s[8 + 3 * c];
                q.td = q.ta = 0;
                if (q.h < 1 || q.h > 4 || q.v < 1 || q.v > 4 || q.tq > 3) JP_FAIL("jpeg: component %d: sampling %dx%d, table %d", c, q.h, q.v, q.tq);
            }
            if (hd.ncomp == 3) {
                if (hd.comp[0].id != 1 || hd.comp[1].id != 2 || hd.comp[2].id != 3) unsupported(hd, OM_JPEG_R_COMPONENTS);
                const Comp* q = hd.comp;
                const bool chroma1 = q[1].h == 1 && q[1].v == 1 && q[2].h == 1 && q[2].v == 1;
                const bool luma_ok = (q[0].h == 1 && q[0].v == 1) || (q[0].h == 2 && q[0].v == 1) || (q[0].h == 2 && q[0].v == 2);
                if (!chroma1 || !luma_ok) unsupported(hd, OM_JPEG_R_SAMPLING);
                hd.hmax = q[0].h; hd.vmax = q[0].v;
            } else if (hd.ncomp == 1) {
                if (hd.comp[0].h != 1 || hd.comp[0].v != 1) unsupported(hd, OM_JPEG_R_SAMPLING);
            }
            if ((long long)hd.width * hd.height * 3 >= (1ll << 31)) unsupported(hd, OM_JPEG_R_SIZE);
            hd.have_sof = true;
        } else if (m == 0xC4) {                                  // DHT: one or more tables
            size_t o = 0;
            while (o < n) {
                if (n - o < 17) JP_FAIL("jpeg: short Huffman table segment");
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) JP_FAIL("jpeg: Huffman table class %d id %d", tc, th);
                Huff& t = tc ? hd.ac[th] : hd.dc[th];
                int total = 0;
                t.counts[0] = 0;
                for (int l = 1; l <= 16; ++l) { t.counts[l] = s[o + l]; total += s[o + l]; }
                if (total > 256 || (size_t)total > n - o - 17) JP_FAIL("jpeg: Huffman table with %d symbols in %zu bytes", total, n - o - 17);
                memcpy(t.vals, s + o + 17, (size_t)total);
                t.nvals = total;
                o += 17 + (size_t)total;
                const int rc = build_huff(t, tc == 0, th);
                if (rc != OM_OK) return rc;
            }
        } else if (m == 0xDB) {                                  // DQT: one or more tables
            size_t o = 0;
            while (o < n) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq > 1 || tq > 3) JP_FAIL("jpeg: quantisation table precision %d id %d", pq, tq);
                const size_t need = 1 + (pq ? 128 : 64);
                if (n - o < need) JP_FAIL("jpeg: short quantisation table segment");
                if (pq) unsupported(hd, OM_JPEG_R_QUANT16);
                for (int k = 0; k < 64; ++k)
                    hd.quant[tq][ZIGZAG[k]] = pq ? (uint16_t)((s[o + 1 + 2 * k] << 8) | s[o + 2 + 2 * k]) : s[o + 1 + k];
                hd.quant_defined[tq] = true;
                o += need;
            }
        } else if (m == 0xCC) {
            unsupported(hd, OM_JPEG_R_ARITHMETIC);
        } else if (m == 0xDC) {
            unsupported(hd, OM_JPEG_R_DNL);
        } else if (m == 0xDD) {
            if (n != 2) JP_FAIL("jpeg: restart interval segment of %zu bytes", n);
            hd.restart = (s[0] << 8) | s[1];
        } else if (m == 0xEE) {
            if (n >= 5 && memcmp(s, "Adobe", 5) == 0) unsupported(hd, OM_JPEG_R_ADOBE);
        } else if (m == 0xE1) {
            if (n >= 6 && memcmp(s, "Exif\0\0", 6) == 0) {
                const int o = exif_orientation(s + 6, n - 6);
                if (o != 0 && o != 1) unsupported(hd, OM_JPEG_R_ORIENTATION);
            }
        } else if (m == 0xDA) {                                  // SOS
            if (!hd.have_sof) JP_FAIL("jpeg: scan before the frame header");
            if (n < 1) JP_FAIL("jpeg: short scan header");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) JP_FAIL("jpeg: scan header of %zu bytes for %d components", n, ns);
            if (ns != hd.ncomp) unsupported(hd, OM_JPEG_R_SCANS);
            else
                for (int c = 0; c < ns && c < 4; ++c) {
                    if (s[1 + 2 * c] != hd.comp[c].id) { unsupported(hd, OM_JPEG_R_SCANS); break; }
                    hd.comp[c].td = s[2 + 2 * c] >> 4;
                    hd.comp[c].ta = s[2 + 2 * c] & 15;
                    if (hd.comp[c].td > 3 || hd.comp[c].ta > 3) JP_FAIL("jpeg: scan component %d: tables %d/%d", c, hd.comp[c].td, hd.comp[c].ta);
                }
            if (hd.reason == OM_JPEG_R_NONE && (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0))
                JP_FAIL("jpeg: a sequential scan with spectral selection %d..%d, approximation 0x%02x", s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]);
            hd.scan = pos;
            break;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
    if (hd.reason == OM_JPEG_R_NONE) {
        for (int c = 0; c < hd.ncomp; ++c) {
            const Comp& q = hd.comp[c];
            if (!hd.quant_defined[q.tq]) JP_FAIL("jpeg: component %d uses quantisation table %d, which is not defined", c, q.tq);
            if (!hd.dc[q.td].defined || !hd.ac[q.ta].defined) JP_FAIL("jpeg: component %d uses an undefined Huffman table (%d/%d)", c, q.td, q.ta);
        }
        hd.mcus_x = (hd.width + 8 * hd.hmax - 1) / (8 * hd.hmax);
        hd.mcus_y = (hd.height + 8 * hd.vmax - 1) / (8 * hd.vmax);
        for (int c = 0; c < hd.ncomp; ++c) {
            hd.bw[c] = hd.mcus_x * hd.comp[c].h;
            hd.bh[c] = hd.mcus_y * hd.comp[c].v;
            hd.cw[c] = (hd.width * hd.comp[c].h + hd.hmax - 1) / hd.hmax;
            hd.ch[c] = (hd.height * hd.comp[c].v + hd.vmax - 1) / hd.vmax;
        }
    }
    return OM_OK;
}

void fill_info(const Header& hd, int32_t* info) {
    memset(info, 0, sizeof(int32_t) * OM_JPEG_INFO_WORDS);
    info[OM_JPEG_I_WIDTH] = hd.width;
    info[OM_JPEG_I_HEIGHT] = hd.height;
    info[OM_JPEG_I_NCOMP] = hd.ncomp;
    info[OM_JPEG_I_SUPPORTED] = hd.reason == OM_JPEG_R_NONE ? 1 : 0;
    info[OM_JPEG_I_REASON] = hd.reason;
    info[OM_JPEG_I_HMAX] = hd.hmax;
    info[OM_JPEG_I_VMAX] = hd.vmax;
    info[OM_JPEG_I_RESTART] = hd.restart;
    if (hd.reason != OM_JPEG_R_NONE) return;
    long long blocks = 0;
    for (int c = 0; c < hd.ncomp; ++c) {
        int32_t* r = info + OM_JPEG_I_COMP + OM_JPEG_COMP_WORDS * c;
        r[0] = hd.comp[c].h; r[1] = hd.comp[c].v; r[2] = hd.bw[c]; r[3] = hd.bh[c]; r[4] = hd.cw[c]; r[5] = hd.ch[c];
        blocks += (long long)hd.bw[c] * hd.bh[c];
    }
    info[OM_JPEG_I_BLOCKS] = (int32_t)blocks;      // < 2^31 / 64 (OM_JPEG_R_SIZE)
}

// The entropy-coded segment as a bit stream: byte stuffing removed, stops at a marker or at the end of the buffer.  Only bits
// that are in the data are ever handed out: a request for more is a truncated stream.
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int n = 0;               // valid bits at the low end of acc
    bool stop = false;       // a marker or the end of the buffer lies at p

    void fill() {
        while (n <= 56 && !stop) {
            if (p >= end) { stop = true; break; }
            unsigned b = *p;
            if (b == 0xFF) {
                if (end - p < 2) { stop = true; break; }
                if (p[1] == 0x00) p += 2;
                else { stop = true; break; }          // a marker (or fill bytes in front of one): left for the caller
            } else {
                ++p;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    // the next k <= 16 bits, zero-padded past the end of the data; nothing is consumed
    unsigned peek(int k) {
        if (n < k) fill();
        return n >= k ? (unsigned)(acc >> (n - k)) & ((1u << k) - 1) : (unsigned)(acc << (k - n)) & ((1u << k) - 1);
    }
    void reset() { acc = 0; n = 0; stop = false; }
};

// one Huffman symbol, or -1 (undefined code) / -2 (the data ends inside it)
inline int decode_symbol(Bits& b, const Huff& t) {
    const unsigned e = t.look[b.peek(LOOK)];
    if (e) {
        const int l = (int)(e >> 8);
        if (l > b.n) return -2;
        b.n -= l;
        return (int)(e & 0xff);
    }
    const unsigned v = b.peek(16);
    for (int l = LOOK + 1; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= t.maxcode[l]) {
            if (l > b.n) return -2;
            b.n -= l;
            return t.vals[t.valoff[l] + code];      // valoff + code < nvals: code lies between the length's first and last code
        }
    }
    return b.n < 16 && b.stop ? -2 : -1;
}

// s more bits as the signed value of category s (1..15)
inline bool receive_extend(Bits& b, int s, int& out) {
    if (b.n < s) b.fill();
    if (b.n < s) return false;
    const int v = (int)((b.acc >> (b.n - s)) & ((1u << s) - 1));
    b.n -= s;
    out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    return true;
}

}  // namespace

extern "C" {

int om_jpeg_info(const uint8_t* bytes, size_t len, int32_t* info) {
    if (!bytes || !info) JP_FAIL("om_jpeg_info: null argument");
    Header* hd = new Header;                           // 10 KiB of tables: not on a worker thread's stack
    const int rc = parse_header(bytes, len, *hd);
    if (rc == OM_OK) fill_info(*hd, info);
    delete hd;
    return rc;
}

int om_jpeg_entropy_decode(const uint8_t* bytes, size_t len, int16_t* coef, size_t cap_bytes, uint16_t* quant, int32_t* info) {
    if (!bytes || !coef || !quant || !info) JP_FAIL("om_jpeg_entropy_decode: null argument");
    Header* hdp = new Header;
    struct Free { Header* h; ~Free() { delete h; } } guard{hdp};
    Header& hd = *hdp;
    int rc = parse_header(bytes, len, hd);
    if (rc != OM_OK) return rc;
    fill_info(hd, info);
    if (hd.reason != OM_JPEG_R_NONE) return OM_OK;      // unsupported: nothing is decoded
    const size_t need = (size_t)info[OM_JPEG_I_BLOCKS] * 64 * sizeof(int16_t);
    if (cap_bytes < need) {
        om::set_error("om_jpeg_entropy_decode: the coefficient buffer has %zu bytes, the stream needs %zu", cap_bytes, need);
        return OM_ENOMEM;
    }
    int16_t* plane[3];
    {
        size_t off = 0;
        for (int c = 0; c < hd.ncomp; ++c) {
            plane[c] = coef + off;
            off += (size_t)hd.bw[c] * hd.bh[c] * 64;
            memcpy(quant + 64 * c, hd.quant[hd.comp[c].tq], 64 * sizeof(uint16_t));
        }
    }
    memset(coef, 0, need);
    Bits b;
    b.p = bytes + hd.scan;
    b.end = bytes + len;
    int pred[3] = {0, 0, 0};
    bool beyond = false;
    const long long mcus = (long long)hd.mcus_x * hd.mcus_y;
    int next_rst = 0;
    long long until_rst = hd.restart ? hd.restart : -1;
    long long m = 0;
    for (int my = 0; my < hd.mcus_y; ++my) {
        for (int mx = 0; mx < hd.mcus_x; ++mx, ++m) {
            if (until_rst == 0) {                       // a restart marker is due in front of this MCU
                b.reset();                              // the rest of the last byte is padding
                const uint8_t* p = b.p;
                if (p >= b.end || *p != 0xFF) JP_FAIL("jpeg: no restart marker in front of MCU %lld", m);
                while (p < b.end && *p == 0xFF) ++p;
                if (p >= b.end) JP_FAIL("jpeg: truncated at a restart marker (MCU %lld)", m);
                if (*p != 0xD0 + next_rst) JP_FAIL("jpeg: marker 0x%02x where RST%d is due (MCU %lld)", *p, next_rst, m);
                b.p = p + 1;
                next_rst = (next_rst + 1) & 7;
                until_rst = hd.restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < hd.ncomp; ++c) {
                const Comp& q = hd.comp[c];
                const Huff& dct = hd.dc[q.td];
                const Huff& act = hd.ac[q.ta];
                const uint16_t* qt = hd.quant[q.tq];
                for (int v = 0; v < q.v; ++v)
                    for (int h = 0; h < q.h; ++h) {
                        int16_t* blk = plane[c] + ((size_t)(my * q.v + v) * hd.bw[c] + (size_t)(mx * q.h + h)) * 64;
                        int s = decode_symbol(b, dct);
                        if (s < 0) JP_FAIL(s == -1 ? "jpeg: undefined Huffman code (MCU %lld)" : "jpeg: the scan is truncated (MCU %lld)", m);
                        int diff = 0;
                        if (s && !receive_extend(b, s, diff)) JP_FAIL("jpeg: the scan is truncated (MCU %lld)", m);
                        pred[c] += diff;
                        if (pred[c] < -32768 || pred[c] > 32767) JP_FAIL("jpeg: DC predictor %d outside int16 (MCU %lld)", pred[c], m);
                        blk[0] = (int16_t)pred[c];
                        if ((long long)(pred[c] < 0 ? -pred[c] : pred[c]) * qt[0] > OM_JPEG_COEF_BOUND) beyond = true;
                        for (int k = 1; k < 64; ++k) {
                            const int rs = decode_symbol(b, act);
                            if (rs < 0) JP_FAIL(rs == -1 ? "jpeg: undefined Huffman code (MCU %lld)" : "jpeg: the scan is truncated (MCU %lld)", m);
                            const int r = rs >> 4, sz = rs & 15;
                            if (sz == 0) {
                                if (r != 15) break;                         // EOB
                                k += 15;
                                if (k > 63) JP_FAIL("jpeg: zero run past coefficient 63 (MCU %lld)", m);
                                continue;
                            }
                            k += r;
                            if (k > 63) JP_FAIL("jpeg: run past coefficient 63 (MCU %lld)", m);
                            int val;
                            if (!receive_extend(b, sz, val)) JP_FAIL("jpeg: the scan is truncated (MCU %lld)", m);
                            const int z = ZIGZAG[k];
                            blk[z] = (int16_t)val;
                            if ((long long)(val < 0 ? -val : val) * qt[z] > OM_JPEG_COEF_BOUND) beyond = true;
                        }
                    }
            }
            if (until_rst > 0) --until_rst;
        }
    }
    (void)mcus;
    // what follows the last MCU is the end of the image: a second scan or anything else is not this stream's format
    {
        const uint8_t* p = b.p;
        if (p >= b.end || *p != 0xFF) JP_FAIL("jpeg: no EOI marker behind the scan");
        while (p < b.end && *p == 0xFF) ++p;
        if (p >= b.end) JP_FAIL("jpeg: truncated in front of the EOI marker");
        if (*p == 0xDA || *p == 0xC4 || *p == 0xDB || *p == 0xDC) {
            info[OM_JPEG_I_SUPPORTED] = 0;
            info[OM_JPEG_I_REASON] = *p == 0xDC ? OM_JPEG_R_DNL : OM_JPEG_R_SCANS;
            return OM_OK;
        }
        if (*p != 0xD9) JP_FAIL("jpeg: marker 0x%02x behind the scan where EOI is due", *p);
    }
    if (beyond) {
        info[OM_JPEG_I_SUPPORTED] = 0;
        info[OM_JPEG_I_REASON] = OM_JPEG_R_RANGE;
    }
    return OM_OK;
}

}  // extern "C"
