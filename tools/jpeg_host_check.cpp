// Stand-alone memory-safety check of the JPEG host entries (orienmask_amd/csrc/om_jpeg.cpp), CPU only:
//
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//         tools/jpeg_host_check.cpp orienmask_amd/csrc/om_jpeg.cpp -o jpeg_host_check
//     ./jpeg_host_check STREAMS.bin [prefix streams] [corruptions per stream]
//
// STREAMS.bin (tests/test_jpeg_cpu.py writes it from tests/golden/jpeg_cases.npz): uint32 n, then n times uint32 length + bytes.
// Every stream, every prefix of the first `prefix streams` of them, and a fixed, seeded set of single-byte corruptions of each
// go through om_jpeg_info and om_jpeg_entropy_decode.  Every input is copied into a heap block of exactly its length and the
// coefficient buffer has exactly the size om_jpeg_info asked for, so that the sanitizer sees a read or a write one byte out.
// Whatever the entries answer is fine -- supported, unsupported or rejected; the two must agree on the geometry, a rejected
// stream must leave a message, and the program must exit clean.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orienmask_hip.h"

namespace om {
static char g_err[512] = "";
void set_error(const char* fmt, ...) {        // the library's own lives in om_model.cpp, behind the HIP headers
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace om

static long n_supported = 0, n_unsupported = 0, n_rejected = 0;

static int run_one(const uint8_t* data, size_t len) {
    uint8_t* in = static_cast<uint8_t*>(malloc(len ? len : 1));      // exactly len bytes are the stream
    if (len) memcpy(in, data, len);
    int32_t info[OM_JPEG_INFO_WORDS], info2[OM_JPEG_INFO_WORDS];
    om::g_err[0] = 0;
    int rc = om_jpeg_info(len ? in : in, len, info);
    int bad = 0;
    if (rc != OM_OK) {
        if (!om::g_err[0]) { fprintf(stderr, "a rejected stream left no message\n"); bad = 1; }
        ++n_rejected;
        // the decoder must reject it as well, without writing anything
        int16_t one[1];
        uint16_t quant[3 * 64];
        if (om_jpeg_entropy_decode(in, len, one, 0, quant, info2) == OM_OK) { fprintf(stderr, "info rejects, decode accepts\n"); bad = 1; }
        free(in);
        return bad;
    }
    const size_t cap = info[OM_JPEG_I_SUPPORTED] ? (size_t)info[OM_JPEG_I_BLOCKS] * 128 : 0;
    if (cap > ((size_t)64 << 20)) {      // a corrupted size field: the stream would be truncated anyway, the buffer is not worth it
        free(in);
        return 0;
    }
    int16_t* coef = static_cast<int16_t*>(malloc(cap ? cap : 1));
    uint16_t* quant = static_cast<uint16_t*>(malloc(3 * 64 * sizeof(uint16_t)));
    om::g_err[0] = 0;
    rc = om_jpeg_entropy_decode(in, len, coef, cap, quant, info2);
    if (rc != OM_OK) {
        if (!om::g_err[0]) { fprintf(stderr, "a rejected stream left no message\n"); bad = 1; }
        ++n_rejected;
    } else {
        if (memcmp(info, info2, sizeof(int32_t) * 3) != 0) { fprintf(stderr, "the two entries disagree on the geometry\n"); bad = 1; }
        if (info2[OM_JPEG_I_SUPPORTED]) {
            ++n_supported;
            long long sum = 0;                                        // every coefficient was written: read them all
            for (size_t k = 0; k < cap / 2; ++k) sum += coef[k];
            for (int k = 0; k < 64 * info2[OM_JPEG_I_NCOMP]; ++k) sum += quant[k];
            if (sum == 0x7fffffffffffffffll) bad = 1;
            if (cap > 128) {                                          // a buffer one block short is refused, not overrun
                int16_t* small = static_cast<int16_t*>(malloc(cap - 128));
                if (om_jpeg_entropy_decode(in, len, small, cap - 128, quant, info2) != OM_ENOMEM) { fprintf(stderr, "short buffer not refused\n"); bad = 1; }
                free(small);
            }
        } else {
            ++n_unsupported;
        }
    }
    free(coef);
    free(quant);
    free(in);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s STREAMS.bin [prefix streams] [corruptions per stream]\n", argv[0]);
        return 2;
    }
    const int n_prefix = argc > 2 ? atoi(argv[2]) : 4;
    const int n_corrupt = argc > 3 ? atoi(argv[3]) : 64;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    std::vector<std::vector<uint8_t>> streams(n);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1) return 2;
        streams[i].resize(len);
        if (len && fread(streams[i].data(), 1, len, f) != len) return 2;
    }
    fclose(f);
    int bad = 0;
    long calls = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const std::vector<uint8_t>& s = streams[i];
        bad |= run_one(s.data(), s.size());
        ++calls;
        if ((int)i < n_prefix)
            for (size_t k = 0; k < s.size(); ++k, ++calls) bad |= run_one(s.data(), k);
        uint64_t state = 0x9E3779B97F4A7C15ull * (i + 1);             // splitmix64: the same corruptions on every run
        std::vector<uint8_t> c(s);
        for (int k = 0; k < n_corrupt && !s.empty(); ++k, ++calls) {
            state += 0x9E3779B97F4A7C15ull;
            uint64_t z = state;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            const size_t at = (size_t)(z % s.size());
            const uint8_t old = c[at];
            c[at] = (uint8_t)(z >> 32);
            bad |= run_one(c.data(), c.size());
            c[at] = old;
        }
    }
    printf("jpeg_host_check: %ld calls over %u streams: %ld supported, %ld unsupported, %ld rejected%s\n", calls, n, n_supported,
           n_unsupported, n_rejected, bad ? " -- FAILED" : "");
    return bad;
}
