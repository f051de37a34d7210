// Device side of the JPEG decoder (include/orienmask_hip.h: om_jpeg_decode_batch): what libjpeg does behind its entropy decoder,
// in its integer arithmetic, bit for bit -- the pin is PIL's Image.open(...).convert('RGB') (libjpeg-turbo, ISLOW IDCT, fancy
// up-sampling), tests/golden/jpeg_cases.npz.  The host (om_jpeg.cpp) has undone the Huffman coding; nothing here is serial.
//
// Two kernels per launch set of up to OM_JPEG_BATCH images, blockIdx.y = the image, its table entry read with scalar loads:
//
//   jpeg_idct_kernel    dequantise, 8x8 accurate-integer IDCT, +128, clamp: the component planes of WHOLE blocks, in the workspace.
//     Eight lanes own a block, 32 blocks per workgroup.  Lane r loads row r of the coefficients and of the quantisation table
//     as 16 bytes each (a block is 128 contiguous bytes: a wave reads 1 KiB per instruction), multiplies and puts the row into
//     LDS; lane c then transforms column c in place (pass 1), lane r row r (pass 2) and stores its 8 samples as 8 bytes.  The
//     block's 8x8 int32 tile has a row pitch of 9 words and a block pitch of 72: in every one of the three phases the lanes
//     of a 32-lane half (4 blocks x 8 lanes) touch 32 different banks -- (8 b + 9 r + e) and (8 b + 9 k + c) mod 32.
//   jpeg_color_kernel   chroma up-sampling to luma resolution ("fancy": triangle filter), YCbCr -> RGB, clamp: the h x w pixels
//     of the image and nothing else.  A lane owns 4 consecutive pixels of the DENSE output, 12 bytes that it stores as three
//     words (rows are not padded, so the four may straddle a row end: each pixel finds its own row and column).  The up-sampled
//     chroma is recomputed from the up to 2 x 2 chroma samples around the pixel rather than staged: the planes were written a
//     moment ago and are read through the caches.
//
// Why two kernels and not one: a fused form needs the chroma blocks around a luma block before it can write a pixel -- a halo
// of one sample in each direction, that is the neighbouring 8x8 blocks' IDCTs again, or a workgroup per MCU row with the row
// above and below.  The planes cost 1.5 bytes written and 1.5 read per pixel of a 4:2:0 image next to the 3 read as coefficients
// and the 3 written as RGB; both kernels are memory-bound and the intermediate is in the Infinity Cache for any batch the
// inference loop uses.
//
// int32 is enough: the host refuses a stream with a |coefficient * quantiser| beyond OM_JPEG_COEF_BOUND (om_jpeg.cpp).
#include "om_common.h"

namespace om {

struct JpegImg {
    const int16_t* coef;     // component after component, [block][64]
    const uint16_t* quant;   // [ncomp][64], natural order
    uint8_t* plane;          // workspace: component planes of whole blocks, component c at plane_off[c], row pitch 8 * bw[c]
    uint8_t* out;            // [h,w,3]
    int w, h, ncomp, hmax, vmax;
    int bw[3], bh[3];        // blocks per row, block rows
    int blk_end[3];          // blocks of components 0..c
    int plane_off[3];
};

struct JpegBatch {
    JpegImg img[OM_JPEG_BATCH];
};

constexpr int JPEG_BLOCKS_PER_WG = 32;
constexpr int JPEG_ROW_PITCH = 9, JPEG_BLOCK_PITCH = 72;

// The 13-bit constants of the accurate-integer IDCT
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
              F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// One 1-D pass over x[0..7] in place: SHIFT = 11 for the columns (pass 1), 18 for the rows (pass 2); rounding add 1 << (SHIFT - 1)
template <int SHIFT>
__device__ __forceinline__ void idct_1d(int x[8]) {
    int z2 = x[2], z3 = x[6];
    int z1 = (z2 + z3) * F_0_541;
    int tmp2 = z1 + z3 * (-F_1_847);
    int tmp3 = z1 + z2 * F_0_765;
    z2 = x[0]; z3 = x[4];
    int tmp0 = (z2 + z3) * 8192;
    int tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175;
    tmp0 *= F_0_298; tmp1 *= F_2_053; tmp2 *= F_3_072; tmp3 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562; z3 *= -F_1_961; z4 *= -F_0_390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    x[0] = (tmp10 + tmp3 + R) >> SHIFT; x[7] = (tmp10 - tmp3 + R) >> SHIFT;
    x[1] = (tmp11 + tmp2 + R) >> SHIFT; x[6] = (tmp11 - tmp2 + R) >> SHIFT;
    x[2] = (tmp12 + tmp1 + R) >> SHIFT; x[5] = (tmp12 - tmp1 + R) >> SHIFT;
    x[3] = (tmp13 + tmp0 + R) >> SHIFT; x[4] = (tmp13 - tmp0 + R) >> SHIFT;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegBatch bt) {
    __shared__ int tile[JPEG_BLOCKS_PER_WG * JPEG_BLOCK_PITCH];
    const JpegImg& q = bt.img[blockIdx.y];
    const int g = (int)threadIdx.x >> 3, r = (int)threadIdx.x & 7;
    const int blk = (int)blockIdx.x * JPEG_BLOCKS_PER_WG + g;
    const int total = q.blk_end[q.ncomp - 1];
    const bool active = blk < total;                  // no lane leaves before the last barrier
    int* t = tile + g * JPEG_BLOCK_PITCH;
    int c = 0, local = blk;
    if (active) {
        if (q.ncomp == 3 && blk >= q.blk_end[0]) {
            c = blk >= q.blk_end[1] ? 2 : 1;
            local = blk - q.blk_end[c - 1];
        }
        const int4 cv = *reinterpret_cast<const int4*>(q.coef + (size_t)blk * 64 + r * 8);
        const int4 qv = *reinterpret_cast<const int4*>(q.quant + c * 64 + r * 8);
        const int cw[4] = {cv.x, cv.y, cv.z, cv.w};
        const unsigned qw[4] = {(unsigned)qv.x, (unsigned)qv.y, (unsigned)qv.z, (unsigned)qv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            t[r * JPEG_ROW_PITCH + 2 * e] = (int)(short)(cw[e] & 0xffff) * (int)(qw[e] & 0xffffu);
            t[r * JPEG_ROW_PITCH + 2 * e + 1] = (cw[e] >> 16) * (int)(qw[e] >> 16);
        }
    }
    __syncthreads();
    int x[8];
    if (active) {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = t[k * JPEG_ROW_PITCH + r];
        idct_1d<11>(x);
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k * JPEG_ROW_PITCH + r] = x[k];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = t[r * JPEG_ROW_PITCH + e];
        idct_1d<18>(x);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo |= (unsigned)clamp255(x[e] + 128) << (8 * e);
            hi |= (unsigned)clamp255(x[e + 4] + 128) << (8 * e);
        }
        const int by = local / q.bw[c], bx = local - by * q.bw[c];
        uint8_t* dst = q.plane + q.plane_off[c] + (size_t)(by * 8 + r) * (size_t)(q.bw[c] * 8) + (size_t)bx * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

// the chroma sample of plane p (row pitch `pitch`, real size cw x ch) at luma position (y, x), 2:1 horizontally
__device__ __forceinline__ int chroma_h2v1(const uint8_t* p, int pitch, int cw, int y, int x) {
    const uint8_t* row = p + (size_t)y * pitch;
    const int i = x >> 1;
    const int v = row[i];
    if (cw <= 2) return v;                                // libjpeg replicates a plane this narrow
    if (x & 1) return i == cw - 1 ? v : (3 * v + row[i + 1] + 2) >> 2;
    return i == 0 ? v : (3 * v + row[i - 1] + 1) >> 2;
}

// ... and 2:1 in both directions: the far row is the one above for an even luma row, below for an odd one, the edge row itself
// at the top and at the bottom of the REAL plane
__device__ __forceinline__ int chroma_h2v2(const uint8_t* p, int pitch, int cw, int ch, int y, int x) {
    const int j = y >> 1, i = x >> 1;
    const uint8_t* near = p + (size_t)j * pitch;
    if (cw <= 2) return near[i];                          // replicated in both directions
    const int jf = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    const uint8_t* far = p + (size_t)jf * pitch;
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__device__ __forceinline__ void jpeg_pixel(const JpegImg& q, int y, int x, int& R, int& G, int& B) {
    const int Y = q.plane[(size_t)y * (size_t)(q.bw[0] * 8) + x];
    if (q.ncomp == 1) {
        R = G = B = Y;
        return;
    }
    const uint8_t* pb = q.plane + q.plane_off[1];
    const uint8_t* pr = q.plane + q.plane_off[2];
    const int pitch = q.bw[1] * 8;
    int cb, cr;
    if (q.hmax == 1) {
        cb = pb[(size_t)y * pitch + x];
        cr = pr[(size_t)y * pitch + x];
    } else {
        const int cw = (q.w + 1) >> 1;
        if (q.vmax == 1) {
            cb = chroma_h2v1(pb, pitch, cw, y, x);
            cr = chroma_h2v1(pr, pitch, cw, y, x);
        } else {
            const int ch = (q.h + 1) >> 1;
            cb = chroma_h2v2(pb, pitch, cw, ch, y, x);
            cr = chroma_h2v2(pr, pitch, cw, ch, y, x);
        }
    }
    cb -= 128; cr -= 128;
    R = clamp255(Y + ((91881 * cr + 32768) >> 16));
    G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    B = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const JpegBatch bt) {
    const JpegImg& q = bt.img[blockIdx.y];
    const int pixels = q.w * q.h;                                        // < 2^31 / 3 (the entry)
    const int p0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    if (p0 >= pixels) return;
    int y = p0 / q.w, x = p0 - y * q.w;
    const int n = pixels - p0 < 4 ? pixels - p0 : 4;
    uint8_t v[12];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int R = 0, G = 0, B = 0;
        if (e < n) {
            jpeg_pixel(q, y, x, R, G, B);
            if (++x == q.w) { x = 0; ++y; }
        }
        v[3 * e] = (uint8_t)R; v[3 * e + 1] = (uint8_t)G; v[3 * e + 2] = (uint8_t)B;
    }
    uint8_t* o = q.out + (size_t)p0 * 3;                                  // 12-byte steps from a 16-byte aligned image
    if (n == 4) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)v[4 * k] | ((uint32_t)v[4 * k + 1] << 8) | ((uint32_t)v[4 * k + 2] << 16) | ((uint32_t)v[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) o[k] = v[k];
    }
}

// One row of the table, checked; *plane_bytes = the workspace bytes of its component planes (a multiple of 16)
static int jpeg_row(const char* who, const int64_t* d, int i, JpegImg* q, size_t* plane_bytes) {
    const int64_t w = d[0], h = d[1], nc = d[2], hmax = d[3], vmax = d[4];
    OM_REQUIRE(w > 0 && h > 0 && w < 65536 && h < 65536 && w * h * 3 < (1ll << 31), OM_EINVAL, "%s: image %d: size %lldx%lld", who, i,
               (long long)w, (long long)h);
    OM_REQUIRE((nc == 1 && hmax == 1 && vmax == 1) || (nc == 3 && ((hmax == 1 && vmax == 1) || (hmax == 2 && (vmax == 1 || vmax == 2)))),
               OM_EINVAL, "%s: image %d: %lld components with luma sampling %lldx%lld are not decoded here", who, i, (long long)nc,
               (long long)hmax, (long long)vmax);
    OM_REQUIRE(d[5] >= 0 && d[5] % 64 == 0 && d[6] >= 0 && d[6] % 64 == 0 && d[7] >= 0 && d[7] % 16 == 0, OM_EINVAL,
               "%s: image %d: offsets %lld (coef), %lld (quant), %lld (out) must be multiples of 64, 64 and 16", who, i, (long long)d[5],
               (long long)d[6], (long long)d[7]);
    const int mx = (int)((w + 8 * hmax - 1) / (8 * hmax)), my = (int)((h + 8 * vmax - 1) / (8 * vmax));
    q->w = (int)w; q->h = (int)h; q->ncomp = (int)nc; q->hmax = (int)hmax; q->vmax = (int)vmax;
    int blocks = 0;
    for (int c = 0; c < 3; ++c) {
        const int ch = c == 0 ? (int)hmax : 1, cv = c == 0 ? (int)vmax : 1;
        q->bw[c] = c < nc ? mx * ch : 0;
        q->bh[c] = c < nc ? my * cv : 0;
        q->plane_off[c] = blocks * 64;
        blocks += q->bw[c] * q->bh[c];
        q->blk_end[c] = blocks;
    }
    *plane_bytes = align_up((size_t)blocks * 64, 16);
    return OM_OK;
}

}  // namespace om

extern "C" {

size_t om_jpeg_workspace_bytes(const int64_t* desc, int n) {
    if (!desc || n <= 0) {
        om::set_error("om_jpeg_workspace_bytes: null table or n = %d", n);
        return 0;
    }
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        om::JpegImg q;
        size_t bytes;
        if (om::jpeg_row("om_jpeg_workspace_bytes", desc + (size_t)OM_JPEG_DESC_WORDS * i, i, &q, &bytes) != OM_OK) return 0;
        total += bytes;
    }
    return total;
}

int om_jpeg_decode_batch(const int64_t* desc, int n, const int16_t* coef, size_t coef_elems, const uint16_t* quant,
                         size_t quant_elems, void* workspace, size_t ws_bytes, uint8_t* out, size_t out_bytes, om_stream stream) {
    OM_REQUIRE(desc && coef && quant && workspace && out, OM_EINVAL, "om_jpeg_decode_batch: null argument");
    OM_REQUIRE(n > 0, OM_EINVAL, "om_jpeg_decode_batch: n = %d images", n);
    OM_REQUIRE((reinterpret_cast<uintptr_t>(coef) | reinterpret_cast<uintptr_t>(quant) | reinterpret_cast<uintptr_t>(workspace) |
                reinterpret_cast<uintptr_t>(out)) % 16 == 0, OM_EINVAL, "om_jpeg_decode_batch: coef, quant, workspace and out must be 16-byte aligned");
    size_t ws_off = 0;
    for (int pass = 0; pass < 2; ++pass) {                    // every row before the first launch: a refused call writes nothing
        ws_off = 0;
        for (int i0 = 0; i0 < n; i0 += OM_JPEG_BATCH) {
            om::JpegBatch bt;
            const int cnt = n - i0 < OM_JPEG_BATCH ? n - i0 : OM_JPEG_BATCH;
            int max_blocks = 0, max_quads = 0;
            for (int k = 0; k < OM_JPEG_BATCH; ++k) {
                if (k >= cnt) { bt.img[k] = bt.img[0]; continue; }      // the unused entries repeat the first: no workgroup reads them
                const int i = i0 + k;
                const int64_t* d = desc + (size_t)OM_JPEG_DESC_WORDS * i;
                om::JpegImg& q = bt.img[k];
                size_t bytes;
                const int rc = om::jpeg_row("om_jpeg_decode_batch", d, i, &q, &bytes);
                if (rc != OM_OK) return rc;
                const size_t blocks = (size_t)q.blk_end[2];
                OM_REQUIRE((size_t)d[5] <= coef_elems && blocks * 64 <= coef_elems - (size_t)d[5], OM_EINVAL,
                           "om_jpeg_decode_batch: image %d: %zu coefficients at %lld do not fit coef (%zu)", i, blocks * 64, (long long)d[5], coef_elems);
                OM_REQUIRE((size_t)d[6] <= quant_elems && (size_t)q.ncomp * 64 <= quant_elems - (size_t)d[6], OM_EINVAL,
                           "om_jpeg_decode_batch: image %d: the tables at %lld do not fit quant (%zu)", i, (long long)d[6], quant_elems);
                const size_t rgb = (size_t)q.w * q.h * 3;
                OM_REQUIRE((size_t)d[7] <= out_bytes && rgb <= out_bytes - (size_t)d[7], OM_EINVAL,
                           "om_jpeg_decode_batch: image %d: %zu bytes at %lld do not fit out (%zu)", i, rgb, (long long)d[7], out_bytes);
                OM_REQUIRE(bytes <= ws_bytes && ws_off <= ws_bytes - bytes, OM_ENOMEM,
                           "om_jpeg_decode_batch: workspace of %zu bytes, image %d needs %zu at %zu", ws_bytes, i, bytes, ws_off);
                q.coef = coef + d[5];
                q.quant = quant + d[6];
                q.out = out + d[7];
                q.plane = static_cast<uint8_t*>(workspace) + ws_off;
                ws_off += bytes;
                const int quads = (q.w * q.h + 3) / 4;
                max_blocks = (int)blocks > max_blocks ? (int)blocks : max_blocks;
                max_quads = quads > max_quads ? quads : max_quads;
            }
            if (pass == 0) continue;
            hipLaunchKernelGGL(om::jpeg_idct_kernel, dim3((unsigned)((max_blocks + om::JPEG_BLOCKS_PER_WG - 1) / om::JPEG_BLOCKS_PER_WG),
                                                          (unsigned)cnt), dim3(256), 0, static_cast<hipStream_t>(stream), bt);
            OM_CHECK_HIP(hipGetLastError());
            hipLaunchKernelGGL(om::jpeg_color_kernel, dim3((unsigned)((max_quads + 255) / 256), (unsigned)cnt), dim3(256), 0,
                               static_cast<hipStream_t>(stream), bt);
            OM_CHECK_HIP(hipGetLastError());
        }
    }
    return OM_OK;
}

}  // extern "C"
