// InferenceVisualizer's device part (reference utils/visualizer.py:33-127): for each image, the kept masks cropped, resized to
// the original image, sorted by resized area and alpha-composited over the image, rounded to uint8 -- in one pass over the
// output, never materialising the reference's [K,h,w,3] colour masks or [K,h,w] cumulative product.
//
//   vis_mask_stats_kernel   one workgroup per kept mask: its resized area (separable form, see below) and the output rectangle
//                           outside which its resized value is exactly 0
//   vis_composite_kernel    one workgroup per 1024 consecutive output pixels (HWC order): ranks the image's masks by area,
//                           keeps those whose rectangle meets the tile, then per pixel samples them in rank order
//
// Numerics (what torch-CPU does in plot_all_mask, visualizer.py:95-100), per pixel and channel with m[k] the resized mask
// values in ascending-area order and a = float32(alpha):
//   cm[k]  = (m[k] * c[k]) * a                             float32
//   t[k]   = 1 - a * m[k]                                  float32
//   A[k]   = float(t[0] * ... * t[k])                      the product in DOUBLE, rounded once (torch's cumprod)
//   out    = ((img * A[K-1]) + cm[0]) + sum_{k>=1} cm[k] * A[k-1]     the sum in float32, sequentially
// A mask whose value is 0 at a pixel multiplies by exactly 1 and adds exactly +0, so skipping it is exact; torch's own sum
// over k uses several accumulators once K is large, which is the only difference from the reference (a few ulp).
//
// Built with -ffp-contract=off: the resize is bilinear.h's, bit-identical to coco_format.hip and to torch-CPU.
#include "om_common.h"
#include "bilinear.h"

namespace om {

constexpr int VIS_THREADS = 256;
constexpr int VIS_PIX_PER_THREAD = 4;                       // 4 HWC pixels = 12 bytes = 3 dwords of output per lane
constexpr int VIS_TILE = VIS_THREADS * VIS_PIX_PER_THREAD;  // pixels per workgroup
constexpr int VIS_MAX_SRC = 4096;                           // cropped mask rows / columns the pre-pass can weigh
constexpr int VIS_FIRST = 1 << 30;                          // list entry flag: the smallest mask (cm[0] enters unweighted)

struct VisMaskStat {                                        // 32 bytes per kept mask in the workspace
    double area;
    int y_lo, y_hi, x_lo, x_hi;                             // output rectangle of possibly nonzero values (empty: lo > hi)
    int pad[2];
};

struct VisImg {
    const float* image;
    uint8_t* out;
    float* out_float;
    const uint8_t* mask;
    const int32_t* keep;
    const float* colors;
    const int32_t* boxes;
    int n, H, W;
    int crop_top, crop_left, ch, cw;                        // cropped region of the network-size mask
    int h, w;
    int with_mask, draw_boxes;
    float alpha, scale_h, scale_w;
};

struct VisBatch {
    VisImg img[OM_VIS_BATCH];
    int mask_first[OM_VIS_BATCH + 1];                       // the image's first entry in the workspace's stats
    int tile_first[OM_VIS_BATCH + 1];                       // the image's first composite workgroup
    int n;
};

// ---- pre-pass: area and extent of one kept mask -------------------------------------------------------------------------
// The area the reference sorts by is sum_{y,x} v(y,x) with v the bilinear value; v is a weighted sum of source pixels, so the
// sum is sum_{i,j} M[i,j] * Ry[i] * Rx[j], Ry[i] (Rx[j]) being the total weight source row i (column j) receives over all
// output rows (columns).  Accumulated in double; the sort key only has to order masks whose areas differ by far more than
// float32 rounding (ties, which torch's unstable argsort leaves open, go to the lower kept index).
__global__ __launch_bounds__(VIS_THREADS) void vis_mask_stats_kernel(const VisBatch bt, VisMaskStat* stats) {
    __shared__ float s_ry[VIS_MAX_SRC], s_rx[VIS_MAX_SRC];
    __shared__ double s_sum[VIS_THREADS / 64];
    __shared__ int s_ext[8];                                // i_lo, i_hi, j_lo, j_hi (source), y_lo, y_hi, x_lo, x_hi (output)
    int im = 0;
    while (im + 1 < bt.n && (int)blockIdx.x >= bt.mask_first[im + 1]) ++im;
    const VisImg& q = bt.img[im];
    const int k = blockIdx.x - bt.mask_first[im], tid = threadIdx.x;
    if (tid < 8) s_ext[tid] = (tid & 1) ? -1 : 0x7fffffff;
    // Total weight of source row i: the output rows whose taps can reach i lie in a short window around its preimage (the tap's
    // source coordinate is scale * (y + 0.5) - 0.5, clamped); each is evaluated exactly and summed in y order (deterministic).
    auto weight = [](int i, float scale, int n_in, int n_out) -> float {
        const float inv = 1.0f / scale;
        int y_lo = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 2;
        int y_hi = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 2;
        y_lo = y_lo < 0 ? 0 : y_lo;
        y_hi = (i == n_in - 1 || y_hi > n_out - 1) ? n_out - 1 : y_hi;
        if (i == 0) y_lo = 0;
        float s = 0.f;
        for (int y = y_lo; y <= y_hi; ++y) {
            int i0, i1;
            float w0, w1;
            tap(y, scale, n_in, i0, i1, w0, w1);
            if (i0 == i) s += w0;
            if (i1 == i) s += w1;
        }
        return s;
    };
    for (int i = tid; i < q.ch; i += VIS_THREADS) s_ry[i] = weight(i, q.scale_h, q.ch, q.h);
    for (int j = tid; j < q.cw; j += VIS_THREADS) s_rx[j] = weight(j, q.scale_w, q.cw, q.w);
    __syncthreads();
    // the source pixels: the cropped rows as one byte range, 16 aligned bytes per lane and load (an aligned 16-byte block that
    // holds a byte of the range lies in that byte's page; bytes outside the range or the crop's columns are skipped)
    const int lane = tid & 63, wave = tid >> 6;
    const uint8_t* plane = q.mask + (size_t)q.keep[k] * q.H * q.W;
    const int lo = q.crop_top * q.W, hi = (q.crop_top + q.ch) * q.W;
    const uintptr_t base = reinterpret_cast<uintptr_t>(plane + lo) & ~(uintptr_t)15;
    const int n_chunks = (int)((reinterpret_cast<uintptr_t>(plane + hi) - base + 15) / 16);
    const int head = (int)(reinterpret_cast<uintptr_t>(plane) - base);     // plane offset of chunk c: 16 c - head
    double acc = 0.0;
    int i_lo = 0x7fffffff, i_hi = -1, j_lo = 0x7fffffff, j_hi = -1;
    for (int c = tid; c < n_chunks; c += VIS_THREADS) {
        const uint4 v = reinterpret_cast<const uint4*>(base)[c];
        if ((v.x | v.y | v.z | v.w) == 0u) continue;
        const uint32_t words[4] = {v.x, v.y, v.z, v.w};
        const int off0 = 16 * c - head;
        int i = (off0 >= 0 ? off0 : off0 - q.W + 1) / q.W;          // floor division: the first chunk may start before the plane
        int j = off0 - i * q.W;
        float part = 0.f;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int off = off0 + b;
            const int ii = i - q.crop_top, jj = j - q.crop_left;
            if (((words[b >> 2] >> (8 * (b & 3))) & 0xffu) && off >= lo && off < hi && jj >= 0 && jj < q.cw) {
                part += s_ry[ii] * s_rx[jj];
                i_lo = min(i_lo, ii); i_hi = max(i_hi, ii);
                j_lo = min(j_lo, jj); j_hi = max(j_hi, jj);
            }
            if (++j == q.W) { j = 0; ++i; }
        }
        acc += (double)part;
    }
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) s_sum[wave] = acc;
    if (i_hi >= 0) {
        atomicMin(&s_ext[0], i_lo); atomicMax(&s_ext[1], i_hi);
        atomicMin(&s_ext[2], j_lo); atomicMax(&s_ext[3], j_hi);
    }
    __syncthreads();
    // output rows / columns whose taps reach the nonzero source rectangle (taps are monotone in the output index: a range)
    const int si_lo = s_ext[0], si_hi = s_ext[1], sj_lo = s_ext[2], sj_hi = s_ext[3];
    if (si_hi >= 0) {
        for (int y = tid; y < q.h; y += VIS_THREADS) {
            int i0, i1;
            float w0, w1;
            tap(y, q.scale_h, q.ch, i0, i1, w0, w1);
            if (i1 >= si_lo && i0 <= si_hi) { atomicMin(&s_ext[4], y); atomicMax(&s_ext[5], y); }
        }
        for (int x = tid; x < q.w; x += VIS_THREADS) {
            int j0, j1;
            float w0, w1;
            tap(x, q.scale_w, q.cw, j0, j1, w0, w1);
            if (j1 >= sj_lo && j0 <= sj_hi) { atomicMin(&s_ext[6], x); atomicMax(&s_ext[7], x); }
        }
    }
    __syncthreads();
    if (tid == 0) {
        VisMaskStat st;
        st.area = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        st.y_lo = s_ext[4]; st.y_hi = s_ext[5]; st.x_lo = s_ext[6]; st.x_hi = s_ext[7];
        st.pad[0] = st.pad[1] = 0;
        stats[bt.mask_first[im] + k] = st;
    }
}

// ---- the composite -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t to_u8(float v) {        // round() half to even, then uint8 (values are within [0, 255])
    v = rintf(v);
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    return (uint32_t)v;
}

__global__ __launch_bounds__(VIS_THREADS) void vis_composite_kernel(const VisBatch bt, const VisMaskStat* stats) {
    __shared__ double s_area[OM_VIS_MAX_KEPT];
    __shared__ int s_sorted[OM_VIS_MAX_KEPT];               // kept index of rank r
    __shared__ int s_list[OM_VIS_MAX_KEPT];                 // masks meeting the tile, in rank order (| VIS_FIRST for rank 0)
    __shared__ int4 s_lext[OM_VIS_MAX_KEPT];                // their output rectangles
    __shared__ int s_blist[OM_VIS_MAX_KEPT];                // boxes meeting the tile, in kept order
    __shared__ int s_count[2];
    int im = 0;
    while (im + 1 < bt.n && (int)blockIdx.x >= bt.tile_first[im + 1]) ++im;
    const VisImg& q = bt.img[im];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long hw = (long long)q.h * q.w;
    const long long t0 = (long long)(blockIdx.x - bt.tile_first[im]) * VIS_TILE;
    const long long t1 = min(hw, t0 + VIS_TILE) - 1;
    // the tile's bounding rectangle
    const int ty0 = (int)(t0 / q.w), ty1 = (int)(t1 / q.w);
    const int tx0 = ty0 == ty1 ? (int)(t0 - (long long)ty0 * q.w) : 0;
    const int tx1 = ty0 == ty1 ? (int)(t1 - (long long)ty1 * q.w) : q.w - 1;
    const bool masks = q.with_mask && q.n > 0;
    const int n = q.n;
    if (masks) {
        const VisMaskStat* st = stats + bt.mask_first[im];
        for (int k = tid; k < n; k += VIS_THREADS) s_area[k] = st[k].area;
        __syncthreads();
        for (int k = tid; k < n; k += VIS_THREADS) {        // rank = number of masks before k in (area, kept index) order
            const double a = s_area[k];
            int r = 0;
            for (int j = 0; j < n; ++j) {
                const double b = s_area[j];
                r += (b < a || (b == a && j < k)) ? 1 : 0;
            }
            s_sorted[r] = k;
        }
        __syncthreads();
        if (wave == 0) {                                    // compact the masks meeting the tile, keeping rank order
            int cnt = 0;
            for (int r0 = 0; r0 < n; r0 += 64) {
                const int r = r0 + lane;
                bool take = false;
                int4 e = make_int4(0, -1, 0, -1);
                int k = 0;
                if (r < n) {
                    k = s_sorted[r];
                    const VisMaskStat& s = st[k];
                    e = make_int4(s.y_lo, s.y_hi, s.x_lo, s.x_hi);
                    take = e.x <= ty1 && e.y >= ty0 && e.z <= tx1 && e.w >= tx0;
                }
                const unsigned long long b = __ballot(take);
                if (take) {
                    const int slot = cnt + __popcll(b & ((1ull << lane) - 1ull));
                    s_list[slot] = k | (r == 0 ? VIS_FIRST : 0);
                    s_lext[slot] = e;
                }
                cnt += __popcll(b);
            }
            if (lane == 0) s_count[0] = cnt;
        }
    }
    if (q.draw_boxes && n > 0 && wave == 1) {               // boxes whose outline may meet the tile, in kept order
        int cnt = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            bool take = false;
            if (k < n) {
                const int4 b = reinterpret_cast<const int4*>(q.boxes)[k];
                const int xa = min(b.x, b.z), xb = max(b.x, b.z), ya = min(b.y, b.w), yb = max(b.y, b.w);
                take = ya <= ty1 && yb >= ty0 && xa <= tx1 && xb >= tx0;
            }
            const unsigned long long bal = __ballot(take);
            if (take) s_blist[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = k;
            cnt += __popcll(bal);
        }
        if (lane == 0) s_count[1] = cnt;
    }
    __syncthreads();
    const int n_list = masks ? s_count[0] : 0;
    const int n_box = (q.draw_boxes && n > 0) ? s_count[1] : 0;

    const long long p0 = t0 + (long long)tid * VIS_PIX_PER_THREAD;
    if (p0 >= hw) return;
    const bool whole = p0 + VIS_PIX_PER_THREAD <= hw;
    float img[VIS_PIX_PER_THREAD][3];
    if (whole) {                                            // 48 contiguous, 16-byte aligned bytes per lane
        const float4* src = reinterpret_cast<const float4*>(q.image + p0 * 3);
        const float4 a = src[0], b = src[1], c = src[2];
        img[0][0] = a.x; img[0][1] = a.y; img[0][2] = a.z; img[1][0] = a.w;
        img[1][1] = b.x; img[1][2] = b.y; img[2][0] = b.z; img[2][1] = b.w;
        img[2][2] = c.x; img[3][0] = c.y; img[3][1] = c.z; img[3][2] = c.w;
    } else {
        for (int e = 0; e < VIS_PIX_PER_THREAD; ++e)
            for (int c = 0; c < 3; ++c) img[e][c] = p0 + e < hw ? q.image[(p0 + e) * 3 + c] : 0.f;
    }
    int py[VIS_PIX_PER_THREAD], px[VIS_PIX_PER_THREAD];
    for (int e = 0; e < VIS_PIX_PER_THREAD; ++e) {
        const long long p = min(p0 + e, hw - 1);
        py[e] = (int)(p / q.w);
        px[e] = (int)(p - (long long)py[e] * q.w);
    }
    float res[VIS_PIX_PER_THREAD][3];
    if (n_list > 0) {
        int r0[VIS_PIX_PER_THREAD], r1[VIS_PIX_PER_THREAD], c0[VIS_PIX_PER_THREAD], c1[VIS_PIX_PER_THREAD];
        float wy0[VIS_PIX_PER_THREAD], wy1[VIS_PIX_PER_THREAD], wx0[VIS_PIX_PER_THREAD], wx1[VIS_PIX_PER_THREAD];
        for (int e = 0; e < VIS_PIX_PER_THREAD; ++e) {
            int i0, i1, j0, j1;
            tap(py[e], q.scale_h, q.ch, i0, i1, wy0[e], wy1[e]);
            tap(px[e], q.scale_w, q.cw, j0, j1, wx0[e], wx1[e]);
            r0[e] = (q.crop_top + i0) * q.W + q.crop_left;
            r1[e] = (q.crop_top + i1) * q.W + q.crop_left;
            c0[e] = j0;
            c1[e] = j1;
        }
        const float alpha = q.alpha;
        const bool small = q.h + q.w <= BILINEAR_SMALL_OUT;
        double P[VIS_PIX_PER_THREAD];
        float first[VIS_PIX_PER_THREAD][3], sum[VIS_PIX_PER_THREAD][3];
        for (int e = 0; e < VIS_PIX_PER_THREAD; ++e) {
            P[e] = 1.0;
            for (int c = 0; c < 3; ++c) first[e][c] = sum[e][c] = 0.f;
        }
        const size_t plane = (size_t)q.H * q.W;
        for (int l = 0; l < n_list; ++l) {
            const int ent = __builtin_amdgcn_readfirstlane(s_list[l]);
            const int k = ent & (VIS_FIRST - 1);
            const bool is_first = (ent & VIS_FIRST) != 0;
            const int4 ext = s_lext[l];
            const uint8_t* m = q.mask + (size_t)q.keep[k] * plane;
            const float col[3] = {q.colors[3 * k], q.colors[3 * k + 1], q.colors[3 * k + 2]};
            float v[VIS_PIX_PER_THREAD];
#pragma unroll
            for (int e = 0; e < VIS_PIX_PER_THREAD; ++e) {
                v[e] = 0.f;
                if (py[e] >= ext.x && py[e] <= ext.y && px[e] >= ext.z && px[e] <= ext.w)
                    v[e] = bilinear_value(small, (float)m[r0[e] + c0[e]], (float)m[r0[e] + c1[e]], (float)m[r1[e] + c0[e]],
                                          (float)m[r1[e] + c1[e]], wx0[e], wx1[e], wy0[e], wy1[e]);
            }
#pragma unroll
            for (int e = 0; e < VIS_PIX_PER_THREAD; ++e) {
                if (v[e] == 0.f) continue;                  // x 1 and + 0: exact to skip
                const float A = (float)P[e];                // A[k-1]
                for (int c = 0; c < 3; ++c) {
                    const float cm = (v[e] * col[c]) * alpha;
                    if (is_first) first[e][c] = cm;
                    else sum[e][c] = sum[e][c] + cm * A;
                }
                P[e] = P[e] * (double)(1.0f - alpha * v[e]);
            }
        }
        for (int e = 0; e < VIS_PIX_PER_THREAD; ++e) {
            const float A = (float)P[e];                    // A[K-1]
            for (int c = 0; c < 3; ++c) {
                float o = img[e][c] * A + first[e][c];
                // plot_all_mask adds the k >= 1 terms only `if image.shape[0] > 1`, i.e. for images taller than one row
                if (q.h > 1) o = o + sum[e][c];
                res[e][c] = o;
            }
        }
    } else {
        for (int e = 0; e < VIS_PIX_PER_THREAD; ++e)
            for (int c = 0; c < 3; ++c) res[e][c] = img[e][c];
    }
    uint32_t u[VIS_PIX_PER_THREAD][3];
    for (int e = 0; e < VIS_PIX_PER_THREAD; ++e)
        for (int c = 0; c < 3; ++c) u[e][c] = to_u8(res[e][c]);
    for (int b = 0; b < n_box; ++b) {                       // outlines: the later box in kept order wins
        const int k = __builtin_amdgcn_readfirstlane(s_blist[b]);
        const int4 bx = reinterpret_cast<const int4*>(q.boxes)[k];
        const int xa = min(bx.x, bx.z), xb = max(bx.x, bx.z), ya = min(bx.y, bx.w), yb = max(bx.y, bx.w);
        const uint32_t cr = to_u8(q.colors[3 * k]), cg = to_u8(q.colors[3 * k + 1]), cb = to_u8(q.colors[3 * k + 2]);
        for (int e = 0; e < VIS_PIX_PER_THREAD; ++e) {
            const int y = py[e], x = px[e];
            const bool on = ((y == bx.y || y == bx.w) && x >= xa && x <= xb) || ((x == bx.x || x == bx.z) && y >= ya && y <= yb);
            if (on) { u[e][0] = cr; u[e][1] = cg; u[e][2] = cb; }
        }
    }
    if (q.out_float)
        for (int e = 0; e < VIS_PIX_PER_THREAD; ++e)
            if (p0 + e < hw)
                for (int c = 0; c < 3; ++c) q.out_float[(p0 + e) * 3 + c] = res[e][c];
    if (whole) {                                            // 12 bytes = 3 dwords, 4-byte aligned (p0 is a multiple of 4)
        uint32_t* dst = reinterpret_cast<uint32_t*>(q.out + p0 * 3);
        dst[0] = u[0][0] | (u[0][1] << 8) | (u[0][2] << 16) | (u[1][0] << 24);
        dst[1] = u[1][1] | (u[1][2] << 8) | (u[2][0] << 16) | (u[2][1] << 24);
        dst[2] = u[2][2] | (u[3][0] << 8) | (u[3][1] << 16) | (u[3][2] << 24);
    } else {
        for (int e = 0; e < VIS_PIX_PER_THREAD; ++e)
            if (p0 + e < hw)
                for (int c = 0; c < 3; ++c) q.out[(p0 + e) * 3 + c] = (uint8_t)u[e][c];
    }
}

}  // namespace om


extern "C" {

size_t om_visualize_workspace_bytes(const om_vis_image* images, int n_images) {
    size_t masks = 0;
    for (int i = 0; images && i < n_images; ++i)
        if (images[i].with_mask && images[i].n_keep > 0) masks += (size_t)images[i].n_keep;
    return (masks > 0 ? masks : 1) * sizeof(om::VisMaskStat);
}

int om_visualize(const om_vis_image* images, int n_images, void* workspace, size_t ws_bytes, om_stream stream) {
    if (n_images == 0) return OM_OK;
    OM_REQUIRE(images && n_images > 0, OM_EINVAL, "om_visualize: bad argument");
    OM_REQUIRE(ws_bytes >= om_visualize_workspace_bytes(images, n_images) && workspace, OM_ENOMEM,
               "om_visualize: workspace of %zu bytes, %zu needed", ws_bytes, om_visualize_workspace_bytes(images, n_images));
    OM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, OM_EINVAL, "om_visualize: workspace not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    om::VisMaskStat* stats = static_cast<om::VisMaskStat*>(workspace);
    int ws_first = 0;
    for (int i0 = 0; i0 < n_images; i0 += OM_VIS_BATCH) {
        om::VisBatch bt;
        bt.n = 0;
        bt.mask_first[0] = 0;
        bt.tile_first[0] = 0;
        for (int i = i0; i < n_images && i < i0 + OM_VIS_BATCH; ++i) {
            const om_vis_image& s = images[i];
            OM_REQUIRE(s.image && s.out && s.h > 0 && s.w > 0 && (long long)s.h * s.w < (1ll << 31) / 3 && s.n_keep >= 0 &&
                           s.n_keep <= OM_VIS_MAX_KEPT,
                       OM_EINVAL, "om_visualize: image %d: bad argument (h %d, w %d, n_keep %d; at most %d kept)", i, s.h, s.w,
                       s.n_keep, OM_VIS_MAX_KEPT);
            OM_REQUIRE(reinterpret_cast<uintptr_t>(s.image) % 16 == 0 && reinterpret_cast<uintptr_t>(s.out) % 4 == 0 &&
                           reinterpret_cast<uintptr_t>(s.out_float) % 4 == 0,
                       OM_EINVAL, "om_visualize: image %d: image must be 16-byte and out 4-byte aligned", i);
            const bool masks = s.with_mask && s.n_keep > 0;
            if (s.n_keep > 0) OM_REQUIRE(s.colors, OM_EINVAL, "om_visualize: image %d: no colours", i);
            if (s.draw_boxes && s.n_keep > 0)
                OM_REQUIRE(s.boxes && reinterpret_cast<uintptr_t>(s.boxes) % 16 == 0, OM_EINVAL,
                           "om_visualize: image %d: boxes missing or not 16-byte aligned", i);
            if (masks) {
                OM_REQUIRE(s.mask && s.keep && s.Hn > 0 && s.Wn > 0, OM_EINVAL, "om_visualize: image %d: no masks", i);
                OM_REQUIRE(s.crop_top >= 0 && s.crop_down >= 0 && s.crop_left >= 0 && s.crop_right >= 0 &&
                               s.crop_top + s.crop_down < s.Hn && s.crop_left + s.crop_right < s.Wn,
                           OM_EINVAL, "om_visualize: image %d: crop (%d,%d,%d,%d) leaves nothing of %dx%d", i, s.crop_left,
                           s.crop_right, s.crop_top, s.crop_down, s.Hn, s.Wn);
                OM_REQUIRE(s.Hn - s.crop_top - s.crop_down <= om::VIS_MAX_SRC && s.Wn - s.crop_left - s.crop_right <= om::VIS_MAX_SRC,
                           OM_EINVAL, "om_visualize: image %d: masks larger than %d pixels", i, om::VIS_MAX_SRC);
            }
            om::VisImg& q = bt.img[bt.n];
            q.image = s.image; q.out = s.out; q.out_float = s.out_float; q.mask = s.mask; q.keep = s.keep;
            q.colors = s.colors; q.boxes = s.boxes;
            q.n = s.n_keep; q.H = s.Hn; q.W = s.Wn;
            q.crop_top = s.crop_top; q.crop_left = s.crop_left;
            q.ch = s.Hn - s.crop_top - s.crop_down; q.cw = s.Wn - s.crop_left - s.crop_right;
            q.h = s.h; q.w = s.w; q.with_mask = masks ? 1 : 0; q.draw_boxes = s.draw_boxes ? 1 : 0;
            q.alpha = s.alpha;
            q.scale_h = masks ? (float)q.ch / (float)s.h : 1.f;     // F.interpolate(size=...): input / output size
            q.scale_w = masks ? (float)q.cw / (float)s.w : 1.f;
            const long long tiles = ((long long)s.h * s.w + om::VIS_TILE - 1) / om::VIS_TILE;
            OM_REQUIRE(bt.tile_first[bt.n] + tiles < (1ll << 31), OM_EINVAL, "om_visualize: too many pixels in one batch");
            bt.mask_first[bt.n + 1] = bt.mask_first[bt.n] + (masks ? s.n_keep : 0);
            bt.tile_first[bt.n + 1] = bt.tile_first[bt.n] + (int)tiles;
            ++bt.n;
        }
        om::VisMaskStat* st_batch = stats + ws_first;
        if (bt.mask_first[bt.n] > 0) {
            hipLaunchKernelGGL(om::vis_mask_stats_kernel, dim3(bt.mask_first[bt.n]), dim3(om::VIS_THREADS), 0, st, bt, st_batch);
            OM_CHECK_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(om::vis_composite_kernel, dim3(bt.tile_first[bt.n]), dim3(om::VIS_THREADS), 0, st, bt,
                           (const om::VisMaskStat*)st_batch);
        OM_CHECK_HIP(hipGetLastError());
        ws_first += bt.mask_first[bt.n];
    }
    return OM_OK;
}

}  // extern "C"
