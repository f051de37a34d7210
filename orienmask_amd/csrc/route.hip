// The training models' plumbing between the convolutions (model/orienmask_yolo_fpnplus.py:74-90, model/orienmask_yolo.py:71-86 of
// the reference): torch.cat of nearest-up-sampled routes, and torch.split, with the backward autograd gives them.
//   route_concat_forward_kernel    y[b, off_i + c, oy, ox] = src_i[b, c, oy / s_i, ox / s_i]: pure copies.  A null source is zeros.
//   route_concat_backward_kernel   dsrc_i[b, c, sy, sx] = the s_i x s_i block of dy summed sequentially in fp32, rows top to
//                                  bottom and left to right within a row, the accumulator starting as the block's first element
//                                  (torch-CPU's upsample_nearest2d backward order); at s = 1 a copy.  A null dsrc is skipped.
// The tensors are fp32, or bf16 through the _bf16 entry points (the kernels' element type T).
// Both kernels walk ONE flat item list with a grid-stride loop: the items of source 0, then of source 1, ...  An item's place in
// its source's list is decoded into (b, c, row, k) with k fastest, so a wave's lanes run along W.  The divisors are fixed per
// launch, so the host turns each into a multiply and a shift (RouteDiv).
// Two forms of each kernel, chosen by the ENTRY POINT from the arguments (route_vector_form), never inside the kernel:
//   vector   W % 4 == 0 and y / dy and every non-null source tensor aligned to 4 elements (16 bytes of fp32, 8 of bf16; the byte
//            counts below are fp32's, bf16's are half).  Forward: an item is 4 output pixels of a row,
//            one 16-byte store; the source side is one 16-byte load (s = 1), two elements (s = 2) or one (s = 4, 8).  Backward: an
//            item is a strip of 4 dy columns (8 at s = 8) by s rows, read as 16-byte loads; it writes 4 (s = 1), 2 (s = 2) or 1
//            (s = 4, 8) elements of dsrc in one store.
//   scalar   anything else (a tensor that starts at an odd element, W % 4 != 0): an item is one element of y / of dsrc.
// The table (pointers, channel offsets, scales, divisors) is a kernel argument by value; its rows are picked with constant indices
// (route_pick), so nothing is indexed dynamically and nothing goes to scratch.  Built with -ffp-contract=off and without SLP
// vectorisation: the block sum's adds stay single fp32 adds in the order written.
#include <climits>

#include "om_common.h"
#include "bf16.h"

namespace om {

constexpr int ROUTE_THREADS = 256;
constexpr int ROUTE_MAX_BLOCKS = 2048;      // 256 CUs x 8 workgroups (8 waves per SIMD); the rest is grid-strided
constexpr int ROUTE_MAX_SRC = 4;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// The element type T of a launch is float or bf16_t; the kernels see floats through these.  A bf16 is widened exactly and a float
// is rounded to bf16 to nearest even (bf16.h), so the forward stays a copy and the backward's block sum, taken in fp32 in the order
// below, is rounded once.  GROUP accesses are 4 elements: 16 bytes of fp32, 8 of bf16.

#define OM_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ float route_load1(const OM_GLOBAL T* p) {
    if constexpr (sizeof(T) == 4) return *p;
    else return bf16_widen(*p);
}
template <typename T>
__device__ __forceinline__ void route_store1(OM_GLOBAL T* p, float v) {
    if constexpr (sizeof(T) == 4) *p = v;
    else *p = (bf16_t)bf16_round(v);
}
template <typename T>
__device__ __forceinline__ f32x4 route_load4(const OM_GLOBAL T* p) {
    if constexpr (sizeof(T) == 4) {
        return *(const OM_GLOBAL f32x4*)p;
    } else {
        const u32x2 t = *(const OM_GLOBAL u32x2*)p;
        return f32x4{bf16_widen(t[0] & 0xffffu), bf16_widen(t[0] >> 16), bf16_widen(t[1] & 0xffffu), bf16_widen(t[1] >> 16)};
    }
}
template <typename T>
__device__ __forceinline__ void route_store4(OM_GLOBAL T* p, f32x4 v) {
    if constexpr (sizeof(T) == 4) *(OM_GLOBAL f32x4*)p = v;
    else *(OM_GLOBAL u32x2*)p = u32x2{bf16_round(v[0]) | (bf16_round(v[1]) << 16), bf16_round(v[2]) | (bf16_round(v[3]) << 16)};
}
template <typename T>
__device__ __forceinline__ void route_store2(OM_GLOBAL T* p, f32x2 v) {
    if constexpr (sizeof(T) == 4) *(OM_GLOBAL f32x2*)p = v;
    else *(OM_GLOBAL uint32_t*)p = bf16_round(v[0]) | (bf16_round(v[1]) << 16);
}

// n / d for every n < 2^31 as (n * mul) >> shift: shift = 31 + ceil(log2 d), mul = ceil(2^shift / d) < 2^32 (Granlund & Montgomery
// 1994, theorem 4.2 with N = 31)
struct RouteDiv {
    uint32_t mul, shift;
};

static RouteDiv route_div(uint32_t d) {
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    RouteDiv r;
    r.shift = 31 + l;
    r.mul = (uint32_t)(((1ull << r.shift) + d - 1) / d);
    return r;
}

__device__ __forceinline__ uint32_t route_quot(uint32_t n, RouteDiv d) { return (uint32_t)(((uint64_t)n * d.mul) >> d.shift); }

struct RouteSeg {
    void* ptr;              // the source (forward, read) or its gradient (backward, written); null: zeros / no items
    uint32_t start;         // first item of this source in the flat list; UINT_MAX for an unused row
    uint32_t chans, off;    // channels, first channel in y / dy
    uint32_t sh;            // log2 of the scale
    uint32_t per_row;       // items per row of the decoded plane
    uint32_t rows;          // rows of the decoded plane: H in the forward, H >> sh in the backward
    RouteDiv by_per_row, by_rows, by_chans;
};

struct RouteTable {
    RouteSeg seg[ROUTE_MAX_SRC];
    uint32_t total;         // items of the whole list
    uint32_t ctot, H, W;    // y / dy is [B, ctot, H, W]
};

// The row an item belongs to.  Starts are non-decreasing and a source without items shares its successor's start, so the last row
// whose start is <= idx is the one.  Constant indices and one select per field: a whole-row copy under a condition would make the
// compiler keep the table in scratch.
#define ROUTE_PICK(field) s.field = hit ? t.seg[k].field : s.field
__device__ __forceinline__ RouteSeg route_pick(const RouteTable& t, uint32_t idx) {
    RouteSeg s = t.seg[0];
#pragma unroll
    for (int k = 1; k < ROUTE_MAX_SRC; ++k) {
        const bool hit = idx >= t.seg[k].start;
        ROUTE_PICK(ptr); ROUTE_PICK(start); ROUTE_PICK(chans); ROUTE_PICK(off); ROUTE_PICK(sh); ROUTE_PICK(per_row); ROUTE_PICK(rows);
        ROUTE_PICK(by_per_row.mul); ROUTE_PICK(by_per_row.shift); ROUTE_PICK(by_rows.mul); ROUTE_PICK(by_rows.shift);
        ROUTE_PICK(by_chans.mul); ROUTE_PICK(by_chans.shift);
    }
    return s;
}
#undef ROUTE_PICK

struct RouteItem {
    uint32_t b, c, row, k;
};

__device__ __forceinline__ RouteItem route_decode(const RouteSeg& s, uint32_t local) {
    RouteItem it;
    uint32_t t = route_quot(local, s.by_per_row);
    it.k = local - t * s.per_row;
    uint32_t u = route_quot(t, s.by_rows);
    it.row = t - u * s.rows;
    it.b = route_quot(u, s.by_chans);
    it.c = u - it.b * s.chans;
    return it;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(ROUTE_THREADS)
route_concat_forward_kernel(const RouteTable t, T* __restrict__ y_) {
    OM_GLOBAL T* __restrict__ y = (OM_GLOBAL T*)y_;
    const uint32_t stride = gridDim.x * ROUTE_THREADS;
    for (uint32_t idx = blockIdx.x * ROUTE_THREADS + threadIdx.x; idx < t.total; idx += stride) {
        const RouteSeg s = route_pick(t, idx);
        const RouteItem it = route_decode(s, idx - s.start);       // row = oy, k = the item's place in the output row
        const OM_GLOBAL T* __restrict__ src = (const OM_GLOBAL T*)s.ptr;
        const uint32_t ws = t.W >> s.sh;
        // first source element of the item: source row oy >> sh of plane (b, c)
        const uint32_t srow = ((it.b * s.chans + it.c) * (t.H >> s.sh) + (it.row >> s.sh)) * ws;
        const uint32_t yrow = ((it.b * t.ctot + s.off + it.c) * t.H + it.row) * t.W;
        if (VEC) {
            const uint32_t ox = it.k * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (src) {
                if (s.sh == 0) {
                    v = route_load4<T>(src + srow + ox);
                } else if (s.sh == 1) {
                    const float a = route_load1<T>(src + srow + (ox >> 1)), c = route_load1<T>(src + srow + (ox >> 1) + 1);
                    v = f32x4{a, a, c, c};
                } else {
                    const float a = route_load1<T>(src + srow + (ox >> s.sh));
                    v = f32x4{a, a, a, a};
                }
            }
            route_store4<T>(y + yrow + ox, v);
        } else {
            route_store1<T>(y + yrow + it.k, src ? route_load1<T>(src + srow + (it.k >> s.sh)) : 0.f);
        }
    }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(ROUTE_THREADS)
route_concat_backward_kernel(const RouteTable t, const T* __restrict__ dy_) {
    const OM_GLOBAL T* __restrict__ dy = (const OM_GLOBAL T*)dy_;
    const uint32_t stride = gridDim.x * ROUTE_THREADS;
    for (uint32_t idx = blockIdx.x * ROUTE_THREADS + threadIdx.x; idx < t.total; idx += stride) {
        const RouteSeg s = route_pick(t, idx);
        const uint32_t local = idx - s.start;
        const RouteItem it = route_decode(s, local);      // row = sy, k = the item's place in the source row
        OM_GLOBAL T* __restrict__ dst = (OM_GLOBAL T*)s.ptr;
        const uint32_t W = t.W;
        // first dy element of the item's top row: row sy << sh of plane (b, off + c)
        const OM_GLOBAL T* __restrict__ top = dy + ((it.b * t.ctot + s.off + it.c) * t.H + (it.row << s.sh)) * W;
        if (VEC) {
            // dsrc is contiguous in item order: item `local` owns elements [local * g, local * g + g), g = 4, 2, 1, 1
            if (s.sh == 0) {
                route_store4<T>(dst + (size_t)local * 4, route_load4<T>(top + it.k * 4));
            } else if (s.sh == 1) {
                const f32x4 r0 = route_load4<T>(top + it.k * 4), r1 = route_load4<T>(top + W + it.k * 4);
                f32x2 o;
                o[0] = ((r0[0] + r0[1]) + r1[0]) + r1[1];
                o[1] = ((r0[2] + r0[3]) + r1[2]) + r1[3];
                route_store2<T>(dst + (size_t)local * 2, o);
            } else if (s.sh == 2) {
                const OM_GLOBAL T* p = top + it.k * 4;
                f32x4 r = route_load4<T>(p);
                float acc = ((r[0] + r[1]) + r[2]) + r[3];
#pragma unroll
                for (int j = 1; j < 4; ++j) {
                    r = route_load4<T>(p + j * W);
                    acc = (((acc + r[0]) + r[1]) + r[2]) + r[3];
                }
                route_store1<T>(dst + local, acc);
            } else {
                const OM_GLOBAL T* p = top + it.k * 8;
                f32x4 r = route_load4<T>(p), q = route_load4<T>(p + 4);
                float acc = ((((((r[0] + r[1]) + r[2]) + r[3]) + q[0]) + q[1]) + q[2]) + q[3];
#pragma unroll
                for (int j = 1; j < 8; ++j) {
                    r = route_load4<T>(p + j * W);
                    q = route_load4<T>(p + j * W + 4);
                    acc = (((((((acc + r[0]) + r[1]) + r[2]) + r[3]) + q[0]) + q[1]) + q[2]) + q[3];
                }
                route_store1<T>(dst + local, acc);
            }
        } else {
            const uint32_t sc = 1u << s.sh;
            const OM_GLOBAL T* p = top + (it.k << s.sh);
            float acc = route_load1<T>(p);
            for (uint32_t i = 1; i < sc; ++i) acc += route_load1<T>(p + i);
            for (uint32_t j = 1; j < sc; ++j) {
                p += W;
                for (uint32_t i = 0; i < sc; ++i) acc += route_load1<T>(p + i);
            }
            route_store1<T>(dst + local, acc);
        }
    }
}

static int route_log2(int s) { return s == 1 ? 0 : s == 2 ? 1 : s == 4 ? 2 : s == 8 ? 3 : -1; }

// The limits both entry points share; -> sum(chans) in *ctot.  Reads chans / scales only after n is known to be in range.
static int route_check(const char* who, const int* chans, const int* scales, int n, int B, int H, int W, int* ctot) {
    OM_REQUIRE(n >= 1 && n <= ROUTE_MAX_SRC, OM_EINVAL, "%s: %d sources; 1 to %d are supported", who, n, ROUTE_MAX_SRC);
    OM_REQUIRE(chans && scales, OM_EINVAL, "%s: null chans / scales", who);
    OM_REQUIRE(B >= 1 && H >= 1 && W >= 1, OM_EINVAL, "%s: B %d, H %d, W %d must be >= 1", who, B, H, W);
    long long c = 0;
    for (int i = 0; i < n; ++i) {
        OM_REQUIRE(chans[i] >= 1, OM_EINVAL, "%s: source %d has %d channels", who, i, chans[i]);
        OM_REQUIRE(route_log2(scales[i]) >= 0, OM_EINVAL, "%s: source %d has scale %d; the scales are 1, 2, 4 and 8", who, i, scales[i]);
        OM_REQUIRE(H % scales[i] == 0 && W % scales[i] == 0, OM_EINVAL, "%s: H %d, W %d are not divisible by scale %d of source %d",
                   who, H, W, scales[i], i);
        c += chans[i];
        OM_REQUIRE(c < (1ll << 31), OM_EINVAL, "%s: %lld channels", who, c);
    }
    // B, c, H, W < 2^31 each: the product of the first two fits a long long, and each further factor is checked before it is taken
    long long total = (long long)B * c;
    OM_REQUIRE(total < (1ll << 31) && total * H < (1ll << 31) && total * H * W < (1ll << 31), OM_EINVAL,
               "%s: B %d x %lld channels x %d x %d is 2^31 elements or more", who, B, c, H, W);
    *ctot = (int)c;
    return OM_OK;
}

// The vector form's conditions, from the arguments alone: rows of whole 4-element groups (group_bytes: 16 of fp32, 8 of bf16), and
// every tensor the kernel touches starting on a group boundary (every plane and row of a contiguous tensor then does, at every scale: W / s is even or the access scalar).
static bool route_vector_form(const void* whole, void* const* parts, int n, int W, int group_bytes) {
    if (W % 4 != 0 || align_bytes(whole) < group_bytes) return false;
    for (int i = 0; i < n; ++i)
        if (parts[i] && align_bytes(parts[i]) < group_bytes) return false;
    return true;
}

static int route_blocks(uint32_t total) {
    const uint32_t need = (total + ROUTE_THREADS - 1) / ROUTE_THREADS;
    return (int)(need < (uint32_t)ROUTE_MAX_BLOCKS ? need : (uint32_t)ROUTE_MAX_BLOCKS);
}

// Fills the table: row i's items, when `active`, are B * chans * rows * per_row.
static void route_table(RouteTable& t, void* const* ptrs, const int* chans, const int* scales, int n, int B, int ctot, int H, int W,
                        bool vec, bool backward) {
    uint32_t start = 0, off = 0;
    for (int i = 0; i < ROUTE_MAX_SRC; ++i) {
        RouteSeg& s = t.seg[i];
        if (i >= n) {
            s = RouteSeg{nullptr, UINT_MAX, 1, 0, 0, 1, 1, route_div(1), route_div(1), route_div(1)};
            continue;
        }
        const uint32_t sh = (uint32_t)route_log2(scales[i]);
        s.ptr = ptrs[i];
        s.start = start;
        s.chans = (uint32_t)chans[i];
        s.off = off;
        s.sh = sh;
        if (backward) {
            s.rows = (uint32_t)H >> sh;
            s.per_row = vec ? (uint32_t)W / (sh == 3 ? 8u : 4u) : (uint32_t)W >> sh;
        } else {
            s.rows = (uint32_t)H;
            s.per_row = vec ? (uint32_t)W / 4u : (uint32_t)W;
        }
        s.by_per_row = route_div(s.per_row);
        s.by_rows = route_div(s.rows);
        s.by_chans = route_div(s.chans);
        if (!backward || ptrs[i]) start += (uint32_t)B * s.chans * s.rows * s.per_row;      // <= B * ctot * H * W < 2^31
        off += s.chans;
    }
    t.total = start;
    t.ctot = (uint32_t)ctot;
    t.H = (uint32_t)H;
    t.W = (uint32_t)W;
}

// The entry points' bodies for the element type T; `who` is the entry point's name in the messages.
template <typename T>
static int route_concat_forward(const char* who, const void* const* src, const int* chans, const int* scales, int n, int B, int H, int W,
                                T* y, om_stream stream) {
    int ctot = 0;
    const int rc = route_check(who, chans, scales, n, B, H, W, &ctot);
    if (rc != OM_OK) return rc;
    OM_REQUIRE(src && y, OM_EINVAL, "%s: null src table or y", who);
    void* ptrs[ROUTE_MAX_SRC] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < n; ++i) ptrs[i] = const_cast<void*>(src[i]);
    const bool vec = route_vector_form(y, ptrs, n, W, 4 * (int)sizeof(T));
    RouteTable t;
    route_table(t, ptrs, chans, scales, n, B, ctot, H, W, vec, false);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(route_blocks(t.total)), block(ROUTE_THREADS);
    if (vec)
        hipLaunchKernelGGL((route_concat_forward_kernel<T, true>), grid, block, 0, st, t, y);
    else
        hipLaunchKernelGGL((route_concat_forward_kernel<T, false>), grid, block, 0, st, t, y);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

template <typename T>
static int route_concat_backward(const char* who, const T* dy, const int* chans, const int* scales, int n, int B, int H, int W,
                                 void* const* dsrc, om_stream stream) {
    int ctot = 0;
    const int rc = route_check(who, chans, scales, n, B, H, W, &ctot);
    if (rc != OM_OK) return rc;
    OM_REQUIRE(dy && dsrc, OM_EINVAL, "%s: null dy or dsrc table", who);
    void* ptrs[ROUTE_MAX_SRC] = {nullptr, nullptr, nullptr, nullptr};
    bool any = false;
    for (int i = 0; i < n; ++i) {
        ptrs[i] = dsrc[i];
        any = any || dsrc[i];
    }
    OM_REQUIRE(any, OM_EINVAL, "%s: every dsrc is null, there is nothing to compute", who);
    const bool vec = route_vector_form(dy, ptrs, n, W, 4 * (int)sizeof(T));
    RouteTable t;
    route_table(t, ptrs, chans, scales, n, B, ctot, H, W, vec, true);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(route_blocks(t.total)), block(ROUTE_THREADS);
    if (vec)
        hipLaunchKernelGGL((route_concat_backward_kernel<T, true>), grid, block, 0, st, t, dy);
    else
        hipLaunchKernelGGL((route_concat_backward_kernel<T, false>), grid, block, 0, st, t, dy);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // namespace om

extern "C" {

int om_route_concat_forward(const float* const src[4], const int chans[4], const int scales[4], int n, int B, int H, int W, float* y,
                            om_stream stream) {
    return om::route_concat_forward<float>("om_route_concat_forward", reinterpret_cast<const void* const*>(src), chans, scales, n, B, H,
                                           W, y, stream);
}

int om_route_concat_forward_bf16(const uint16_t* const src[4], const int chans[4], const int scales[4], int n, int B, int H, int W,
                                 uint16_t* y, om_stream stream) {
    return om::route_concat_forward<om::bf16_t>("om_route_concat_forward_bf16", reinterpret_cast<const void* const*>(src), chans, scales,
                                                n, B, H, W, y, stream);
}

int om_route_concat_backward(const float* dy, const int chans[4], const int scales[4], int n, int B, int H, int W, float* const dsrc[4],
                             om_stream stream) {
    return om::route_concat_backward<float>("om_route_concat_backward", dy, chans, scales, n, B, H, W,
                                            reinterpret_cast<void* const*>(dsrc), stream);
}

int om_route_concat_backward_bf16(const uint16_t* dy, const int chans[4], const int scales[4], int n, int B, int H, int W,
                                  uint16_t* const dsrc[4], om_stream stream) {
    return om::route_concat_backward<om::bf16_t>("om_route_concat_backward_bf16", dy, chans, scales, n, B, H, W,
                                                 reinterpret_cast<void* const*>(dsrc), stream);
}

}  // extern "C"
