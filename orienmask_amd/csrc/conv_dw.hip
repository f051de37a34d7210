// The weight and bias gradients of the training model's convolutions, float32 and bf16 (orienmask_amd/train.py: conv2d's and
// conv2d_bf16's backward), for conv_train.h's three geometries: ONE kernel, split rule and host body for both types.  NCHW
// contiguous; x and dy float32 on v_mfma_f32_32x32x2_f32, or bf16 (widened exactly, every product exact in float32) on
// v_mfma_f32_32x32x16_bf16; dw and db float32.  The data gradients are conv_grad.hip and conv_grad_bf16.hip.
//
// ARITHMETIC CONTRACT (tests/test_conv_grad_weight_bits.py pins the bits; test_conv_grad.py and test_conv_grad_bf16.py the accuracy)
//   dw[co,ci,kh,kw] = sum_{b,oy,ox} dy[b,co,oy,ox] * x[b,ci,oy*s+kh-pad,ox*s+kw-pad]
//        GEMM: rows = co (first operand: dy), columns = ci (second operand: x, one 32 x 32 accumulator per tap), k = the flat output
//        pixel (b, oy, ox); both operands are contiguous along k in memory.  k is split over workgroups (blockIdx.x) by dw_splits: a
//        function of the shape and om::device_compute_units only, the same for both types.  Three levels of float32-or-wider sums:
//        a matrix-instruction accumulator takes DW_CHAIN_PIX = 32 pixels (at 1x1 the chain's instructions go in turn to NCH
//        accumulators -- float32: four, 8 pixels each; bf16: two, one instruction each -- which are then summed pairwise), is added
//        into a second float32 accumulator and cleared (at most 64 such additions per workgroup); with more than one split the
//        workgroup's tile goes to partial[split][co][ci][tap] in the caller's workspace and conv_dw_reduce_kernel sums the splits of
//        an element in split order in double and rounds once.  No atomics: the same bits on every run.  (float32: one chain over
//        the 18 pixels of a 3 x 3 map at B = 2 measured 2.12 x torch-CPU-float32's error over the tensor's scale on in-network operands.)
//   db[co] = sum dy[b,co,:,:] in double, one workgroup per channel, in a fixed order, rounded once to float32.
//
// STRUCTURE   WCO waves along co (32 each), 4 / WCO along ci (32 each).  Both operands lie in LDS as [channel][pixel], so the k of one
//   instruction is one read per lane: a float, or 8 consecutive bf16 as 16 bytes.  x is staged per tap (each pixel's tap address
//   computed, zero outside the map): simple and exact, and 9 loads per pixel and channel at 3x3.  Staging the rows with their halo
//   once and reading taps as shifts would cut that to ~1.1; left for later.
//
// BUDGET (gfx950 code objects)   3x3 holds 9 x 16 accumulators twice (first and second level) = 288 registers before any operand, so it
//   cannot fit the 256 of __launch_bounds__(256, 2) without spilling inside the main loop: __launch_bounds__(256), one workgroup per
//   SIMD set and up to 512 registers, no scratch.  LDS at most 53.6 KiB (float32), 55.5 KiB (bf16).  Per instantiation: DESIGN 3.19, 3.29.
// Every load and store is bounds-checked per element (any B, cin, cout, H, W >= 1); every global access is of one element, so no
// alignment beyond the element's own is assumed; rows and columns of a tile outside the tensor are staged as zeros and never stored.
#include "conv_train.h"
#include "bf16.h"

namespace om {

constexpr int DW_THREADS = 256;
constexpr int DW_CHAIN_PIX = 32;        // pixels (= products) of a first-level chain
constexpr int DW_SPLIT_PIX = 2048;      // most pixels of a workgroup, i.e. at most 64 first-level chains in its second-level sum
constexpr int DW_MIN_PIX = 256;         // fewest pixels a split is cut down to when the launch would leave compute units idle

// The operand policies.  KI: pixels of one matrix instruction, of which a lane holds KI / 2 consecutive ones (frag) from pixel
// fk * KI / 2 on; PAD: elements an LDS row of KP pixels is padded by; kp: pixels per staged step; nch: interleaved accumulators.
struct DwF32 {
    typedef float elem;
    typedef float frag;
    static constexpr int KI = 2, PAD = 1;
    static constexpr int kp(int WCI, int TAPS) { return 32 / WCI; }
    static constexpr int nch(int TAPS) { return TAPS == 1 ? 4 : 1; }
    static __device__ __forceinline__ frag load(const elem* p) { return *p; }
    static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};

struct DwBf16 {
    typedef bf16_t elem;
    typedef __bf16 frag __attribute__((ext_vector_type(8)));
    static constexpr int KI = 16, PAD = 8;                          // rows stay 16-byte aligned
    static constexpr int kp(int WCI, int TAPS) { return TAPS == 9 && WCI == 4 ? 16 : 32; }      // (9 taps of 128 ci at 32 pixels would not fit)
    static constexpr int nch(int TAPS) { return TAPS == 1 ? 2 : 1; }
    static __device__ __forceinline__ frag load(const elem* p) { return __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(p)); }
    static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

template <typename T>
struct DwArgs {
    const T* x; const T* dy;
    float* out;                 // dw, or the partial tiles [splits][cout][cin][taps]
    int cin, cout, H, W, Ho, Wo, HoWo, stride, pad;
    int K;                      // B * Ho * Wo
    int chunk;                  // pixels per split
    size_t n;                   // cout * cin * taps
};

// element r of a chain: its NCH accumulators summed pairwise
template <int NCH>
__device__ __forceinline__ float dw_chain(const f32x16* acc, int r) {
    if constexpr (NCH == 4) return (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
    else if constexpr (NCH == 2) return acc[0][r] + acc[1][r];
    else return acc[0][r];
}

template <typename Op, int WCO, int TAPS>
__global__ void __launch_bounds__(DW_THREADS) conv_dw_kernel(const DwArgs<typename Op::elem> a) {
    typedef typename Op::elem elem;
    constexpr int WCI = 4 / WCO, COT = 32 * WCO, CIT = 32 * WCI;
    constexpr int KP = Op::kp(WCI, TAPS), KI = Op::KI, LD = KP + Op::PAD;
    constexpr int G = DW_THREADS / KP;              // threads per pixel column of the staging
    constexpr int KS = TAPS == 1 ? 1 : 3;
    constexpr int CHAIN_STEPS = DW_CHAIN_PIX / KP;
    static_assert(DW_CHAIN_PIX % KP == 0, "a chain is a whole number of steps");
    // 1x1: instruction i of a step goes to accumulator i % NCH, so no chain in an accumulator is longer than DW_CHAIN_PIX / NCH products
    constexpr int NCH = Op::nch(TAPS);
    static_assert((KP / KI) % NCH == 0, "every step gives each accumulator the same number of instructions");
    __shared__ __attribute__((aligned(sizeof(typename Op::frag)))) elem s_dy[COT * LD];         // [co][pixel]
    __shared__ __attribute__((aligned(sizeof(typename Op::frag)))) elem s_x[TAPS * CIT * LD];   // [tap][ci][pixel]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wco = wave / WCI, wci = wave % WCI;
    const int fi = lane & 31, fk = lane >> 5;
    const int split = blockIdx.x, co0 = blockIdx.y * COT, ci0 = blockIdx.z * CIT;
    const int k_begin = split * a.chunk;
    const int k_end = min(a.K, k_begin + a.chunk);
    const int kp = tid % KP, g = tid / KP;
    const size_t hw = (size_t)a.H * a.W;
    const bool live = co0 + wco * 32 < a.cout && ci0 + wci * 32 < a.cin;      // this wave's block holds an element of dw

    f32x16 acc[TAPS * NCH], tot[TAPS];
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp) clear16(tot[tp]);
#pragma unroll
    for (int i = 0; i < TAPS * NCH; ++i) clear16(acc[i]);

    int step = 0;               // staged steps in the open chain
    for (int k0 = k_begin; k0 < k_end; k0 += KP) {
        const int k = k0 + kp;
        const bool valid = k < k_end;
        const int kb = valid ? k : k_end - 1;
        const int b = kb / a.HoWo, qq = kb - b * a.HoWo;
        const int oy = qq / a.Wo, ox = qq - oy * a.Wo;
        __syncthreads();                            // the previous step's reads are done
        {
            const elem* p = a.dy + (size_t)b * a.cout * a.HoWo + qq;
            for (int cl = g; cl < COT; cl += G) {
                const int co = co0 + cl;
                elem v = 0;
                if (valid && co < a.cout) v = p[(size_t)co * a.HoWo];
                s_dy[cl * LD + kp] = v;
            }
        }
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) {
            const int iy = oy * a.stride + tp / KS - a.pad, ix = ox * a.stride + tp % KS - a.pad;
            const bool tv = valid && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const elem* p = a.x + (size_t)b * a.cin * hw + (tv ? (size_t)iy * a.W + ix : 0);
            for (int cl = g; cl < CIT; cl += G) {
                const int ci = ci0 + cl;
                elem v = 0;
                if (tv && ci < a.cin) v = p[(size_t)ci * hw];
                s_x[(tp * CIT + cl) * LD + kp] = v;
            }
        }
        __syncthreads();
        if (live) {
            const elem* ap = s_dy + (wco * 32 + fi) * LD + fk * (KI / 2);
            const elem* bp = s_x + (wci * 32 + fi) * LD + fk * (KI / 2);
#pragma unroll
            for (int i = 0; i < KP / KI; ++i) {
                const typename Op::frag av = Op::load(ap + i * KI);
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp)
                    acc[tp * NCH + i % NCH] = Op::mfma(av, Op::load(bp + tp * CIT * LD + i * KI), acc[tp * NCH + i % NCH]);
            }
            if (++step == CHAIN_STEPS) {            // the chain ends
                step = 0;
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) tot[tp][r] += dw_chain<NCH>(acc + tp * NCH, r);
#pragma unroll
                    for (int c = 0; c < NCH; ++c) clear16(acc[tp * NCH + c]);
                }
            }
        }
    }
    if (!live) return;
    // D layout: column (ci) = lane & 31, row (co) = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)
    const int ci = ci0 + wci * 32 + fi;
    if (ci >= a.cin) return;
    float* o = a.out + (size_t)split * a.n;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + wco * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
        if (co >= a.cout) continue;
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) {
            const float rest = dw_chain<NCH>(acc + tp * NCH, r);      // an unfinished chain (zeros after a finished one)
            o[((size_t)co * a.cin + ci) * TAPS + tp] = tot[tp][r] + rest;
        }
    }
}

// dw[e] = the splits' partial[s][e] summed in split order, in double, rounded once
__global__ void __launch_bounds__(DW_THREADS) conv_dw_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, size_t n,
                                                                    int splits) {
    const size_t e = (size_t)blockIdx.x * DW_THREADS + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int i = 0; i < splits; ++i) s += (double)partial[(size_t)i * n + e];
    dw[e] = (float)s;
}

__device__ __forceinline__ double dw_widen(float v) { return (double)v; }
__device__ __forceinline__ double dw_widen(bf16_t v) { return (double)bf16_widen(v); }

// db[co] = sum over b and the plane of dy[b,co]: per-thread sums over a fixed stride, wave shuffles, four LDS slots
template <typename T>
__global__ void __launch_bounds__(DW_THREADS) conv_dbias_kernel(const T* __restrict__ dy, float* __restrict__ db, int B, int cout, int HoWo) {
    __shared__ double lds[DW_THREADS / 64];
    const int co = blockIdx.x;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const T* p = dy + ((size_t)b * cout + co) * HoWo;
        for (int i = threadIdx.x; i < HoWo; i += DW_THREADS) s += dw_widen(p[i]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) db[co] = (float)((lds[0] + lds[1]) + (lds[2] + lds[3]));
}

// ---------------------------------------------------------------------------------------------------------------- host
static int dw_wco(int cout) { return cout > 64 ? 4 : cout > 32 ? 2 : 1; }

// splits of the weight gradient's k: at most DW_SPLIT_PIX pixels each; more, down to DW_MIN_PIX pixels each, while the launch
// has fewer than two workgroups per compute unit
static int dw_splits(const ConvGeom& g, int* chunk) {
    const int wco = dw_wco(g.cout), wci = 4 / wco;
    const long long tiles = (long long)((g.cout + 32 * wco - 1) / (32 * wco)) * ((g.cin + 32 * wci - 1) / (32 * wci));
    long long s = ((long long)g.K + DW_SPLIT_PIX - 1) / DW_SPLIT_PIX;
    const long long want = (2ll * device_compute_units() + tiles - 1) / tiles;
    const long long most = ((long long)g.K + DW_MIN_PIX - 1) / DW_MIN_PIX;
    if (s < want) s = want < most ? want : most;
    if (s < 1) s = 1;
    *chunk = (int)(((long long)g.K + s - 1) / s);
    return (int)(((long long)g.K + *chunk - 1) / *chunk);
}

template <typename Op, int WCO, int TAPS>
static void launch_dw(const DwArgs<typename Op::elem>& a, int splits, hipStream_t st) {
    constexpr int COT = 32 * WCO, CIT = 32 * (4 / WCO);
    const dim3 grid(splits, (a.cout + COT - 1) / COT, (a.cin + CIT - 1) / CIT);
    hipLaunchKernelGGL((conv_dw_kernel<Op, WCO, TAPS>), grid, dim3(DW_THREADS), 0, st, a);
}

static size_t grad_workspace_bytes(int B, int cin, int H, int W, int cout, int ksize, int stride) {
    ConvGeom g;
    if (!conv_geometry(B, cin, H, W, cout, ksize, stride, &g)) return 0;
    int chunk;
    const int splits = dw_splits(g, &chunk);
    return splits > 1 ? (size_t)splits * g.n * sizeof(float) : 0;
}

template <typename Op>
static int grad_weight(const char* who, const typename Op::elem* x, const typename Op::elem* dy, int B, int cin, int H, int W, int cout,
                       int ksize, int stride, float* dw, float* dbias, void* workspace, size_t ws_bytes, om_stream stream) {
    OM_REQUIRE(x && dy && (dw || dbias), OM_EINVAL, "%s: null pointer", who);
    ConvGeom g;
    if (!conv_geometry(B, cin, H, W, cout, ksize, stride, &g)) return conv_geometry_refused(who, B, cin, H, W, cout, ksize, stride);
    int chunk;
    const int splits = dw_splits(g, &chunk);
    const size_t need = dw && splits > 1 ? (size_t)splits * g.n * sizeof(float) : 0;
    OM_REQUIRE(need == 0 || (workspace && ws_bytes >= need), OM_ENOMEM, "%s: workspace of %zu bytes, need %zu", who,
               workspace ? ws_bytes : (size_t)0, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    DwArgs<typename Op::elem> a = {};
    a.x = x; a.dy = dy; a.out = splits > 1 ? static_cast<float*>(workspace) : dw;
    a.cin = cin; a.cout = cout; a.H = H; a.W = W; a.Ho = g.Ho; a.Wo = g.Wo; a.HoWo = g.HoWo; a.stride = stride; a.pad = g.pad;
    a.K = g.K; a.chunk = chunk; a.n = g.n;
    const int wco = dw_wco(cout);
    if (!dw) {
        // a frozen weight with a trainable bias: only the bias gradient below
    } else if (ksize == 1) {
        if (wco == 4) launch_dw<Op, 4, 1>(a, splits, st);
        else if (wco == 2) launch_dw<Op, 2, 1>(a, splits, st);
        else launch_dw<Op, 1, 1>(a, splits, st);
    } else {
        if (wco == 4) launch_dw<Op, 4, 9>(a, splits, st);
        else if (wco == 2) launch_dw<Op, 2, 9>(a, splits, st);
        else launch_dw<Op, 1, 9>(a, splits, st);
    }
    if (dw && splits > 1) {
        const unsigned blocks = (unsigned)((g.n + DW_THREADS - 1) / DW_THREADS);
        hipLaunchKernelGGL(conv_dw_reduce_kernel, dim3(blocks), dim3(DW_THREADS), 0, st, static_cast<const float*>(workspace), dw, g.n, splits);
    }
    if (dbias) hipLaunchKernelGGL(conv_dbias_kernel<typename Op::elem>, dim3(cout), dim3(DW_THREADS), 0, st, dy, dbias, B, cout, g.HoWo);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // namespace om

extern "C" {

size_t om_conv2d_grad_workspace_bytes(int B, int cin, int H, int W, int cout, int ksize, int stride) {
    return om::grad_workspace_bytes(B, cin, H, W, cout, ksize, stride);
}

size_t om_conv2d_bf16_grad_workspace_bytes(int B, int cin, int H, int W, int cout, int ksize, int stride) {
    return om::grad_workspace_bytes(B, cin, H, W, cout, ksize, stride);
}

int om_conv2d_grad_weight(const float* x, const float* dy, int B, int cin, int H, int W, int cout, int ksize, int stride, float* dw,
                          float* dbias, void* workspace, size_t ws_bytes, om_stream stream) {
    return om::grad_weight<om::DwF32>("om_conv2d_grad_weight", x, dy, B, cin, H, W, cout, ksize, stride, dw, dbias, workspace, ws_bytes, stream);
}

int om_conv2d_bf16_grad_weight(const uint16_t* x, const uint16_t* dy, int B, int cin, int H, int W, int cout, int ksize, int stride,
                               float* dw, float* dbias, void* workspace, size_t ws_bytes, om_stream stream) {
    return om::grad_weight<om::DwBf16>("om_conv2d_bf16_grad_weight", x, dy, B, cin, H, W, cout, ksize, stride, dw, dbias, workspace, ws_bytes,
                                       stream);
}

}  // extern "C"
