// The part of the reference's Conv -> BatchNorm2d -> LeakyReLU(0.1) block that is not the convolution (model/base.py:104-137,
// 278-279; 88 of the network's 90 convolutions), with the residual add of a DarkNet block (model/backbone/darknet.py:14-15), for
// TRAINING: batch statistics, the running-buffer update, and the backward.  NCHW contiguous, as torch's convolution leaves it; the
// activations (x, residual, y, dy, dx) fp32, or bf16 through the _bf16 entry points (the element type T of every kernel below).
//   bn_fwd_kernel   phase STATS   per-workgroup partial sums of a channel           -> workspace
//                   phase APPLY   finalise the channel, write save_mean / save_invstd / running buffers, y = leaky(z) (+ residual)
//                   phase FUSED   both in one launch, one workgroup per channel (small layers are launch-bound)
//                   phase EVAL    APPLY with the running statistics; no buffer changes
//   bn_bwd_kernel   the same three phases for (sum dz, sum dz * (x - mean)) and dx; the LeakyReLU mask is recomputed from x
//   bn_sync_*       the phases as separate entry points with the cross-rank all-gather between them (SyncBatchNorm), further down
// A channel is B planes of H*W elements.  Work is counted in UNITS of V elements (V = 4 where H*W is a multiple of 4 and every
// tensor is aligned to 4 elements -- 16 bytes of fp32, 8 of bf16 --, else 1): unit u of channel c lies in plane u / (HW/V), so a unit never straddles planes and one 32-bit division
// serves a unit.  A workgroup takes tiles of BN_THREADS * BN_UNROLL units, strided by the number of workgroups of its channel,
// and issues the BN_UNROLL loads of every stream before it uses one.
// Arithmetic: every element is widened to double, every intermediate is a double, and each output is rounded to float32 once (the
// vector double rate is far above what a pass at memory speed needs).  The forward's sums are taken around a shift K (the channel's
// first element), so the variance is sum((x-K)^2) - sum(x-K)^2/n on numbers of the size of the spread, never E[x^2] - E[x]^2.
// Per-thread sums -> wave shuffles -> four LDS slots -> per-workgroup partials in the caller's workspace -> one fixed-order sum per
// channel: no atomics, the same bits on every run.  Compiled with -ffp-contract=off: z = fma(x - mean, gamma * invstd, beta) is
// written out once and is the SAME expression, on the same doubles, in the forward and in the backward's mask.
// bf16: load_unit / store_unit are the only places that see the element type.  An element is widened exactly, and an output is the
// float32 the fp32 kernel stores, rounded to bf16 to nearest even.  The unit is 4 elements in BOTH types (8 bytes of bf16): the
// unit decides which thread sums which elements, so one geometry gives the bf16 kernel the fp32 kernel's summation order and with
// it the same doubles -- its float32 outputs have the bits of the fp32 kernel on the widened input, and its bf16 outputs are that
// kernel's, rounded.  (A 16-byte unit of 8 bf16 hands each thread its neighbour's elements as well: another order of the same sums,
// and save_mean's remainder word, which keeps 48 bits of the mean, then differs in most channels.)
#include "om_common.h"
#include "bf16.h"
#include "bn_channel.h"

namespace om {

constexpr int BN_THREADS = 256;
constexpr int BN_UNROLL = 4;                      // loads in flight per thread and stream
constexpr int BN_TILE = BN_THREADS * BN_UNROLL;   // units per tile
constexpr int BN_MAX_BLOCKS = 2048;               // 256 CUs x 8 workgroups
constexpr long long BN_FUSED_MAX = 16384;         // elements per channel up to which one workgroup does the whole channel

enum { BN_STATS = 0, BN_APPLY = 1, BN_FUSED = 2, BN_EVAL = 3 };

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct BnGeom {
    int C;
    unsigned plane_units;      // H*W / V
    unsigned units;            // B * plane_units: units per channel
    unsigned n_tiles;          // ceil(units / BN_TILE)
    double n;                  // elements per channel
};

struct BnFwdArgs {
    const void* x; const float* gamma; const float* beta; const void* residual;      // x, residual, y: the element type T
    float* running_mean; float* running_var; long long* num_batches_tracked;
    void* y; float* save_mean; float* save_invstd;
    double* partial;           // [C][splits][2]
    int splits;                // workgroups per channel that wrote partials
    double momentum, eps;
    float slope;
};

struct BnBwdArgs {
    const void* x; const void* dy; const float* gamma; const float* beta; const float* save_mean; const float* save_invstd;   // x, dy, dx: T
    void* dx; float* dgamma; float* dbeta;
    double* partial;
    int splits;
    int training;
    float slope;
};

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// bf16_t, bf16_widen (exact) and bf16_round (to nearest even): bf16.h, shared with route.hip.

template <typename T>
__device__ __forceinline__ float load_elem(const void* __restrict__ p, size_t i) {
    if constexpr (sizeof(T) == 4) return static_cast<const float*>(p)[i];
    else return bf16_widen(static_cast<const bf16_t*>(p)[i]);
}

// THE I/O points: unit idx of V elements of type T <-> V floats
template <typename T, int V>
__device__ __forceinline__ void load_unit(const void* __restrict__ p, size_t idx, float (&o)[V]) {
    if constexpr (V == 1) {
        o[0] = load_elem<T>(p, idx);
    } else if constexpr (sizeof(T) == 4) {
        const f32x4 t = static_cast<const f32x4*>(p)[idx];
        o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
    } else {
        const u32x2 t = static_cast<const u32x2*>(p)[idx];
        o[0] = bf16_widen(t[0] & 0xffffu); o[1] = bf16_widen(t[0] >> 16);
        o[2] = bf16_widen(t[1] & 0xffffu); o[3] = bf16_widen(t[1] >> 16);
    }
}

template <typename T, int V>
__device__ __forceinline__ void store_unit(void* __restrict__ p, size_t idx, const float (&o)[V]) {
    if constexpr (V == 1) {
        if constexpr (sizeof(T) == 4) static_cast<float*>(p)[idx] = o[0];
        else static_cast<bf16_t*>(p)[idx] = (bf16_t)bf16_round(o[0]);
    } else if constexpr (sizeof(T) == 4) {
        static_cast<f32x4*>(p)[idx] = f32x4{o[0], o[1], o[2], o[3]};
    } else {
        static_cast<u32x2*>(p)[idx] = u32x2{bf16_round(o[0]) | (bf16_round(o[1]) << 16), bf16_round(o[2]) | (bf16_round(o[3]) << 16)};
    }
}

// index, in units, of unit u of channel c
__device__ __forceinline__ size_t unit_index(const BnGeom& g, int c, unsigned u) {
    const unsigned b = u / g.plane_units, p = u - b * g.plane_units;
    return ((size_t)b * g.C + c) * g.plane_units + p;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// (a, b) summed over the workgroup in a fixed order; every thread returns with the totals
__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();            // the slots may still be read from the previous call
    if (lane == 0) { lds[2 * w] = a; lds[2 * w + 1] = b; }
    __syncthreads();
    a = (lds[0] + lds[2]) + (lds[4] + lds[6]);
    b = (lds[1] + lds[3]) + (lds[5] + lds[7]);
}

// the channel's partials, written by `splits` workgroups, summed in a fixed order
__device__ __forceinline__ void sum_partials(const double* __restrict__ partial, int c, int splits, double& a, double& b, double* lds) {
    a = 0.0; b = 0.0;
    for (int i = threadIdx.x; i < splits; i += BN_THREADS) {
        a += partial[((size_t)c * splits + i) * 2];
        b += partial[((size_t)c * splits + i) * 2 + 1];
    }
    block_sum2(a, b, lds);
}

// BnChannel, split_hi_lo, bn_channel and bn_z (THE expression of z, in the forward and in the backward's mask): bn_channel.h,
// shared with the frozen block's epilogue in conv_fwd.hip.

// ---------------------------------------------------------------------------------------------------------------- forward
template <typename T, int V>
__device__ __forceinline__ void fwd_sums(const BnFwdArgs& a, const BnGeom& g, int c, int s, int S, float K, double& s1, double& s2) {
    s1 = 0.0; s2 = 0.0;
    const double Kd = (double)K;
    for (unsigned tile = s; tile < g.n_tiles; tile += S) {
        float v[BN_UNROLL][V];
        bool ok[BN_UNROLL];
#pragma unroll
        for (int k = 0; k < BN_UNROLL; ++k) {
            const unsigned u = tile * BN_TILE + k * BN_THREADS + threadIdx.x;
            ok[k] = u < g.units;
            if (ok[k]) load_unit<T, V>(a.x, unit_index(g, c, u), v[k]);
        }
#pragma unroll
        for (int k = 0; k < BN_UNROLL; ++k) {
            if (!ok[k]) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double d = (double)v[k][e] - Kd;
                s1 += d;
                s2 = fma(d, d, s2);
            }
        }
    }
}

template <typename T, int V>
__device__ __forceinline__ void fwd_apply(const BnFwdArgs& a, const BnGeom& g, int c, int s, int S, const BnChannel& ch) {
    const bool has_res = a.residual != nullptr;
    const double slope = (double)a.slope;
    for (unsigned tile = s; tile < g.n_tiles; tile += S) {
        float v[BN_UNROLL][V], r[BN_UNROLL][V];
        size_t idx[BN_UNROLL];
        bool ok[BN_UNROLL];
#pragma unroll
        for (int k = 0; k < BN_UNROLL; ++k) {
            const unsigned u = tile * BN_TILE + k * BN_THREADS + threadIdx.x;
            ok[k] = u < g.units;
            if (ok[k]) {
                idx[k] = unit_index(g, c, u);
                load_unit<T, V>(a.x, idx[k], v[k]);
                if (has_res) load_unit<T, V>(a.residual, idx[k], r[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < BN_UNROLL; ++k) {
            if (!ok[k]) continue;
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double z = bn_z(v[k][e], ch);
                double y = z > 0.0 ? z : z * slope;
                if (has_res) y = y + (double)r[k][e];
                o[e] = (float)y;                                // the only rounding to float32
            }
            store_unit<T, V>(a.y, idx[k], o);
        }
    }
}

template <typename T, int V>
__global__ void __launch_bounds__(BN_THREADS) bn_fwd_kernel(BnFwdArgs a, BnGeom g, int phase) {
    __shared__ double lds[8];
    const int s = blockIdx.x, S = gridDim.x, c = blockIdx.y;
    float mean_hi, mean_lo = 0.f, invstd_hi, invstd_lo;
    if (phase == BN_EVAL) {
        mean_hi = a.running_mean[c];
        split_hi_lo(1.0 / sqrt((double)a.running_var[c] + a.eps), invstd_hi, invstd_lo);
    } else {
        const float K = load_elem<T>(a.x, (size_t)c * g.plane_units * V);      // the channel's first element (image 0)
        double s1, s2;
        if (phase == BN_APPLY) {
            sum_partials(a.partial, c, a.splits, s1, s2, lds);
        } else {
            fwd_sums<T, V>(a, g, c, s, S, K, s1, s2);
            block_sum2(s1, s2, lds);
            if (phase == BN_STATS) {
                if (threadIdx.x == 0) {
                    a.partial[((size_t)c * S + s) * 2] = s1;
                    a.partial[((size_t)c * S + s) * 2 + 1] = s2;
                }
                return;
            }
        }
        const double shifted = s1 / g.n;
        const double mean_d = (double)K + shifted;
        double var_d = (s2 - s1 * shifted) / g.n;               // biased
        if (var_d < 0.0) var_d = 0.0;
        split_hi_lo(mean_d, mean_hi, mean_lo);
        split_hi_lo(1.0 / sqrt(var_d + a.eps), invstd_hi, invstd_lo);
        if (s == 0 && threadIdx.x == 0) {
            if (a.running_mean) a.running_mean[c] = (float)(a.momentum * mean_d + (1.0 - a.momentum) * (double)a.running_mean[c]);
            if (a.running_var) {
                const double unbiased = var_d * (g.n / (g.n - 1.0));
                a.running_var[c] = (float)(a.momentum * unbiased + (1.0 - a.momentum) * (double)a.running_var[c]);
            }
            if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
        }
    }
    if (s == 0 && threadIdx.x == 0) {
        a.save_mean[c] = mean_hi;   a.save_mean[g.C + c] = mean_lo;
        a.save_invstd[c] = invstd_hi; a.save_invstd[g.C + c] = invstd_lo;
    }
    const BnChannel ch = bn_channel(mean_hi, mean_lo, invstd_hi, invstd_lo, a.gamma[c], a.beta[c]);
    fwd_apply<T, V>(a, g, c, s, S, ch);
}

// ---------------------------------------------------------------------------------------------------------------- backward
template <typename T, int V>
__device__ __forceinline__ void bwd_sums(const BnBwdArgs& a, const BnGeom& g, int c, int s, int S, const BnChannel& ch, double& sb,
                                         double& sg) {
    sb = 0.0; sg = 0.0;
    const double slope = (double)a.slope;
    for (unsigned tile = s; tile < g.n_tiles; tile += S) {
        float v[BN_UNROLL][V], d[BN_UNROLL][V];
        bool ok[BN_UNROLL];
#pragma unroll
        for (int k = 0; k < BN_UNROLL; ++k) {
            const unsigned u = tile * BN_TILE + k * BN_THREADS + threadIdx.x;
            ok[k] = u < g.units;
            if (ok[k]) {
                const size_t idx = unit_index(g, c, u);
                load_unit<T, V>(a.x, idx, v[k]);
                load_unit<T, V>(a.dy, idx, d[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < BN_UNROLL; ++k) {
            if (!ok[k]) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double z = bn_z(v[k][e], ch);
                const double dz = z > 0.0 ? (double)d[k][e] : (double)d[k][e] * slope;
                sb += dz;
                sg = fma(dz, (double)v[k][e] - ch.mean, sg);
            }
        }
    }
}

template <typename T, int V>
__device__ __forceinline__ void bwd_apply(const BnBwdArgs& a, const BnGeom& g, int c, int s, int S, const BnChannel& ch, double c1,
                                          double c2) {
    const double slope = (double)a.slope;
    for (unsigned tile = s; tile < g.n_tiles; tile += S) {
        float v[BN_UNROLL][V], d[BN_UNROLL][V];
        size_t idx[BN_UNROLL];
        bool ok[BN_UNROLL];
#pragma unroll
        for (int k = 0; k < BN_UNROLL; ++k) {
            const unsigned u = tile * BN_TILE + k * BN_THREADS + threadIdx.x;
            ok[k] = u < g.units;
            if (ok[k]) {
                idx[k] = unit_index(g, c, u);
                load_unit<T, V>(a.x, idx[k], v[k]);
                load_unit<T, V>(a.dy, idx[k], d[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < BN_UNROLL; ++k) {
            if (!ok[k]) continue;
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double xm = (double)v[k][e] - ch.mean;
                const double z = fma(xm, ch.w, ch.beta);        // bn_z, with x - mean shared
                const double dz = z > 0.0 ? (double)d[k][e] : (double)d[k][e] * slope;
                const double t = fma(-xm, c2, dz - c1);
                o[e] = (float)(t * ch.w);
            }
            store_unit<T, V>(a.dx, idx[k], o);
        }
    }
}

template <typename T, int V>
__global__ void __launch_bounds__(BN_THREADS) bn_bwd_kernel(BnBwdArgs a, BnGeom g, int phase) {
    __shared__ double lds[8];
    const int s = blockIdx.x, S = gridDim.x, c = blockIdx.y;
    const BnChannel ch = bn_channel(a.save_mean[c], a.save_mean[g.C + c], a.save_invstd[c], a.save_invstd[g.C + c], a.gamma[c], a.beta[c]);
    double sb, sg;
    if (phase == BN_APPLY) {
        sum_partials(a.partial, c, a.splits, sb, sg, lds);
    } else {
        bwd_sums<T, V>(a, g, c, s, S, ch, sb, sg);
        block_sum2(sb, sg, lds);
        if (phase == BN_STATS) {
            if (threadIdx.x == 0) {
                a.partial[((size_t)c * S + s) * 2] = sb;
                a.partial[((size_t)c * S + s) * 2 + 1] = sg;
            }
            return;
        }
    }
    // sg = sum dz * (x - mean): dgamma = sg * invstd, and xhat * dgamma / M = (x - mean) * (sg * invstd^2 / M)
    if (s == 0 && threadIdx.x == 0) {
        a.dbeta[c] = (float)sb;
        a.dgamma[c] = (float)(sg * ch.invstd);
    }
    if (!a.dx) return;
    const double c1 = a.training ? sb / g.n : 0.0;
    const double c2 = a.training ? sg * ch.invstd * ch.invstd / g.n : 0.0;
    bwd_apply<T, V>(a, g, c, s, S, ch, c1, c2);
}

// ---------------------------------------------------------------------------------------------------------------- several ranks
// The same two phases with the cross-rank exchange between them (SyncBatchNorm).  Each rank reduces its own slice of the batch to a
// per-channel RECORD of doubles [3][C] = (n, mean, M2 = sum (x - mean)^2); the caller all-gathers the records, and every rank merges
// the SAME R records in rank order with the pairwise formula, so the statistics and the running buffers have the same bits on every
// rank without a broadcast.  The backward exchanges (sum dz, sum dz * xhat) the same way.  With R == 1 every expression below is the
// unsynchronised kernel's: the record holds K + s1/n and s2 - s1 * (s1/n), and var = M2 / n.
template <typename T, int V>
__global__ void __launch_bounds__(BN_THREADS) bn_sync_stats_kernel(BnFwdArgs a, BnGeom g, double* __restrict__ record) {
    __shared__ double lds[8];
    const int c = blockIdx.y;
    const float K = load_elem<T>(a.x, (size_t)c * g.plane_units * V);          // the channel's first element on this rank
    double s1, s2;
    if (a.splits > 0) {
        sum_partials(a.partial, c, a.splits, s1, s2, lds);
    } else {
        fwd_sums<T, V>(a, g, c, 0, 1, K, s1, s2);
        block_sum2(s1, s2, lds);
    }
    if (threadIdx.x != 0) return;
    const double shifted = s1 / g.n;
    double m2 = s2 - s1 * shifted;
    if (m2 < 0.0) m2 = 0.0;
    record[c] = g.n;
    record[g.C + c] = (double)K + shifted;
    record[2 * g.C + c] = m2;
}

template <typename T, int V>
__global__ void __launch_bounds__(BN_THREADS) bn_sync_fwd_kernel(BnFwdArgs a, BnGeom g, const double* __restrict__ records, int R,
                                                                 double* __restrict__ n_total_out) {
    const int s = blockIdx.x, S = gridDim.x, c = blockIdx.y;
    // every workgroup of every rank merges the same doubles in the same order
    double n = records[c], mean_d = records[g.C + c], m2 = records[2 * g.C + c];
    for (int r = 1; r < R; ++r) {
        const double* rec = records + (size_t)r * 3 * g.C;
        const double nr = rec[c], delta = rec[g.C + c] - mean_d, tot = n + nr;
        m2 += rec[2 * g.C + c] + delta * delta * n * nr / tot;
        mean_d += delta * nr / tot;
        n = tot;
    }
    const double var_d = m2 / n;                                    // biased
    float mean_hi, mean_lo, invstd_hi, invstd_lo;
    split_hi_lo(mean_d, mean_hi, mean_lo);
    split_hi_lo(1.0 / sqrt(var_d + a.eps), invstd_hi, invstd_lo);
    if (s == 0 && threadIdx.x == 0) {
        if (a.running_mean) a.running_mean[c] = (float)(a.momentum * mean_d + (1.0 - a.momentum) * (double)a.running_mean[c]);
        if (a.running_var) {
            const double unbiased = var_d * (n / (n - 1.0));
            a.running_var[c] = (float)(a.momentum * unbiased + (1.0 - a.momentum) * (double)a.running_var[c]);
        }
        if (c == 0) {
            if (a.num_batches_tracked) *a.num_batches_tracked += 1;
            *n_total_out = n;
        }
        a.save_mean[c] = mean_hi;   a.save_mean[g.C + c] = mean_lo;
        a.save_invstd[c] = invstd_hi; a.save_invstd[g.C + c] = invstd_lo;
    }
    const BnChannel ch = bn_channel(mean_hi, mean_lo, invstd_hi, invstd_lo, a.gamma[c], a.beta[c]);
    fwd_apply<T, V>(a, g, c, s, S, ch);
}

// sums: [2][C] doubles (sum dz, sum dz * xhat) of this rank; dgamma / dbeta are this rank's own, as in torch's SyncBatchNorm
template <typename T, int V>
__global__ void __launch_bounds__(BN_THREADS) bn_sync_bwd_sums_kernel(BnBwdArgs a, BnGeom g, double* __restrict__ sums) {
    __shared__ double lds[8];
    const int c = blockIdx.y;
    const BnChannel ch = bn_channel(a.save_mean[c], a.save_mean[g.C + c], a.save_invstd[c], a.save_invstd[g.C + c], a.gamma[c], a.beta[c]);
    double sb, sg;
    if (a.splits > 0) {
        sum_partials(a.partial, c, a.splits, sb, sg, lds);
    } else {
        bwd_sums<T, V>(a, g, c, 0, 1, ch, sb, sg);
        block_sum2(sb, sg, lds);
    }
    if (threadIdx.x != 0) return;
    const double dg = sg * ch.invstd;                               // sg = sum dz * (x - mean)
    sums[c] = sb;
    sums[g.C + c] = dg;
    a.dbeta[c] = (float)sb;
    a.dgamma[c] = (float)dg;
}

template <typename T, int V>
__global__ void __launch_bounds__(BN_THREADS) bn_sync_dx_kernel(BnBwdArgs a, BnGeom g, const double* __restrict__ sums_all, int R,
                                                                const double* __restrict__ n_total) {
    const int s = blockIdx.x, S = gridDim.x, c = blockIdx.y;
    const BnChannel ch = bn_channel(a.save_mean[c], a.save_mean[g.C + c], a.save_invstd[c], a.save_invstd[g.C + c], a.gamma[c], a.beta[c]);
    double sb = sums_all[c], dg = sums_all[g.C + c];
    for (int r = 1; r < R; ++r) {
        sb += sums_all[(size_t)r * 2 * g.C + c];
        dg += sums_all[(size_t)r * 2 * g.C + g.C + c];
    }
    const double n = *n_total;
    // xhat * dgamma / N = (x - mean) * (dgamma * invstd / N)
    bwd_apply<T, V>(a, g, c, s, S, ch, sb / n, dg * ch.invstd / n);
}

// workgroups per channel for the two-launch form
static int bn_splits(unsigned n_tiles, int C) {
    int per = BN_MAX_BLOCKS / C;
    if (per < 1) per = 1;
    return (unsigned)per < n_tiles ? per : (int)n_tiles;
}

static bool bn_geometry(int B, int C, int H, int W, int V, BnGeom* g) {
    const long long hw = (long long)H * W, m = hw * B;
    if (B < 1 || C < 1 || C > 65535 || H < 1 || W < 1 || m >= (1ll << 31) - BN_TILE) return false;
    g->C = C;
    g->plane_units = (unsigned)(hw / V);
    g->units = (unsigned)(m / V);
    g->n_tiles = (g->units + BN_TILE - 1) / BN_TILE;
    g->n = (double)m;
    return true;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a 4-element unit of T may be read at p (a null tensor is not read)
template <typename T>
static bool unit_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0; }

#define BN_LAUNCH(kernel, vec, grid, st, ...)                                                                      \
    do {                                                                                                           \
        if (vec) hipLaunchKernelGGL((om::kernel<T, 4>), grid, dim3(om::BN_THREADS), 0, st, __VA_ARGS__);           \
        else hipLaunchKernelGGL((om::kernel<T, 1>), grid, dim3(om::BN_THREADS), 0, st, __VA_ARGS__);               \
    } while (0)

// The entry points' bodies for the element type T; `who` is the entry point's name in the messages.
template <typename T>
static int bn_act_forward(const char* who, const void* x, int B, int C, int H, int W, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, int training, double momentum,
                          double eps, float slope, const void* residual, void* y, float* save_mean, float* save_invstd,
                          void* workspace, size_t ws_bytes, om_stream stream) {
    OM_REQUIRE(x && gamma && beta && y && save_mean && save_invstd, OM_EINVAL, "%s: null pointer", who);
    OM_REQUIRE(y != x && y != residual, OM_EINVAL, "%s: y must not alias x or the residual (x is what the backward reads)", who);
    OM_REQUIRE(training || (running_mean && running_var), OM_EINVAL, "%s: eval mode needs the running statistics", who);
    OM_REQUIRE(eps > 0.0 && momentum >= 0.0 && momentum <= 1.0, OM_EINVAL, "%s: eps %g, momentum %g", who, eps, momentum);
    const bool vec = ((long long)H * W) % 4 == 0 && unit_aligned<T>(x) && unit_aligned<T>(y) && unit_aligned<T>(residual);
    BnGeom g;
    OM_REQUIRE(bn_geometry(B, C, H, W, vec ? 4 : 1, &g), OM_EINVAL, "%s: shape [%d,%d,%d,%d] (C <= 65535, B*H*W < 2^31)", who, B, C, H, W);
    OM_REQUIRE(!training || g.n >= 2.0, OM_EINVAL, "%s: training needs more than 1 value per channel, got shape [%d,%d,%d,%d]", who,
               B, C, H, W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    BnFwdArgs a;
    a.x = x; a.gamma = gamma; a.beta = beta; a.residual = residual;
    a.running_mean = running_mean; a.running_var = running_var; a.num_batches_tracked = reinterpret_cast<long long*>(num_batches_tracked);
    a.y = y; a.save_mean = save_mean; a.save_invstd = save_invstd;
    a.partial = static_cast<double*>(workspace); a.splits = 0;
    a.momentum = momentum; a.eps = eps; a.slope = slope;
    const int S = bn_splits(g.n_tiles, C);
    if (!training) {
        BN_LAUNCH(bn_fwd_kernel, vec, dim3(S, C), st, a, g, (int)BN_EVAL);
    } else if (g.n <= (double)BN_FUSED_MAX || S == 1) {
        BN_LAUNCH(bn_fwd_kernel, vec, dim3(1, C), st, a, g, (int)BN_FUSED);
    } else {
        OM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= (size_t)C * S * 2 * sizeof(double), OM_EINVAL,
                   "%s: workspace of %zu bytes, need %zu (16-byte aligned)", who, ws_bytes, (size_t)C * S * 2 * sizeof(double));
        a.splits = S;
        BN_LAUNCH(bn_fwd_kernel, vec, dim3(S, C), st, a, g, (int)BN_STATS);
        BN_LAUNCH(bn_fwd_kernel, vec, dim3(S, C), st, a, g, (int)BN_APPLY);
    }
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

template <typename T>
static int bn_act_backward(const char* who, const void* x, const void* dy, int B, int C, int H, int W, const float* gamma,
                           const float* beta, const float* save_mean, const float* save_invstd, int training, float slope, void* dx,
                           float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, om_stream stream) {
    OM_REQUIRE(x && dy && gamma && beta && save_mean && save_invstd && dgamma && dbeta, OM_EINVAL, "%s: null pointer", who);
    OM_REQUIRE(dx != x, OM_EINVAL, "%s: dx must not alias x", who);
    const bool vec = ((long long)H * W) % 4 == 0 && unit_aligned<T>(x) && unit_aligned<T>(dy) && unit_aligned<T>(dx);
    BnGeom g;
    OM_REQUIRE(bn_geometry(B, C, H, W, vec ? 4 : 1, &g), OM_EINVAL, "%s: shape [%d,%d,%d,%d] (C <= 65535, B*H*W < 2^31)", who, B, C, H, W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    BnBwdArgs a;
    a.x = x; a.dy = dy; a.gamma = gamma; a.beta = beta; a.save_mean = save_mean; a.save_invstd = save_invstd;
    a.dx = dx; a.dgamma = dgamma; a.dbeta = dbeta;
    a.partial = static_cast<double*>(workspace); a.splits = 0;
    a.training = training ? 1 : 0; a.slope = slope;
    const int S = bn_splits(g.n_tiles, C);
    if (g.n <= (double)BN_FUSED_MAX || S == 1) {
        BN_LAUNCH(bn_bwd_kernel, vec, dim3(1, C), st, a, g, (int)BN_FUSED);
    } else {
        OM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= (size_t)C * S * 2 * sizeof(double), OM_EINVAL,
                   "%s: workspace of %zu bytes, need %zu (16-byte aligned)", who, ws_bytes, (size_t)C * S * 2 * sizeof(double));
        a.splits = S;
        BN_LAUNCH(bn_bwd_kernel, vec, dim3(S, C), st, a, g, (int)BN_STATS);
        BN_LAUNCH(bn_bwd_kernel, vec, dim3(dx ? S : 1, C), st, a, g, (int)BN_APPLY);       // without dx only the per-channel sums are finalised
    }
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

template <typename T>
static int bn_sync_stats(const char* who, const void* x, int B, int C, int H, int W, double* record, void* workspace, size_t ws_bytes,
                         om_stream stream) {
    OM_REQUIRE(x && record, OM_EINVAL, "%s: null pointer", who);
    const bool vec = ((long long)H * W) % 4 == 0 && unit_aligned<T>(x);
    BnGeom g;
    OM_REQUIRE(bn_geometry(B, C, H, W, vec ? 4 : 1, &g), OM_EINVAL, "%s: shape [%d,%d,%d,%d] (C <= 65535, B*H*W < 2^31)", who, B, C, H, W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    BnFwdArgs a = {};
    a.x = x;
    a.partial = static_cast<double*>(workspace); a.splits = 0;
    const int S = bn_splits(g.n_tiles, C);
    if (!(g.n <= (double)BN_FUSED_MAX || S == 1)) {
        OM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= (size_t)C * S * 2 * sizeof(double), OM_EINVAL,
                   "%s: workspace of %zu bytes, need %zu (16-byte aligned)", who, ws_bytes, (size_t)C * S * 2 * sizeof(double));
        BN_LAUNCH(bn_fwd_kernel, vec, dim3(S, C), st, a, g, (int)BN_STATS);
        a.splits = S;
    }
    BN_LAUNCH(bn_sync_stats_kernel, vec, dim3(1, C), st, a, g, record);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

template <typename T>
static int bn_sync_forward(const char* who, const void* x, int B, int C, int H, int W, const double* records, int R, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, double momentum,
                           double eps, float slope, const void* residual, void* y, float* save_mean, float* save_invstd,
                           double* n_total_out, om_stream stream) {
    OM_REQUIRE(x && records && gamma && beta && y && save_mean && save_invstd && n_total_out, OM_EINVAL, "%s: null pointer", who);
    OM_REQUIRE(R >= 1, OM_EINVAL, "%s: R = %d ranks, need at least 1", who, R);
    OM_REQUIRE(y != x && y != residual, OM_EINVAL, "%s: y must not alias x or the residual (x is what the backward reads)", who);
    OM_REQUIRE(eps > 0.0 && momentum >= 0.0 && momentum <= 1.0, OM_EINVAL, "%s: eps %g, momentum %g", who, eps, momentum);
    const bool vec = ((long long)H * W) % 4 == 0 && unit_aligned<T>(x) && unit_aligned<T>(y) && unit_aligned<T>(residual);
    BnGeom g;
    OM_REQUIRE(bn_geometry(B, C, H, W, vec ? 4 : 1, &g), OM_EINVAL, "%s: shape [%d,%d,%d,%d] (C <= 65535, B*H*W < 2^31)", who, B, C, H, W);
    // every rank contributes at least one value per channel, so N >= B*H*W + R - 1
    OM_REQUIRE(g.n + (double)(R - 1) >= 2.0, OM_EINVAL,
               "%s: training needs more than 1 value per channel over all ranks, got shape [%d,%d,%d,%d] on %d rank(s)", who, B, C, H, W, R);
    hipStream_t st = static_cast<hipStream_t>(stream);
    BnFwdArgs a = {};
    a.x = x; a.gamma = gamma; a.beta = beta; a.residual = residual;
    a.running_mean = running_mean; a.running_var = running_var; a.num_batches_tracked = reinterpret_cast<long long*>(num_batches_tracked);
    a.y = y; a.save_mean = save_mean; a.save_invstd = save_invstd;
    a.momentum = momentum; a.eps = eps; a.slope = slope;
    int S = bn_splits(g.n_tiles, C);
    if (g.n <= (double)BN_FUSED_MAX) S = 1;
    BN_LAUNCH(bn_sync_fwd_kernel, vec, dim3(S, C), st, a, g, records, R, n_total_out);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

template <typename T>
static int bn_sync_backward_sums(const char* who, const void* x, const void* dy, int B, int C, int H, int W, const float* gamma,
                                 const float* beta, const float* save_mean, const float* save_invstd, float slope, double* sums,
                                 float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, om_stream stream) {
    OM_REQUIRE(x && dy && gamma && beta && save_mean && save_invstd && sums && dgamma && dbeta, OM_EINVAL, "%s: null pointer", who);
    const bool vec = ((long long)H * W) % 4 == 0 && unit_aligned<T>(x) && unit_aligned<T>(dy);
    BnGeom g;
    OM_REQUIRE(bn_geometry(B, C, H, W, vec ? 4 : 1, &g), OM_EINVAL, "%s: shape [%d,%d,%d,%d] (C <= 65535, B*H*W < 2^31)", who, B, C, H, W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    BnBwdArgs a = {};
    a.x = x; a.dy = dy; a.gamma = gamma; a.beta = beta; a.save_mean = save_mean; a.save_invstd = save_invstd;
    a.dgamma = dgamma; a.dbeta = dbeta;
    a.partial = static_cast<double*>(workspace); a.splits = 0;
    a.training = 1; a.slope = slope;
    const int S = bn_splits(g.n_tiles, C);
    if (!(g.n <= (double)BN_FUSED_MAX || S == 1)) {
        OM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= (size_t)C * S * 2 * sizeof(double), OM_EINVAL,
                   "%s: workspace of %zu bytes, need %zu (16-byte aligned)", who, ws_bytes, (size_t)C * S * 2 * sizeof(double));
        BN_LAUNCH(bn_bwd_kernel, vec, dim3(S, C), st, a, g, (int)BN_STATS);
        a.splits = S;
    }
    BN_LAUNCH(bn_sync_bwd_sums_kernel, vec, dim3(1, C), st, a, g, sums);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

template <typename T>
static int bn_sync_backward_dx(const char* who, const void* x, const void* dy, int B, int C, int H, int W, const float* gamma,
                               const float* beta, const float* save_mean, const float* save_invstd, float slope, const double* sums_all,
                               int R, const double* n_total, void* dx, om_stream stream) {
    OM_REQUIRE(x && dy && gamma && beta && save_mean && save_invstd && sums_all && n_total && dx, OM_EINVAL, "%s: null pointer", who);
    OM_REQUIRE(R >= 1, OM_EINVAL, "%s: R = %d ranks, need at least 1", who, R);
    OM_REQUIRE(dx != x, OM_EINVAL, "%s: dx must not alias x", who);
    const bool vec = ((long long)H * W) % 4 == 0 && unit_aligned<T>(x) && unit_aligned<T>(dy) && unit_aligned<T>(dx);
    BnGeom g;
    OM_REQUIRE(bn_geometry(B, C, H, W, vec ? 4 : 1, &g), OM_EINVAL, "%s: shape [%d,%d,%d,%d] (C <= 65535, B*H*W < 2^31)", who, B, C, H, W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    BnBwdArgs a = {};
    a.x = x; a.dy = dy; a.gamma = gamma; a.beta = beta; a.save_mean = save_mean; a.save_invstd = save_invstd;
    a.dx = dx;
    a.training = 1; a.slope = slope;
    int S = bn_splits(g.n_tiles, C);
    if (g.n <= (double)BN_FUSED_MAX) S = 1;
    BN_LAUNCH(bn_sync_dx_kernel, vec, dim3(S, C), st, a, g, sums_all, R, n_total);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

#undef BN_LAUNCH

}  // namespace om

extern "C" {

size_t om_bn_act_workspace_bytes(int B, int C, int H, int W) {
    om::BnGeom g;
    if (!om::bn_geometry(B, C, H, W, 1, &g)) return 0;
    return (size_t)C * om::bn_splits(g.n_tiles, C) * 2 * sizeof(double);
}

int om_bn_act_forward(const float* x, int B, int C, int H, int W, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, int training, double momentum, double eps, float slope,
                      const float* residual, float* y, float* save_mean, float* save_invstd, void* workspace, size_t ws_bytes,
                      om_stream stream) {
    return om::bn_act_forward<float>("om_bn_act_forward", x, B, C, H, W, gamma, beta, running_mean, running_var, num_batches_tracked,
                                     training, momentum, eps, slope, residual, y, save_mean, save_invstd, workspace, ws_bytes, stream);
}

int om_bn_act_forward_bf16(const uint16_t* x, int B, int C, int H, int W, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, int64_t* num_batches_tracked, int training, double momentum, double eps, float slope,
                           const uint16_t* residual, uint16_t* y, float* save_mean, float* save_invstd, void* workspace,
                           size_t ws_bytes, om_stream stream) {
    return om::bn_act_forward<om::bf16_t>("om_bn_act_forward_bf16", x, B, C, H, W, gamma, beta, running_mean, running_var,
                                          num_batches_tracked, training, momentum, eps, slope, residual, y, save_mean, save_invstd,
                                          workspace, ws_bytes, stream);
}

int om_bn_act_backward(const float* x, const float* dy, int B, int C, int H, int W, const float* gamma, const float* beta,
                       const float* save_mean, const float* save_invstd, int training, float slope, float* dx, float* dgamma,
                       float* dbeta, void* workspace, size_t ws_bytes, om_stream stream) {
    return om::bn_act_backward<float>("om_bn_act_backward", x, dy, B, C, H, W, gamma, beta, save_mean, save_invstd, training, slope, dx,
                                      dgamma, dbeta, workspace, ws_bytes, stream);
}

int om_bn_act_backward_bf16(const uint16_t* x, const uint16_t* dy, int B, int C, int H, int W, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, int training, float slope, uint16_t* dx, float* dgamma,
                            float* dbeta, void* workspace, size_t ws_bytes, om_stream stream) {
    return om::bn_act_backward<om::bf16_t>("om_bn_act_backward_bf16", x, dy, B, C, H, W, gamma, beta, save_mean, save_invstd, training,
                                           slope, dx, dgamma, dbeta, workspace, ws_bytes, stream);
}

int om_bn_sync_stats(const float* x, int B, int C, int H, int W, double* record, void* workspace, size_t ws_bytes, om_stream stream) {
    return om::bn_sync_stats<float>("om_bn_sync_stats", x, B, C, H, W, record, workspace, ws_bytes, stream);
}

int om_bn_sync_stats_bf16(const uint16_t* x, int B, int C, int H, int W, double* record, void* workspace, size_t ws_bytes,
                          om_stream stream) {
    return om::bn_sync_stats<om::bf16_t>("om_bn_sync_stats_bf16", x, B, C, H, W, record, workspace, ws_bytes, stream);
}

int om_bn_sync_forward(const float* x, int B, int C, int H, int W, const double* records, int R, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked, double momentum, double eps, float slope,
                       const float* residual, float* y, float* save_mean, float* save_invstd, double* n_total_out, om_stream stream) {
    return om::bn_sync_forward<float>("om_bn_sync_forward", x, B, C, H, W, records, R, gamma, beta, running_mean, running_var,
                                      num_batches_tracked, momentum, eps, slope, residual, y, save_mean, save_invstd, n_total_out, stream);
}

int om_bn_sync_forward_bf16(const uint16_t* x, int B, int C, int H, int W, const double* records, int R, const float* gamma,
                            const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, double momentum,
                            double eps, float slope, const uint16_t* residual, uint16_t* y, float* save_mean, float* save_invstd,
                            double* n_total_out, om_stream stream) {
    return om::bn_sync_forward<om::bf16_t>("om_bn_sync_forward_bf16", x, B, C, H, W, records, R, gamma, beta, running_mean, running_var,
                                           num_batches_tracked, momentum, eps, slope, residual, y, save_mean, save_invstd, n_total_out,
                                           stream);
}

int om_bn_sync_backward_sums(const float* x, const float* dy, int B, int C, int H, int W, const float* gamma, const float* beta,
                             const float* save_mean, const float* save_invstd, float slope, double* sums, float* dgamma, float* dbeta,
                             void* workspace, size_t ws_bytes, om_stream stream) {
    return om::bn_sync_backward_sums<float>("om_bn_sync_backward_sums", x, dy, B, C, H, W, gamma, beta, save_mean, save_invstd, slope,
                                            sums, dgamma, dbeta, workspace, ws_bytes, stream);
}

int om_bn_sync_backward_sums_bf16(const uint16_t* x, const uint16_t* dy, int B, int C, int H, int W, const float* gamma,
                                  const float* beta, const float* save_mean, const float* save_invstd, float slope, double* sums,
                                  float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, om_stream stream) {
    return om::bn_sync_backward_sums<om::bf16_t>("om_bn_sync_backward_sums_bf16", x, dy, B, C, H, W, gamma, beta, save_mean, save_invstd,
                                                 slope, sums, dgamma, dbeta, workspace, ws_bytes, stream);
}

int om_bn_sync_backward_dx(const float* x, const float* dy, int B, int C, int H, int W, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_invstd, float slope, const double* sums_all, int R,
                           const double* n_total, float* dx, om_stream stream) {
    return om::bn_sync_backward_dx<float>("om_bn_sync_backward_dx", x, dy, B, C, H, W, gamma, beta, save_mean, save_invstd, slope,
                                          sums_all, R, n_total, dx, stream);
}

int om_bn_sync_backward_dx_bf16(const uint16_t* x, const uint16_t* dy, int B, int C, int H, int W, const float* gamma,
                                const float* beta, const float* save_mean, const float* save_invstd, float slope,
                                const double* sums_all, int R, const double* n_total, uint16_t* dx, om_stream stream) {
    return om::bn_sync_backward_dx<om::bf16_t>("om_bn_sync_backward_dx_bf16", x, dy, B, C, H, W, gamma, beta, save_mean, save_invstd,
                                               slope, sums_all, R, n_total, dx, stream);
}

}  // extern "C"
