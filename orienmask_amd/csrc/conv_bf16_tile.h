// The bf16 convolution tile on v_mfma_f32_32x32x16_bf16 that conv_fwd_bf16.hip (the forward) and conv_grad_bf16.hip (the data gradient
// at stride 1, which is the forward convolution of dy with the weight transposed and flipped) share: conv_bf16_kernel, its arguments
// and its launch rule.  The head of conv_fwd_bf16.hip describes the tile, the k order, the LDS images and the chain.  WT selects the
// weight gather only: false reads w[co][ci][tap] of a [cout,cin,k,k] weight; true reads w[ci][co][taps-1-tap] of a [cin,cout,k,k]
// one (the kernel's cin = the real weight's cout), so the kernel's row `co` is the real input channel.  Both round with bf16_round
// while packing.  Nothing else differs, so what the forward guarantees of y (order a function of the geometry only) holds of dx.
#pragma once
#include "conv_train.h"
#include "bn_channel.h"
#include "bf16.h"

namespace om {

constexpr int CB_THREADS = 256;
constexpr int CB_MT = 128;              // pixels of a tile: four waves of 32

enum { EPB_BIAS = 0, EPB_FROZEN = 1 };

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct FwdBf16Args {
    const bf16_t* x; const float* w; const float* bias; void* y;
    int y_is_f32;
    int cin, cout, H, W, Ho, Wo, HoWo;
    int P;                      // B * Ho * Wo
    // EPB_FROZEN only
    const float* gamma; const float* beta; const float* running_mean; const float* running_var; const bf16_t* residual;
    double eps;
    float slope;
};

__device__ __forceinline__ uint32_t pack2(uint32_t lo, uint32_t hi) { return lo | (hi << 16); }

template <int TN, int KS, int S, int EPI, bool WT = false>
__global__ void __launch_bounds__(CB_THREADS, 2) conv_bf16_kernel(const FwdBf16Args a) {
    constexpr int TAPS = KS * KS, NT = TN * 32;
    constexpr int KSTEPS = KS == 1 ? 4 : 1, KC = 16 * KSTEPS;       // input channels per staged chunk
    constexpr int NROW = KS == 1 ? 1 : (S == 1 ? 3 : 6);            // LDS rows per k-step
    constexpr int SEG = KS == 1 ? CB_MT : (S == 1 ? CB_MT + 2 : CB_MT + 1);
    constexpr int POSN = NROW * SEG;                                // staged positions
    constexpr int XU = (KC / 8) * POSN, NIX = (XU + CB_THREADS - 1) / CB_THREADS;       // units of 8 channels of a position
    constexpr int WBLK = NT * 2 + 1;                                // 16-byte words of a tap block (one to spare)
    constexpr int WU = (KC / 8) * TAPS * NT, NIW = (WU + CB_THREADS - 1) / CB_THREADS;  // units of 8 channels of a (co, tap)
    __shared__ long long s_off[POSN];
    __shared__ uint4 s_x[KSTEPS * POSN * 2];                        // [k-step][position][half of 8 ci]
    __shared__ uint4 s_w[KSTEPS * TAPS * WBLK];                     // [k-step][tap][co][half of 8 ci]
    __shared__ BnAffine s_ch[EPI == EPB_FROZEN ? NT : 1];           // the record of channel co0 + t

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 31, fk = lane >> 5;
    const long long g0 = (long long)blockIdx.x * CB_MT;
    const int co0 = blockIdx.y * NT;
    const size_t hw = (size_t)a.H * a.W;

    // the position table (conv_fwd.hip's)
    for (int p = tid; p < POSN; p += CB_THREADS) {
        const int row = p / SEG, j = p - row * SEG;
        int r, odd = 0;
        long long g;
        if (KS == 1) { r = 0; g = g0 + j; }
        else if (S == 1) { r = row; g = g0 + j - 1; }
        else { r = row >> 1; odd = row & 1; g = g0 + j - odd; }
        long long off = -1;
        if (g >= 0 && g < a.P && !(S == 2 && !odd && j == CB_MT)) {      // (the E rows have one position to spare)
            const int b = (int)(g / a.HoWo), q = (int)(g - (long long)b * a.HoWo);
            const int oy = q / a.Wo, ox = q - oy * a.Wo;
            const int iy = oy * S + r - KS / 2, ix = S == 1 ? ox : 2 * ox + odd;
            if ((unsigned)iy < (unsigned)a.H && ix < a.W) off = (long long)((size_t)b * a.cin * hw + (size_t)iy * a.W + ix);
        }
        s_off[p] = off;
    }

    if constexpr (EPI == EPB_FROZEN) {
        if (tid < NT) {
            const int co = co0 + tid;
            BnAffine ch = {};
            if (co < a.cout) ch = bn_affine_eval(a.running_mean[co], a.running_var[co], a.eps, a.gamma[co], a.beta[co]);
            s_ch[tid] = ch;
        }
    }

    // this lane's pixel and the column taps that stay in its row
    const long long g = g0 + wave * 32 + fi;
    const bool live = g < a.P;
    const int b = live ? (int)(g / a.HoWo) : 0, q = live ? (int)(g - (long long)b * a.HoWo) : 0;
    const int ox = q % a.Wo;
    const bool ok0 = ox >= 1, ok2 = S == 2 || ox + 1 < a.Wo;

    // two levels: the matrix instruction's chain holds one staged chunk (acc), the chunks are added in chunk order (tot)
    f32x16 acc[TN], tot[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n) { clear16(acc[n]); clear16(tot[n]); }

    uint4 px[NIX], pw[NIW];     // the chunk in flight, as it will lie in LDS
    auto load = [&](int ci0) {
#pragma unroll
        for (int i = 0; i < NIX; ++i) {
            const int u = tid + i * CB_THREADS;
            const int oct = u / POSN, p = u - oct * POSN;
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0u;
            if (u < XU) {
                const long long off = s_off[p];
                const int ci = ci0 + oct * 8;
                if (off >= 0) {
                    const bf16_t* src = a.x + (size_t)off + (size_t)ci * hw;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (ci + j < a.cin) v[j] = src[(size_t)j * hw];
                }
            }
            px[i] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
        }
#pragma unroll
        for (int i = 0; i < NIW; ++i) {
            const int u = tid + i * CB_THREADS;
            const int tap = u % TAPS, rest = u / TAPS;
            const int cl = rest % NT, oct = rest / NT;
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0u;
            const int co = co0 + cl, ci = ci0 + oct * 8;
            if (u < WU && co < a.cout) {
                // WT: the weight is [cin][cout][taps] and is read transposed and flipped (the head of this file)
                const float* src = WT ? a.w + ((size_t)ci * a.cout + co) * TAPS + (TAPS - 1 - tap)
                                      : a.w + ((size_t)co * a.cin + ci) * TAPS + tap;
                const size_t cstep = WT ? (size_t)a.cout * TAPS : (size_t)TAPS;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (ci + j < a.cin) v[j] = bf16_round(src[(size_t)j * cstep]);
            }
            pw[i] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < NIX; ++i) {
            const int u = tid + i * CB_THREADS;
            const int oct = u / POSN, p = u - oct * POSN;
            if (u < XU) s_x[((oct >> 1) * POSN + p) * 2 + (oct & 1)] = px[i];
        }
#pragma unroll
        for (int i = 0; i < NIW; ++i) {
            const int u = tid + i * CB_THREADS;
            const int tap = u % TAPS, rest = u / TAPS;
            const int cl = rest % NT, oct = rest / NT;
            if (u < WU) s_w[((oct >> 1) * TAPS + tap) * WBLK + cl * 2 + (oct & 1)] = pw[i];
        }
    };

    __syncthreads();            // the table
    load(0);
    for (int ci0 = 0; ci0 < a.cin; ci0 += KC) {
        store();
        __syncthreads();
        if (ci0 + KC < a.cin) load(ci0 + KC);               // in flight under this chunk's matrix instructions
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
#pragma unroll
            for (int r = 0; r < KS; ++r) {
#pragma unroll
                for (int c = 0; c < KS; ++c) {
                    // the LDS row and shift of column tap c (see the head of conv_fwd.hip)
                    const int row = KS == 1 ? 0 : (S == 1 ? r : 2 * r + (c != 1 ? 1 : 0));
                    const int shift = KS == 1 ? 0 : (S == 1 ? c : (c == 2 ? 1 : 0));
                    const bool ok = KS == 1 || c == 1 || (c == 0 ? ok0 : ok2);
                    uint4 bq = s_x[(ks * POSN + row * SEG + shift + wave * 32 + fi) * 2 + fk];
                    if (!ok) bq = make_uint4(0u, 0u, 0u, 0u);
                    const bf16x8 bv = __builtin_bit_cast(bf16x8, bq);
                    const uint4* wp = s_w + (ks * TAPS + r * KS + c) * WBLK + fi * 2 + fk;
#pragma unroll
                    for (int n = 0; n < TN; ++n)
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wp[n * 64]), bv, acc[n], 0, 0, 0);
                }
            }
        }
        // the chunk's chain ends here: one float32 add per element into the second level (0 + acc is exact for the first chunk)
#pragma unroll
        for (int n = 0; n < TN; ++n) { tot[n] += acc[n]; clear16(acc[n]); }
        __syncthreads();        // the chunk is consumed: the next store may overwrite it
    }
    // D layout: column (pixel) = lane & 31, row (co) = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)
    if (!live) return;
    const size_t base = (size_t)b * a.cout * a.HoWo + q;
    if constexpr (EPI == EPB_FROZEN) {
        bf16_t* o = static_cast<bf16_t*>(a.y) + base;
        const bool has_res = a.residual != nullptr;
        const bf16_t* rp = has_res ? a.residual + base : nullptr;
        const double slope = (double)a.slope;
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            // 16 loads in flight, under one uniform branch: a channel beyond cout reads the last channel's plane (in bounds) and
            // is never stored
            float res[16];
            if (has_res) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + n * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
                    res[r] = bf16_widen(rp[(size_t)(co < a.cout ? co : a.cout - 1) * a.HoWo]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) res[r] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cl = n * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
                const BnAffine ch = s_ch[cl];
                if (co0 + cl < a.cout)
                    o[(size_t)(co0 + cl) * a.HoWo] = (bf16_t)bf16_round(frozen_out((double)tot[n][r], ch, slope, has_res, res[r]));
            }
        }
    } else {
#pragma unroll
        for (int n = 0; n < TN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + n * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
                if (co < a.cout) {
                    float v = tot[n][r];
                    if (a.bias) v = v + a.bias[co];
                    const size_t at = base + (size_t)co * a.HoWo;
                    if (a.y_is_f32) static_cast<float*>(a.y)[at] = v;
                    else static_cast<bf16_t*>(a.y)[at] = (bf16_t)bf16_round(v);
                }
            }
    }
}

template <int TN, int KS, int S, int EPI, bool WT = false>
static void launch_bf16(const FwdBf16Args& a, hipStream_t st) {
    const dim3 grid((a.P + CB_MT - 1) / CB_MT, (a.cout + TN * 32 - 1) / (TN * 32));
    hipLaunchKernelGGL((conv_bf16_kernel<TN, KS, S, EPI, WT>), grid, dim3(CB_THREADS), 0, st, a);
}

template <int KS, int S, int EPI, bool WT = false>
static void launch_bf16_geometry(const FwdBf16Args& a, hipStream_t st) {
    // 64 output channels per workgroup; 32 where there are no more, or where 64 would leave compute units without a workgroup
    // (the sum of an element does not depend on the choice)
    const long long tiles = ((long long)a.P + CB_MT - 1) / CB_MT * ((a.cout + 63) / 64);
    if (a.cout > 32 && tiles >= device_compute_units()) launch_bf16<2, KS, S, EPI, WT>(a, st);
    else launch_bf16<1, KS, S, EPI, WT>(a, st);
}

template <int EPI>
static void launch_bf16_any(const FwdBf16Args& a, int ksize, int stride, hipStream_t st) {
    if (ksize == 1) launch_bf16_geometry<1, 1, EPI>(a, st);
    else if (stride == 1) launch_bf16_geometry<3, 1, EPI>(a, st);
    else launch_bf16_geometry<3, 2, EPI>(a, st);
}

static FwdBf16Args make_bf16(const ConvGeom& g, const uint16_t* x, const float* w, void* y) {
    FwdBf16Args a = {};
    a.x = x; a.w = w; a.y = y;
    a.cin = g.cin; a.cout = g.cout; a.H = g.H; a.W = g.W; a.Ho = g.Ho; a.Wo = g.Wo; a.HoWo = g.HoWo; a.P = g.K;
    return a;
}

}  // namespace om
