// The forward of the training model's convolutions (orienmask_amd/train.py: conv2d with forward='hip'), for the three geometries
// the two models contain: 1x1 stride 1 pad 0, 3x3 stride 1 pad 1, 3x3 stride 2 pad 1.  fp32 NCHW contiguous; fp32 operands on
// v_mfma_f32_32x32x2_f32 (an fmaf chain per output element).  Ho = (H + 2*pad - ks)/s + 1.
//
//   conv_fwd_kernel   y[b,co,oy,ox] = bias[co] + sum_{ci,kh,kw} x[b,ci,oy*s+kh-pad,ox*s+kw-pad] * w[co,ci,kh,kw]
//       GEMM: rows = co (first operand: weights), columns = output pixels (second operand: x), k = (ci, tap): conv_dx_kernel
//       (conv_grad.hip) with the roles of ci and co swapped.  A lane owns one pixel, so every y store of a wave is 32 consecutive
//       floats of one channel plane (where the 32 pixels lie in one image), and every x load is a run along W.
//       TILES SPAN IMAGES: the 128 pixels of a tile are consecutive values of the flat index g = b*Ho*Wo + oy*Wo + ox over the whole
//       batch, so a 17 x 17 map fills 128-pixel tiles as a 544 x 544 map does.  Nothing is derived from the tile's position: at the
//       start the workgroup writes a table of one entry per staged POSITION (a cell of the tile or of its halo, for one row tap):
//       the cell's own (b, oy, ox) give the offset of the input element the position holds, or -1 where the row lies above or below
//       the map, the column beyond it, or the cell outside the batch.  A cell next to an image boundary therefore reads zero, never
//       the neighbouring image's row.  Per lane, from its own (b, oy, ox): the mask of the column taps that leave the row.
//       Stride 1: position p of row tap r holds input cell g0 + p - 1 + (r-1)*W (the tile with a one-cell halo), tap (r, c) of
//       tile cell j reads position j + c: the column taps are +-1 shifts of one LDS row.
//       Stride 2: output cell (oy, ox) reads input (2*oy+kh-1, 2*ox+kw-1).  Per row tap two LDS rows: E[p] = column 2*ox of cell
//       g0 + p, O[p] = column 2*ox + 1 of cell g0 + p - 1; the taps kw = 0, 1, 2 read O[j], E[j], O[j+1], all at unit lane stride
//       (no two-float stride, no bank conflict).  The left tap of ox = 0 is masked per lane; every other absent tap (odd H or W:
//       the last row's lower tap, the last column's right tap) is a -1 of the table.
//       Weights: per co the KC input channels of a chunk are one run of KC*taps contiguous floats of w[co][ci][tap], copied as it
//       lies into an LDS row of KC*taps + 1 floats (the odd length keeps the 32 rows a wave reads on 32 banks).
//       DOUBLE-BUFFERED: the global loads of chunk n+1 are issued into registers before the matrix instructions of chunk n and
//       written to the other LDS buffer after them: one barrier per chunk, and no load waits in front of a matrix instruction.
//       Chains: a matrix-instruction accumulator takes the KC input channels of a chunk times the column taps of ONE row tap (at
//       most 32 products: 8 x 3 at 3x3, 32 at 1x1), then is added into a double per element and cleared; y is that double plus
//       the bias (as double), rounded once.  Chunks in ci order, row taps in kh order: the order for an element depends on the
//       geometry only, not on the tile, the image or B.  k is never split; no workspace, no atomics: the same bits on every run.
//   EPI_FROZEN        the same kernel with the frozen Conv -> BatchNorm -> LeakyReLU (+ residual) block's epilogue instead of the
//       bias (om_conv2d_frozen_forward): the convolution output never reaches memory.  At the start, beside the position table,
//       thread t of the first NT writes the record of channel co0 + t to LDS: exactly the doubles bn_fwd_kernel's EVAL phase
//       builds (bn_channel.h; invstd = 1/sqrt((double)running_var + eps) through split_hi_lo, mean = (double)running_mean), zeros
//       where co0 + t >= cout.  One record per channel and workgroup, not one per lane: the double sqrt and division of 32 records
//       per lane would cost more than the matrix instructions of a 64-channel 1x1 layer.  Per element, with h the double sum:
//       z = fma(h - mean, gamma * invstd, beta), y = (float)((z > 0 ? z : z * slope) + residual), all double, rounded once, with
//       contraction switched off for the function (this file is not built with -ffp-contract=off).  The 16 residuals of a
//       32-channel block are loaded before the block's first store.
// Every load and store is bounds-checked per element (any B, cin, cout, H, W >= 1; no alignment is assumed); rows and columns of a
// tile that lie outside the tensor are staged as zeros and never stored.
#include "conv_train.h"
#include "bn_channel.h"

namespace om {

constexpr int CF_THREADS = 256;
constexpr int CF_MT = 128;              // pixels of a tile: four waves of 32

enum { EPI_BIAS = 0, EPI_FROZEN = 1 };

struct FwdArgs {
    const float* x; const float* w; const float* bias; float* y;
    int cin, cout, H, W, Ho, Wo, HoWo;
    int P;                      // B * Ho * Wo
    // EPI_FROZEN only
    const float* gamma; const float* beta; const float* running_mean; const float* running_var; const float* residual;
    double eps;
    float slope;
};

// (the frozen block's output for one element is bn_channel.h's frozen_out, shared with conv_fwd_bf16.hip)

// TN blocks of 32 output channels per wave (every wave takes the tile's whole co range and 32 of its pixels)
template <int TN, int KS, int S, int EPI>
__global__ void __launch_bounds__(CF_THREADS) conv_fwd_kernel(const FwdArgs a) {
    constexpr int TAPS = KS * KS, NT = TN * 32;
    constexpr int KC = KS == 1 ? 32 : 8;                    // input channels per staged chunk
    constexpr int NROW = KS == 1 ? 1 : (S == 1 ? 3 : 6);    // LDS rows per input channel
    constexpr int SEG = KS == 1 ? CF_MT : (S == 1 ? CF_MT + 2 : CF_MT + 1);
    constexpr int POSN = NROW * SEG;                        // staged positions per input channel
    constexpr int XE = KC * POSN, NIX = (XE + CF_THREADS - 1) / CF_THREADS;
    constexpr int LDW = KC * TAPS + 1;
    constexpr int WE = NT * KC * TAPS, NIW = WE / CF_THREADS;
    static_assert(WE % CF_THREADS == 0, "the weight chunk is a whole number of rounds");
    __shared__ long long s_off[POSN];
    __shared__ float s_x[2][XE];                            // [ci][row][position]
    __shared__ float s_w[2][NT * LDW];                      // [co][ci][tap]
    __shared__ BnAffine s_ch[EPI == EPI_FROZEN ? NT : 1];   // the record of channel co0 + t

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 31, fk = lane >> 5;
    const long long g0 = (long long)blockIdx.x * CF_MT;
    const int co0 = blockIdx.y * NT;
    const size_t hw = (size_t)a.H * a.W;

    // the position table
    for (int p = tid; p < POSN; p += CF_THREADS) {
        const int row = p / SEG, j = p - row * SEG;
        int r, odd = 0;
        long long g;
        if (KS == 1) { r = 0; g = g0 + j; }
        else if (S == 1) { r = row; g = g0 + j - 1; }
        else { r = row >> 1; odd = row & 1; g = g0 + j - odd; }
        long long off = -1;
        if (g >= 0 && g < a.P && !(S == 2 && !odd && j == CF_MT)) {      // (the E rows have one position to spare)
            const int b = (int)(g / a.HoWo), q = (int)(g - (long long)b * a.HoWo);
            const int oy = q / a.Wo, ox = q - oy * a.Wo;
            const int iy = oy * S + r - KS / 2, ix = S == 1 ? ox : 2 * ox + odd;
            if ((unsigned)iy < (unsigned)a.H && ix < a.W) off = (long long)((size_t)b * a.cin * hw + (size_t)iy * a.W + ix);
        }
        s_off[p] = off;
    }

    if constexpr (EPI == EPI_FROZEN) {
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

    f32x16 acc[TN];
    double tot[TN][16];         // the second level: every chain enters it once
#pragma unroll
    for (int n = 0; n < TN; ++n) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[n][r] = 0.f; tot[n][r] = 0.0; }
    }

    float px[NIX], pw[NIW];     // the chunk in flight
    auto load = [&](int ci0) {
#pragma unroll
        for (int i = 0; i < NIX; ++i) {
            const int e = tid + i * CF_THREADS;
            const int kc = e / POSN, p = e - kc * POSN;
            float v = 0.f;
            if (e < XE) {
                const long long off = s_off[p];
                const int ci = ci0 + kc;
                if (off >= 0 && ci < a.cin) v = a.x[(size_t)off + (size_t)ci * hw];
            }
            px[i] = v;
        }
        const int krun = (a.cin - ci0) * TAPS;              // floats of a co row from this chunk's first channel on
#pragma unroll
        for (int i = 0; i < NIW; ++i) {
            const int e = tid + i * CF_THREADS;
            const int cl = e / (KC * TAPS), kk = e - cl * (KC * TAPS);
            const int co = co0 + cl;
            float v = 0.f;
            if (co < a.cout && kk < krun) v = a.w[((size_t)co * a.cin + ci0) * TAPS + kk];
            pw[i] = v;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NIX; ++i) {
            const int e = tid + i * CF_THREADS;
            if (e < XE) s_x[buf][e] = px[i];
        }
#pragma unroll
        for (int i = 0; i < NIW; ++i) {
            const int e = tid + i * CF_THREADS;
            const int cl = e / (KC * TAPS), kk = e - cl * (KC * TAPS);
            s_w[buf][cl * LDW + kk] = pw[i];
        }
    };

    __syncthreads();            // the table
    load(0);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int ci0 = 0; ci0 < a.cin; ci0 += KC, buf ^= 1) {
        const bool more = ci0 + KC < a.cin;
        if (more) load(ci0 + KC);                           // in flight under this chunk's matrix instructions
        const float* xb = s_x[buf] + wave * 32 + fi;
        const float* wb = s_w[buf] + fi * LDW;
#pragma unroll
        for (int r = 0; r < KS; ++r) {
#pragma unroll
            for (int c = 0; c < KS; ++c) {
                // the LDS row and shift of column tap c (see the head of the file)
                const int row = KS == 1 ? 0 : (S == 1 ? r : 2 * r + (c != 1 ? 1 : 0));
                const int shift = KS == 1 ? 0 : (S == 1 ? c : (c == 2 ? 1 : 0));
                const bool ok = KS == 1 || c == 1 || (c == 0 ? ok0 : ok2);
                const float* dp = xb + row * SEG + shift;
                const float* wp = wb + r * KS + c;
#pragma unroll
                for (int kk = 0; kk < KC / 2; ++kk) {
                    const int kc = 2 * kk + fk;
                    const float dv = dp[kc * POSN];
                    const float bv = ok ? dv : 0.f;
#pragma unroll
                    for (int n = 0; n < TN; ++n)
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[n * 32 * LDW + kc * TAPS], bv, acc[n], 0, 0, 0);
                }
            }
            // the chain ends: KC input channels x the row's column taps (at most 32 products)
#pragma unroll
            for (int n = 0; n < TN; ++n) {
#pragma unroll
                for (int i = 0; i < 16; ++i) { tot[n][i] += (double)acc[n][i]; acc[n][i] = 0.f; }
            }
        }
        if (more) store(buf ^ 1);                           // the buffer the previous chunk read, behind the barrier that ended it
        __syncthreads();
    }
    // D layout: column (pixel) = lane & 31, row (co) = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)
    if (!live) return;
    const size_t base = (size_t)b * a.cout * a.HoWo + q;
    float* o = a.y + base;
    if constexpr (EPI == EPI_FROZEN) {
        const bool has_res = a.residual != nullptr;
        const float* rp = has_res ? a.residual + base : nullptr;
        const double slope = (double)a.slope;
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            // 16 loads in flight, under one uniform branch and none per element: a channel beyond cout reads the last channel's
            // plane (in bounds) and is never stored
            float res[16];
            if (has_res) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + n * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
                    res[r] = rp[(size_t)(co < a.cout ? co : a.cout - 1) * a.HoWo];
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) res[r] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cl = n * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
                const BnAffine ch = s_ch[cl];
                if (co0 + cl < a.cout) o[(size_t)(co0 + cl) * a.HoWo] = frozen_out(tot[n][r], ch, slope, has_res, res[r]);
            }
        }
    } else {
#pragma unroll
        for (int n = 0; n < TN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + n * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
                if (co < a.cout) o[(size_t)co * a.HoWo] = (float)(tot[n][r] + (a.bias ? (double)a.bias[co] : 0.0));
            }
    }
}

template <int TN, int KS, int S, int EPI>
static void launch_fwd(const FwdArgs& a, hipStream_t st) {
    const dim3 grid((a.P + CF_MT - 1) / CF_MT, (a.cout + TN * 32 - 1) / (TN * 32));
    hipLaunchKernelGGL((conv_fwd_kernel<TN, KS, S, EPI>), grid, dim3(CF_THREADS), 0, st, a);
}

template <int KS, int S, int EPI>
static void launch_fwd_geometry(const FwdArgs& a, hipStream_t st) {
    // 64 output channels per workgroup; 32 where there are no more, or where 64 would leave compute units without a workgroup
    // (k is never split)
    const long long tiles = ((long long)a.P + CF_MT - 1) / CF_MT * ((a.cout + 63) / 64);
    if (a.cout > 32 && tiles >= device_compute_units()) launch_fwd<2, KS, S, EPI>(a, st);
    else launch_fwd<1, KS, S, EPI>(a, st);
}

static FwdArgs make_fwd(const ConvGeom& g, const float* x, const float* w, float* y) {
    FwdArgs a = {};
    a.x = x; a.w = w; a.y = y;
    a.cin = g.cin; a.cout = g.cout; a.H = g.H; a.W = g.W; a.Ho = g.Ho; a.Wo = g.Wo; a.HoWo = g.HoWo; a.P = g.K;
    return a;
}

template <int EPI>
static void launch_fwd_any(const FwdArgs& a, int ksize, int stride, hipStream_t st) {
    if (ksize == 1) launch_fwd_geometry<1, 1, EPI>(a, st);
    else if (stride == 1) launch_fwd_geometry<3, 1, EPI>(a, st);
    else launch_fwd_geometry<3, 2, EPI>(a, st);
}

}  // namespace om

extern "C" int om_conv2d_forward(const float* x, const float* w, const float* bias, int B, int cin, int H, int W, int cout, int ksize,
                                 int stride, float* y, om_stream stream) {
    OM_REQUIRE(x && w && y, OM_EINVAL, "om_conv2d_forward: null pointer");
    om::ConvGeom g;
    if (!om::conv_geometry(B, cin, H, W, cout, ksize, stride, &g))
        return om::conv_geometry_refused("om_conv2d_forward", B, cin, H, W, cout, ksize, stride);
    om::FwdArgs a = om::make_fwd(g, x, w, y);
    a.bias = bias;
    om::launch_fwd_any<om::EPI_BIAS>(a, ksize, stride, static_cast<hipStream_t>(stream));
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

extern "C" int om_conv2d_frozen_forward(const float* x, const float* w, int B, int cin, int H, int W, int cout, int ksize, int stride,
                                        const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                        double eps, float slope, const float* residual, float* y, om_stream stream) {
    OM_REQUIRE(x && w && y && gamma && beta && running_mean && running_var, OM_EINVAL, "om_conv2d_frozen_forward: null pointer");
    OM_REQUIRE(y != x && y != w && y != residual, OM_EINVAL,
               "om_conv2d_frozen_forward: y must not alias x, w or the residual (a workgroup reads what another has written)");
    om::ConvGeom g;
    if (!om::conv_geometry(B, cin, H, W, cout, ksize, stride, &g))
        return om::conv_geometry_refused("om_conv2d_frozen_forward", B, cin, H, W, cout, ksize, stride);
    OM_REQUIRE(eps > 0.0, OM_EINVAL, "om_conv2d_frozen_forward: eps %g", eps);
    om::FwdArgs a = om::make_fwd(g, x, w, y);
    a.gamma = gamma; a.beta = beta; a.running_mean = running_mean; a.running_var = running_var; a.residual = residual;
    a.eps = eps; a.slope = slope;
    om::launch_fwd_any<om::EPI_FROZEN>(a, ksize, stride, static_cast<hipStream_t>(stream));
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}
