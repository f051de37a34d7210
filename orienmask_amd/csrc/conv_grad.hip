// The data gradient of the training model's convolutions (orienmask_amd/train.py: conv2d), for the three geometries the two models
// contain: 1x1 stride 1 pad 0, 3x3 stride 1 pad 1, 3x3 stride 2 pad 1.  fp32 NCHW contiguous, as the training activations are;
// fp32 operands on v_mfma_f32_32x32x2_f32 (an fmaf chain per output element), fp32 accumulation.  Ho = (H + 2*pad - ks)/s + 1.
// The weight and bias gradients, and the workspace query, are conv_dw.hip.
//
//   conv_dx_kernel   dx[b,ci,iy,ix] = sum_{co,kh,kw} dy[b,co,oy,ox] * w[co,ci,kh,kw],   iy = oy*s + kh - pad, ix = ox*s + kw - pad
//       GEMM: rows = ci (first operand: weights), columns = pixels (second operand: dy), k = (co, tap).  A lane owns one pixel, so
//       every dx store of a wave is 32 consecutive floats of one channel plane, and every dy load is a run along W.
//       The pixels of a tile are 32*WM consecutive cells q = sy*Wo + sx of ONE image's (Ho, Wo) grid.  At stride 1 that grid is the
//       input's; at stride 2 the input pixels fall into four PARITY CLASSES (py, px) = (iy & 1, ix & 1), each a (Ho, Wo) grid of its
//       own with iy = 2*sy + py, ix = 2*sx + px, and a class is a tile family of its own (blockIdx.z): a pixel of class py has the
//       row taps kh = 1 (py = 0: oy = sy) or kh = 0, 2 (py = 1: oy = sy + 1, sy), and likewise along x, so the classes have 1, 2, 2
//       and 4 taps and no product with an absent tap is formed.  In all geometries a tap (kh, kw) of cell q reads dy at the flat
//       cell q + rshift*Wo + cshift: per k-chunk of KC output channels and per ROW tap the workgroup stages the run of 32*WM + 2
//       cells (the tile with its one-cell halo) once; the column taps are +-1 shifts of the same LDS row, masked where sx + cshift
//       leaves the row (a flat cell outside [0, Ho*Wo) is staged as zero, which is exactly the rows above and below the map).
//       The weights of a chunk are KC runs of NT*taps contiguous floats of w[co][ci][tap], scattered into LDS as [tap][co][ci]:
//       no transposed copy of the weights is needed.
//       Chains: a matrix-instruction accumulator takes the KC output channels of a chunk times the column taps of ONE row tap (at
//       most 32 products: 8 x 3 at 3x3, 32 at 1x1), then is added into a double per element and cleared; dx is that double rounded
//       once.  (One fp32 chain over k = 576 measured 1.1e-6 of the tensor's scale, four times torch-CPU-float32's error.)
// Every load and store is bounds-checked per element (any B, cin, cout, H, W >= 1; no alignment is assumed); rows and columns of a
// tile that lie outside the tensor are staged as zeros and never stored.
#include "conv_train.h"

namespace om {

constexpr int CG_THREADS = 256;
constexpr int CG_DX_WIDE_CELLS = 512;   // dx: cells per image from which the 128-pixel tile is used

// the row taps and column taps of one tile family: tap r reads dy at cell q + rshift[r] * Wo (weights row kh[r]), likewise columns
struct CgTaps {
    int nr, nc;
    int kh[3], rshift[3];
    int kw[3], cshift[3];
    int py, px;                 // stride 2: the parity class; 0 otherwise
};

struct DxArgs {
    const float* dy; const float* w; float* dx;
    int cin, cout, H, W, Ho, Wo, HoWo, stride;
    int n_classes;
    CgTaps cls[4];
};

// ---------------------------------------------------------------------------------------------------------------- data gradient
// WM waves along the pixels (32 each), 4 / WM along ci (TN blocks of 32 each).
template <int WM, int TN, int TAPS>
__global__ void __launch_bounds__(CG_THREADS) conv_dx_kernel(const DxArgs a) {
    constexpr int WN = 4 / WM, MT = WM * 32, NT = WN * TN * 32;
    constexpr int KC = TAPS == 1 ? 32 : 8;          // output channels per staged chunk
    constexpr int NR = TAPS == 1 ? 1 : 3;           // row taps staged at most
    constexpr int SEG = MT + 2;                     // the tile's cells with a one-cell halo
    __shared__ float s_w[TAPS * KC * NT];           // [tap][co][ci]
    __shared__ float s_dy[KC * NR * SEG];           // [co][row tap][cell]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int fi = lane & 31, fk = lane >> 5;
    const int cls = blockIdx.z % a.n_classes, b = blockIdx.z / a.n_classes;
    const CgTaps& t = a.cls[cls];
    const int nr = t.nr, nc = t.nc;
    const int q0 = blockIdx.x * MT, ci0 = blockIdx.y * NT;
    const int q = q0 + wm * 32 + fi;                // this lane's cell
    const int sy = q / a.Wo, sx = q - sy * a.Wo;
    unsigned colmask = 0;
    for (int c = 0; c < nc; ++c) colmask |= ((unsigned)(sx + t.cshift[c]) < (unsigned)a.Wo ? 1u : 0u) << c;

    f32x16 acc[TN];
    double tot[TN][16];         // the second level: every chain enters it once
#pragma unroll
    for (int n = 0; n < TN; ++n) {
        clear16(acc[n]);
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[n][r] = 0.0;
    }

    const float* dyb = a.dy + (size_t)b * a.cout * a.HoWo;
    for (int co0 = 0; co0 < a.cout; co0 += KC) {
        __syncthreads();                            // the previous chunk's reads are done
        for (int e = tid; e < KC * nr * SEG; e += CG_THREADS) {
            const int rr = e / SEG, j = e - rr * SEG;
            const int kc = rr / nr, r = rr - kc * nr;
            const int co = co0 + kc;
            const int cell = q0 + t.rshift[r] * a.Wo + j - 1;
            float v = 0.f;
            if (co < a.cout && (unsigned)cell < (unsigned)a.HoWo) v = dyb[(size_t)co * a.HoWo + cell];
            s_dy[(kc * NR + r) * SEG + j] = v;
        }
        for (int e = tid; e < KC * NT * TAPS; e += CG_THREADS) {
            const int kc = e / (NT * TAPS), rem = e - kc * (NT * TAPS);
            const int cl = rem / TAPS, tap = rem - cl * TAPS;
            const int co = co0 + kc, ci = ci0 + cl;
            float v = 0.f;
            if (co < a.cout && ci < a.cin) v = a.w[((size_t)co * a.cin + ci) * TAPS + tap];
            s_w[(tap * KC + kc) * NT + cl] = v;
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            for (int c = 0; c < nc; ++c) {
                const int tap = TAPS == 1 ? 0 : t.kh[r] * 3 + t.kw[c];
                const float* wp = s_w + tap * KC * NT + wn * TN * 32 + fi;
                const float* dp = s_dy + r * SEG + wm * 32 + fi + 1 + t.cshift[c];
                const bool ok = ((colmask >> c) & 1u) != 0;
#pragma unroll
                for (int kk = 0; kk < KC / 2; ++kk) {
                    const int kc = 2 * kk + fk;
                    const float dv = dp[kc * NR * SEG];
                    const float bv = ok ? dv : 0.f;
#pragma unroll
                    for (int n = 0; n < TN; ++n)
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[kc * NT + n * 32], bv, acc[n], 0, 0, 0);
                }
            }
            // the chain ends: KC output channels x the row's column taps (at most 32 products)
#pragma unroll
            for (int n = 0; n < TN; ++n) {
#pragma unroll
                for (int i = 0; i < 16; ++i) tot[n][i] += (double)acc[n][i];
                clear16(acc[n]);
            }
        }
    }
    // D layout: column (pixel) = lane & 31, row (ci) = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)
    const int iy = sy * a.stride + t.py, ix = sx * a.stride + t.px;
    if (q >= a.HoWo || iy >= a.H || ix >= a.W) return;
    const size_t hw = (size_t)a.H * a.W;
    float* o = a.dx + (size_t)b * a.cin * hw + (size_t)iy * a.W + ix;
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + (wn * TN + n) * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
            if (ci < a.cin) o[(size_t)ci * hw] = (float)tot[n][r];
        }
}

// ---------------------------------------------------------------------------------------------------------------- host
static void cg_taps_stride1(int ks, CgTaps* t) {
    *t = CgTaps{};
    t->nr = t->nc = ks;
    for (int i = 0; i < ks; ++i) {
        t->kh[i] = t->kw[i] = i;
        t->rshift[i] = t->cshift[i] = ks / 2 - i;
    }
}

// stride 2, 3x3, pad 1: parity 0 takes tap 1 at shift 0; parity 1 takes tap 0 at shift +1 and tap 2 at shift 0
static void cg_taps_stride2(int py, int px, CgTaps* t) {
    *t = CgTaps{};
    t->py = py; t->px = px;
    if (py == 0) { t->nr = 1; t->kh[0] = 1; t->rshift[0] = 0; }
    else { t->nr = 2; t->kh[0] = 0; t->rshift[0] = 1; t->kh[1] = 2; t->rshift[1] = 0; }
    if (px == 0) { t->nc = 1; t->kw[0] = 1; t->cshift[0] = 0; }
    else { t->nc = 2; t->kw[0] = 0; t->cshift[0] = 1; t->kw[1] = 2; t->cshift[1] = 0; }
}

template <int WM, int TN, int TAPS>
static void launch_dx(const DxArgs& a, int B, hipStream_t st) {
    constexpr int MT = WM * 32, NT = (4 / WM) * TN * 32;
    const dim3 grid((a.HoWo + MT - 1) / MT, (a.cin + NT - 1) / NT, B * a.n_classes);
    hipLaunchKernelGGL((conv_dx_kernel<WM, TN, TAPS>), grid, dim3(CG_THREADS), 0, st, a);
}

}  // namespace om

extern "C" {

int om_conv2d_grad_input(const float* dy, const float* w, int B, int cin, int H, int W, int cout, int ksize, int stride, float* dx,
                         void* workspace, size_t ws_bytes, om_stream stream) {
    (void)workspace; (void)ws_bytes;                // the data gradient needs no scratch
    OM_REQUIRE(dy && w && dx, OM_EINVAL, "om_conv2d_grad_input: null pointer");
    om::ConvGeom g;
    if (!om::conv_geometry(B, cin, H, W, cout, ksize, stride, &g))
        return om::conv_geometry_refused("om_conv2d_grad_input", B, cin, H, W, cout, ksize, stride);
    hipStream_t st = static_cast<hipStream_t>(stream);
    om::DxArgs a = {};
    a.dy = dy; a.w = w; a.dx = dx;
    a.cin = cin; a.cout = cout; a.H = H; a.W = W; a.Ho = g.Ho; a.Wo = g.Wo; a.HoWo = g.HoWo; a.stride = stride;
    if (stride == 1) {
        a.n_classes = 1;
        om::cg_taps_stride1(ksize, &a.cls[0]);
    } else {
        a.n_classes = 4;
        for (int c = 0; c < 4; ++c) om::cg_taps_stride2(c >> 1, c & 1, &a.cls[c]);
    }
    const bool wide = g.HoWo >= om::CG_DX_WIDE_CELLS;
    if (ksize == 1) {
        if (wide) om::launch_dx<4, 2, 1>(a, B, st);
        else om::launch_dx<1, 1, 1>(a, B, st);
    } else {
        if (wide) om::launch_dx<4, 2, 9>(a, B, st);
        else om::launch_dx<1, 1, 9>(a, B, st);
    }
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // extern "C"
