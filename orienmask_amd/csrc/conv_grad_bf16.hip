// The bf16 data gradient of the training model's convolutions (orienmask_amd/train.py: conv2d_bf16_backward with backend 'hip'; the
// models with amp='bf16', conv_forward='hip', conv_grad='hip'), for conv_train.h's three geometries.  NCHW contiguous; dy bf16, w
// the float32 master weight, on v_mfma_f32_32x32x16_bf16.  What conv_grad.hip is to float32.  The weight and bias gradients, and the
// workspace query, are conv_dw.hip.
//
// ARITHMETIC CONTRACT (tests/test_conv_grad_bf16.py pins it)
//   dy is bf16 and is widened exactly.  w is rounded with bf16.h's bf16_round while it is staged: that is what the forward
//   multiplied by, so the gradient is the gradient of the function that ran; there is no cast kernel and no bf16 copy of the weight.
//   Every product of two bf16 values is exact in float32; all accumulation is float32 or wider.
//   dx   the float32 output (dx_is_f32 = 1) is the sum, the bf16 output is bf16_round of the same sum.  Two float32 levels per
//        element over k = cout * (the taps that reach the pixel), in the order output channels (blocks of 16) > tap: a chain in the
//        matrix instruction's accumulators holds a block of output channels (stride 1: a staged chunk of conv_bf16_tile.h, 16 at
//        3x3 and 64 at 1x1; stride 2: CGB_DX2_FOLD = 64) and is then added into a second float32 accumulator and cleared.  (One
//        chain over the whole k reached 4.3 x torch-CPU's error in the stride-2 dx of an in-network layer: DESIGN 3.30.)  The
//        order is a function of the geometry only -- not of B, the tile or the device -- so an image's dx has the same bits alone
//        and in any batch.
//
// STRUCTURE
//   stride 1   the forward convolution of dy (cout channels in) with w'[ci][co][2-kh][2-kw] (1x1: w transposed): conv_bf16_tile.h's
//        kernel with its transposed weight gather (WT), nothing else: position table, halo row, column-tap masks, LDS images,
//        budget are the forward's (the head of conv_fwd_bf16.hip).
//   stride 2   conv_dx2_bf16_kernel: conv_grad.hip's four PARITY CLASSES (py, px) = (iy & 1, ix & 1) of the input pixel, one
//        launch each.  A class is a grid of Hc x Wc = ceil((H - py) / 2) x ceil((W - px) / 2) cells (sy, sx) with iy = 2 sy + py,
//        ix = 2 sx + px, so every element of dx belongs to exactly one class and is written by it, the last row or column of an odd
//        or even H, W included (a class without cells is not launched).  Parity 0 has the one tap kh = 1 at oy = sy; parity 1 the
//        taps kh = 0 at oy = sy + 1 and kh = 2 at oy = sy: 1, 2, 2 and 4 taps, and no product with an absent tap is formed.  Tiles
//        span images (128 consecutive values of the flat cell index b * Hc * Wc + sy * Wc + sx), a lane owns one cell, a wave 32 cells
//        and TN blocks of 32 input channels.  dy is staged PER TAP, [tap][cell][16 co] bf16 through a per-(tap, cell) offset table
//        (-1 where oy = Ho or ox = Wo: staged as zero): a shift of one staged row cannot serve here, because the class grid may be
//        one column narrower than dy's.  Weights as [tap][ci][16 co] bf16, gathered from w[co][ci][kh][kw] and rounded while packing.
//        One LDS buffer, the chunk in flight in registers, as the forward.
//
// BUDGET (gfx950 code objects)
//   stride 1: conv_bf16_tile.h, __launch_bounds__(256, 2).  stride 2: __launch_bounds__(256, 2), LDS at most 28.1 KiB.
//   The figures per instantiation are in DESIGN 3.29.
// Every load and store is bounds-checked per element (any B, cin, cout, H, W >= 1); every global access is of one element, so no
// alignment beyond the element's own is assumed and there is one path only.
#include "conv_bf16_tile.h"

namespace om {

constexpr int CGB_THREADS = 256;
constexpr int CGB_MT = 128;             // dx stride 2: cells of a tile
constexpr int CGB_DX2_FOLD = 64;        // dx stride 2: output channels of a first-level chain (four staged chunks of 16)

struct Dx2Args {
    const bf16_t* dy; const float* w; void* dx;
    int dx_is_f32;
    int cin, cout, H, W, Ho, Wo, HoWo;
    int Hc, Wc, HcWc;           // the class grid
    int P;                      // B * Hc * Wc
};

// ---------------------------------------------------------------------------------------------------------------- dx, stride 2
// NR, NC: row and column taps of the class (1: parity 0, 2: parity 1)
template <int TN, int NR, int NC>
__global__ void __launch_bounds__(CGB_THREADS, 2) conv_dx2_bf16_kernel(const Dx2Args a) {
    constexpr int NTAP = NR * NC, NT = TN * 32, PY = NR - 1, PX = NC - 1;
    constexpr int POSN = NTAP * CGB_MT;                             // staged (tap, cell) positions
    constexpr int XU = 2 * POSN, NIX = XU / CGB_THREADS;            // units of 8 channels of a position
    constexpr int WBLK = NT * 2 + 1;                                // 16-byte words of a tap block (one to spare)
    constexpr int WU = 2 * NTAP * NT, NIW = (WU + CGB_THREADS - 1) / CGB_THREADS;
    __shared__ long long s_off[POSN];
    __shared__ uint4 s_x[POSN * 2];                                 // [tap][cell][half of 8 co]
    __shared__ uint4 s_w[NTAP * WBLK];                              // [tap][ci][half of 8 co]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 31, fk = lane >> 5;
    const long long g0 = (long long)blockIdx.x * CGB_MT;
    const int ci0 = blockIdx.y * NT;
    const size_t hw = (size_t)a.H * a.W;

    for (int p = tid; p < POSN; p += CGB_THREADS) {
        const int t = p / CGB_MT, j = p - t * CGB_MT;
        const int r = t / NC, c = t - r * NC;
        const long long g = g0 + j;
        long long off = -1;
        if (g < a.P) {
            const int b = (int)(g / a.HcWc), q = (int)(g - (long long)b * a.HcWc);
            const int sy = q / a.Wc, sx = q - sy * a.Wc;
            const int oy = sy + (PY && r == 0 ? 1 : 0), ox = sx + (PX && c == 0 ? 1 : 0);
            if (oy < a.Ho && ox < a.Wo) off = (long long)((size_t)b * a.cout * a.HoWo + (size_t)oy * a.Wo + ox);
        }
        s_off[p] = off;
    }

    // two levels: the matrix instruction's chain holds CGB_DX2_FOLD output channels (acc), the chains are added in order (tot)
    f32x16 acc[TN], tot[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n) { clear16(acc[n]); clear16(tot[n]); }

    uint4 px[NIX], pw[NIW];     // the chunk in flight, as it will lie in LDS
    auto load = [&](int co0) {
#pragma unroll
        for (int i = 0; i < NIX; ++i) {
            const int u = tid + i * CGB_THREADS;
            const int oct = u / POSN, p = u - oct * POSN;
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0u;
            const long long off = s_off[p];
            const int co = co0 + oct * 8;
            if (off >= 0) {
                const bf16_t* src = a.dy + (size_t)off + (size_t)co * a.HoWo;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (co + j < a.cout) v[j] = src[(size_t)j * a.HoWo];
            }
            px[i] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
        }
#pragma unroll
        for (int i = 0; i < NIW; ++i) {
            const int u = tid + i * CGB_THREADS;
            const int t = u % NTAP, rest = u / NTAP;
            const int cl = rest % NT, oct = rest / NT;
            const int r = t / NC, c = t - r * NC;
            const int kh = PY ? (r == 0 ? 0 : 2) : 1, kw = PX ? (c == 0 ? 0 : 2) : 1;
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0u;
            const int ci = ci0 + cl, co = co0 + oct * 8;
            if (u < WU && ci < a.cin) {
                const float* src = a.w + ((size_t)co * a.cin + ci) * 9 + kh * 3 + kw;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (co + j < a.cout) v[j] = bf16_round(src[(size_t)j * a.cin * 9]);
            }
            pw[i] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < NIX; ++i) {
            const int u = tid + i * CGB_THREADS;
            const int oct = u / POSN, p = u - oct * POSN;
            s_x[p * 2 + oct] = px[i];
        }
#pragma unroll
        for (int i = 0; i < NIW; ++i) {
            const int u = tid + i * CGB_THREADS;
            const int t = u % NTAP, rest = u / NTAP;
            const int cl = rest % NT, oct = rest / NT;
            if (u < WU) s_w[t * WBLK + cl * 2 + oct] = pw[i];
        }
    };

    __syncthreads();            // the table
    load(0);
    for (int co0 = 0; co0 < a.cout; co0 += 16) {
        store();
        __syncthreads();
        if (co0 + 16 < a.cout) load(co0 + 16);              // in flight under this chunk's matrix instructions
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
            const bf16x8 bv = __builtin_bit_cast(bf16x8, s_x[(t * CGB_MT + wave * 32 + fi) * 2 + fk]);
            const uint4* wp = s_w + t * WBLK + fi * 2 + fk;
#pragma unroll
            for (int n = 0; n < TN; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wp[n * 64]), bv, acc[n], 0, 0, 0);
        }
        // a chain ends after CGB_DX2_FOLD output channels and at the last chunk: one float32 add per element into the second level
        if ((co0 + 16) % CGB_DX2_FOLD == 0 || co0 + 16 >= a.cout) {
#pragma unroll
            for (int n = 0; n < TN; ++n) { tot[n] += acc[n]; clear16(acc[n]); }
        }
        __syncthreads();        // the chunk is consumed: the next store may overwrite it
    }
    // D layout: column (cell) = lane & 31, row (ci) = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)
    const long long g = g0 + wave * 32 + fi;
    if (g >= a.P) return;
    const int b = (int)(g / a.HcWc), q = (int)(g - (long long)b * a.HcWc);
    const int sy = q / a.Wc, sx = q - sy * a.Wc;
    const int iy = 2 * sy + PY, ix = 2 * sx + PX;           // inside the map: that is what the class grid is
    const size_t base = (size_t)b * a.cin * hw + (size_t)iy * a.W + ix;
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + n * 32 + 8 * (r >> 2) + 4 * fk + (r & 3);
            if (ci < a.cin) {
                const size_t at = base + (size_t)ci * hw;
                if (a.dx_is_f32) static_cast<float*>(a.dx)[at] = tot[n][r];
                else static_cast<bf16_t*>(a.dx)[at] = (bf16_t)bf16_round(tot[n][r]);
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------- host
template <int NR, int NC>
static void launch_dx2(Dx2Args a, int B, hipStream_t st) {
    a.Hc = (a.H - (NR - 1) + 1) / 2;
    a.Wc = (a.W - (NC - 1) + 1) / 2;
    if (a.Hc < 1 || a.Wc < 1) return;               // H = 1 or W = 1 has no odd row or column
    a.HcWc = a.Hc * a.Wc;
    a.P = B * a.HcWc;
    const unsigned tiles = (unsigned)((a.P + CGB_MT - 1) / CGB_MT);
    // 64 input channels per workgroup where there are more than 32 (the sum of an element does not depend on the choice)
    if (a.cin > 32) hipLaunchKernelGGL((conv_dx2_bf16_kernel<2, NR, NC>), dim3(tiles, (a.cin + 63) / 64), dim3(CGB_THREADS), 0, st, a);
    else hipLaunchKernelGGL((conv_dx2_bf16_kernel<1, NR, NC>), dim3(tiles, 1), dim3(CGB_THREADS), 0, st, a);
}

}  // namespace om

extern "C" {

int om_conv2d_bf16_grad_input(const uint16_t* dy, const float* w, int B, int cin, int H, int W, int cout, int ksize, int stride,
                              void* dx, int dx_is_f32, void* workspace, size_t ws_bytes, om_stream stream) {
    (void)workspace; (void)ws_bytes;                // the data gradient needs no scratch
    OM_REQUIRE(dy && w && dx, OM_EINVAL, "om_conv2d_bf16_grad_input: null pointer");
    OM_REQUIRE((const void*)dx != (const void*)dy && (const void*)dx != (const void*)w, OM_EINVAL,
               "om_conv2d_bf16_grad_input: dx must not alias dy or w (a workgroup reads what another has written)");
    om::ConvGeom g;
    if (!om::conv_geometry(B, cin, H, W, cout, ksize, stride, &g))
        return om::conv_geometry_refused("om_conv2d_bf16_grad_input", B, cin, H, W, cout, ksize, stride);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (stride == 1) {
        // the forward of dy: the kernel's input channels are cout, its output channels cin, its map the input's
        om::ConvGeom t;
        if (!om::conv_geometry(B, cout, H, W, cin, ksize, 1, &t))
            return om::conv_geometry_refused("om_conv2d_bf16_grad_input", B, cin, H, W, cout, ksize, stride);
        om::FwdBf16Args a = om::make_bf16(t, dy, w, dx);
        a.y_is_f32 = dx_is_f32 ? 1 : 0;
        if (ksize == 1) om::launch_bf16_geometry<1, 1, om::EPB_BIAS, true>(a, st);
        // 3x3: 32 input channels per workgroup only.  With 64 the transposed gather (a 64-bit address per weight, where the
        // forward's are immediate offsets from one) spills 26 registers inside the main loop; the sum does not depend on it.
        else om::launch_bf16<1, 3, 1, om::EPB_BIAS, true>(a, st);
    } else {
        om::Dx2Args a = {};
        a.dy = dy; a.w = w; a.dx = dx; a.dx_is_f32 = dx_is_f32 ? 1 : 0;
        a.cin = cin; a.cout = cout; a.H = H; a.W = W; a.Ho = g.Ho; a.Wo = g.Wo; a.HoWo = g.HoWo;
        om::launch_dx2<1, 1>(a, B, st);
        om::launch_dx2<1, 2>(a, B, st);
        om::launch_dx2<2, 1>(a, B, st);
        om::launch_dx2<2, 2>(a, B, st);
    }
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // extern "C"
