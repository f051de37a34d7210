// What the training convolutions share (conv_fwd.hip, conv_grad.hip, conv_dw.hip): the geometries and size limits of their four entry points, the
// text that refuses a shape outside them, and the matrix instruction's accumulator type with its clear (conv_fwd.hip clears its
// accumulators lane by lane inside the loops that also touch the double sums).
#pragma once
#include "om_common.h"

namespace om {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void clear16(f32x16& v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.f;
}

struct ConvGeom {
    int B, cin, cout, H, W, Ho, Wo, HoWo, ks, stride, pad, taps;
    int K;              // B * Ho * Wo
    size_t n;           // cout * cin * taps
};

// fills *g; false for anything but 1x1 stride 1 pad 0, 3x3 stride 1 pad 1 and 3x3 stride 2 pad 1 within the size limits
static inline bool conv_geometry(int B, int cin, int H, int W, int cout, int ksize, int stride, ConvGeom* g) {
    if (!((ksize == 1 && stride == 1) || (ksize == 3 && (stride == 1 || stride == 2)))) return false;
    if (B < 1 || cin < 1 || cout < 1 || H < 1 || W < 1) return false;
    g->B = B; g->cin = cin; g->cout = cout; g->H = H; g->W = W; g->ks = ksize; g->stride = stride;
    g->pad = ksize / 2; g->taps = ksize * ksize;
    g->Ho = (H + 2 * g->pad - ksize) / stride + 1;
    g->Wo = (W + 2 * g->pad - ksize) / stride + 1;
    const long long howo = (long long)g->Ho * g->Wo, n = (long long)cout * cin * g->taps;
    // 32-bit pixel and element counts (split * chunk stays below 2^31), and grid dimensions y / z below 65536
    if ((long long)B * H * W >= (1ll << 30) || n >= (1ll << 31) || B > 16383 || cin > (1 << 20) || cout > (1 << 20)) return false;
    g->HoWo = (int)howo;
    g->K = (int)(howo * B);
    g->n = (size_t)n;
    return true;
}

// OM_EINVAL with the refusal of entry `who` as the last error
static inline int conv_geometry_refused(const char* who, int B, int cin, int H, int W, int cout, int ksize, int stride) {
    set_error("%s: [%d,%d,%d,%d] -> %d channels, ksize %d stride %d: the geometries are 1x1 stride 1, 3x3 stride 1 and 3x3 stride 2 "
              "(B <= 16383, B*H*W below 2^30, cout*cin*ksize^2 below 2^31)", who, B, cin, H, W, cout, ksize, stride);
    return OM_EINVAL;
}

}  // namespace om
