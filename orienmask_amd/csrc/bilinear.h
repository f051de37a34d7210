// The bilinear sampler of F.interpolate(mode='bilinear', align_corners=False) as torch-CPU evaluates it for a 0/1 mask, shared by
// coco_format.hip (COCOMetrics._recover_shape_segm) and visualize.hip (InferenceVisualizer._recover_shape_segm): both must give
// the same resized value for the same source pixel.  Translation units that include it are built with -ffp-contract=off, so
// the only fused operations are the explicit fmaf calls below, in torch's operation order.
#pragma once
#include <hip/hip_runtime.h>

namespace om {

// Output index d along one axis -> the two source taps (i0, i1) and their weights (w0, w1); scale = n_in / n_out.
__device__ __forceinline__ void tap(int d, float scale, int n_in, int& i0, int& i1, float& w0, float& w1) {
    float src = fmaf(scale, (float)d + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    w1 = src - (float)i0;
    w0 = 1.0f - w1;
}

// The four taps a00 (row i0, column j0), a01, a10, a11 blended along the columns, then along the rows (outputs with
// height + width > BILINEAR_SMALL_OUT).
__device__ __forceinline__ float bilinear_blend(float a00, float a01, float a10, float a11, float wx0, float wx1, float wy0,
                                                float wy1) {
    const float top = fmaf(a00, wx0, a01 * wx1);
    const float bot = fmaf(a10, wx0, a11 * wx1);
    return fmaf(top, wy0, bot * wy1);
}

// torch-CPU resizes with another kernel when the output's height + width is at most BILINEAR_SMALL_OUT (the loop it prefers for
// small outputs, vectorised over channels): the four weights h_i * w_j are rounded first and the taps summed left to right.
// (torch also takes that loop at every size when it runs on one thread and the tensor has exactly 3 channels; the oracle and
// the parity tests run torch multi-threaded.)
constexpr int BILINEAR_SMALL_OUT = 128;

__device__ __forceinline__ float bilinear_blend_small(float a00, float a01, float a10, float a11, float wx0, float wx1, float wy0,
                                                      float wy1) {
    const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
    return fmaf(a11, w11, fmaf(a10, w10, fmaf(a00, w00, a01 * w01)));
}

// the blend torch uses for an output of out_h + out_w pixels along its two sides (small: out_h + out_w <= BILINEAR_SMALL_OUT)
__device__ __forceinline__ float bilinear_value(bool small, float a00, float a01, float a10, float a11, float wx0, float wx1,
                                                float wy0, float wy1) {
    return small ? bilinear_blend_small(a00, a01, a10, a11, wx0, wx1, wy0, wy1)
                 : bilinear_blend(a00, a01, a10, a11, wx0, wx1, wy0, wy1);
}

}  // namespace om
