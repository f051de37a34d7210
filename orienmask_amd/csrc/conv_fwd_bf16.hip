// The bf16 forward of the training model's convolutions (orienmask_amd/train.py: conv2d_bf16, and conv_bn_leaky_frozen on bf16
// activations; the models with amp='bf16', conv_forward='hip'), for conv_train.h's three geometries: 1x1 stride 1 pad 0, 3x3 stride
// 1 pad 1, 3x3 stride 2 pad 1.  NCHW contiguous; x bf16, w the float32 master weight, on v_mfma_f32_32x32x16_bf16.
//
//   conv_bf16_kernel  y[b,co,oy,ox] = bias[co] + sum_{ci,kh,kw} x[b,ci,oy*s+kh-pad,ox*s+kw-pad] * bf16(w[co,ci,kh,kw])
//       GEMM as conv_fwd.hip's: rows = co (first operand: weights), columns = output pixels (second operand: x).  A lane owns one
//       pixel; a wave takes 32 pixels and the tile's whole co range (TN blocks of 32).  The tile, its position table (TILES SPAN
//       IMAGES: 128 consecutive values of the flat index g = b*Ho*Wo + oy*Wo + ox; -1 where a staged cell lies outside the map or
//       the batch), the stride-1 halo row and the stride-2 E / O rows, and the per-lane column-tap masks are conv_fwd.hip's scheme,
//       word for word; see the head of that file.
//       K ORDER: one matrix instruction takes 16 consecutive input channels of ONE tap (lane l holds k = 8*(l>>5) ... + 7 of its
//       row or column), so k runs  chunk (KC = 16 or 64 input channels) > k-step of 16 channels > kh > kw.  Channels beyond cin are
//       staged as zeros in both operands (backbone.conv1, cin = 3: 13 of every 16 k are padding).
//       LDS: x as [k-step][position][16 ci] bf16, 32 bytes per position: the 64 lanes of a wave read one contiguous 2 KiB run (16
//       bytes each), and the column taps are shifts of the position as in the float32 kernel.  The staging transposes: a thread
//       gathers 8 channels of one position (8 two-byte loads, each of them a run along W across the lanes) and writes them as one
//       16-byte store.  Weights as [k-step][tap][co][16 ci] bf16, a tap block padded by 16 bytes: a thread gathers the 8 channels
//       of one (co, tap) from the float32 master weight, rounds each with bf16_round (nearest, ties to even: what autocast's weight
//       cast produces) and writes one 16-byte store.  There is no cast kernel and no bf16 copy of the weight.
//       One LDS buffer; the chunk in flight is held in registers: its global loads are issued before the matrix instructions of
//       the chunk in LDS and written after the barrier that ends them (two barriers per chunk).
//       INHERITED from conv_fwd.hip, knowingly: every wave reads the tile's whole weight block from LDS (a 2 x 2 wave grid would
//       read (NT/2 + 64) rows per wave instead of (NT + 32): the same 96 at NT = 64).  NOT inherited: one wave per SIMD -- the
//       kernel has no double level (two float32 levels: 64 accumulator registers at TN = 2), is held to 256 registers
//       (__launch_bounds__(256, 2): 154 to 256 are used, one spilled at 3x3 stride 2) and takes at most 51 KiB of LDS, so two
//       workgroups share a CU.
//       WHERE THE TIME GOES: in the staging, not in the matrix instructions.  Every global load moves one element
//       per lane (128 bytes of x per wave instruction), as many load instructions per input channel as conv_fwd.hip issues.
//       CHAIN: two float32 levels per output element.  The matrix instruction's accumulators hold the chain of ONE staged chunk (16
//       input channels x 9 taps = 144 products at 3x3, 64 input channels at 1x1; every product of two bf16 values is exact in
//       float32); where the chunk ends the chain is added into a second float32 accumulator and cleared, so the chunks' sums are
//       added in ci order (a single chunk: 0 + chain, the chain itself).  One chain over the whole k held the tests' own bound
//       (k * 2^-23 * S) but was up to 4.6 x further from float64 than torch-CPU's float32 on in-network operands, over the
//       project's bar of 2 x in y and in the stride-1 dx of most 3x3 layers; a bf16 output hides that, the float32
//       output and the frozen epilogue do not.  No double level.  Chunks in ci order, k-steps, kh, kw in order: the order for an
//       element is a function of the geometry only, not of the tile, the image, B or TN.  k is never split; no workspace, no
//       atomics.
//   Epilogues         plain: y32 = sum + bias (one float32 add; none without a bias), stored as float32 or as bf16_round(y32).
//       EPI_FROZEN: bn_channel.h's frozen_out on (double)sum with the bf16 residual widened, its float32 result through bf16_round:
//       bit for bit om_bn_act_forward(training=0) on the float32 output of the plain entry, rounded to bf16.  The channel records
//       (bn_affine_eval) are built once per channel and workgroup.
// Every load and store is bounds-checked per element (any B, cin, cout, H, W >= 1); every global access is of one element (2 bytes
// of x / residual / a bf16 y, 4 of w / bias / a float32 y), so no alignment beyond the element's own is assumed and there is one
// path only.
// The kernel and its launch rule are conv_bf16_tile.h, shared with conv_grad_bf16.hip.
#include "conv_bf16_tile.h"

extern "C" int om_conv2d_bf16_forward(const uint16_t* x, const float* w, const float* bias, int B, int cin, int H, int W, int cout,
                                      int ksize, int stride, void* y, int y_is_f32, om_stream stream) {
    OM_REQUIRE(x && w && y, OM_EINVAL, "om_conv2d_bf16_forward: null pointer");
    om::ConvGeom g;
    if (!om::conv_geometry(B, cin, H, W, cout, ksize, stride, &g))
        return om::conv_geometry_refused("om_conv2d_bf16_forward", B, cin, H, W, cout, ksize, stride);
    om::FwdBf16Args a = om::make_bf16(g, x, w, y);
    a.bias = bias;
    a.y_is_f32 = y_is_f32 ? 1 : 0;
    om::launch_bf16_any<om::EPB_BIAS>(a, ksize, stride, static_cast<hipStream_t>(stream));
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

extern "C" int om_conv2d_bf16_frozen_forward(const uint16_t* x, const float* w, int B, int cin, int H, int W, int cout, int ksize,
                                             int stride, const float* gamma, const float* beta, const float* running_mean,
                                             const float* running_var, double eps, float slope, const uint16_t* residual,
                                             uint16_t* y, om_stream stream) {
    OM_REQUIRE(x && w && y && gamma && beta && running_mean && running_var, OM_EINVAL, "om_conv2d_bf16_frozen_forward: null pointer");
    OM_REQUIRE(y != x && (const void*)y != (const void*)w && y != residual, OM_EINVAL,
               "om_conv2d_bf16_frozen_forward: y must not alias x, w or the residual (a workgroup reads what another has written)");
    om::ConvGeom g;
    if (!om::conv_geometry(B, cin, H, W, cout, ksize, stride, &g))
        return om::conv_geometry_refused("om_conv2d_bf16_frozen_forward", B, cin, H, W, cout, ksize, stride);
    OM_REQUIRE(eps > 0.0, OM_EINVAL, "om_conv2d_bf16_frozen_forward: eps %g", eps);
    om::FwdBf16Args a = om::make_bf16(g, x, w, y);
    a.gamma = gamma; a.beta = beta; a.running_mean = running_mean; a.running_var = running_var; a.residual = residual;
    a.eps = eps; a.slope = slope;
    om::launch_bf16_any<om::EPB_FROZEN>(a, ksize, stride, static_cast<hipStream_t>(stream));
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}
