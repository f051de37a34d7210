// The per-channel arithmetic of the BatchNorm + LeakyReLU block, shared by bn_act.hip (training and eval passes over a stored
// convolution output) and conv_fwd.hip (the frozen block's epilogue, on the convolution's double sum).  One definition, so z has
// the same bits wherever it is computed from the same operands.  Nothing here contains a multiply followed by an add that the
// compiler could contract, except frozen_out, which switches contraction off for itself: the only fused operation is the explicit
// fma of bn_z, so the bits do not depend on -ffp-contract.
#pragma once

namespace om {

// What the element-wise passes know about a channel, in double.  mean and invstd are carried as float32 pairs (value, remainder) in
// the save vectors, so the backward rebuilds exactly the doubles the forward used and z has the same bits in both.
struct BnChannel {
    double mean, invstd, w, beta;      // w = gamma * invstd
};

__device__ __forceinline__ void split_hi_lo(double v, float& hi, float& lo) {
    hi = (float)v;
    lo = (float)(v - (double)hi);
}

__device__ __forceinline__ BnChannel bn_channel(float mean_hi, float mean_lo, float invstd_hi, float invstd_lo, float gamma, float beta) {
    BnChannel ch;
    ch.mean = (double)mean_hi + (double)mean_lo;
    ch.invstd = (double)invstd_hi + (double)invstd_lo;
    ch.w = (double)gamma * ch.invstd;
    ch.beta = (double)beta;
    return ch;
}

// What z needs of a channel: the record the frozen convolution's epilogue keeps per output channel (conv_fwd.hip).
struct BnAffine {
    double mean, w, beta;              // w = gamma * invstd
};

// z = gamma * xhat + beta: THE expression of the forward and of the backward's mask (one fma on exact operands).  x is a stored
// float32 activation widened by the caller's conversion, or the frozen convolution's double sum.
__device__ __forceinline__ double bn_z(double x, double mean, double w, double beta) { return fma(x - mean, w, beta); }
__device__ __forceinline__ double bn_z(double x, const BnChannel& ch) { return bn_z(x, ch.mean, ch.w, ch.beta); }
__device__ __forceinline__ double bn_z(double x, const BnAffine& ch) { return bn_z(x, ch.mean, ch.w, ch.beta); }

// The record of a frozen channel from its running statistics: exactly the doubles bn_fwd_kernel's EVAL phase builds (invstd =
// 1/sqrt((double)running_var + eps) carried through split_hi_lo, mean = (double)running_mean).  conv_fwd.hip and conv_fwd_bf16.hip
// build it once per channel and workgroup.
__device__ __forceinline__ BnAffine bn_affine_eval(float running_mean, float running_var, double eps, float gamma, float beta) {
    float invstd_hi, invstd_lo;
    split_hi_lo(1.0 / sqrt((double)running_var + eps), invstd_hi, invstd_lo);
    const BnChannel ch = bn_channel(running_mean, 0.f, invstd_hi, invstd_lo, gamma, beta);
    return BnAffine{ch.mean, ch.w, ch.beta};
}

// The frozen block's output for one element: fwd_apply's expressions (bn_act.hip, built with -ffp-contract=off) on the convolution
// sum h (conv_fwd.hip: its double sum; conv_fwd_bf16.hip: its float32 accumulator widened).  The convolution files are built with
// contraction on, and z * slope + res must stay a rounded product and a rounded sum: the pragma takes the contract flag off the
// operations written in this function (the __dmul_rn / __dadd_rn intrinsics are plain operators in the toolchain's header, which a
// later inlining pass could still fuse); bn_z's only fused operation is its explicit fma.
__device__ __forceinline__ float frozen_out(double h, const BnAffine& ch, double slope, bool has_res, float res) {
#pragma clang fp contract(off)
    const double z = bn_z(h, ch);
    double y = z > 0.0 ? z : z * slope;
    if (has_res) y = y + (double)res;
    return (float)y;                                        // the only rounding to float32
}

}  // namespace om
