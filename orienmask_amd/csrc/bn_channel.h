// The per-channel arithmetic of the BatchNorm + LeakyReLU block, shared by bn_act.hip (training and eval passes over a stored
// convolution output) and conv_fwd.hip (the frozen block's epilogue, on the convolution's double sum).  One definition, so z has
// the same bits wherever it is computed from the same operands.  Nothing here contains a multiply followed by an add that the
// compiler could contract: the only fused operation is the explicit fma of bn_z, so the bits do not depend on -ffp-contract.
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

}  // namespace om
