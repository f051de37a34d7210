// bf16 <-> float32 for the kernels that take bf16 activations (bn_act.hip, route.hip): ONE definition of the two conversions, in
// plain integer arithmetic.  A bf16 is the upper half of a float32, so widening is exact.  Narrowing rounds to nearest, ties to
// even: adding 0x7fff plus the lowest kept bit carries into the kept half exactly when the dropped half is above a tie, or at a
// tie with the kept bit odd; the carry runs on into the exponent, so the largest finite values become inf, and subnormals need no
// case of their own.  NaN -> 0x7fc0.  This is torch's .to(torch.bfloat16), word for word (tests/bf16_np.py, tests/test_amp_cpu.py).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace om {

typedef uint16_t bf16_t;                          // the bits of a bfloat16

__device__ __forceinline__ float bf16_widen(uint32_t h) { return __uint_as_float(h << 16); }

__device__ __forceinline__ uint32_t bf16_round(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

}  // namespace om
