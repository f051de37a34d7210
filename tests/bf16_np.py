"""numpy bit-level restatement of the float32 <-> bf16 conversions of the _bf16 kernels (csrc/bn_act.hip, csrc/route.hip), shared by
the amp tests.

  round_bits   float32 array -> uint16 bf16 bits, round to nearest, ties to even: add 0x7fff plus the lowest kept bit to the word
               and keep the upper half; the carry runs into the exponent, so the largest finite values round to inf; NaN -> 0x7fc0
               (what torch's .to(torch.bfloat16) gives)
  widen        uint16 bf16 bits -> the float32 with those upper 16 bits, exactly
  quantise     float32 array -> the float32 array of its bf16-rounded values

test_amp_cpu.py holds round_bits to torch.Tensor.to(torch.bfloat16) on the CPU; the GPU tests then use it as the rounding of the
fp32 kernels' outputs that the bf16 kernels' outputs must equal bit for bit."""
import numpy as np


def round_bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    out = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7fffffff) > 0x7f800000
    out[nan] = 0x7fc0
    return out


def widen(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def quantise(a):
    return widen(round_bits(a))
