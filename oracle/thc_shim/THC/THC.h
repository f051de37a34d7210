// Minimal stand-in for the THC header that eval/src/nms_kernel.cu includes.  TEST INFRASTRUCTURE ONLY (oracle/build_ref_cuda.py).
// torch >= 1.11 no longer ships THC; nms_kernel.cu needs only these four names from it.  The build runs this file through torch's
// hipify together with the staged kernel source, so it is written in CUDA spelling.
#pragma once
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDACachingAllocator.h>
#include <c10/util/Exception.h>

struct THCState;

template <typename T>
__host__ __device__ inline T THCCeilDiv(T a, T b) {
  return (a + b - 1) / b;
}

// the caching allocator stands in for THC's; the state argument is unused (the staged source passes nullptr)
inline void* THCudaMalloc(THCState*, size_t bytes) { return c10::cuda::CUDACachingAllocator::raw_alloc(bytes); }
inline void THCudaFree(THCState*, void* p) { c10::cuda::CUDACachingAllocator::raw_delete(p); }

// Checks the status and then waits for the current stream.  CUDA returns from a device-to-host cudaMemcpyAsync into pageable
// memory only once the copy is done, and nms_cuda reads mask_host right after that call; the wait keeps that guarantee.
#define THCudaCheck(expr)                                                                      \
  do {                                                                                         \
    const cudaError_t thc_err_ = (expr);                                                       \
    TORCH_CHECK(thc_err_ == cudaSuccess, "THCudaCheck: ", cudaGetErrorString(thc_err_));       \
    const cudaError_t thc_sync_ = cudaStreamSynchronize(at::cuda::getCurrentCUDAStream());     \
    TORCH_CHECK(thc_sync_ == cudaSuccess, "THCudaCheck: ", cudaGetErrorString(thc_sync_));     \
  } while (0)
