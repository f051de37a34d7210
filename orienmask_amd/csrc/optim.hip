// The optimizer step of the reference's training loop (trainer/trainer.py:53: torch.optim.SGD built by trainer/builder.py:118-130)
// as ONE launch over every tensor of every parameter group.  orienmask_amd/optim.py keeps the tables; this file is the kernel:
//   sgd_step_kernel   a grid of at most SGD_MAX_BLOCKS workgroups walks the chunk table (tensor, chunk-in-tensor), so the
//                     18-element orientation bias and the 4.7 M-element 3x3 weight are served by the same grid.  A chunk is
//                     OM_SGD_CHUNK elements: 16 B per lane per access where parameter, gradient and momentum buffer are all
//                     16-byte aligned, one element per lane otherwise (a view one element into a flat buffer) and for the last
//                     n % 4 elements.  lr, weight_decay, momentum, dampening and the three pointers come from the tensor's row
//                     of the DEVICE table: a scheduler step changes a row, never the launch.
// Arithmetic: torch.optim.SGD's, in torch-CPU's float32 rounding: every x.add(y, alpha=a) of the update
// is ONE fused multiply-add fma(y, float32(a), x); buf.mul_(momentum) is a product rounded on its own.  The fmas are written out
// and the file is built with -ffp-contract=off, so the compiler neither splits them nor folds buf * momentum into the next one.
#include "om_common.h"

namespace om {

constexpr int SGD_THREADS = 256;
constexpr int SGD_MAX_BLOCKS = 2048;                                   // 256 CUs x 8 workgroups; the rest is grid-strided
constexpr int SGD_VEC_PER_THREAD = OM_SGD_CHUNK / 4 / SGD_THREADS;     // float4 accesses per thread and stream in a chunk
static_assert(OM_SGD_CHUNK % (4 * SGD_THREADS) == 0, "a chunk is a whole number of float4 rounds of the workgroup");
static_assert(sizeof(om_sgd_tensor) == 64 && sizeof(om_sgd_chunk) == 8, "table rows as orienmask_amd/optim.py packs them");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gfloat4;

struct SgdHyper {
    float neg_lr, wd, momentum, one_minus_damp;
    bool has_wd, has_mom, first, nesterov, maximize;
};

// one element of torch.optim.SGD's update; `buf` is read only when has_mom && !first, and is the value to store when has_mom
__device__ __forceinline__ float sgd_element(const SgdHyper& h, float p, float g, float& buf) {
    float d = h.maximize ? -g : g;
    if (h.has_wd) d = fmaf(p, h.wd, d);
    if (h.has_mom) {
        if (h.first) {
            buf = d;
        } else {
            const float scaled = buf * h.momentum;          // rounded before the fma (buf.mul_(momentum))
            buf = fmaf(d, h.one_minus_damp, scaled);
        }
        d = h.nesterov ? fmaf(buf, h.momentum, d) : buf;
    }
    return fmaf(d, h.neg_lr, p);
}

__global__ void __launch_bounds__(SGD_THREADS)
sgd_step_kernel(const om_sgd_tensor* __restrict__ tensors, int n_tensors, const om_sgd_chunk* __restrict__ chunks, int n_chunks) {
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const om_sgd_chunk ck = chunks[c];
        if ((unsigned)ck.tensor >= (unsigned)n_tensors || ck.chunk < 0) continue;
        const om_sgd_tensor t = tensors[ck.tensor];
        const long long n = t.n;
        const long long start = (long long)ck.chunk * OM_SGD_CHUNK;
        if ((t.flags & OM_SGD_SKIP) || start >= n) continue;
        SgdHyper h;
        h.neg_lr = t.neg_lr; h.wd = t.weight_decay; h.momentum = t.momentum; h.one_minus_damp = t.one_minus_dampening;
        h.has_wd = t.flags & OM_SGD_HAS_WD; h.has_mom = (t.flags & OM_SGD_HAS_MOMENTUM) && t.buf;
        h.first = t.flags & OM_SGD_FIRST; h.nesterov = t.flags & OM_SGD_NESTEROV; h.maximize = t.flags & OM_SGD_MAXIMIZE;
        const bool read_buf = h.has_mom && !h.first;
        // the pointers come out of the table: tell the compiler they are global memory (global_load, not flat_load)
        gfloat* __restrict__ P = (gfloat*)t.param;
        const gfloat* __restrict__ G = (const gfloat*)t.grad;
        gfloat* __restrict__ Bf = (gfloat*)t.buf;
        const long long stop = (start + OM_SGD_CHUNK < n) ? start + OM_SGD_CHUNK : n;
        const bool aligned = ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) |
                               (h.has_mom ? reinterpret_cast<uintptr_t>(t.buf) : (uintptr_t)0)) & 15) == 0;
        if (aligned) {
            // start is a multiple of 4, so the chunk's float4s are [start / 4, stop / 4) and at most 3 elements remain
            const long long v0 = start / 4, v1 = stop / 4;
            gfloat4* P4 = (gfloat4*)P;
            const gfloat4* G4 = (const gfloat4*)G;
            gfloat4* B4 = (gfloat4*)Bf;
            f32x4 p[SGD_VEC_PER_THREAD], g[SGD_VEC_PER_THREAD], b[SGD_VEC_PER_THREAD];
#pragma unroll
            for (int k = 0; k < SGD_VEC_PER_THREAD; ++k) {
                const long long i = v0 + k * SGD_THREADS + threadIdx.x;
                if (i < v1) {
                    p[k] = P4[i];
                    g[k] = G4[i];
                    b[k] = read_buf ? B4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int k = 0; k < SGD_VEC_PER_THREAD; ++k) {
                const long long i = v0 + k * SGD_THREADS + threadIdx.x;
                if (i < v1) {
                    f32x4 q, nb;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float bv = b[k][e];
                        q[e] = sgd_element(h, p[k][e], g[k][e], bv);
                        nb[e] = bv;
                    }
                    P4[i] = q;
                    if (h.has_mom) B4[i] = nb;
                }
            }
            const long long i = v1 * 4 + threadIdx.x;       // the tail of an element count that is not a multiple of 4
            if (i < stop) {
                float bv = read_buf ? Bf[i] : 0.f;
                P[i] = sgd_element(h, P[i], G[i], bv);
                if (h.has_mom) Bf[i] = bv;
            }
        } else {
            for (long long i = start + threadIdx.x; i < stop; i += SGD_THREADS) {
                float bv = read_buf ? Bf[i] : 0.f;
                P[i] = sgd_element(h, P[i], G[i], bv);
                if (h.has_mom) Bf[i] = bv;
            }
        }
    }
}

}  // namespace om

extern "C" {

int om_sgd_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                om_stream stream) {
    OM_REQUIRE(table && chunks, OM_EINVAL, "om_sgd_step: null table");
    OM_REQUIRE(n_tensors > 0 && n_chunks > 0, OM_EINVAL, "om_sgd_step: %d tensors in %d chunks", n_tensors, n_chunks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (table_host) {       // the rows are at hand: refuse a row the kernel could only pass over
        for (int i = 0; i < n_tensors; ++i) {
            const om_sgd_tensor& t = table_host[i];
            if (t.flags & OM_SGD_SKIP) continue;
            OM_REQUIRE(t.param && t.grad && t.n > 0 && (!(t.flags & OM_SGD_HAS_MOMENTUM) || t.buf), OM_EINVAL,
                       "om_sgd_step: row %d has a null pointer or no elements", i);
        }
        OM_CHECK_HIP(hipMemcpyAsync(table, table_host, (size_t)n_tensors * sizeof(om_sgd_tensor), hipMemcpyHostToDevice, st));
    }
    const int blocks = n_chunks < om::SGD_MAX_BLOCKS ? n_chunks : om::SGD_MAX_BLOCKS;
    hipLaunchKernelGGL(om::sgd_step_kernel, dim3(blocks), dim3(om::SGD_THREADS), 0, st, table, n_tensors, chunks, n_chunks);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // extern "C"
