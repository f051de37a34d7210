// The optimizer step of the reference's training loop (trainer/trainer.py:53: torch.optim.SGD built by trainer/builder.py:118-130)
// and of the Adam family, as ONE launch over every tensor of every parameter group.  orienmask_amd/optim.py keeps the tables; this
// file is the kernels.  DESIGN.md section 3.16 has the arithmetic and the protocols; here is how the file is put together.
//
// The work list.  A grid of at most SGD_MAX_BLOCKS workgroups strides over the chunk table (tensor, chunk-in-tensor), so the
// 18-element orientation bias and the 4.7 M-element 3x3 weight are served by the same grid.  A chunk is OM_SGD_CHUNK elements of one
// row of the DEVICE table (om_sgd_tensor or om_adam_tensor): pointers and hyper-parameters come from the row, so a scheduler step
// changes a row, never the launch.  with_chunk is the one decode of a chunk; all four kernels below run their chunk's work in it.
//
//   step_kernel<Rule, CLIP, EMA>   the walker.  Per chunk it asks the rule to prepare the row, then walks the parameter, the
//                     gradient, the rule's state streams and (EMA) the tensor's float32 shadow: 16 B per lane per access where every
//                     stream it touches is 16-byte aligned, all loads of a chunk ahead of its arithmetic; one element per lane for
//                     the last n % 4 elements and for a chunk with a misaligned stream (a view one element into a flat buffer).
//                     CLIP: coefficient and skip decision come from the state block clip_finish_kernel wrote; every gradient
//                     element enters the update as g * coef, rounded once, and a skipped step returns before it touches anything.
//                     EMA: with the new parameter p' still in registers, e' = ema_element(p', e, omd); the shadow pointers come from
//                     a device array of their own (null = not averaged); omd = float32(1 - decay_k) is an argument in the plain
//                     form and a word of the EMA state block in the clipped form.  Parameter and state get the bits they get
//                     without it.  The walker owns the shadow; a rule never sees it.
//   SgdRule, AdamRule   what differs between the update rules: the row type, the clip-side arguments (SgdClip / AdamClip), the
//                     number of state streams (the momentum buffer; exp_avg and exp_avg_sq), the preparation of a row -- its
//                     hyper-parameters, whether state is read and whether it is written, under CLIP from the device-side words
//                     (SGD: valid_since decides a tensor's first step; Adam: the applied-step count selects the bias corrections
//                     from a host-built table, no pow on the device) -- and the element function (sgd_element / adam_element).
//   grad_sumsq_kernel<Row>   (clipping) the same grid over the same chunk table: one float64 sum of squared gradient elements per
//                     chunk into `partials`.  Element j of a chunk belongs to lane (j / 4) % 256 whatever the gradient's alignment; a
//                     lane adds its elements in ascending order, the 256 lanes are combined by a fixed tree (block_tree_sum).  A
//                     float32 square is exact in float64, so the norm's bits depend on values and element counts alone.
//   clip_finish_kernel<Rule, EMA>   (clipping) ONE workgroup: lane l adds partials l, l + 256, ... in ascending order, the same tree,
//                     then lane 0 decides (clip_decide: norm, torch's coefficient, skip, the running statistics, under EMA the decay
//                     of this update and its count) with plain stores into the state block.  For a rule that counts applied steps
//                     on the device (Adam), lane l then adds 1 to the count of rows l, l + 256, ... that are flagged
//                     OM_ADAM_DEVICE_COUNTED and not skipped, unless the step is skipped (one writer per word).
//   ema_swap_kernel<Row>   the same grid over the same chunk table: parameter and shadow exchanged as raw 32-bit words.
// No atomics anywhere: a step repeats bit for bit.
//
// Arithmetic: torch's, in torch-CPU's float32 rounding.  Every fused multiply-add and every separately rounded operation is
// written out (fmaf, __fmul_rn, ...) and the file is built with -ffp-contract=off, so the compiler neither splits nor forms one.
//
// Host side: each extern "C" entry checks its own arguments and makes one call of run_step<Rule> (stage the table, size the grid,
// pick the <CLIP, EMA> instance, launch one or three kernels) or run_swap<Row>.
#include "om_common.h"

// one tensor of the Adam step as orienmask_amd/optim.py packs it (ADAM_ROW); include/orienmask_hip.h documents the fields
struct om_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    double lr;
    float w, beta2, omb2, eps;
    float weight_decay, dm, nss, bc2s;
    int32_t bias_table;
    uint32_t flags;
    uint32_t reserved[2];
};
static_assert(sizeof(om_adam_tensor) == 96 && offsetof(om_adam_tensor, lr) == 40 && offsetof(om_adam_tensor, flags) == 84,
              "the Adam row as orienmask_amd/optim.py packs it");
static_assert(OM_ADAM_SKIP == OM_SGD_SKIP, "the norm kernel and the walker test one bit for both row types");

namespace om {

constexpr int SGD_THREADS = 256;
constexpr int SGD_MAX_BLOCKS = 2048;                                   // 256 CUs x 8 workgroups; the rest is grid-strided
constexpr int SGD_VEC_PER_THREAD = OM_SGD_CHUNK / 4 / SGD_THREADS;     // float4 accesses per thread and stream in a chunk
static_assert(OM_SGD_CHUNK % (4 * SGD_THREADS) == 0, "a chunk is a whole number of float4 rounds of the workgroup");
static_assert(sizeof(om_sgd_tensor) == 64 && sizeof(om_sgd_chunk) == 8, "table rows as orienmask_amd/optim.py packs them");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gfloat4;

// chunk c of the work list: body(t, slot, start, stop) with the chunk's row, the row's slot in the table and its elements
// [start, stop) -- unless the chunk is passed over (an entry that points outside the table, or past the row's end).  The row's
// flags are the body's business.  c is the same for the whole workgroup, and so is everything derived here.  A callback, not
// out-parameters: the body is compiled knowing 0 <= start < stop, as it was when the decode stood in each kernel.
template <class Row, class Body>
__device__ __forceinline__ void with_chunk(const Row* __restrict__ tensors, int n_tensors, const om_sgd_chunk* __restrict__ chunks,
                                           int c, Body&& body) {
    const om_sgd_chunk ck = chunks[c];
    if ((unsigned)ck.tensor >= (unsigned)n_tensors || ck.chunk < 0) return;
    const Row t = tensors[ck.tensor];
    const long long n = t.n;
    const long long start = (long long)ck.chunk * OM_SGD_CHUNK;
    if (start >= n) return;
    body(t, ck.tensor, start, (start + OM_SGD_CHUNK < n) ? start + OM_SGD_CHUNK : n);
}

// the sum of one double per lane over the workgroup in a FIXED order: within a wave lane l takes l ^ 32, ^ 16, ... ^ 1 (after the
// step with distance d, lanes l < d hold the sums of the pairs (l, l + d) of the step before), then (w0 + w1) + (w2 + w3) over the
// four waves through LDS.  The result is valid in thread 0.  tests/clip_np.py restates this order.
__device__ __forceinline__ double block_tree_sum(double v, double* wave_sums) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();                                        // the previous use of wave_sums has been read
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    return (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
}
static_assert(SGD_THREADS == 256, "block_tree_sum combines four waves of 64");

template <class Row>
__global__ void __launch_bounds__(SGD_THREADS)
grad_sumsq_kernel(const Row* __restrict__ tensors, int n_tensors, const om_sgd_chunk* __restrict__ chunks, int n_chunks,
                  double* __restrict__ partials) {
    __shared__ double wave_sums[SGD_THREADS / 64];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        double acc = 0.0;
        with_chunk(tensors, n_tensors, chunks, c, [&](const Row& t, int, long long start, long long stop) {
            if (t.flags & OM_SGD_SKIP) return;
            const gfloat* __restrict__ G = (const gfloat*)t.grad;
            const bool aligned = (reinterpret_cast<uintptr_t>(t.grad) & 15) == 0;
            const gfloat4* G4 = (const gfloat4*)G;
            f32x4 g[SGD_VEC_PER_THREAD];
            // group i of four elements [4 i, 4 i + 4) belongs to lane (i - start / 4) % 256 in both forms
#pragma unroll
            for (int k = 0; k < SGD_VEC_PER_THREAD; ++k) {
                const long long i = start / 4 + k * SGD_THREADS + threadIdx.x;
                if (aligned && 4 * i + 4 <= stop) {
                    g[k] = G4[i];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[k][e] = (4 * i + e < stop) ? G[4 * i + e] : 0.f;     // + 0.0 changes no sum
                }
            }
#pragma unroll
            for (int k = 0; k < SGD_VEC_PER_THREAD; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double x = (double)g[k][e];
                    acc += x * x;                           // the square of a float32 is exact in float64
                }
        });
        const double total = block_tree_sum(acc, wave_sums);
        if (threadIdx.x == 0) partials[c] = total;          // every chunk writes: a passed-over one writes 0
    }
}

// what the averaging forms read beside the tables (unused by step_kernel<Rule, CLIP, false> and clip_finish_kernel<Rule, false>)
struct SgdEma {
    float* const* shadows;      // n_tensors device pointers, null = the tensor is not averaged
    double* state;              // the OM_EMA_* block (clipped form; null in the plain form)
    float omd;                  // float32(1 - decay_k) of this step (plain form: the host knows k)
    double decay;               // clipped form: clip_finish_kernel<Rule, true> derives omd on the device
    int warmup;
};

// the decision of a clipped step, taken by ONE lane from the sum of squares S: norm, coefficient, skip and the running statistics
// into the state block, and under EMA the decay of this update and its count.  Returns the skip decision.
template <bool EMA>
__device__ __forceinline__ bool clip_decide(double S, float max_norm, int mode, long long step, double* __restrict__ state,
                                            const SgdEma& ema) {
    const float norm = (float)__dsqrt_rn(S);
    // torch: max_norm / (total_norm + 1e-6) is (total_norm + 1e-6).reciprocal() * max_norm, each operation rounded to float32
    float coef = __fmul_rn(__fdiv_rn(1.0f, __fadd_rn(norm, 1e-6f)), max_norm);
    if (coef > 1.0f) coef = 1.0f;                           // clamp(max=1): NaN stays NaN
    const bool finite = isfinite(norm);
    long long* words = reinterpret_cast<long long*>(state);
    state[OM_CLIP_NORM_OFF] = (double)norm;
    state[OM_CLIP_COEF_OFF] = (double)coef;
    words[OM_CLIP_SKIP_OFF] = ((mode & OM_CLIP_SKIP_NONFINITE) && !finite) ? 1 : 0;
    words[OM_CLIP_STEPS_OFF] += 1;
    if (finite) {
        state[OM_CLIP_SUM_OFF] += (double)norm;
        if ((double)norm > state[OM_CLIP_MAX_OFF]) state[OM_CLIP_MAX_OFF] = (double)norm;
        if (coef < 1.0f) words[OM_CLIP_CLIPPED_OFF] += 1;
    } else {
        words[OM_CLIP_NONFINITE_OFF] += 1;
        if (words[OM_CLIP_FIRST_NONFINITE_OFF] == 0) words[OM_CLIP_FIRST_NONFINITE_OFF] = step;
    }
    if constexpr (EMA) {
        // an applied step is one more EMA update: its decay from the count so far, in float64, rounded to float32 once
        if (words[OM_CLIP_SKIP_OFF] == 0) {
            long long* updates = reinterpret_cast<long long*>(ema.state) + OM_EMA_UPDATES_OFF;
            const double k = (double)*updates;
            double d = ema.decay;
            if (ema.warmup) {
                const double ramp = (1.0 + k) / (10.0 + k);
                if (ramp < d) d = ramp;
            }
            ema.state[OM_EMA_OMD_OFF] = (double)(float)(1.0 - d);
            *updates += 1;
        }
    }
    return words[OM_CLIP_SKIP_OFF] != 0;
}

// `words` is the rule's per-tensor int64 array: read only where the rule counts applied steps there (Rule::COUNTED)
template <class Rule, bool EMA>
__global__ void __launch_bounds__(SGD_THREADS)
clip_finish_kernel(const double* __restrict__ partials, int n_chunks, float max_norm, int mode, long long step,
                   double* __restrict__ state, const SgdEma ema, const typename Rule::Row* __restrict__ tensors, int n_tensors,
                   long long* __restrict__ words) {
    __shared__ double wave_sums[SGD_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += SGD_THREADS) acc += partials[i];
    const double S = block_tree_sum(acc, wave_sums);
    bool skip = false;
    if (threadIdx.x == 0) skip = clip_decide<EMA>(S, max_norm, mode, step, state, ema);
    if constexpr (Rule::COUNTED) {
        __shared__ int skipped;
        if (threadIdx.x == 0) skipped = skip ? 1 : 0;
        __syncthreads();
        if (skipped) return;                                // every count stays
        for (int i = threadIdx.x; i < n_tensors; i += SGD_THREADS) {
            const unsigned f = tensors[i].flags;
            if ((f & OM_ADAM_DEVICE_COUNTED) && !(f & OM_ADAM_SKIP)) words[i] += 1;
        }
    }
}

// ---- the update rules -------------------------------------------------------------------------------------------------------
// A rule names its Row, Clip and Hyper types, STATES (its state streams) and COUNTED, and has two functions:
//   prepare<CLIP>(t, slot, clip, h, state, reads, writes)   the row's hyper-parameters into h, its state pointers into state[],
//                     and whether the state streams are read and written for this row.  A stream that is neither is not touched:
//                     it stays out of the alignment test and its pointer may be null.
//   element<CLIP>(h, coef, p, g, s)   one element's new parameter; s[] holds the state values read (0 where not) and receives the
//                     values to store.

// what the clipped form of the SGD step reads beside the tables
struct SgdClip {
    const double* state;        // the OM_CLIP_* block clip_finish_kernel wrote on this stream
    long long* valid_since;     // per tensor: the step that first applied an update to an OM_SGD_DEVICE_FIRST row, 0 = none yet
    long long step;             // this step's number (from 1)
};

struct SgdHyper {
    float neg_lr, wd, momentum, one_minus_damp;
    bool has_wd, has_mom, first, nesterov, maximize;
};

// one element of torch.optim.SGD's update; `buf` is read only when has_mom && !first, and is the value to store when has_mom
template <bool CLIP>
__device__ __forceinline__ float sgd_element(const SgdHyper& h, float coef, float p, float g, float& buf) {
    if constexpr (CLIP) g = __fmul_rn(g, coef);             // the clipped gradient, rounded once, ahead of everything else
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

struct SgdRule {
    typedef om_sgd_tensor Row;
    typedef SgdClip Clip;
    typedef SgdHyper Hyper;
    static constexpr int STATES = 1;                        // the momentum buffer
    static constexpr bool COUNTED = false;

    template <bool CLIP>
    static __device__ __forceinline__ void prepare(const Row& t, int slot, const Clip& clip, Hyper& h, float* (&state)[STATES],
                                                   bool& reads, bool& writes) {
        h.neg_lr = t.neg_lr; h.wd = t.weight_decay; h.momentum = t.momentum; h.one_minus_damp = t.one_minus_dampening;
        h.has_wd = t.flags & OM_SGD_HAS_WD; h.has_mom = (t.flags & OM_SGD_HAS_MOMENTUM) && t.buf;
        h.first = t.flags & OM_SGD_FIRST; h.nesterov = t.flags & OM_SGD_NESTEROV; h.maximize = t.flags & OM_SGD_MAXIMIZE;
        if constexpr (CLIP) {
            if ((t.flags & OM_SGD_DEVICE_FIRST) && h.has_mom) {
                // first = no step has been applied to this tensor yet.  Another chunk of the tensor may already have written this
                // step's number: both values mean "first", and every writer stores the same value.
                const long long since = clip.valid_since[slot];
                h.first = since == 0 || since == clip.step;
                if (since == 0 && threadIdx.x == 0) clip.valid_since[slot] = clip.step;
            }
        }
        state[0] = t.buf;                                   // null without momentum
        writes = h.has_mom;
        reads = h.has_mom && !h.first;                      // a first step writes a buffer the host left uninitialised
    }

    template <bool CLIP>
    static __device__ __forceinline__ float element(const Hyper& h, float coef, float p, float g, float (&s)[STATES]) {
        return sgd_element<CLIP>(h, coef, p, g, s[0]);
    }
};

// what the clipped Adam step reads beside the tables
struct AdamClip {
    const double* state;        // the OM_CLIP_* block clip_finish_kernel wrote on this stream
    const long long* counts;    // per tensor: applied steps INCLUDING this one (rows under OM_ADAM_DEVICE_COUNTED)
    const double* bias;         // the bias tables, one after the other: row k = (1 - beta1**k, (1 - beta2**k) ** 0.5)
    const long long* bias_dir;  // per table: (first row in `bias`, rows); from its last row on both corrections are 1.0
    int n_bias;
};

struct AdamHyper {
    float w, wm1, beta2, omb2, eps, wd, dm, nss, bc2s;
    bool low, maximize, has_wd, decoupled;
};

// one element of torch.optim.Adam / AdamW (_single_tensor_adam, amsgrad=False); m and v are read and are the values to store
template <bool CLIP>
__device__ __forceinline__ float adam_element(const AdamHyper& h, float coef, float p, float g, float& m, float& v) {
    if constexpr (CLIP) g = __fmul_rn(g, coef);             // the clipped gradient, rounded once, ahead of everything else
    if (h.maximize) g = -g;
    if (h.has_wd) {
        if (h.decoupled) p = __fmul_rn(p, h.dm);            // param.mul_(1 - lr * weight_decay)
        else g = fmaf(p, h.wd, g);                          // grad.add(param, alpha=weight_decay)
    }
    const float d = __fsub_rn(g, m);
    m = h.low ? fmaf(h.w, d, m) : fmaf(h.wm1, d, g);        // exp_avg.lerp_(grad, 1 - beta1): both weight branches of lerp
    v = fmaf(__fmul_rn(h.omb2, g), g, __fmul_rn(v, h.beta2));   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    // sqrtf and / are hipcc's correctly rounded forms (its default); __fsqrt_rn would be the 1-ulp native instruction
    const float den = __fadd_rn(sqrtf(v) / h.bc2s, h.eps);
    return __fadd_rn(p, __fdiv_rn(__fmul_rn(h.nss, m), den));   // addcdiv_: three roundings, no fma
}

struct AdamRule {
    typedef om_adam_tensor Row;
    typedef AdamClip Clip;
    typedef AdamHyper Hyper;
    static constexpr int STATES = 2;                        // exp_avg, exp_avg_sq
    static constexpr bool COUNTED = true;                   // clip_finish_kernel keeps the applied-step counts

    template <bool CLIP>
    static __device__ __forceinline__ void prepare(const Row& t, int slot, const Clip& clip, Hyper& h, float* (&state)[STATES],
                                                   bool& reads, bool& writes) {
        h.w = t.w; h.wm1 = __fsub_rn(t.w, 1.0f); h.beta2 = t.beta2; h.omb2 = t.omb2; h.eps = t.eps; h.wd = t.weight_decay;
        h.dm = t.dm; h.nss = t.nss; h.bc2s = t.bc2s;
        h.low = fabsf(t.w) < 0.5f; h.maximize = t.flags & OM_ADAM_MAXIMIZE; h.has_wd = t.flags & OM_ADAM_HAS_WD;
        h.decoupled = t.flags & OM_ADAM_DECOUPLED;
        if constexpr (CLIP) {
            if (t.flags & OM_ADAM_DEVICE_COUNTED) {
                // this step's number for this tensor is on the device alone: the corrections come from the host's table
                const long long k = clip.counts[slot];
                double bc1 = 1.0, bc2s = 1.0;
                if ((unsigned)t.bias_table < (unsigned)clip.n_bias) {
                    const long long first = clip.bias_dir[2 * t.bias_table], rows = clip.bias_dir[2 * t.bias_table + 1];
                    if (k >= 0 && k < rows) {
                        bc1 = clip.bias[2 * (first + k)];
                        bc2s = clip.bias[2 * (first + k) + 1];
                    }
                }
                h.nss = (float)(-__ddiv_rn(t.lr, bc1));
                h.bc2s = (float)bc2s;
            }
        }
        state[0] = t.exp_avg;
        state[1] = t.exp_avg_sq;
        reads = writes = true;
    }

    template <bool CLIP>
    static __device__ __forceinline__ float element(const Hyper& h, float coef, float p, float g, float (&s)[STATES]) {
        return adam_element<CLIP>(h, coef, p, g, s[0], s[1]);
    }
};

// ---- the walker -------------------------------------------------------------------------------------------------------------
// the shadow's update with the parameter's new value: the difference rounded once, then ONE fused multiply-add
__device__ __forceinline__ float ema_element(float p_new, float e, float omd) {
    return fmaf(__fsub_rn(p_new, e), omd, e);
}

template <class Rule, bool CLIP, bool EMA>
__global__ void __launch_bounds__(SGD_THREADS)
step_kernel(const typename Rule::Row* __restrict__ tensors, int n_tensors, const om_sgd_chunk* __restrict__ chunks, int n_chunks,
            const typename Rule::Clip clip, const SgdEma ema) {
    constexpr int STATES = Rule::STATES;
    float coef = 1.0f;
    if constexpr (CLIP) {
        if (reinterpret_cast<const long long*>(clip.state)[OM_CLIP_SKIP_OFF] != 0) return;      // nothing is touched
        coef = (float)clip.state[OM_CLIP_COEF_OFF];
    }
    float omd = 0.f;
    if constexpr (EMA) omd = CLIP ? (float)ema.state[OM_EMA_OMD_OFF] : ema.omd;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x)      // the callback is the loop's body and is indented as that
      with_chunk(tensors, n_tensors, chunks, c, [&](const typename Rule::Row& t, int slot, long long start, long long stop) {
        if (t.flags & OM_SGD_SKIP) return;
        typename Rule::Hyper h;
        float* state[STATES];
        bool reads, writes;
        Rule::template prepare<CLIP>(t, slot, clip, h, state, reads, writes);
        // the pointers come out of the table: tell the compiler they are global memory (global_load, not flat_load)
        gfloat* __restrict__ P = (gfloat*)t.param;
        const gfloat* __restrict__ G = (const gfloat*)t.grad;
        gfloat* __restrict__ S[STATES];
        gfloat* __restrict__ E = nullptr;                   // the shadow; null: this tensor is not averaged
        if constexpr (EMA) E = (gfloat*)ema.shadows[slot];
        const bool has_ema = EMA && E != nullptr;
        uintptr_t address_bits = reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) |
                                 (has_ema ? reinterpret_cast<uintptr_t>(E) : (uintptr_t)0);
#pragma unroll
        for (int s = 0; s < STATES; ++s) {
            S[s] = (gfloat*)state[s];
            address_bits |= writes ? reinterpret_cast<uintptr_t>(state[s]) : (uintptr_t)0;
        }
        long long scalar_from = start;
        if ((address_bits & 15) == 0) {
            // start is a multiple of 4, so the chunk's float4s are [start / 4, stop / 4) and at most 3 elements remain
            const long long v0 = start / 4, v1 = stop / 4;
            gfloat4* P4 = (gfloat4*)P;
            const gfloat4* G4 = (const gfloat4*)G;
            gfloat4* E4 = (gfloat4*)E;
            f32x4 p[SGD_VEC_PER_THREAD], g[SGD_VEC_PER_THREAD], st[STATES][SGD_VEC_PER_THREAD], e4[EMA ? SGD_VEC_PER_THREAD : 1];
#pragma unroll
            for (int k = 0; k < SGD_VEC_PER_THREAD; ++k) {
                const long long i = v0 + k * SGD_THREADS + threadIdx.x;
                if (i < v1) {
                    p[k] = P4[i];
                    g[k] = G4[i];
#pragma unroll
                    for (int s = 0; s < STATES; ++s) st[s][k] = reads ? ((gfloat4*)S[s])[i] : f32x4{0.f, 0.f, 0.f, 0.f};
                    if constexpr (EMA) e4[k] = has_ema ? E4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int k = 0; k < SGD_VEC_PER_THREAD; ++k) {
                const long long i = v0 + k * SGD_THREADS + threadIdx.x;
                if (i < v1) {
                    f32x4 q, ns[STATES], ne;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float sv[STATES];
#pragma unroll
                        for (int s = 0; s < STATES; ++s) sv[s] = st[s][k][e];
                        q[e] = Rule::template element<CLIP>(h, coef, p[k][e], g[k][e], sv);
#pragma unroll
                        for (int s = 0; s < STATES; ++s) ns[s][e] = sv[s];
                        if constexpr (EMA) ne[e] = ema_element(q[e], e4[k][e], omd);
                    }
                    P4[i] = q;
                    if (writes) {
#pragma unroll
                        for (int s = 0; s < STATES; ++s) ((gfloat4*)S[s])[i] = ns[s];
                    }
                    if constexpr (EMA) {
                        if (has_ema) E4[i] = ne;
                    }
                }
            }
            scalar_from = v1 * 4;                           // the tail of an element count that is not a multiple of 4
        }
        for (long long i = scalar_from + threadIdx.x; i < stop; i += SGD_THREADS) {
            float sv[STATES];
#pragma unroll
            for (int s = 0; s < STATES; ++s) sv[s] = reads ? S[s][i] : 0.f;
            const float ev = has_ema ? E[i] : 0.f;
            const float q = Rule::template element<CLIP>(h, coef, P[i], G[i], sv);
            P[i] = q;
            if (writes) {
#pragma unroll
                for (int s = 0; s < STATES; ++s) S[s][i] = sv[s];
            }
            if (has_ema) E[i] = ema_element(q, ev, omd);
        }
      });
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned int guint;
typedef __attribute__((address_space(1))) u32x4 guint4;

// parameter <-> shadow, element for element, as 32-bit words (a NaN keeps its payload); rows without a shadow are passed over, a
// row's flags are not read (a tensor that had no gradient in the latest step is exchanged like any other)
template <class Row>
__global__ void __launch_bounds__(SGD_THREADS)
ema_swap_kernel(const Row* __restrict__ tensors, int n_tensors, const om_sgd_chunk* __restrict__ chunks, int n_chunks,
                float* const* __restrict__ shadows) {
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x)
      with_chunk(tensors, n_tensors, chunks, c, [&](const Row& t, int slot, long long start, long long stop) {
        guint* __restrict__ P = (guint*)t.param;
        guint* __restrict__ E = (guint*)shadows[slot];
        if (!P || !E) return;
        const bool aligned = ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(shadows[slot])) & 15) == 0;
        long long scalar_from = start;
        if (aligned) {
            const long long v0 = start / 4, v1 = stop / 4;
            guint4* P4 = (guint4*)P;
            guint4* E4 = (guint4*)E;
            u32x4 p[SGD_VEC_PER_THREAD], e[SGD_VEC_PER_THREAD];
#pragma unroll
            for (int k = 0; k < SGD_VEC_PER_THREAD; ++k) {
                const long long i = v0 + k * SGD_THREADS + threadIdx.x;
                if (i < v1) {
                    p[k] = P4[i];
                    e[k] = E4[i];
                }
            }
#pragma unroll
            for (int k = 0; k < SGD_VEC_PER_THREAD; ++k) {
                const long long i = v0 + k * SGD_THREADS + threadIdx.x;
                if (i < v1) {
                    P4[i] = e[k];
                    E4[i] = p[k];
                }
            }
            scalar_from = v1 * 4;                           // at most 3 elements remain
        }
        for (long long i = scalar_from + threadIdx.x; i < stop; i += SGD_THREADS) {
            const unsigned int pv = P[i], ev = E[i];
            P[i] = ev;
            E[i] = pv;
        }
      });
}

}  // namespace om

namespace {

inline bool row_ok(const om_sgd_tensor& t) { return t.param && t.grad && t.n > 0 && (!(t.flags & OM_SGD_HAS_MOMENTUM) || t.buf); }
inline bool row_ok(const om_adam_tensor& t) { return t.param && t.grad && t.exp_avg && t.exp_avg_sq && t.n > 0; }

// the checks and the table copy every entry shares; `who` names the entry in the message
template <class Row>
int stage_table(const char* who, const Row* table_host, Row* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                bool rows_are_stepped, hipStream_t st) {
    OM_REQUIRE(table && chunks, OM_EINVAL, "%s: null table", who);
    OM_REQUIRE(n_tensors > 0 && n_chunks > 0, OM_EINVAL, "%s: %d tensors in %d chunks", who, n_tensors, n_chunks);
    if (table_host) {       // the rows are at hand: refuse a row the kernel could only pass over
        for (int i = 0; i < n_tensors && rows_are_stepped; ++i) {
            const Row& t = table_host[i];
            if (t.flags & OM_SGD_SKIP) continue;
            OM_REQUIRE(row_ok(t), OM_EINVAL, "%s: row %d has a null pointer or no elements", who, i);
        }
        OM_CHECK_HIP(hipMemcpyAsync(table, table_host, (size_t)n_tensors * sizeof(Row), hipMemcpyHostToDevice, st));
    }
    return OM_OK;
}

int check_clip(const char* who, const double* partials, const double* state, const long long* valid_since, float max_norm,
               int mode, long long step) {
    OM_REQUIRE(partials && state && valid_since, OM_EINVAL, "%s: null pointer", who);
    OM_REQUIRE(max_norm > 0.f && std::isfinite(max_norm), OM_EINVAL, "%s: max_norm %g is not positive and finite", who,
               (double)max_norm);
    OM_REQUIRE((mode & ~OM_CLIP_SKIP_NONFINITE) == 0 && step >= 1, OM_EINVAL, "%s: mode %d, step %lld", who, mode, step);
    OM_REQUIRE((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(state) |
                reinterpret_cast<uintptr_t>(valid_since)) % 8 == 0, OM_EINVAL, "%s: misaligned pointer", who);
    return OM_OK;
}

inline int grid_of(int n_chunks) { return n_chunks < om::SGD_MAX_BLOCKS ? n_chunks : om::SGD_MAX_BLOCKS; }

// the norm's side of a clipped step; partials == null: the plain step, one launch
struct ClipNorm {
    double* partials;
    double* state;
    long long* words;           // the rule's per-tensor int64 array (valid_since / counts)
    float max_norm;
    int mode;
    long long step;
};

template <class Rule, bool CLIP, bool EMA>
int launch_step(typename Rule::Row* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks, const ClipNorm& norm,
                const typename Rule::Clip& clip, const om::SgdEma& ema, hipStream_t st) {
    const dim3 grid(grid_of(n_chunks)), block(om::SGD_THREADS);
    if constexpr (CLIP) {
        hipLaunchKernelGGL(om::grad_sumsq_kernel<typename Rule::Row>, grid, block, 0, st, table, n_tensors, chunks, n_chunks,
                           norm.partials);
        OM_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL((om::clip_finish_kernel<Rule, EMA>), dim3(1), block, 0, st, norm.partials, n_chunks, norm.max_norm,
                           norm.mode, norm.step, norm.state, ema, table, n_tensors, norm.words);
        OM_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((om::step_kernel<Rule, CLIP, EMA>), grid, block, 0, st, table, n_tensors, chunks, n_chunks, clip, ema);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

// every step entry after its own argument checks: the table, then the step in its form (averaged: ema.shadows is not null)
template <class Rule>
int run_step(const char* who, const typename Rule::Row* table_host, typename Rule::Row* table, int n_tensors,
             const om_sgd_chunk* chunks, int n_chunks, const ClipNorm& norm, const typename Rule::Clip& clip, const om::SgdEma& ema,
             hipStream_t st) {
    if (int rc = stage_table(who, table_host, table, n_tensors, chunks, n_chunks, true, st)) return rc;
    if (norm.partials)
        return ema.shadows ? launch_step<Rule, true, true>(table, n_tensors, chunks, n_chunks, norm, clip, ema, st)
                           : launch_step<Rule, true, false>(table, n_tensors, chunks, n_chunks, norm, clip, ema, st);
    return ema.shadows ? launch_step<Rule, false, true>(table, n_tensors, chunks, n_chunks, norm, clip, ema, st)
                       : launch_step<Rule, false, false>(table, n_tensors, chunks, n_chunks, norm, clip, ema, st);
}

template <class Row>
int run_swap(const char* who, const Row* table_host, Row* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
             float* const* shadows, hipStream_t st) {
    OM_REQUIRE(shadows, OM_EINVAL, "%s: null shadows", who);
    if (int rc = stage_table(who, table_host, table, n_tensors, chunks, n_chunks, false, st)) return rc;
    hipLaunchKernelGGL(om::ema_swap_kernel<Row>, dim3(grid_of(n_chunks)), dim3(om::SGD_THREADS), 0, st, table, n_tensors, chunks,
                       n_chunks, shadows);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // namespace

extern "C" {

int om_sgd_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                om_stream stream) {
    return run_step<om::SgdRule>("om_sgd_step", table_host, table, n_tensors, chunks, n_chunks, ClipNorm{}, om::SgdClip{},
                                 om::SgdEma{}, static_cast<hipStream_t>(stream));
}

int om_sgd_ema_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                    float* const* shadows, float omd, om_stream stream) {
    OM_REQUIRE(shadows, OM_EINVAL, "om_sgd_ema_step: null shadows");
    OM_REQUIRE(omd > 0.f && omd <= 1.f, OM_EINVAL, "om_sgd_ema_step: omd %g is not 1 - decay of a decay in [0, 1)", (double)omd);
    return run_step<om::SgdRule>("om_sgd_ema_step", table_host, table, n_tensors, chunks, n_chunks, ClipNorm{}, om::SgdClip{},
                                 om::SgdEma{shadows, nullptr, omd, 0.0, 0}, static_cast<hipStream_t>(stream));
}

int om_sgd_clip_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                     double* partials, double* state, long long* valid_since, float max_norm, int mode, long long step,
                     om_stream stream) {
    OM_REQUIRE(table && chunks, OM_EINVAL, "om_sgd_clip_step: null pointer");
    if (int rc = check_clip("om_sgd_clip_step", partials, state, valid_since, max_norm, mode, step)) return rc;
    return run_step<om::SgdRule>("om_sgd_clip_step", table_host, table, n_tensors, chunks, n_chunks,
                                 ClipNorm{partials, state, valid_since, max_norm, mode, step},
                                 om::SgdClip{state, valid_since, step}, om::SgdEma{}, static_cast<hipStream_t>(stream));
}

int om_sgd_clip_ema_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks,
                         int n_chunks, double* partials, double* state, long long* valid_since, float max_norm, int mode,
                         long long step, float* const* shadows, double* ema_state, double decay, int warmup, om_stream stream) {
    OM_REQUIRE(table && chunks && shadows && ema_state, OM_EINVAL, "om_sgd_clip_ema_step: null pointer");
    if (int rc = check_clip("om_sgd_clip_ema_step", partials, state, valid_since, max_norm, mode, step)) return rc;
    OM_REQUIRE(reinterpret_cast<uintptr_t>(ema_state) % 8 == 0, OM_EINVAL, "om_sgd_clip_ema_step: misaligned pointer");
    OM_REQUIRE(decay > 0.0 && decay < 1.0, OM_EINVAL, "om_sgd_clip_ema_step: decay %g is not inside (0, 1)", decay);
    return run_step<om::SgdRule>("om_sgd_clip_ema_step", table_host, table, n_tensors, chunks, n_chunks,
                                 ClipNorm{partials, state, valid_since, max_norm, mode, step},
                                 om::SgdClip{state, valid_since, step}, om::SgdEma{shadows, ema_state, 0.f, decay, warmup != 0},
                                 static_cast<hipStream_t>(stream));
}

int om_ema_swap(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                float* const* shadows, om_stream stream) {
    return run_swap("om_ema_swap", table_host, table, n_tensors, chunks, n_chunks, shadows, static_cast<hipStream_t>(stream));
}

int om_adam_step(const void* table_host, void* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                 float* const* shadows, float omd, om_stream stream) {
    OM_REQUIRE(!shadows || (omd > 0.f && omd <= 1.f), OM_EINVAL, "om_adam_step: omd %g is not 1 - decay of a decay in [0, 1)",
               (double)omd);
    const om_adam_tensor* rows_host = static_cast<const om_adam_tensor*>(table_host);
    if (rows_host)          // ahead of the staging copy: a refused call leaves the device table as it was
        for (int i = 0; i < n_tensors; ++i)
            OM_REQUIRE(!(rows_host[i].flags & OM_ADAM_DEVICE_COUNTED), OM_EINVAL,
                       "om_adam_step: row %d is device-counted; that needs om_adam_clip_step", i);
    return run_step<om::AdamRule>("om_adam_step", rows_host, static_cast<om_adam_tensor*>(table), n_tensors, chunks, n_chunks,
                                  ClipNorm{}, om::AdamClip{}, shadows ? om::SgdEma{shadows, nullptr, omd, 0.0, 0} : om::SgdEma{},
                                  static_cast<hipStream_t>(stream));
}

int om_adam_clip_step(const void* table_host, void* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks, double* partials,
                      double* state, long long* counts, const double* bias, const long long* bias_dir, int n_bias_tables,
                      float max_norm, int mode, long long step, float* const* shadows, double* ema_state, double decay, int warmup,
                      om_stream stream) {
    OM_REQUIRE(table && chunks, OM_EINVAL, "om_adam_clip_step: null pointer");
    if (int rc = check_clip("om_adam_clip_step", partials, state, counts, max_norm, mode, step)) return rc;
    OM_REQUIRE(n_bias_tables >= 0 && (n_bias_tables == 0 || (bias && bias_dir)), OM_EINVAL,
               "om_adam_clip_step: %d bias tables without their rows", n_bias_tables);
    OM_REQUIRE((reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(bias_dir)) % 8 == 0, OM_EINVAL,
               "om_adam_clip_step: misaligned pointer");
    if (shadows) {
        OM_REQUIRE(ema_state && reinterpret_cast<uintptr_t>(ema_state) % 8 == 0, OM_EINVAL,
                   "om_adam_clip_step: shadows without an aligned EMA state block");
        OM_REQUIRE(decay > 0.0 && decay < 1.0, OM_EINVAL, "om_adam_clip_step: decay %g is not inside (0, 1)", decay);
    }
    return run_step<om::AdamRule>("om_adam_clip_step", static_cast<const om_adam_tensor*>(table_host),
                                  static_cast<om_adam_tensor*>(table), n_tensors, chunks, n_chunks,
                                  ClipNorm{partials, state, counts, max_norm, mode, step},
                                  om::AdamClip{state, counts, bias, bias_dir, n_bias_tables},
                                  shadows ? om::SgdEma{shadows, ema_state, 0.f, decay, warmup != 0} : om::SgdEma{},
                                  static_cast<hipStream_t>(stream));
}

int om_adam_ema_swap(const void* table_host, void* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                     float* const* shadows, om_stream stream) {
    return run_swap("om_adam_ema_swap", static_cast<const om_adam_tensor*>(table_host), static_cast<om_adam_tensor*>(table),
                    n_tensors, chunks, n_chunks, shadows, static_cast<hipStream_t>(stream));
}

}  // extern "C"
