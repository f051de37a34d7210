// The training loop's per-step bookkeeping on the device (include/orienmask_hip.h: om_loss_accumulate): what the host did after
// every om_loss -- the per-scale and cross-scale aggregation of eval/base.py:29-32,90-121, EvalCounter.update of every key
// (eval/counter.py) and the loop's own isfinite(loss) (trainer/trainer.py:57) -- as ONE launch of one wave.
//   loss_accumulate_kernel   lane k owns key k (65 keys at 3 scales: lane 0 takes the last one too).  Every lane derives the few
//                            float32 values its key needs from the result vector (at most 21 additions and 6 products), then adds
//                            its (value, items) pair into the float64 block: one owner per pair, so no atomics and a fixed order.
//                            Lane 0 also writes loss_sum and latches the status words.
// Arithmetic: __fadd_rn / __fmul_rn throughout and the file is built with -ffp-contract=off: each operation is rounded once, in
// the order the header states, which is the order tests/loss_counter_np.py restates.
#include "om_common.h"

namespace om {

static_assert(OM_LOSS_TERMS + 1 == OM_LOSS_METRICS, "a scale has as many loss keys (7 terms and their sum) as metric keys");
constexpr int CNT_ROWS = OM_LOSS_METRICS;                  // keys per scale and kind
constexpr int CNT_LANES = 64;

struct CounterParams {
    const float* result;
    double* block;
    float* loss_sum;
    long long step;
    float w[OM_MAX_SCALES];
    int S, with_metrics;
};

// element i of a three-element array by selection: an index known only at run time would put the array into scratch memory
__device__ __forceinline__ float pick(const float* v, int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : v[2]); }

// sum over the scales s < S of w[s] * v[s], left to right from the first scale
__device__ __forceinline__ float weighted_sum(const float* w, const float* v, int S) {
    float acc = __fmul_rn(w[0], v[0]);
#pragma unroll
    for (int s = 1; s < OM_MAX_SCALES; ++s)
        if (s < S) acc = __fadd_rn(acc, __fmul_rn(w[s], v[s]));
    return acc;
}

__global__ __launch_bounds__(CNT_LANES) void loss_accumulate_kernel(const CounterParams p) {
    const int S = p.S;
    const int n_loss = CNT_ROWS * (S + 1);                 // loss keys: per scale 7 terms + the scale sum, then the 8 cross rows
    const int n_keys = 1 + 2 * n_loss;
    const float w[OM_MAX_SCALES] = {p.w[0], p.w[1], p.w[2]};
    float ssum[OM_MAX_SCALES];
#pragma unroll
    for (int s = 0; s < OM_MAX_SCALES; ++s) {
        const float* t = p.result + (s < S ? s : 0) * OM_LOSS_SCALE_FLOATS;        // scales >= S: read scale 0, never used
        float acc = t[0];
#pragma unroll
        for (int j = 1; j < OM_LOSS_TERMS; ++j) acc = __fadd_rn(acc, t[j]);
        ssum[s] = acc;
    }
    const float loss_sum = weighted_sum(w, ssum, S);
    for (int k = threadIdx.x; k < n_keys; k += CNT_LANES) {
        float value = loss_sum, items = 1.0f;
        if (k >= 1 && k <= n_loss) {
            const int sc = (k - 1) / CNT_ROWS, j = (k - 1) % CNT_ROWS;
            if (sc < S) {
                value = j < OM_LOSS_TERMS ? p.result[sc * OM_LOSS_SCALE_FLOATS + j] : pick(ssum, sc);
            } else {
                float v[OM_MAX_SCALES];
#pragma unroll
                for (int s = 0; s < OM_MAX_SCALES; ++s)
                    v[s] = j < OM_LOSS_TERMS ? p.result[(s < S ? s : 0) * OM_LOSS_SCALE_FLOATS + j] : ssum[s];
                value = weighted_sum(w, v, S);
            }
        } else if (k > n_loss) {
            if (!p.with_metrics) continue;
            const int sc = (k - 1 - n_loss) / CNT_ROWS, j = (k - 1 - n_loss) % CNT_ROWS;
            const float* m = p.result + OM_LOSS_TERMS + 2 * j;
            if (sc < S) {
                value = m[sc * OM_LOSS_SCALE_FLOATS];
                items = m[sc * OM_LOSS_SCALE_FLOATS + 1];
            } else {
                value = m[0];
                items = m[1];
#pragma unroll
                for (int s = 1; s < OM_MAX_SCALES; ++s) {
                    if (s >= S) break;
                    value = __fadd_rn(value, m[s * OM_LOSS_SCALE_FLOATS]);
                    items = __fadd_rn(items, m[s * OM_LOSS_SCALE_FLOATS + 1]);
                }
            }
        }
        double* pair = p.block + OM_COUNTER_STAGE_OFF + 2 * k;
        pair[0] += (double)value;
        pair[1] += (double)items;
    }
    if (threadIdx.x == 0) {
        *p.loss_sum = loss_sum;
        long long bits = (long long)(reinterpret_cast<const int32_t*>(p.result)[OM_LOSS_FLAG_OFF]);
        if (!isfinite(loss_sum)) bits |= OM_COUNTER_FLAG_NONFINITE_LOSS;
        if (bits) {
            long long* word = reinterpret_cast<long long*>(p.block + OM_COUNTER_FLAG_OFF);
            long long* first = reinterpret_cast<long long*>(p.block + OM_COUNTER_STEP_OFF);
            const long long old = *word;
            if (old == 0) *first = p.step;
            *word = old | bits;
        }
    }
}

}  // namespace om

extern "C" int om_loss_accumulate(const float* result, int num_scales, const float* scales_weight, int with_metrics, long long step,
                                  double* counter, float* loss_sum, om_stream stream) {
    OM_REQUIRE(num_scales >= 1 && num_scales <= OM_MAX_SCALES, OM_EINVAL, "om_loss_accumulate: %d scales (1..%d)", num_scales,
               OM_MAX_SCALES);
    OM_REQUIRE(result && scales_weight && counter && loss_sum, OM_EINVAL, "om_loss_accumulate: null pointer");
    OM_REQUIRE(reinterpret_cast<uintptr_t>(counter) % 8 == 0 && reinterpret_cast<uintptr_t>(result) % 4 == 0 &&
               reinterpret_cast<uintptr_t>(loss_sum) % 4 == 0, OM_EINVAL, "om_loss_accumulate: misaligned pointer");
    om::CounterParams p = {};
    p.result = result;
    p.block = counter;
    p.loss_sum = loss_sum;
    p.step = step;
    p.S = num_scales;
    p.with_metrics = with_metrics != 0;
    for (int s = 0; s < num_scales; ++s) p.w[s] = scales_weight[s];
    hipLaunchKernelGGL(om::loss_accumulate_kernel, dim3(1), dim3(om::CNT_LANES), 0, static_cast<hipStream_t>(stream), p);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}
