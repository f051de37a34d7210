"""numpy restatement of om_loss_accumulate (include/orienmask_hip.h, csrc/loss_counter.hip): the per-step derived values in
float32, one rounding per operation, sums left to right; the (sum, items) pairs in float64; the sticky status words.

`mutant` breaks it on purpose (tests/test_loss_counter_cpu.py checks that its comparison notices each):
  "metrics_always"   the metric keys are counted although with_metrics is 0
  "weight_twice"     scales_weight applied twice in the cross-scale rows
  "step_overwrite"   a later bad step overwrites the latched step
"""
import numpy as np

MAX_SCALES, TERMS, METRICS = 3, 7, 8
SCALE_FLOATS = TERMS + 2 * METRICS
FLAG_OFF = MAX_SCALES * SCALE_FLOATS
RESULT_FLOATS = FLAG_OFF + 1
MAX_KEYS = 1 + 2 * (MAX_SCALES + 1) * METRICS
STAGE_OFF, EPOCH_OFF, BLOCK_FLAG_OFF = 0, 2 * MAX_KEYS, 4 * MAX_KEYS
STEP_OFF = BLOCK_FLAG_OFF + 1
BLOCK_DOUBLES = BLOCK_FLAG_OFF + 2
FLAG_NONFINITE_LOSS = 256

f32 = np.float32


def new_block():
    return np.zeros(BLOCK_DOUBLES, np.float64)


def status(block):
    """(flags, first bad step) of a block."""
    return tuple(int(v) for v in block[BLOCK_FLAG_OFF:].view(np.int64))


def step_values(result, num_scales, scales_weight, mutant=None):
    """(loss_sum, values[1 + 8 (S + 1)] float32, metrics[8 (S + 1), 2] float32) of one result vector, in key order."""
    S = num_scales
    r = np.asarray(result, f32)[:FLAG_OFF].reshape(MAX_SCALES, SCALE_FLOATS)[:S]
    w = [f32(v) for v in scales_weight[:S]]
    if mutant == "weight_twice":
        w = [f32(v * v) for v in w]
    v = np.zeros((S, TERMS + 1), f32)
    for s in range(S):
        acc = r[s, 0]
        for j in range(1, TERMS):
            acc = f32(acc + r[s, j])
        v[s, :TERMS], v[s, TERMS] = r[s, :TERMS], acc
    cross = np.zeros(TERMS + 1, f32)
    for j in range(TERMS + 1):
        acc = f32(w[0] * v[0, j])
        for s in range(1, S):
            acc = f32(acc + f32(w[s] * v[s, j]))
        cross[j] = acc
    loss_sum = cross[TERMS]
    m = r[:, TERMS:].reshape(S, METRICS, 2)
    cm = m[0].copy()
    for s in range(1, S):
        cm = (cm + m[s]).astype(f32)
    values = np.concatenate([[loss_sum], v.reshape(-1), cross]).astype(f32)
    return loss_sum, values, np.concatenate([m.reshape(-1, 2), cm]).astype(f32)


def accumulate(block, result, num_scales, scales_weight, with_metrics, step, mutant=None):
    """One call: adds into `block` (float64 [BLOCK_DOUBLES]) in place, returns loss_sum (float32)."""
    with np.errstate(all="ignore"):
        loss_sum, values, mets = step_values(result, num_scales, scales_weight, mutant)
    n = values.size
    pairs = block[STAGE_OFF:STAGE_OFF + 2 * n].reshape(n, 2)
    pairs[:, 0] += values.astype(np.float64)
    pairs[:, 1] += 1.0
    if with_metrics or mutant == "metrics_always":
        block[2 * n:2 * (n + mets.shape[0])].reshape(-1, 2)[...] += mets.astype(np.float64)
    word = block[BLOCK_FLAG_OFF:].view(np.int64)
    bits = int(np.asarray(result, f32)[FLAG_OFF:].view(np.int32)[0])
    if not np.isfinite(loss_sum):
        bits |= FLAG_NONFINITE_LOSS
    if bits:
        if word[0] == 0 or mutant == "step_overwrite":
            word[1] = step
        word[0] |= bits
    return loss_sum
