"""The yardstick of the weight-EMA tests (om_sgd_ema_step / om_sgd_clip_ema_step, csrc/optim.hip; orienmask_amd.optim.SGD(ema_decay=...)),
restated in numpy on top of optim_np (the step) and clip_np (the clipped step).  DESIGN.md section 3.16.2.

Every parameter tensor has a float32 shadow `e`, a bit copy of the parameter before the first step.  On every APPLIED step, with p' the
parameter's new value, every element does

    diff = p' - e                  rounded once to float32
    e'   = fma(diff, omd, e)       one rounding (optim_np.fma32)

    omd  = float32(1 - d_k)        d_k = decay, or with warm-up min(decay, (1 + k) / (10 + k)); one add, one add, one divide, one min,
                                   one subtract, all in float64; k = EMA updates applied so far

  * the parameter and the momentum buffer are what optim_np.sgd_step_many / clip_np.clipped_step give: the average does not touch them
  * nonfinite="skip": a skipped step leaves every shadow and k unchanged
  * a tensor without a gradient in a step keeps its shadow; k is global and still advances
  * NaN and Inf propagate as the arithmetic gives them

The keyword switches of `omd_at`, `ema_update` and `run` (MUTANTS) exist for tests/test_ema_cpu.py's mutants only.
"""
import numpy as np

import clip_np as C
import optim_np as N

F32 = np.float32
MUTANTS = ("average_old_p", "count_skipped", "unfused", "blend", "ignore_warmup", "f32_decay")


def decay_at(k, decay, warmup=True):
    """d_k in float64."""
    d = np.float64(decay)
    if warmup:
        d = min(d, (np.float64(1.0) + np.float64(k)) / (np.float64(10.0) + np.float64(k)))
    return np.float64(d)


def omd_at(k, decay, warmup=True, ignore_warmup=False, f32_decay=False):
    """float32(1 - d_k).  Mutants: the warm-up ignored; 1 - float32(d_k) computed in float32."""
    d = decay_at(k, decay, warmup and not ignore_warmup)
    if f32_decay:
        return F32(F32(1.0) - F32(d))
    return F32(np.float64(1.0) - d)


def ema_update(e, p_new, omd, unfused=False, blend=False):
    """The shadow after one update.  Mutants: e + omd * diff with the product rounded on its own; e * d + p * (1 - d)."""
    e = np.asarray(e, F32)
    p_new = np.asarray(p_new, F32)
    omd = F32(omd)
    with np.errstate(all="ignore"):
        if blend:
            d = F32(F32(1.0) - omd)
            return ((e * d).astype(F32) + (p_new * omd).astype(F32)).astype(F32)
        diff = (p_new - e).astype(F32)
        if unfused:
            return (e + (diff * omd).astype(F32)).astype(F32)
        return N.fma32(diff, omd, e)


def run(ps, grads_per_step, hypers, decay, warmup=True, max_norm=None, nonfinite="propagate", average_old_p=False,
        count_skipped=False, **mutant):
    """The plain (max_norm None), clipped and skip forms over several steps.  ps: float32 arrays in storage order; grads_per_step:
    per step a list of arrays or None; hypers: one dict or one per tensor.  -> per step (params, buffers, shadows, k, skipped).
    Mutants: the average of the parameter BEFORE the update; k advancing on a skipped step; omd_at's and ema_update's."""
    omd_kw = {key: mutant.pop(key) for key in ("ignore_warmup", "f32_decay") if key in mutant}
    cur = [np.array(p, F32).reshape(-1) for p in ps]
    bufs = [None] * len(cur)
    shadows = [p.copy() for p in cur]
    k, out = 0, []
    for grads in grads_per_step:
        grads = [None if g is None else np.asarray(g, F32).reshape(-1) for g in grads]
        if max_norm is None:
            new, bufs = N.sgd_step_many(cur, grads, bufs, hypers)
            skipped = False
        else:
            new, bufs, _, _, skipped = C.clipped_step(cur, grads, bufs, hypers, max_norm, nonfinite)
        if not skipped:
            omd = omd_at(k, decay, warmup, **omd_kw)
            shadows = [e if g is None else ema_update(e, old if average_old_p else p, omd, **mutant)
                       for e, old, p, g in zip(shadows, cur, new, grads)]
            k += 1
        elif count_skipped:
            k += 1
        cur = new
        out.append(([p.copy() for p in cur], [None if b is None else b.copy() for b in bufs], [e.copy() for e in shadows], k, skipped))
    return out
