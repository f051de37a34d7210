"""The case table of the weight-EMA tests: tests/test_ema.py runs every case on the GPU against ema_np.run, tests/test_ema_cpu.py runs
the same table on numpy alone and checks that each case tells the yardstick from the mutants it names (``catches``).

A case: ``params`` (float32 arrays in STORAGE order), ``grads`` (per step, per tensor: an array in storage order, or None), ``hypers``
(one dict, or one per tensor: then the optimizer gets one group per tensor), ``decay`` / ``warmup``, ``max_norm`` / ``nonfinite`` (the
clipped forms), ``offset`` (per tensor: the parameter is a view that many elements into a flat buffer) and ``shapes`` (per tensor:
None, or an (N, C, H, W) shape whose parameter is channels-last, i.e. permuted-dense).  The sizes are the smallest that reach every
path of the kernel: the scalar tail (1, 3), one float4 (4), a tail after float4s (1003), a full chunk (4096), a chunk boundary (4097)
and a last partial float4 in a third chunk (2 * 4096 + 5)."""
import functools

import numpy as np

import ema_np as E
import optim_np as N

F32 = np.float32
COUNTS = [1, 3, 4, 1003, 4096, 4097, 2 * 4096 + 5]
ARITHMETIC = ("average_old_p", "unfused", "blend")           # what any case with a few hundred ordinary values tells apart


def _draw(rs, n, scale=1.0):
    return (np.where(rs.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-3.0, 2.0, n) * scale).astype(F32)


def _random_case(seed, counts, steps=N.SGD_STEPS, grad_scale=1.0, **kw):
    rs = np.random.RandomState(seed)
    case = dict(params=[_draw(rs, n) for n in counts], grads=[[_draw(rs, n, grad_scale) for n in counts] for _ in range(steps)],
                hypers=N.HYPER_SETS["momentum_decay"], decay=0.9998, warmup=False, max_norm=None, nonfinite="propagate",
                offset=[0] * len(counts), shapes=[None] * len(counts), catches=ARITHMETIC + ("f32_decay",))
    case.update(kw)
    return case


def _cases():
    out = {}
    out["counts"] = _random_case(1, COUNTS)
    # the warm-up ramp (d = 0.1, 2/11, 0.25, 4/13 over four steps): float32(1 - d) and 1 - float32(d) mostly agree there, so these
    # name the ignored warm-up instead of the float32 decay
    for i, (name, hyper) in enumerate(sorted(N.HYPER_SETS.items())):
        out["hyper_" + name] = _random_case(10 + i, [1003, 4097], hypers=hyper, warmup=True, catches=ARITHMETIC + ("ignore_warmup",))
    # zeros of both signs, denormals, +-Inf and NaN in parameter and gradient (optim_np.special_inputs) beside an ordinary tensor
    p, grads = N.special_inputs()
    out["special"] = _random_case(3, [p.size, 1003], decay=0.9, catches=ARITHMETIC)
    out["special"]["params"][0] = p
    for step, g in zip(out["special"]["grads"], grads):
        step[0] = g
    out["unaligned"] = _random_case(4, [1003, 4097, 3, 4096], hypers=N.HYPER_SETS["nesterov"], offset=[1, 1, 1, 1])
    # a few hundred elements: decay 0.9, so that omd * diff is large enough beside e for the unfused product's rounding to show
    out["channels_last"] = _random_case(5, [2 * 3 * 4 * 5, 4 * 8 * 3 * 3, 18], shapes=[(2, 3, 4, 5), (4, 8, 3, 3), None], decay=0.9)
    out["grad_none"] = _random_case(6, [1003, 4097, 18])
    out["grad_none"]["grads"][1][1] = out["grad_none"]["grads"][2][1] = None          # the middle row, in the two middle steps
    rs = np.random.RandomState(7)
    out["per_tensor_groups"] = _random_case(7, COUNTS, hypers=[
        dict(lr=float(10.0 ** rs.uniform(-3, -2)), momentum=0.9, weight_decay=float(rs.choice([0.0, 1e-4, 5e-4])),
             nesterov=bool(i % 2)) for i in range(len(COUNTS))])
    # gradient norms in the hundreds against max_norm 0.5: every coefficient is far below 1
    out["clip_below_one"] = _random_case(8, COUNTS, max_norm=0.5)
    # finite, Inf, finite, NaN, finite: three applied steps, and a warm-up that depends on how many were applied
    skip = _random_case(9, [1003, 4097, 18], steps=5, warmup=True, max_norm=1.0, nonfinite="skip",
                        catches=ARITHMETIC + ("count_skipped", "ignore_warmup"))
    skip["grads"][1][1][100] = np.inf
    skip["grads"][3][0][7] = np.nan
    out["skip"] = skip
    # decay 0.5: (1 + k) / (10 + k) reaches 0.5 exactly at k = 8, so eleven steps cross the cap; 1 - 0.5 is exact in both formats
    out["warmup_cross"] = _random_case(11, [1003, 18], steps=11, decay=0.5, warmup=True, catches=ARITHMETIC + ("ignore_warmup",))
    return out


CASES = _cases()


def run_case(case, **mutant):
    return E.run(case["params"], case["grads"], case["hypers"], case["decay"], case["warmup"], case["max_norm"], case["nonfinite"],
                 **mutant)


@functools.lru_cache(maxsize=None)
def reference(name):
    """ema_np.run of a case, computed once and shared by the tests; nobody writes into it."""
    return run_case(CASES[name])
