"""The forms of one step agree with each other, bit for bit.  csrc/optim.hip has ONE walker, step_kernel<Rule, CLIP, EMA>, behind
the plain, the averaged, the clipped and the clipped-and-averaged form of both update rules; the plain form is compared with the
numpy restatements by test_optim.py and test_adam.py, so this file needs no yardstick and no tolerance: with a bound of 1e30 the
clip coefficient clamps to exactly 1.0f and ``g * 1.0f`` is ``g``, and the EMA leaves the step alone, hence every form must give
the parameters and the optimizer state the plain form gives, and the two averaging forms the same shadows."""
import functools

import numpy as np
import pytest
import torch

from orienmask_amd import optim as O
from optim_harness import dev, _np  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu

RULES = {
    "sgd_no_momentum": ("SGD", dict(lr=1e-2, momentum=0, weight_decay=0)),                     # the row's buf is a null pointer
    "sgd_nesterov": ("SGD", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=5e-4)),
    "adam": ("HipAdam", dict(lr=1e-2, weight_decay=1e-2)),
    "adamw": ("HipAdamW", dict(lr=1e-2, weight_decay=1e-2)),
}
PLACEMENTS = ("aligned", "param_views", "grad_views")
FORMS = {
    "plain": dict(),
    "ema": dict(ema_decay=0.999),
    "clip": dict(max_grad_norm=1e30),
    "clip_ema": dict(max_grad_norm=1e30, ema_decay=0.999),
    "clip_ema_skip": dict(max_grad_norm=1e30, ema_decay=0.999, nonfinite="skip"),
}
COUNTS = (1, 3, 4, 4095, 4096, 4097, 2 * 4096 + 5)
STEPS = 3
NO_GRAD = (1, COUNTS.index(4097))                             # (step, tensor): in the second step this tensor has no gradient
STATE_KEYS = ("momentum_buffer", "exp_avg", "exp_avg_sq")


@functools.lru_cache(maxsize=None)
def _inputs():
    """The seeded values every run starts from: (parameters, gradients per step)."""
    rs = np.random.RandomState(20)
    params = [rs.standard_normal(n).astype(np.float32) for n in COUNTS]
    grads = [[rs.standard_normal(n).astype(np.float32) for n in COUNTS] for _ in range(STEPS)]
    return params, grads


def _place(dev, values, off_grid):
    """``values`` on the device: a tensor of its own, or a view one float into a flat buffer."""
    if not off_grid:
        t = torch.from_numpy(values).to(dev)
    else:
        t = torch.zeros(values.size + 8, device=dev)[1: 1 + values.size]
        t.copy_(torch.from_numpy(values))
    assert t.data_ptr() % 16 == (4 if off_grid else 0)
    return t


def _bits(t):
    return _np(t).view(np.uint32)


def _run(dev, rule, placement, form):
    """Three steps of one form -> per step (parameter bits, state bits by key, shadow bits or None, Adam's step counts)."""
    assert O.OM_SGD_CHUNK == 4096
    cls, hyper = RULES[rule]
    values, grads = _inputs()
    params = [torch.nn.Parameter(_place(dev, v, placement == "param_views")) for v in values]
    opt = getattr(O, cls)(params, **hyper, **FORMS[form])
    seen = []
    for s in range(STEPS):
        for i, p in enumerate(params):
            p.grad = None if (s, i) == NO_GRAD else _place(dev, grads[s][i], placement == "grad_views")
        opt.step()
        opt.state_dict()                                      # skip mode: brings Adam's device-side counts into state[p]["step"]
        torch.cuda.synchronize()
        state = [{k: _bits(opt.state[p][k]) for k in STATE_KEYS if k in opt.state.get(p, {})} for p in params]
        counts = [float(opt.state[p]["step"]) for p in params if "step" in opt.state.get(p, {})]
        shadows = [_bits(opt.ema_shadow(p)) for p in params] if "ema_decay" in FORMS[form] else None
        seen.append(([_bits(p) for p in params], state, shadows, counts))
    return seen


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("rule", sorted(RULES))
def test_every_form_gives_the_plain_forms_bits(dev, rule, placement):
    runs = {form: _run(dev, rule, placement, form) for form in FORMS}
    want_keys = {"sgd_no_momentum": set(), "sgd_nesterov": {"momentum_buffer"}}.get(rule, {"exp_avg", "exp_avg_sq"})
    for s in range(STEPS):
        p0, state0, _, counts0 = runs["plain"][s]
        for i in range(len(COUNTS)):
            assert set(state0[i]) == want_keys, (rule, placement, s, i, sorted(state0[i]))
        if rule.startswith("adam"):
            assert counts0 == [float(s + 1 - (s >= NO_GRAD[0] and i == NO_GRAD[1])) for i in range(len(COUNTS))]
        for form in FORMS:
            p, state, shadows, counts = runs[form][s]
            for i in range(len(COUNTS)):
                where = (rule, placement, form, "step", s, "tensor", i)
                assert np.array_equal(p[i], p0[i]), where + ("param",)
                assert set(state[i]) == want_keys, where + (sorted(state[i]),)
                for k in want_keys:
                    assert np.array_equal(state[i][k], state0[i][k]), where + (k,)
            assert counts == counts0, (rule, placement, form, "step", s, counts, counts0)
        e0 = runs["ema"][s][2]
        for form in ("clip_ema", "clip_ema_skip"):
            for i in range(len(COUNTS)):
                assert np.array_equal(runs[form][s][2][i], e0[i]), (rule, placement, form, "step", s, "tensor", i, "shadow")
        # the shadow moved: it is the parameter's bit copy before the first step and an average after it
        assert any(not np.array_equal(e0[i], p0[i]) for i in range(len(COUNTS)))
