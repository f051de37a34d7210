"""The checkers of the crowd tests: what tests/test_loss_crowd.py asserts of the HIP kernels against the restatement, written
once so that tests/test_loss_crowd_cpu.py can show that each of them has teeth; not a test module.

Every checker raises AssertionError and returns the worst figure it saw.  The bounds are the project's existing ones:
REL = 1e-5 on terms and float metrics, counts exact, the target rules of tests/test_loss.py::test_fixture_targets, and
loss_grad_np.mismatches with its default bounds equal to 0."""
import numpy as np

import loss_grad_np
from test_loss_cpu import TIOU_ULP, _tiou_ulps

REL = 1e-5
TARGET_KEYS = dict(bbox_pos_mask="pos", bbox_neg_mask="neg", bbox_pos_scale="pscale", orien_mask="omask")


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def check_values(got, want, tag):
    """got / want: per scale (7 weighted terms, 8 (numerator, count) pairs).  Terms and numerators within REL, counts exact."""
    worst = 0.0
    assert len(got) == len(want), tag
    for s, ((gt, gm), (wt, wm)) in enumerate(zip(got, want)):
        for k, (a, b) in enumerate(zip(gt, wt)):
            worst = max(worst, _rel(float(a), float(b)))
            assert _rel(float(a), float(b)) <= REL, (tag, s, "term", k, float(a), float(b))
        for k, ((gn, gc), (wn, wc)) in enumerate(zip(gm, wm)):
            assert float(gc) == float(wc), (tag, s, "count", k, gc, wc)
            assert _rel(float(gn), float(wn)) <= REL, (tag, s, "metric", k, gn, wn)
    return worst


def check_targets(got, want, smooth, tag):
    """One scale's targets (the restatement's key names; the device's are mapped by TARGET_KEYS): orien_mask and torien bit for
    bit, pos / pscale / txy / neg equal, twh within 1 ulp, tcls' positive entries equal and all others the smoothing value, tiou
    within TIOU_ULP with the same zeros."""
    names = ("pos", "neg", "pscale", "txy", "twh", "tiou", "tcls", "omask", "torien")
    got = {TARGET_KEYS.get(k, k): v for k, v in got.items()}
    got = {k: np.asarray(got[k]) for k in names}
    assert np.array_equal(got["omask"].astype(np.int64), np.asarray(want["omask"], np.int64)), (tag, "orien_mask")
    assert np.array_equal(got["torien"], want["torien"]), (tag, "torien")
    for k in ("pos", "pscale", "txy", "neg"):
        assert np.array_equal(got[k], want[k]), (tag, k)
    ulp = np.abs(got["twh"].view(np.int32).astype(np.int64) - np.asarray(want["twh"], np.float32).view(np.int32).astype(np.int64))
    assert ulp.max(initial=0) <= 1, (tag, "twh", ulp.max())
    on = got["tcls"] > 0.5
    assert np.array_equal(on, want["tcls"] > 0.5), (tag, "tcls")
    assert np.all(got["tcls"][~on] == np.float32(smooth)), (tag, "tcls off")
    assert _tiou_ulps(got["tiou"], want["tiou"]) <= TIOU_ULP, (tag, "tiou")


def check_grads(got, want, tag):
    """got / want: per scale (g_bbox, g_orien, ...).  loss_grad_np.mismatches with its default bounds must be 0 for both heads.
    Returns the largest error as a fraction of the bound."""
    worst = 0.0
    for s, (g, w) in enumerate(zip(got, want)):
        for k, name in ((0, "bbox"), (1, "orien")):
            a, r = np.asarray(g[k], np.float64), np.asarray(w[k], np.float64)
            n = loss_grad_np.mismatches(a, r)
            assert n == 0, (tag, s, name, n)
            tol = 1e-5 * np.abs(r) + 1e-6 * (np.abs(r).max() if r.size else 0.0)
            live = tol > 0
            if live.any():
                worst = max(worst, float((np.abs(a - r)[live] / tol[live]).max()))
    return worst


def check_near_zero(near, tag):
    """A case's near-threshold counts (four forward, three of the gradient, per scale) must all be 0."""
    assert all(v == 0 for row in near for v in row), (tag, near)


def restatement_values(rec):
    return [(v[0], v[1]) for v in rec.values]


def check_record(got, want, smooth, tag):
    """A whole restatement record (loss_cases.run_restatement) against another: values, every scale's targets, gradients."""
    check_values(restatement_values(got), restatement_values(want), tag)
    for s in range(len(want.values)):
        check_targets(got.values[s][2], want.values[s][2], smooth, (tag, s))
    check_grads(got.grads, want.grads, tag)
