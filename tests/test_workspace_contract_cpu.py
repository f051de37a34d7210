"""The teeth of tests/workspace_poison.py, on numpy stand-ins for kernels (no GPU).

Each stand-in computes the same thing -- out[i] = 2 * x[i] and the number of positive x -- in a caller-provided workspace, and
each but the first breaks the "contents undefined on entry" contract in one of the ways a kernel does.  STAND_INS names, per
stand-in, the patterns that MUST expose it and those that NEED NOT (they may or may not); every other pattern must pass, so a
tool that cries wolf fails here as surely as one that sees nothing.
"""
import numpy as np
import pytest

from workspace_poison import PATTERNS, WorkspaceDependence, agree, fill, first_difference, raw, stale

N = 37              # elements; the workspace has a tail of TAIL floats behind them, as a tile has behind a ragged edge
TAIL = 11
X = np.linspace(-1.0, 2.0, N).astype(np.float32)


def _buffers():
    return dict(ws=np.empty(N + TAIL, np.float32), cnt=np.empty(1, np.int32), out=np.empty(N, np.float32),
                n_pos=np.empty(1, np.int32))


def clean(b, x=X):
    """Writes what it reads: the contract kept."""
    b["ws"][:N] = x
    b["cnt"][0] = 0
    b["cnt"][0] += int((x > 0).sum())
    b["out"][:] = 2 * b["ws"][:N]
    b["n_pos"][0] = b["cnt"][0]


def times_zero(b, x=X):
    """Reads a workspace element it never wrote and 'masks' it by multiplying with zero: 0 * NaN is NaN, 0 * 5.2e36 is 0."""
    clean(b, x)
    b["out"][3] += np.float32(0) * b["ws"][N + 2]


def trusted_counter(b, x=X):
    """Counts into a word it trusts to start at zero (a missing clear)."""
    b["ws"][:N] = x
    b["cnt"][0] += np.int32((x > 0).sum())
    b["out"][:] = 2 * b["ws"][:N]
    b["n_pos"][0] = b["cnt"][0]


def summed_tail(b, x=X):
    """Sums a whole tile, tail included, behind a NaN guard (`v == v`): the guard swallows 0xFF, tiny floats vanish in the sum,
    a large finite value does neither."""
    clean(b, x)
    tile = b["ws"][N - 5:N + TAIL]
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.float32(0)
        for v in tile:
            if v == v:
                s = np.float32(s + v)
        b["out"][0] = np.float32(s - b["ws"][N - 5:N].sum(dtype=np.float32)) + 2 * x[0]


def unwritten_output(b, x=X):
    """Leaves one element of its output unwritten (a ragged last block that returns early)."""
    ws, cnt, out, n_pos = b["ws"], b["cnt"], b["out"], b["n_pos"]
    ws[:N] = x
    cnt[0] = int((x > 0).sum())
    out[:N - 1] = 2 * ws[:N - 1]
    n_pos[0] = cnt[0]


# name -> (stand-in, patterns that must expose it, patterns that need not)
STAND_INS = {
    "clean__caught_by_none": (clean, (), ()),
    "times_zero__caught_by_FF__not_7C_01": (times_zero, (0xFF,), ()),
    "trusted_counter__caught_by_01_FF__7C_need_not": (trusted_counter, (0x01, 0xFF), (0x7C,)),
    "summed_tail__caught_by_7C__not_FF_01": (summed_tail, (0x7C,), ()),
    "unwritten_output__caught_by_every_fill_through_the_output": (unwritten_output, (0xFF, 0x7C, 0x01), ()),
}


def _run_of(fn, b):
    def run():
        fn(b)
        return dict(out=b["out"].copy(), n_pos=b["n_pos"].copy())
    return run


def test_patterns_are_the_four_fills_with_the_baseline_first():
    assert PATTERNS == (0x00, 0xFF, 0x7C, 0x01)
    f = np.empty(2, np.float32); h = np.empty(2, np.float16); i = np.empty(2, np.int32)
    fill(f, 0xFF); fill(h, 0xFF); fill(i, 0xFF)
    assert np.isnan(f).all() and np.isnan(h).all() and (i == -1).all()
    fill(f, 0x7C); fill(h, 0x7C); fill(i, 0x7C)
    assert np.isfinite(f).all() and f[0] > 5e36 and not np.isfinite(h).any() and i[0] == 0x7C7C7C7C
    fill(f, 0x01); fill(i, 0x01)
    assert 0 < f[0] < 1e-37 and i[0] == 0x01010101
    fill(f, 0x00)
    assert raw(f).tolist() == [0] * 8


@pytest.mark.parametrize("name", list(STAND_INS))
def test_each_stand_in_is_caught_by_exactly_its_patterns(name):
    fn, must, need_not = STAND_INS[name]
    for pat in PATTERNS[1:]:
        b = _buffers()
        run = _run_of(fn, b)
        if pat in must:
            with pytest.raises(WorkspaceDependence) as e:
                agree(run, b.values(), patterns=(0x00, pat))
            assert e.value.pattern == pat and "0x%02X" % pat in str(e.value), str(e.value)
        elif pat not in need_not:
            agree(run, b.values(), patterns=(0x00, pat))
    b = _buffers()
    if must:
        with pytest.raises(WorkspaceDependence):
            agree(_run_of(fn, b), b.values())
    else:
        base = agree(_run_of(fn, b), b.values())
        assert np.array_equal(base["out"], 2 * X) and int(base["n_pos"][0]) == int((X > 0).sum())      # ... and held to the expectation


def test_the_message_names_output_index_and_pattern():
    b = _buffers()
    with pytest.raises(WorkspaceDependence) as e:
        agree(_run_of(times_zero, b), b.values())
    assert (e.value.output, e.value.index, e.value.pattern) == ("out", 3, 0xFF)
    assert "'out'" in str(e.value) and "element 3" in str(e.value) and "0xFF" in str(e.value)
    b = _buffers()
    with pytest.raises(WorkspaceDependence) as e:
        agree(_run_of(unwritten_output, b), b.values())
    assert (e.value.output, e.value.index) == ("out", N - 1)


def test_the_comparison_is_raw_bytes():
    """Signed zeros and NaN payloads count; equal NaNs do not."""
    assert first_difference(np.float32([0.0]), np.float32([-0.0])) is not None
    a = np.array([0x7FC00000], np.uint32).view(np.float32); b = np.array([0x7FC00001], np.uint32).view(np.float32)
    assert first_difference(a, a.copy()) is None and first_difference(a, b) is not None
    assert first_difference([a, a], [a, b])[0] == "out1"
    assert first_difference(dict(x=a), dict(y=a))[0] == "<keys>"


def test_a_result_that_only_the_output_fill_reaches_needs_the_outputs_in_owned():
    """With the outputs left out of `owned`, an unwritten output element keeps the first run's value and the dependence hides:
    why agree() fills workspaces and outputs alike."""
    b = _buffers()
    b["out"][:] = 0
    agree(_run_of(unwritten_output, b), [b["ws"], b["cnt"]])


class _Cached:
    """A wrapper object that keeps its workspace between calls, as the Python wrappers of the library do."""

    def __init__(self, fn, poison=None):
        self.fn, self.b = fn, _buffers()
        for t in self.b.values():
            fill(t, 0x00 if poison is None else poison)

    def __call__(self, x):
        self.fn(self.b, x)
        return dict(out=self.b["out"].copy(), n_pos=self.b["n_pos"].copy())


@pytest.mark.parametrize("fn,caught", [(clean, False), (trusted_counter, True), (summed_tail, False), (times_zero, True)])
def test_stale(fn, caught):
    """loud = large values everywhere, quiet = the ordinary input.  A fresh object's workspace is 0xFF; the cached one holds what
    the loud run left (and a counter that went on counting)."""
    loud = np.full(N, 1.0e30, np.float32)
    obj = _Cached(fn)

    def check():
        return stale(lambda: obj(loud), lambda: obj(X.copy()), lambda: _Cached(fn, poison=0xFF)(X.copy()))

    if caught:
        with pytest.raises(WorkspaceDependence):
            check()
    else:
        check()


def test_raw_takes_scalars_and_torch_tensors():
    import torch
    assert raw(torch.tensor(7, dtype=torch.int64)).tolist() == [7, 0, 0, 0, 0, 0, 0, 0] and raw(np.int32(1)).size == 4
    assert first_difference(dict(a=torch.tensor(7)), dict(a=torch.tensor(8)))[:2] == ("a", 0)
    t = torch.zeros(3, dtype=torch.float16)
    fill(t, 0x7C)
    assert not torch.isfinite(t).any() and raw(t).tolist() == [0x7C] * 6
    with pytest.raises(ValueError):
        fill(torch.zeros(4, 4).t(), 0xFF)


def test_fresh_allocations_patches_torch_empty_only_inside_the_block():
    import torch
    from workspace_poison import CurrentPattern, FreshAllocations
    real = (torch.empty, torch.empty_like)
    fresh = FreshAllocations()
    seen = []

    def run():
        with fresh:
            assert torch.empty is not real[0] and torch.empty_like is not real[1]
            t = torch.empty(5)                      # host memory is the wrapper's own business: left alone, still allocated
            assert t.shape == (5,) and torch.empty_like(t).shape == (5,)
            seen.append(fresh.value)
        assert (torch.empty, torch.empty_like) == real
        return np.zeros(1)

    agree(run, [fresh, CurrentPattern()])
    assert seen == [0x00, 0xFF, 0x7C, 0x01]
    with pytest.raises(KeyError):
        with fresh:
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like) == real
