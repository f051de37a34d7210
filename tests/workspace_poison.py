"""Workspace poisoning: does an entry's result depend on what its caller-provided memory held on entry?

Every entry of the library works in memory the caller allocates (torch.empty on the Python side) and keeps.  The contract is
"contents undefined on entry": the entry must write, clear or mask whatever it later reads.  A test run hands a kernel fresh
memory or a neighbouring test's finite floats; a long-lived process hands it another layer's activations, NaN tensors, old
tickets and counts.  This module fills such memory with byte patterns chosen for what they decode to and compares the results
bit for bit.  It holds no GPU code: fill() works on numpy arrays and on torch tensors of any device alike.

PATTERNS (one byte each, repeated over the whole buffer):
  0x00  zeros in every type.  The fill that HIDES a missing clear -- counters start at 0, sums start at 0.0 -- and therefore the
        baseline the other results are compared with.
  0xFF  NaN as float32, fp16 and bf16 (all exponent bits and mantissa bits set); -1 as a signed integer; a counter at its
        maximum as an unsigned one.  Catches a read that is multiplied by zero or masked after arithmetic (0 * NaN = NaN), and
        any counter, ticket or flag trusted to start at zero.
  0x7C  the high byte of fp16's +Inf: as fp16 the repeated byte is non-finite (0x7C7C, exponent all ones); as float32 and bf16
        it is 5.2e36 -- FINITE, so it survives `x * 0` unnoticed but not a sum, a max or a comparison: the pattern that catches
        an accumulated tile tail or pad row even where a NaN test or a `!(x > t)` mask would swallow 0xFF; as int32 a large
        positive integer (2088533116): an index or count far past any bound.
  0x01  tiny positive floats (2.4e-38 as float32, 1.5e-5 as fp16); SMALL POSITIVE integers (16843009 as int32, 1 per byte,
        257 per int16) -- what a plausible stale ticket, count or histogram bin looks like: the pattern that catches a counter
        trusted to start at zero while leaving every float sum numerically unchanged.

agree(run, owned)            every pattern gives the bytes the 0x00 fill gives; returns the 0x00 result for the caller to hold
                             to the case's own expectation (independence alone would pass a kernel that is wrong in the same
                             way every time).
stale(loud, quiet, fresh)    a quiet run after a loud one on the same cached object equals the quiet run on a new object whose
                             workspace was poisoned with 0xFF.
"""
import numpy as np

PATTERNS = (0x00, 0xFF, 0x7C, 0x01)


class WorkspaceDependence(AssertionError):
    """A result changed with the bytes an owned buffer held on entry.  `pattern`, `output` and `index` name the first difference."""

    def __init__(self, msg, pattern=None, output=None, index=None):
        super().__init__(msg)
        self.pattern, self.output, self.index = pattern, output, index


class CurrentPattern:
    """An `owned` entry that holds no memory: after agree() has filled the buffers, `value` is the pattern they hold, so that
    run() can check what must keep its fill (rows of an output beyond a count)."""

    def __init__(self):
        self.value = None

    def poison(self, pattern):
        self.value = pattern


class FreshAllocations(CurrentPattern):
    """An `owned` entry for memory a Python wrapper allocates itself: inside `with`, every tensor torch.empty / torch.empty_like
    returns on a device other than the CPU is filled with the current pattern before the wrapper sees it -- its workspaces,
    scratch and outputs alike, as whatever the caching allocator last had there would be.  torch.zeros and torch.full are left
    alone: what the wrapper initialises is the wrapper's contract with the library."""

    def __init__(self, pattern=0x00):
        self.value = pattern
        self._saved = None

    def __enter__(self):
        import torch
        self._saved = (torch.empty, torch.empty_like)

        def poisoned(real):
            def alloc(*a, **k):
                t = real(*a, **k)
                if t.device.type != "cpu" and t.numel():
                    # a permuted-dense result (empty_like of a channels-last tensor): fill its storage, which it owns whole
                    flat = t if t.is_contiguous() else t.as_strided((t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)
                    fill(flat, self.value)
                return t
            return alloc

        torch.empty, torch.empty_like = poisoned(self._saved[0]), poisoned(self._saved[1])
        return self

    def __exit__(self, *exc):
        import torch
        torch.empty, torch.empty_like = self._saved
        self._saved = None
        return False


def fill(buf, pattern):
    """Set every byte of `buf` (numpy array or torch tensor, any dtype, any device) to `pattern`; an object with a poison()
    method (CurrentPattern, FreshAllocations) is told the pattern instead."""
    if hasattr(buf, "poison"):
        buf.poison(pattern)
        return
    if isinstance(buf, np.ndarray):
        buf.view(np.uint8)[...] = pattern
        return
    import torch
    if not buf.is_contiguous():
        raise ValueError("fill: a non-contiguous tensor cannot be viewed as bytes; pass the tensor that owns the storage")
    if buf.numel():
        buf.view(torch.uint8).fill_(pattern)


def raw(t):
    """The bytes of a result (CPU tensor, numpy array or scalar) as a flat uint8 numpy array."""
    if not isinstance(t, np.ndarray):
        if hasattr(t, "detach"):
            t = t.detach()
            if t.device.type != "cpu":
                raise ValueError("run() must return CPU tensors (the copy orders the comparison behind the kernels)")
            import torch
            t = t.contiguous().reshape(-1)          # (a 0-dim tensor cannot be viewed as bytes)
            t = t.view(torch.uint8).numpy() if t.numel() else np.zeros(0, np.uint8)
        else:
            t = np.asarray(t)
    return np.ascontiguousarray(t).reshape(-1).view(np.uint8)


def _itemsize(t):
    if hasattr(t, "element_size"):
        return int(t.element_size())
    return int(np.asarray(t).itemsize)


def _named(res):
    if isinstance(res, dict):
        return list(res.items())
    if isinstance(res, (list, tuple)):
        return [("out%d" % i, r) for i, r in enumerate(res)]
    return [("out", res)]


def first_difference(got, want):
    """(output name, element index, got bytes, want bytes) of the first raw difference between two results, or None."""
    g, w = _named(got), _named(want)
    if [k for k, _ in g] != [k for k, _ in w]:
        return ("<keys>", 0, [k for k, _ in g], [k for k, _ in w])
    for (k, a), (_, b) in zip(g, w):
        ra, rb = raw(a), raw(b)
        if ra.size != rb.size:
            return (k, min(ra.size, rb.size), "%d bytes" % ra.size, "%d bytes" % rb.size)
        d = np.flatnonzero(ra != rb)
        if d.size:
            isz = _itemsize(a)
            e = int(d[0]) // isz
            return (k, e, bytes(ra[e * isz:(e + 1) * isz]).hex(), bytes(rb[e * isz:(e + 1) * isz]).hex())
    return None


def agree(run, owned, patterns=PATTERNS):
    """For each pattern: fill every buffer in `owned` (workspaces AND outputs), call run(), which returns the DEFINED part of
    the outputs as CPU tensors / arrays (one, a sequence or a dict).  Every result must equal the 0x00 result as raw bytes (NaN
    payloads and signed zeros count).  Raises WorkspaceDependence naming the first differing output, element index and pattern;
    returns the 0x00 result."""
    owned = list(owned)
    base = None
    for pat in (0x00,) + tuple(p for p in patterns if p != 0x00):
        for t in owned:
            fill(t, pat)
        res = run()
        if pat == 0x00:
            base = res
            continue
        diff = first_difference(res, base)
        if diff is not None:
            raise WorkspaceDependence("result depends on the memory's contents on entry: output %r, element %d differs under fill "
                                      "0x%02X (got %s, 0x00 fill gave %s)" % (diff[0], diff[1], pat, diff[2], diff[3]),
                                      pattern=pat, output=diff[0], index=diff[1])
    return base


def stale(run_loud, run_quiet, fresh_quiet):
    """run_loud() then run_quiet() on one cached object, against fresh_quiet(): the quiet case on a NEW object whose workspace
    the callable poisoned with 0xFF.  The results must be raw-equal; returns the fresh result."""
    run_loud()
    got = run_quiet()
    want = fresh_quiet()
    diff = first_difference(got, want)
    if diff is not None:
        raise WorkspaceDependence("a run after another on the same cached workspace differs from a fresh object's: output %r, "
                                  "element %d (got %s, fresh %s)" % (diff[0], diff[1], diff[2], diff[3]),
                                  pattern=None, output=diff[0], index=diff[1])
    return want
