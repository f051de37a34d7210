"""numpy restatement of csrc/route.hip: torch.cat of nearest-up-sampled sources and its backward, and the case table the route
tests share.

  forward      y[b, off_i + c, oy, ox] = src_i[b, c, oy // s_i, ox // s_i], by indexing; a source given as None is zeros
  backward     dsrc_i[b, c, sy, sx] = the s_i x s_i block of dy summed sequentially in float32: the accumulator starts as the
               block's first element, rows top to bottom, left to right within a row
  backward64   the same block sum in float64, and the block sum of |dy| in float64 (the scale of the error bound)
  gamma        (s^2 - 1) u / (1 - (s^2 - 1) u), u = 2^-24: the bound on a sequential float32 sum of s^2 terms, relative to sum |dy|

The split along the channels is the same pair with the roles swapped and every scale 1: split = backward, its gradient = forward."""
import numpy as np

# (B, H, W, [(C_i, s_i)]): H, W are the concatenated tensor's
CASES = [
    (1, 1, 1, [(1, 1)]),
    (2, 8, 8, [(3, 8)]),
    (3, 3, 6, [(5, 1)]),
    (2, 2, 6, [(1, 2), (2, 1)]),
    (3, 6, 10, [(3, 2), (5, 1)]),
    (2, 12, 12, [(256, 2), (512, 1)]),
    (2, 24, 24, [(64, 8), (64, 4), (64, 2), (64, 1)]),
    (2, 40, 32, [(64, 8), (64, 4), (64, 2), (64, 1)]),
    (2, 24, 24, [(64, 2), (128, 1)]),
    (5, 8, 16, [(7, 4), (1, 8), (2, 2), (3, 1)]),
    (2, 136, 136, [(64, 8), (64, 4), (64, 2), (64, 1)]),
]
U = 2.0 ** -24


def case_id(case):
    B, H, W, parts = case
    return "%dx%dx%d-" % (B, H, W) + "+".join("%dx%d" % p for p in parts)


def chans_scales(case):
    return [c for c, _ in case[3]], [s for _, s in case[3]]


def inputs(case, seed):
    """-> (sources, dy): float32 N(0,1) from one PCG64 stream."""
    B, H, W, parts = case
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    srcs = [rng.standard_normal((B, c, H // s, W // s)).astype(np.float32) for c, s in parts]
    dy = rng.standard_normal((B, sum(c for c, _ in parts), H, W)).astype(np.float32)
    return srcs, dy


def forward(srcs, chans, scales, B, H, W):
    y = np.zeros((B, sum(chans), H, W), np.float32)
    oy, ox = np.arange(H), np.arange(W)
    off = 0
    for src, c, s in zip(srcs, chans, scales):
        if src is not None:
            assert src.shape == (B, c, H // s, W // s) and src.dtype == np.float32
            y[:, off:off + c] = src[:, :, (oy // s)[:, None], (ox // s)[None, :]]
        off += c
    return y


def _blocks(dy, off, c, s):
    """-> [B, c, H/s, s, W/s, s] view of dy's channels off .. off + c."""
    B, _, H, W = dy.shape
    return dy[:, off:off + c].reshape(B, c, H // s, s, W // s, s)


def backward(dy, chans, scales):
    assert dy.dtype == np.float32
    out, off = [], 0
    for c, s in zip(chans, scales):
        blk = _blocks(dy, off, c, s)
        acc = blk[:, :, :, 0, :, 0].copy()
        for r in range(s):
            for q in range(s):
                if r or q:
                    acc = (acc + blk[:, :, :, r, :, q]).astype(np.float32)
        out.append(acc)
        off += c
    return out


def backward64(dy, chans, scales):
    """-> [(sum, sum of |dy|)] per source, float64."""
    out, off = [], 0
    d = dy.astype(np.float64)
    for c, s in zip(chans, scales):
        blk = _blocks(d, off, c, s)
        out.append((blk.sum(axis=(3, 5)), np.abs(blk).sum(axis=(3, 5))))
        off += c
    return out


def gamma(s):
    k = s * s - 1
    return k * U / (1 - k * U)


def within_bound(got, dy, chans, scales):
    """Every element of every gradient within gamma(s) * sum |dy| of the float64 sum; -> the worst error / bound (0 where s = 1,
    which must be exact)."""
    worst = 0.0
    for g, (truth, mag), s in zip(got, backward64(dy, chans, scales), scales):
        if g is None:
            continue
        err = np.abs(g.astype(np.float64) - truth)
        if s == 1:
            assert not err.any()
            continue
        bound = gamma(s) * mag
        assert (err <= bound).all(), (s, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
