"""tests/conv_cases.py against a restatement of its own, no GPU: the float64 expectation of a layer case evaluated output by output
without conv2d, and the padded scale / shift vectors."""
import pytest
import torch

from conv_cases import LayerCase

CASES = [
    # B, H, W, cin, cout, k, stride, leaky, residual
    (1, 3, 5, 8, 6, 3, 1, 1, True),
    (2, 4, 4, 4, 5, 1, 2, 0, False),
    (1, 6, 4, 3, 7, 3, 2, 1, True),       # stride 2 with padding taps on the top / left only
]


def _per_pixel(c, x):
    """out[b, o, i, j] = act(scale[o] * sum over (ch, dy, dx) of x[b, ch, i s + dy - p, j s + dx - p] w[o, ch, dy, dx] + shift[o]) + res"""
    x, w, p = x.double(), c.w.double(), c.k // 2
    out = torch.zeros(c.B, c.cout, c.Ho, c.Wo, dtype=torch.float64)
    for b in range(c.B):
        for o in range(c.cout):
            for i in range(c.Ho):
                for j in range(c.Wo):
                    acc = 0.0
                    for dy in range(c.k):
                        for dx in range(c.k):
                            y, xx = i * c.stride + dy - p, j * c.stride + dx - p
                            if 0 <= y < c.H and 0 <= xx < c.W:
                                acc += float((x[b, :, y, xx] * w[o, :, dy, dx]).sum())
                    v = acc * float(c.scale[o].double()) + float(c.shift[o].double())
                    if c.leaky and v <= 0:
                        v = v * 0.1
                    out[b, o, i, j] = v + (float(c.res[b, o, i, j].double()) if c.use_res else 0.0)
    return out


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_expectation_equals_per_pixel_evaluation(case, half):
    c = LayerCase(sum(case), case, half=half)
    assert c.want.dtype == torch.float64 and c.want.shape == (c.B, c.cout, c.Ho, c.Wo)
    assert c.x.dtype == c.w.dtype == (torch.float16 if half else torch.float32)
    assert (c.res is not None) == case[8]
    # float64 sums of at most cin k k = 72 terms in another order: a few 1e-15 of the scale; anything wrong in the formula is O(1)
    x2 = torch.randn(c.x.shape, generator=c.g)
    for x, want in ((c.x, c.want), (x2, c.expected(x2))):
        ref = _per_pixel(c, x)
        assert (want - ref).abs().max().item() <= 1e-13 * ref.abs().max().item()
    again = LayerCase(sum(case), case, half=half)               # the draw is the seed's alone
    assert all(torch.equal(getattr(c, n), getattr(again, n)) for n in ("x", "w", "scale", "shift", "want"))


@pytest.mark.parametrize("case", CASES)
def test_padded_vectors_are_zero_beyond_cout(case):
    c = LayerCase(sum(case), case)
    for cpad in (32, 64):
        sp, hp = c.padded(cpad)
        assert sp.shape == hp.shape == (cpad,) and sp.dtype == hp.dtype == torch.float32
        assert torch.equal(sp[:c.cout], c.scale) and torch.equal(hp[:c.cout], c.shift)
        assert (sp[c.cout:] == 0).all() and (hp[c.cout:] == 0).all()
        e = (torch.arange(cpad) % 5 - 2).to(torch.int32)         # exponents of split weights: powers of two, exact in fp32
        ss, hs = c.padded(cpad, e)
        assert torch.equal(hs, hp) and (ss[c.cout:] == 0).all()
        assert torch.equal(ss[:c.cout], c.scale * 2.0 ** -e[:c.cout].float())
    assert LayerCase.nhwc(None, "cpu") is None
    assert torch.equal(LayerCase.nhwc(c.x, "cpu"), c.x.permute(0, 2, 3, 1)) and LayerCase.nhwc(c.x, "cpu").is_contiguous()
