"""GPU: the fused stride-1 3x3 kernel (conv_wino14.hip) on layers whose column blocks differ in width and rows per block, whose row
blocks cross the zero row two images share, or that are smaller than one block -- against the two-kernel wide form (one block
shape per layer, its own zero rows: an independent bit-exact reference), a float64 convolution, and the same image computed alone."""
import ctypes

import pytest
import torch

from orienmask_amd import lib as omlib

pytestmark = pytest.mark.gpu

CASES = [
    # B, H, W, cin, cout, residual
    (2, 20, 68, 16, 128, False),     # blocks of 9 and 8 tile columns with 14 and 16 rows; row blocks across the image seam
    (1, 40, 136, 16, 128, False),    # 34 tile columns: two classes, several blocks in one of them
    (2, 9, 66, 48, 128, True),       # the last tile column has two pixels; three chunks
    (3, 17, 17, 32, 128, True),      # one block of five tile columns, 25 rows over three images
    (1, 3, 272, 16, 128, False),     # fewer padded rows than a block has room for
    (2, 1, 34, 16, 128, True),       # every image row lies between two zero rows
    (2, 20, 68, 16, 64, False),      # one N tile: no wide form
]
GUARD = 4096        # floats in front of and behind the output view


@pytest.fixture(scope="module")
def dev(built):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    omlib.load()
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("case", CASES)
def test_wino14_blocks_layer(dev, case):
    from orienmask_amd.pack import winograd14_weights_split
    B, H, W, cin, cout, use_res = case
    L = omlib.load()
    g = torch.Generator().manual_seed(sum(case) + 41)
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.2
    res = torch.randn(B, H, W, cout, generator=g) if use_res else None
    us, e = winograd14_weights_split(w, cout)
    sps = (scale.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double()[:cout])).float().to(dev)
    hd, ud, xd = shift.to(dev), us.to(dev), x.to(dev)
    rd = res.to(dev) if use_res else None
    st = omlib.current_stream_ptr(dev)
    nbytes = L.om_conv2d_wino14_wide_scratch_bytes(B, H, W, cin)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)

    def run(nb, wide=False):
        """the first nb images; the output view between two guard bands, NaN before the launch"""
        n = nb * H * W * cout
        buf = torch.full((GUARD + n + GUARD,), 12345.0, device=dev)
        buf[GUARD:GUARD + n] = float("nan")
        out = buf[GUARD:GUARD + n]
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        args = (_p(xd), nb, H, W, cin, cin, _p(ud), _p(sps), _p(hd), cout, 1, _p(rd) if use_res else None, cout if use_res else 0,
                _p(out), cout)
        if wide:
            rc = L.om_conv2d_wino14_wide(*args, _p(scratch), nbytes, _p(status), st)
        else:
            rc = L.om_conv2d_wino14_split(*args, _p(status), st)
        omlib.check(rc, "wino14 wide" if wide else "wino14 fused")
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        host = buf.cpu()
        assert (host[:GUARD] == 12345.0).all() and (host[GUARD + n:] == 12345.0).all(), case
        return host[GUARD:GUARD + n].view(nb, H, W, cout)

    got = run(B)
    assert torch.isfinite(got).all(), case
    want = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, 1, 1)
    want = want * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    want = torch.where(want > 0, want, want * 0.1)
    if use_res:
        want = want + res.permute(0, 3, 1, 2).double()
    err = (got.permute(0, 3, 1, 2).double() - want).abs().max().item() / max(want.abs().max().item(), 1e-12)
    print("wino14 blocks %s: %.2e" % (case, err))
    assert err < 5e-6, (case, err)       # the bound of test_hip_parity.py::test_wino14_split_layer_matches_torch
    if cout % 128 == 0:
        wide = run(B, wide=True)
        assert torch.equal(wide, got), (case, (wide - got).abs().max())
    alone = run(1)
    assert torch.equal(alone[0], got[0]), case
