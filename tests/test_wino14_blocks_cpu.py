"""CPU: how the fused stride-1 3x3 kernel (conv_wino14.hip) cuts a layer into blocks, through the host-only query
om_conv2d_wino14_blocks.  A block is R padded rows x Ct tile columns of four pixels; the kernel's matrix tile holds 128 entries
(R * Ct <= 128) and a plane of its LDS 144 ((R + 2) * Ct <= 144)."""
import ctypes

import pytest

from orienmask_amd import lib as omlib

BM, EMAX = 128, 144


def _blocks(B, H, W):
    L = omlib.load()
    cls = (ctypes.c_int * 10)()
    pitch, tiles = ctypes.c_int(0), ctypes.c_longlong(0)
    n = L.om_conv2d_wino14_blocks(B, H, W, cls, ctypes.byref(pitch), ctypes.byref(tiles))
    return [tuple(cls[5 * k:5 * k + 5]) for k in range(n)], pitch.value, tiles.value


def _uniform_tiles(B, H, W):
    """One block shape for the whole layer, a zero row above and below every image: the tile columns cut into 1..8 equal blocks,
    each with the most rows the two bounds allow; the cut with the fewest blocks."""
    TW, gtot = (W + 3) // 4, B * (H + 2)
    best = None
    for split in range(1, 9):
        ct = -(-TW // split)
        r = BM // ct
        while r > 1 and (r + 2) * ct > EMAX:
            r -= 1
        if r < 1 or (r + 2) * ct > EMAX:
            continue
        r = min(r, gtot)
        tiles = -(-TW // ct) * -(-gtot // r)
        best = tiles if best is None else min(best, tiles)
    return best


@pytest.mark.parametrize("B", [1, 2, 3, 32])
def test_wino14_blocks_cover_the_layer_once(built, B):
    for H in (1, 3, 17, 20, 34, 68, 136, 272):
        for W in (4, 5, 17, 34, 66, 68, 136, 272):
            classes, pitch, tiles = _blocks(B, H, W)
            what = (B, H, W, classes, pitch, tiles)
            TW = (W + 3) // 4
            assert 1 <= len(classes) <= 2 and pitch in (H + 1, H + 2), what
            gtot = B * pitch + (1 if pitch == H + 1 else 0)        # shared zero rows: one more above the first image
            covered = [0] * TW
            nxt, total = 0, 0
            for t0, ct, ncb, r, nrb in classes:
                assert t0 == nxt and ncb >= 1, what
                # narrower than six tile columns (halo columns a large share of a block's pixels) only as ONE equal cut: where the
                # uniform rule's own narrow cut needs strictly fewer blocks (32 x 136 x 17: five blocks of one column, 175 for 176),
                # or "never more than the uniform rule" below could not hold
                assert ct >= min(6, TW) or (len(classes) == 1 and ct == -(-TW // ncb)), what
                assert 1 <= r and r * ct <= BM and (r + 2) * ct <= EMAX, what
                for cb in range(ncb):
                    assert t0 + cb * ct < TW, what                  # no block without a tile column of the image
                    for t in range(t0 + cb * ct, min(t0 + (cb + 1) * ct, TW)):
                        covered[t] += 1
                # row blocks [rb * r, (rb + 1) * r): every padded row 0 .. gtot - 1 in exactly one, none without a row
                assert (nrb - 1) * r < gtot <= nrb * r, what
                nxt = t0 + ncb * ct
                total += ncb * nrb
            assert covered == [1] * TW, what
            assert tiles == total and tiles <= _uniform_tiles(B, H, W), (what, _uniform_tiles(B, H, W))


def test_wino14_blocks_bench_shapes(built):
    """The 544^2 forward's maps at 32 images: blocks sized per column block, then with the zero row shared."""
    for size, per_block, shared in ((272, 4672, 4663), (136, 1184, 1177), (68, 300, 297), (34, 83, 81)):
        classes, pitch, tiles = _blocks(32, size, size)
        assert tiles <= (shared if pitch == size + 1 else per_block), (size, classes, pitch, tiles)
