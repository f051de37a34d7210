"""CPU tests that the crowd tests have teeth (no GPU, and the reference is not read: only the fixtures and the restatements).

  * every directed case of tests/loss_cases.py is clean (all near-threshold counts 0) and the cases module covers, by its own
    arithmetic, every count of the ladder, every pile size, every seam value and a pile winner beyond index 256;
  * the kernel-shaped restatement (tests/loss_tiled_np.py: 16 x 64 forward tiles, 64 x 64 gradient tiles plus halo, culls in
    rounds of 64, the adjoint gathered per quarter pixel) equals LossNP / LossGradNP on every case;
  * each plausible kernel error of loss_tiled_np.MUTANTS fails the GPU test's own checkers (tests/loss_crowd_checks.py) on the
    directed case named here;
  * the crowd fixtures are those cases, as the reference computed them, within the size caps and with all near counts 0.
"""
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, golden_files
import loss_cases
import loss_crowd_checks as checks
import loss_grad_np
import loss_np
import loss_tiled_np

TARGET_NAMES = ("omask", "torien", "pos", "neg", "pscale", "txy", "twh", "tiou", "tcls")
# mutant -> (the directed case that catches it, the checker that does)
CAUGHT_BY = {1: ("order", "targets"), 2: ("order", "targets"), 3: ("order", "targets"), 4: ("pile", "targets"),
             5: ("pile", "targets"), 6: ("pile", "targets"), 7: ("ladder_65_0_130_1", "targets"), 8: ("seams", "targets"),
             9: ("seams", "grads"), 10: ("seams", "grads"), 11: ("tie", "targets")}


def _smooth(cfg):
    return np.float32(1.0 / max(cfg["num_classes"], 40) if cfg["label_smooth"] else 0)


@pytest.mark.parametrize("name", loss_cases.NAMES)
def test_case_is_clean_and_tiled_restatement_equals_restatement(name):
    """The case's seven near-threshold counts per scale are 0; the restatement passes every checker against itself; the tiled
    restatement, unmutated, gives LossNP's targets bit for bit and passes the value and gradient checkers."""
    cfg = loss_cases.build(name)[0]
    ref = loss_cases.reference(name)
    checks.check_near_zero(ref.near, name)
    checks.check_record(ref, ref, _smooth(cfg), name)
    got = loss_tiled_np.run(name)
    checks.check_record(got, ref, _smooth(cfg), name)
    for s in range(len(ref.values)):
        for k in TARGET_NAMES:
            a, b = got.values[s][2][k], ref.values[s][2][k]
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, s, k)
    assert got.near == ref.near


@pytest.mark.parametrize("mutant", sorted(loss_tiled_np.MUTANTS))
def test_mutant_is_caught(mutant):
    name, by = CAUGHT_BY[mutant]
    cfg = loss_cases.build(name)[0]
    ref = loss_cases.reference(name)
    got = loss_tiled_np.run(name, mutant)
    if by == "targets":
        caught = 0
        for s in range(len(ref.values)):
            try:
                checks.check_targets(got.values[s][2], ref.values[s][2], _smooth(cfg), (name, s))
            except AssertionError:
                caught += 1
        assert caught, (mutant, loss_tiled_np.MUTANTS[mutant], name)
    else:                                   # an error of the gradient's cull alone: the forward is untouched
        checks.check_values(checks.restatement_values(got), checks.restatement_values(ref), name)
        for s in range(len(ref.values)):
            checks.check_targets(got.values[s][2], ref.values[s][2], _smooth(cfg), (name, s))
        with pytest.raises(AssertionError):
            checks.check_grads(got.grads, ref.grads, name)
    with pytest.raises(AssertionError):
        checks.check_record(got, ref, _smooth(cfg), name)


def test_cases_cover_counts_piles_seams():
    counts, offsets, shapes = set(), set(), []
    for name in loss_cases.NAMES:
        gi = loss_cases.build(name)[2][2]
        counts |= set(np.diff(gi).tolist())
        offsets |= set(gi[:-1].tolist())
        shapes.append(np.diff(gi).tolist())
    assert set(loss_cases.LADDER_COUNTS) <= counts, counts
    assert any(g0 % 64 for g0 in offsets) and any(g0 % 256 and g0 > 256 for g0 in offsets), offsets
    assert any(0 in c[1:-1] and c[-1] == 0 for c in shapes), shapes                 # an empty image in the middle and at the end
    for name in loss_cases.LIMIT:
        assert max(np.diff(loss_cases.build(name)[2][2])) == 1024
    # piles: exactly the planted sizes on the planted cells, classes all different in one and repeated in another, one winner
    # (the highest index on the cell) beyond 256 with members in several rounds
    for name in ("pile", "pile_smooth", "pile_c1"):
        cfg, _, target = loss_cases.build(name)
        sizes = loss_cases.pile_sizes(cfg, target)
        planted = {(0, s, loss_cases._pile_key(cfg, s, anchor, cell)): idx for s, anchor, cell, idx, _ in loss_cases.PILES}
        assert all(sizes[k] == sorted(v) for k, v in planted.items())
        assert sorted(len(v) for v in planted.values()) == sorted(loss_cases.PILE_SIZES)
    cls = [c for *_, c in loss_cases.PILES]
    assert any(len(set(c)) == len(c) >= 5 for c in cls) and any(len(set(c)) < len(c) for c in cls)
    assert any(max(idx) > 256 and len({j // 64 for j in idx}) >= 3 for _, _, _, idx, _ in loss_cases.PILES)
    cfg, _, target = loss_cases.build("ladder_300_7_pile9")
    assert 9 in {len(v) for v in loss_cases.pile_sizes(cfg, target).values()}
    # seams
    cfg, _, target = loss_cases.build("seams")
    e = loss_cases.roi_edges(cfg, target)
    H, W = cfg["image_size"]
    assert H >= 128 and W >= 128
    assert set(loss_cases.SEAM_X2) <= e["x2"] and set(loss_cases.SEAM_X1) <= e["x1"]
    assert set(loss_cases.SEAM_Y2) <= e["y2"] and set(loss_cases.SEAM_Y1) <= e["y1"]
    m = loss_cases.match(cfg, target[0], 2)
    assert any((m.x1 == W - 1) & (m.x2 == W)) and any((m.y1 == H - 1) & (m.y2 == H))
    # order: three rounds
    assert [j // 64 for j in loss_cases.ORDER_INDICES] == [0, 1, 2]


def test_crowd_fixtures_are_the_cases_and_within_caps():
    old_largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if "crowd" not in f)
    total = 0
    for case, (stem, hseed, full) in loss_cases.FIXTURE_CASES.items():
        cfg, heads, target = loss_cases.build(case)
        for path, load in (("loss_%s.npz" % stem, loss_np.load_fixture), ("grad_loss_%s.npz" % stem, loss_grad_np.load_grad_fixture)):
            assert path in golden_files("loss_crowd_") + golden_files("grad_loss_crowd_")
            size = os.path.getsize(os.path.join(GOLDEN, path))
            assert size <= old_largest, (path, size)
            total += size
            g, fcfg, fheads, ftarget = load(os.path.join(GOLDEN, path))[:4]
            assert all(fcfg[k] == cfg[k] for k in cfg), path
            assert all(np.array_equal(a, b) and zlib.crc32(np.ascontiguousarray(a)) == zlib.crc32(np.ascontiguousarray(b))
                       for a, b in zip(ftarget, target)), path
            assert all(np.array_equal(a.numpy(), c.numpy()) and np.array_equal(b.numpy(), d.numpy())
                       for (a, b), (c, d) in zip(fheads, heads)), path
            assert all(not g["near_%d" % s].any() for s in range(3)), path
            if path.startswith("loss_"):
                assert ("t0_pos" in g.files) == full, path
    assert total <= 3e6, total
