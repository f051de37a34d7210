"""CPU: the directed augmentation cases (tests/augment_cases.py) are well-formed, their conditions can be met by a float32
composition (augment_np.render_image32 through the checkers the GPU tests use), and each plausible bug fails them."""
import numpy as np
import pytest

import augment_cases as K
import augment_np as A
from test_augment_cpu import SEAM_EPS
from orienmask_amd import augment

LATTICE = K.lattice_cases()
GROUPS = {"lattice": LATTICE["u8"] + LATTICE["frac"] + LATTICE["wide"], "geometry": K.geometry_cases(), "graymean": K.graymean_cases(),
          "batch": K.batch_cases(), "noop": K.noop_cases()}


def test_collate_accepts_every_case_and_factors_are_float32():
    cases = K.all_cases()
    assert len({c.id for c in cases}) == len(cases)
    for f in K.factors(cases):
        assert float(np.float32(f)) == f and float(np.float32(1 - f)) == 1 - f and float(np.float32(f * 360)) == f * 360, f
    for c in cases:
        pb = augment.collate([K.planned(c)])
        assert pb.out_hw == K.plan_of(c)['out'] and pb.N == len(c.masks), c.id
        assert pb.any_contrast == any(code == K.C for code, _ in c.ops)
    frac = augment.collate([K.planned(c) for c in K.batch_cases()])
    assert frac.image.dtype.is_floating_point and frac.B == 5 and frac.any_contrast
    u8 = augment.collate([K.planned(c) for c in K.batch_cases()[:4]])
    assert not u8.image.dtype.is_floating_point
    for name in ("u8", "frac"):
        assert augment.collate([K.planned(c) for c in LATTICE[name]]).B == len(K.chains())
    assert augment.collate([K.planned(c) for c in K.graymean_cases()]).out_hw == (32, 32)


def test_case_tables_cover_what_they_claim():
    ids = [cid for cid, _ in K.chains()]
    assert len(ids) == len(set(ids)) == 15 + 6 + 4 + 72
    orders = {tuple(code for code, _ in ops) for _, ops in K.chains() if len(ops) == 4}
    assert len(orders) == 24
    subsets = {frozenset(code for code, _ in ops) for _, ops in K.chains() if len(ops) in (2, 3)}
    assert len(subsets) == 10
    assert LATTICE["u8"][0].image.shape == (1, 1331, 3) and LATTICE["u8"][0].image.dtype == np.uint8
    frac = K.planned(LATTICE["frac"][0])['image']
    assert frac.dtype == np.float32 and (frac != np.round(frac)).all()
    plans = {c.id: K.plan_of(c) for c in GROUPS["geometry"]}
    row = {cid: augment.sample_row(p, 0, 0, 0, 2) for cid, p in plans.items()}
    assert [cid for cid in plans if row[cid]['area2x']] == ["geo_area2x_odd_last"]
    p = plans["geo_area2x_odd_last"]
    assert p['crop'][0] % 2 == 1 and p['crop'][1] % 2 == 1 and p['crop'][0] + p['crop'][2] == p['src_h'] and p['crop'][1] + p['crop'][3] == p['src_w']
    for cid in K.ONE_AXIS:
        ch, cw, (nh, nw) = plans[cid]['crop'][2], plans[cid]['crop'][3], plans[cid]['resize'][:2]
        assert (ch == 2 * nh) != (cw == 2 * nw)
    assert plans["geo_crop_w1"]['crop'][3] == 1 and plans["geo_crop_h1"]['crop'][2] == 1
    assert plans["geo_nw1"]['resize'][1] == 1 and plans["geo_nh1"]['resize'][0] == 1
    assert plans["geo_pad_bottom_flush"]['resize'][0] + plans["geo_pad_bottom_flush"]['resize'][2] == plans["geo_pad_bottom_flush"]['out'][0]
    assert (plans["geo_plane_15x17"]['out'][0] * plans["geo_plane_15x17"]['out'][1]) % 16 != 0
    c = plans["geo_corner_up"]['crop']
    assert c[0] + c[2] == plans["geo_corner_up"]['src_h'] and c[1] + c[3] == plans["geo_corner_up"]['src_w']
    chunk = {c.id: -(-c.image.shape[0] * c.image.shape[1] // A.GRAY_BLOCKS) for c in K.all_cases()}
    assert chunk[K.BIG] == 586 and -(-chunk[K.BIG] // A.GRAY_THREADS) == 3
    assert max(v for cid, v in chunk.items() if not cid.startswith(K.BIG)) <= A.GRAY_THREADS     # every other source: one pass


def test_branches_agree_with_jitter_outside_the_seam():
    for c in LATTICE["u8"][::7] + LATTICE["frac"][::5] + K.graymean_cases()[-1:]:
        a, alt, seam = A.jitter_branches(c.image, c.ops, SEAM_EPS)
        assert np.array_equal(a, A.jitter(c.image, c.ops)), c.id
        assert np.array_equal(a[~seam], alt[~seam]), c.id
    # a chain whose hue op nothing follows: alt differs from a on seam pixels only, and does differ there
    img = K.lattice_u8()
    a, alt, seam = A.jitter_branches(img, [(K.B, 1.0625), (K.H, 0.109375)], SEAM_EPS)
    assert seam.any() and np.array_equal(a[~seam], alt[~seam]) and (a[seam] != alt[seam]).any()
    assert A.jitter_branches(img, [(K.B, 1.0625)], SEAM_EPS)[2].sum() == 0


def _standin_worst(name, cases):
    worst = K.Worst("stand-in, " + name)
    for c in cases:
        worst.add(K.check_image(K.standin(c), c), c.id)
    print(worst)
    return worst


def test_conditions_can_be_met_lattice():
    """The float32 stand-in passes every lattice chain on both sources under the checker and bounds of the GPU test."""
    no_hue = [c for c in GROUPS["lattice"] if K.bound_of(c) == K.BOUND_NO_HUE]
    hue = [c for c in GROUPS["lattice"] if K.bound_of(c) == K.BOUND_HUE]
    assert len(no_hue) == 2 * 14 and len(hue) == 2 * 83 + 3
    _standin_worst("lattice without hue", no_hue)
    _standin_worst("lattice with hue", hue)
    for c in LATTICE["u8"]:
        if c.ops[0][0] == K.H:         # g - b is exact on integers: the float32 hue cannot be on the other side of the seam
            assert K.check_image(K.standin(c), c)["alt"] == 0, c.id


def test_conditions_can_be_met_geometry_graymean_batch_noop():
    for name in ("geometry", "graymean", "batch"):
        _standin_worst(name, GROUPS[name])
    for c in GROUPS["geometry"]:
        K.check_pad(K.standin(c), c)
    for c in GROUPS["graymean"][1:4]:
        assert K.check_pad(K.standin(c), c) > 0
    for c in GROUPS["noop"]:
        assert np.array_equal(K.standin(c)[:, 0].T.view(np.uint32), c.image[0].astype(np.float32).view(np.uint32))


MUTATIONS = ["sector_swap", "gray_bgr", "mean_of_crop", "mean_before_ops", "hue_clip_255", "area2x_one_axis", "mean_first_pass",
             "hue_wrap", "image_edge"]


def _caught(mut, cases):
    return [c.id for c in cases if K.fails(K.check_image, K.standin(c, (mut,)), c)]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_directed_cases_catch_mutation(mut):
    """Each plausible bug, put into the stand-in, fails the checker on some directed case."""
    cases = [c for g in ("lattice", "geometry", "graymean", "batch") for c in GROUPS[g]]
    caught = _caught(mut, cases)
    print("%s: caught by %d of %d cases, e.g. %s" % (mut, len(caught), len(cases), caught[:4]))
    assert caught, "mutation %s is not caught by any directed case" % mut
    if mut == "mean_first_pass":        # the 300x500 source is the one that reaches the second pass of the reduction loop
        assert set(caught) == {K.BIG, K.BIG + "_hsc"}
    if mut == "area2x_one_axis":
        assert set(caught) == set(K.ONE_AXIS)
    if mut == "mean_of_crop":
        assert {K.BIG, "gray_1x257", "gray_16x16", "bat_contrast"} <= set(caught)
    if mut == "hue_clip_255":
        assert all(cid.startswith("lat_wide") for cid in caught)
    if mut == "image_edge":
        assert "geo_corner_up" in caught


def test_float64_mutations_move_the_restatement_too():
    """The same mutations in the float64 jitter / place_image change the expected value beyond the bound (they are not no-ops
    there either)."""
    cases = {c.id: c for c in K.all_cases()}
    for mut, cid in (("sector_swap", "lat_u8_h+0.109375"), ("gray_bgr", "lat_u8_s+0.5"), ("mean_of_crop", K.BIG), ("mean_before_ops", K.BIG + "_hsc"),
                     ("hue_clip_255", "lat_wide_h-"), ("area2x_one_axis", "geo_rows2x"), ("mean_first_pass", K.BIG)):
        c = cases[cid]
        plan = K.plan_of(c)
        assert np.abs(A.render_image(c.image, plan, (mut,)) - A.render_image(c.image, plan)).max() > 10 * K.bound_of(c), (mut, cid)
