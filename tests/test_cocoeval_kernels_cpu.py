"""The case tables of tests/cocoeval_cases.py, checked without a GPU.

Three things are proved here, so that tests/test_cocoeval_kernels.py (the same tables through the C API, on the GPU) means what
it says:
  1. every case really hits the edge it is named for -- judged by the restatement tests/cocoeval_np.py alone;
  2. tests/cocoeval_bitmap_np.py, a numpy model of the kernels' own algorithm, equals the restatement on every case;
  3. teeth: every mutant of that model -- a mistake a kernel could make -- differs from the restatement on at least one named
     case, so the table would catch that mistake in the kernels.

One mutant of the list cannot be caught by any case: what (int)NaN gives on a zero-length edge.  test_nan_cast_value_never_
reaches_a_toggle says why and proves it over the table and a seeded family of polygons; the kernel's comment claims less
("every value <= 0 gives the same mask")."""
import numpy as np
import pytest

import cocoeval_bitmap_np as B
import cocoeval_cases as C
import cocoeval_np as ref


# ----------------------------------------------------------------------------------------------- shared, computed once
_REF = {}


def ref_mask(name):
    """the restatement's [h, w] mask of a mask case, computed once and never written to"""
    if name not in _REF:
        _, h, w, segm = C.mask_case(name) if not name.startswith("iou_") else next(c for c in C.iou_mask_cases() if c[0] == name)
        m = ref.ann_mask(segm, h, w, strict=False)
        m.setflags(write=False)
        _REF[name] = m
    return _REF[name]


def trace_of(name):
    """what rle_fr_poly did on each polygon of a polygon case"""
    _, h, w, segm = C.mask_case(name)
    out = []
    for p in segm:
        if len(segm[0]) == 4:
            p = [p[0], p[1], p[0], p[1] + p[3], p[0] + p[2], p[1] + p[3], p[0] + p[2], p[1]]
        t = {}
        ref.rle_fr_poly([float(v) for v in p], h, w, trace=t)
        out.append(t)
    return out


def names(prefix):
    got = [c[0] for c in C.mask_cases() if c[0].startswith(prefix)]
    assert got, prefix
    return got


def model_differs(name, variant):
    _, h, w, segm = C.mask_case(name)
    words, stats = B.build_mask(segm, h, w, variant)
    want = ref_mask(name)
    return not np.array_equal(words, B.pack(want)) or stats != B.stats_of(want)


# -------------------------------------------------------------------------------------------- 1. the cases hit their edges
def test_sizes_cover_the_scan_and_word_shapes():
    assert {h for h, _ in C.SIZES} >= {1, 31, 32, 33, 64, 65, 97}
    assert {w for _, w in C.SIZES} >= {1, 2, 9, 65, 129, 130, 256, 257}
    words = {(h, w): w * ((h + 31) // 32) for h, w in C.SIZES}
    assert words[(32, 256)] == 256 and words[(32, 257)] == 257 and words[(33, 129)] == 258 and words[(97, 130)] == 520
    assert max(h for h, _ in C.SIZES) <= 97 and max(w for _, w in C.SIZES) <= 257
    used = {(c[1], c[2]) for c in C.mask_cases()}
    assert used == set(C.SIZES)
    # the scan: fewer words than threads, as many, one more, two and three words per thread, w == 1, h < 32, h % 32 == 0
    n_words = sorted(set(words.values()))
    assert min(n_words) < 256 and 256 in n_words and 257 in n_words and any(256 < n <= 512 for n in n_words)
    assert any(n > 512 for n in n_words)
    assert any(w == 1 for _, w in used) and any(h < 32 for h, _ in used) and any(h % 32 == 0 for h, _ in used)


def test_star_families_and_vertex_counts():
    for n in C.STAR_VERTICES:
        cases = names("star_%d_" % n)
        assert len(cases) >= 3
        for name in cases:
            segm = C.mask_case(name)[3]
            assert len(segm[0]) == 2 * n
            assert np.array_equal(np.round(segm[0], 2), segm[0])
    assert len(names("star_4096_")) + len(names("doubled_2048_")) <= 4           # the slow ones: a handful
    assert len(C.mask_case("doubled_2048_is_4096_32x257")[3][0]) == 2 * C.MAX_POLY_VERTICES
    past_a_wave = [c[0] for c in C.mask_cases() if isinstance(c[3], list) and max(len(p) for p in c[3]) > 128]
    assert len(past_a_wave) >= 20


@pytest.mark.parametrize("prefix", ["doubled_", "closed_", "triple_at_"])
def test_zero_length_edges_give_a_nan_slope(prefix):
    """a repeated vertex divides 0 / 0 inside rle_fr_poly: the point's v is (int)NaN, INT_MIN in the restatement"""
    for name in names(prefix):
        if "_4096_" in name or "_1000_" in name:
            continue                                         # the same construction; traced at the quicker sizes
        assert any(-2 ** 31 in t["v"] for t in trace_of(name)), name


def test_triple_runs_sit_at_index_0_and_64():
    for name, at in (("triple_at_0_33x129", 0), ("triple_at_64_33x129", 64)):
        p = np.array(C.mask_case(name)[3][0]).reshape(-1, 2)
        assert np.array_equal(p[at], p[at + 1]) and np.array_equal(p[at], p[at + 2]) and len(p) == 102
    p = np.array(C.mask_case("triple_at_0_and_64_33x129")[3][0]).reshape(-1, 2)
    assert np.array_equal(p[0], p[2]) and np.array_equal(p[66], p[68]) and not np.array_equal(p[2], p[3])


def test_closed_polygons_repeat_their_first_vertex():
    for name in names("closed_"):
        p = C.mask_case(name)[3][0]
        assert p[-2:] == p[:2]


def test_rectangles_reach_y_equal_h():
    """a boundary point with yd == h: in an inner column it toggles the top of the next one, in the last column nothing"""
    for name in names("rect_to_h_inner_") + names("rect_past_h_inner_"):
        _, h, w, _ = C.mask_case(name)
        t = trace_of(name)[0]
        assert any(y == h for y in t["y"]), name
        if w > 3:
            assert any(y == h and x < w - 1 for x, y in zip(t["x"], t["y"])), name
            assert ref_mask(name)[h - 1].any() and not ref_mask(name)[:, -1].any()
    for name in names("rect_to_h_last_column_") + names("rect_past_h_last_column_") + names("rect_whole_image_and_more_"):
        _, h, w, _ = C.mask_case(name)
        t = trace_of(name)[0]
        assert any(y == h and x == w - 1 for x, y in zip(t["x"], t["y"])), name
        assert ref_mask(name)[h - 1, w - 1] == 1, name


def test_outside_and_negative_cases():
    for name in names("outside_partly_"):
        _, h, w, segm = C.mask_case(name)
        v = np.array(segm[0]).reshape(-1, 2)
        assert ((v < 0) | (v > [w, h])).any() and 0 < ref_mask(name).sum() < h * w, name
    for name in names("outside_wholly_"):
        assert ref_mask(name).sum() == 0, name
    for name in names("outside_around_"):
        assert ref_mask(name).all(), name
    for name in names("outside_") + names("negative_small_"):
        _, h, w, segm = C.mask_case(name)
        v = np.array(segm[0]).reshape(-1, 2)
        assert (np.abs(v) <= 2 * np.array([w, h]) + 1e-9).all() and (v > -2 * np.array([w, h])).all(), name
    sides = {n.split("_")[2] for n in names("outside_partly_")}
    assert sides == {"left", "right", "top", "bottom"}
    for name in names("negative_small_"):
        v = np.array(C.mask_case(name)[3][0])
        assert (v < 0).any() and (np.trunc(5 * v + .5) != np.floor(5 * v + .5)).any()          # (int) truncates toward zero
        t = trace_of(name)[0]
        assert min(t["u"]) <= 0


def test_grid_cases_sit_on_their_grid():
    for step in (0.1, 0.3, 0.5):
        for name in names("grid_%s_" % str(step).replace(".", "p")):
            if "steps" in name:
                continue
            v = np.array(C.mask_case(name)[3][0])
            assert np.allclose(v / step, np.round(v / step), atol=1e-6), name
            assert ref_mask(name).any()
    v = np.array(C.mask_case("grid_0p1_steps_33x129")[3][0])
    assert {int(round(10 * x)) % 10 for x in v} == {1, 3, 5}


def test_box_quirk_odd_trailing_and_polygon_counts():
    for name in names("box_quirk_"):
        assert all(len(p) == 4 for p in C.mask_case(name)[3])
    for name in names("odd_trailing_"):
        p = C.mask_case(name)[3][0]
        assert len(p) % 2 == 1
        _, h, w, _ = C.mask_case(name)
        assert np.array_equal(ref_mask(name), ref.ann_mask([p[:-1]], h, w))
    seen = set()
    for how in ("disjoint", "overlapping"):
        for name in names("polys_"):
            if how not in name:
                continue
            _, h, w, segm = C.mask_case(name)
            seen.add(len(segm))
            each = [ref.ann_mask([p], h, w) for p in segm]
            overlap = int(sum(int(m.sum()) for m in each)) - int(ref_mask(name).sum())
            assert (overlap == 0) == (how == "disjoint"), name
    assert seen == {1, 2, 3, 5}
    assert ref_mask("poly_empty_mask_33x129").sum() == 0
    assert B.stats_of(ref_mask("poly_empty_mask_33x129")) == (0, 129, -1)
    assert ref_mask("polys_2_one_empty_33x129").sum() > 0


def _chars_per_count(s):
    out, n = [], 0
    for ch in s.encode("ascii"):
        n += 1
        if not (ch - 48) & 0x20:
            out.append(n)
            n = 0
    return out, n                                            # n > 0: the string ends inside a count


def test_sequence_cases_hit_their_edges():
    for h, w in C.SIZES:
        masks = dict(C.base_masks(h, w))
        assert masks["zeros"].sum() == 0 and masks["ones"].all() and masks["first_pixel"].T.ravel()[0] == 1
        assert masks["last_pixel"].T.ravel()[-1] == 1 and masks["last_pixel"].sum() == 1
        if w > 1:
            flat = masks["column_straddle"].T.ravel()
            assert flat[h - 1] == 1 and flat[h] == 1          # a run crosses the column boundary
        for kind in ("counts", "string"):
            for name, m in masks.items():
                assert np.array_equal(ref_mask("%s_%s_%dx%d" % (kind, name, h, w)), m)
    # to_string / rle_fr_string against hand-encoded strings: 0 -> '0', 16 -> 48 + (16 | 32), 48 + 0
    assert C.to_string([0]) == "0" and C.to_string([1]) == "1" and C.to_string([16]) == "`0" and C.to_string([15]) == "?"
    assert ref.rle_fr_string("`0") == [16] and ref.rle_fr_string("0?1") == [0, 15, 1]
    for name in names("string_"):
        segm = C.mask_case(name)[3]
        if "truncated" in name or "wraps" in name:
            continue
        c = ref.rle_fr_string(segm["counts"])
        assert C.to_string(c) == segm["counts"], name
    for name in names("counts_first_zero") + names("string_first_zero"):
        c = C.mask_case(name)[3]["counts"]
        assert (c if isinstance(c, list) else ref.rle_fr_string(c))[0] == 0 and ref_mask(name)[0, 0] == 1
    for name in names("counts_zero_run") + names("counts_two_zero_runs") + names("string_zero_run_cancels"):
        c = C.mask_case(name)[3]["counts"]
        c = c if isinstance(c, list) else ref.rle_fr_string(c)
        assert 0 in c[1:], name
    for name in names("counts_overrun") + names("string_overrun"):
        _, h, w, segm = C.mask_case(name)
        c = segm["counts"] if isinstance(segm["counts"], list) else ref.rle_fr_string(segm["counts"])
        assert sum(c) > h * w, name
    for name in names("counts_stop_short") + names("string_stop_short"):
        _, h, w, segm = C.mask_case(name)
        c = segm["counts"] if isinstance(segm["counts"], list) else ref.rle_fr_string(segm["counts"])
        assert sum(c) < h * w and ref_mask(name).sum() == 4 and not ref_mask(name)[:, 1:].any(), name
    per, rest = _chars_per_count(C.mask_case("string_4_chars_negative_difference_97x257")[3]["counts"])
    assert rest == 0 and per.count(4) == 2 and per[1] == 4 and per[3] == 4
    big = C.mask_case("counts_same_as_4_chars_97x257")[3]["counts"]
    assert big[3] - big[1] < -16384 and sum(big) == 97 * 257
    assert np.array_equal(ref_mask("string_4_chars_negative_difference_97x257"), ref_mask("counts_same_as_4_chars_97x257"))
    for name in names("string_overrun_5_chars"):
        assert 5 in _chars_per_count(C.mask_case(name)[3]["counts"])[0]
    for name in names("string_negative_count_wraps"):
        assert ref.rle_fr_string(C.mask_case(name)[3]["counts"])[3] == 2 ** 32 - 31
    for name in names("string_truncated"):
        s = C.mask_case(name)[3]["counts"]
        assert _chars_per_count(s)[1] > 0 and (s.encode()[-1] - 48) & 0x20, name
    assert ref.rle_fr_string(C.mask_case("string_truncated_97x257")[3]["counts"]) == [(97 * 257 - 100) & 1023]
    assert ref_mask("string_truncated_97x257").sum() == 0
    assert ref_mask("string_truncated_in_difference_97x257").sum() == 1700


def test_scan_and_merge_edges_are_in_the_table():
    carry_before_tail, three_sources, single_source = [], [], []
    for name, h, w, segm in C.mask_cases():
        m = ref_mask(name)
        mh = m.shape[0]
        if mh % 32 and m.shape[1] > 1 and (m[mh - 1, :-1] & m[0, 1:]).any():
            carry_before_tail.append(name)                   # a run of ones leaves a partial last word and enters the next column
        if isinstance(segm, list) and len(segm) >= 3:
            three_sources.append(name)
        if not isinstance(segm, list) or len(segm) == 1:
            single_source.append(name)
    assert len(carry_before_tail) >= 10 and any(n.startswith("rect_past_h") for n in carry_before_tail)
    assert len(three_sources) >= 4 and len(single_source) >= 100


def _iou_table():
    cases = C.iou_mask_cases()
    masks = [ref_mask(c[0]) for c in cases]
    crowd = C.iou_crowd()
    return cases, masks, crowd, ref.mask_iou(masks, masks, crowd)


def test_iou_table_has_its_edges():
    cases, masks, crowd, want = _iou_table()
    idx = {c[0]: i for i, c in enumerate(cases)}
    assert (want == -1).any() and (want == 0).any() and ((want > 0) & (want < 1)).any() and (want == 1).any()
    assert any(crowd) and not all(crowd)
    e = idx["poly_empty_mask_33x129"]
    assert masks[e].sum() == 0 and (want[e][[m.shape == (33, 129) for m in masks]] == 0).all()
    left, right = B.stats_of(masks[idx["outside_partly_left_33x129"]]), B.stats_of(masks[idx["outside_partly_right_33x129"]])
    assert left[2] < right[1] and want[idx["outside_partly_left_33x129"], idx["outside_partly_right_33x129"]] == 0
    a, b, c = (idx["iou_last_partial_word_%s_33x129" % k] for k in "abc")
    inter = masks[a] & masks[b]
    assert inter.any() and not inter[:32].any()              # overlap only in row 32: the second, partial word of a column
    assert want[a, b] == 20 / (120 + 50 - 20)
    assert (masks[a] & masks[c]).any() and not (masks[a] & masks[c])[32:].any()
    for i, j in ((a, idx["star_65_33x129"]), (idx["star_65_33x129"], idx["counts_checker_33x129"])):
        si, sj = B.stats_of(masks[i]), B.stats_of(masks[j])
        assert (si[1], si[2]) != (sj[1], sj[2]) and want[i, j] > 0                  # area outside the shared columns
    assert any(crowd[j] and 0 < want[i, j] != want[j, i] for i in range(len(cases)) for j in range(len(cases)))


def test_box_table_has_its_edges():
    dets, gts, crowd = C.box_table()
    want = ref.bb_iou(dets.tolist(), gts.tolist(), crowd.tolist())
    w = np.minimum(dets[:, None, 0] + dets[:, None, 2], gts[None, :, 0] + gts[None, :, 2]) - np.maximum(dets[:, None, 0], gts[None, :, 0])
    hh = np.minimum(dets[:, None, 1] + dets[:, None, 3], gts[None, :, 1] + gts[None, :, 3]) - np.maximum(dets[:, None, 1], gts[None, :, 1])
    assert ((w == 0) & (hh > 0)).any() and ((hh == 0) & (w > 0)).any() and ((w == 0) & (hh == 0)).any()
    assert (dets[:, 2] * dets[:, 3] == 0).sum() >= 3 and (gts[:, 2] * gts[:, 3] == 0).sum() >= 2
    assert (dets[:, :2] < 0).any() and (gts[:, :2] < 0).any() and crowd.any() and not crowd.all()
    assert (want == 1).any() and (want == 0).any() and ((want > 0) & (want < 1)).sum() > 20
    assert np.isfinite(want).all()
    neg = (dets[:, None, 0] < 0) & (gts[None, :, 0] < 0) & (want > 0)
    assert neg.any()
    assert (want[:, crowd.astype(bool)] > 0).any()


def _group(name):
    return next(g for g in C.match_groups() if g["name"] == name)


def _restated(g):
    """(dt_match, dt_ignore, gt_matched) of a group as [40, .] arrays from the restatement, lane t + 10 a"""
    return ref.Eval.match_lanes(g["gts"], g["dts"], g["ious"])


def test_match_groups_hit_their_edges():
    groups = C.match_groups()
    assert [g["name"] for g in groups][1:-1].count("dets_without_gts") == 1          # empty sides in the middle of the launch
    assert [g["name"] for g in groups][1:-1].count("gts_without_dets") == 1
    for g in groups:
        assert g["ious"].dtype == np.float64 and g["ious"].shape == (len(g["dts"]), len(g["gts"]))
        sc = [d["score"] for d in g["dts"]]
        assert sc == sorted(sc, reverse=True) and len(set(sc)) == len(sc) and all(d["id"] > 0 for d in g["dts"])
    g = _group("tie_later_gt_wins")
    assert (g["ious"][0] == 0.7).all()                       # equal IoUs on unmatched, regular GTs
    dtm, _, _ = _restated(g)
    assert dtm[0, 0] == 13 and dtm[0, 1] == 12 and dtm[0, 2] == 11          # the later GT wins each time
    g = _group("iou_at_thresholds")
    d = np.diag(g["ious"])
    assert all((d == t).sum() >= 1 for t in C.IOU_THRS) and all(v in d for v in (0.5, 0.55, 0.6, 0.7, 0.95))
    dtm, _, _ = _restated(g)
    for t, thr in enumerate(C.IOU_THRS):
        assert np.array_equal(dtm[t] != 0, d >= thr)         # at a threshold: matched; one ulp below: not
    g = _group("iou_one_and_clamp")
    assert (g["ious"] == 1.0).any() and (g["ious"] == 1 - 1e-10).any()
    g = _group("crowd_matched_by_several")
    dtm, dti, gtm = _restated(g)
    assert (dtm[0, :3] == 42).sum() >= 2 and dti[0, 0] == 1 and g["gts"][1]["iscrowd"] == 1
    g = _group("ignored_gt_not_taken_after_regular")
    dtm, dti, _ = _restated(g)
    assert dtm[10, 0] == 52 and g["ious"][0, 0] > g["ious"][0, 1] and dti[10, 0] == 0        # small: 0.95 on the crowd GT and
    assert dtm[0, 0] == 54 and dtm[20, 0] == 53 and dtm[30, 0] == 54      # 0.9 on an ignored one are passed by; other lanes, other GTs
    g = _group("gt_id_zero")
    dtm, dti, gtm = _restated(g)
    assert g["gts"][0]["id"] == 0 and dtm[0, 0] == 0 and gtm[0, 0] == 1 and dtm[0, 1] == 71
    assert dti[10, 1] == 0 and dti[20, 0] == 1               # "unmatched" by id 0 and out of the lane's area range: ignored
    g = _group("areas_at_range_edges")
    assert {1024.0, 9216.0} <= {x["area"] for x in g["gts"]} and {1024.0, 9216.0} <= {x["area"] for x in g["dts"]}
    recs = ref.Eval.match_direct(g["gts"], g["dts"], g["ious"])
    assert recs[1]["gtIgnore"][0] == 0 and recs[2]["gtIgnore"][0] == 0 and recs[2]["gtIgnore"][1] == 0 and recs[3]["gtIgnore"][1] == 0
    assert recs[2]["gtIgnore"][2] == 1 and recs[2]["gtIgnore"][3] == 1
    g = _group("hundred_dets_ninety_gts")
    assert g["ious"].shape == (100, 90) and any(x["iscrowd"] for x in g["gts"])
    ties = sum(len(set(r[r >= 0.5])) < (r >= 0.5).sum() for r in g["ious"])
    assert ties > 50


def test_host_vertex_limit():
    from orienmask_amd import cocoeval as CE
    assert CE.MAX_POLY_VERTICES == C.MAX_POLY_VERTICES
    h, w, srcs = CE._sources([C.star(4096, 97, 130)], 97, 130)
    assert srcs[0][1].size == 8192
    with pytest.raises(ValueError):
        CE._sources([C.star(4097, 97, 130)], 97, 130)
    CE._sources([C.star(4096, 97, 130) + [1.0]], 97, 130)     # an odd trailing number is no vertex


# ------------------------------------------------------------------------------- 2. the model equals the restatement
def test_model_equals_restatement_on_every_mask_case():
    for name, h, w, segm in C.mask_cases():
        assert not model_differs(name, None), name
    for name, h, w, segm in C.iou_mask_cases():
        words, stats = B.build_mask(segm, h, w)
        assert np.array_equal(words, B.pack(ref_mask(name))) and stats == B.stats_of(ref_mask(name)), name
        got, pad = B.unpack(words, *ref_mask(name).shape)
        assert np.array_equal(got, ref_mask(name)) and not pad


def _model_ious(variant=None):
    cases, masks, crowd, _ = _iou_table()
    built = [(B.pack(m), B.stats_of(m), m.shape) for m in masks]
    out = np.zeros((len(cases), len(cases)))
    for i, (a, sa, sza) in enumerate(built):
        for j, (b, sb, szb) in enumerate(built):
            out[i, j] = B.mask_iou(a, sa, b, sb, sza, szb, crowd[j], variant)
    return out


def test_model_equals_restatement_on_the_iou_table():
    want = _iou_table()[3]
    assert _model_ious().tobytes() == want.tobytes()


def test_model_equals_restatement_on_every_match_group():
    for g in C.match_groups():
        got = B.match(g["gts"], g["dts"], g["ious"], ref.IOU_THRS, ref.AREA_RNG)
        for x, y, what in zip(got, _restated(g), ("dt_match", "dt_ignore", "gt_matched")):
            assert np.array_equal(x, y), (g["name"], what)


# ------------------------------------------------------------------------------------------------------------ 3. teeth
MASK_MUTANT_FAMILIES = {
    "first_64_vertices": ("star_65_", "star_129_", "star_1000_", "closed_65_"),
    "prev_not_recomputed": ("star_65_", "star_128_", "star_129_", "star_1000_", "triple_at_64_"),
    "yh_dropped": ("rect_to_h_", "rect_past_h_"),
    "no_cancel": ("counts_zero_run", "counts_two_zero_runs", "string_zero_run", "outside_wholly_", "doubled_3_"),
    "carry_after_tail": ("rect_", "counts_ones_", "counts_checker_", "string_column_straddle_"),
    "no_tail_mask": ("rect_", "counts_ones_", "string_last_pixel_", "star_3_"),
}


@pytest.mark.parametrize("variant", sorted(MASK_MUTANT_FAMILIES))
def test_mask_mutant_is_caught(variant):
    caught = [n for p in MASK_MUTANT_FAMILIES[variant] for n in names(p) if model_differs(n, variant)]
    print("%s (%s): caught by %d cases, e.g. %s" % (variant, B.VARIANTS[variant], len(caught), caught[:4]))
    assert caught, "no case tells the mutant %r from the restatement" % variant


def test_iou_mutant_is_caught():
    cases, _, _, want = _iou_table()
    got = _model_ious("union_of_shared_columns")
    i, j = np.nonzero(got != want)
    print("union_of_shared_columns: caught by %d pairs, e.g. %s" % (len(i), [(cases[a][0], cases[b][0]) for a, b in zip(i[:2], j[:2])]))
    assert len(i) > 0


MATCH_MUTANT_GROUPS = {
    "first_tie_wins": "tie_later_gt_wins",
    "crowd_once": "crowd_matched_by_several",
    "ignored_pass_not_stopped": "ignored_gt_not_taken_after_regular",
    "area_exclusive": "areas_at_range_edges",
}


@pytest.mark.parametrize("variant", sorted(MATCH_MUTANT_GROUPS))
def test_match_mutant_is_caught(variant):
    caught = []
    for g in C.match_groups():
        got = B.match(g["gts"], g["dts"], g["ious"], ref.IOU_THRS, ref.AREA_RNG, variant)
        if any(not np.array_equal(x, y) for x, y in zip(got, _restated(g))):
            caught.append(g["name"])
    print("%s (%s): caught by %s" % (variant, B.VARIANTS[variant], caught))
    assert MATCH_MUTANT_GROUPS[variant] in caught            # by the group made for it


def test_every_mutant_has_a_test():
    assert set(B.VARIANTS) == set(MASK_MUTANT_FAMILIES) | set(MATCH_MUTANT_GROUPS) | {"union_of_shared_columns", "nan_large"}


def test_nan_cast_value_never_reaches_a_toggle():
    """The mutant 'nan_large' ((int)NaN is a large positive value) is not caught by any case, and cannot be.  A zero-length edge
    has one point, (u, v) = (x_j, (int)NaN).  v is read only where u differs from the neighbouring point's u, and both
    neighbours are the end of the edge before (vertex j) and the start of the edge after (vertex j + 1 = vertex j): their u is
    x_j too, exactly on a dx >= dy edge and as (int)(x_j + s * t + .5) otherwise, which is x_j for x_j >= 0.  For x_j < 0 the
    truncation toward zero can give x_j + 1, but then xd < 0 and the point is dropped.  So the device's 0, x86's INT_MIN and any
    other value give the same toggles: the divergence the kernel documents is harmless, and more so than its comment claims.
    Proved here on every polygon of the table and on a seeded family of small polygons with repeated vertices."""
    def same(xy, h, w):
        a = np.sort(B.poly_toggles(xy, h, w))
        return np.array_equal(a, np.sort(B.poly_toggles(xy, h, w, "nan_large")))
    n_nan = 0
    for name, h, w, segm in C.mask_cases():
        if isinstance(segm, list) and len(segm[0]) != 4:
            for p in segm:
                n_nan += int((B.poly_points(p, B.INT_MAX)[3] == B.INT_MAX).any())
                assert same(p, h, w), name
            assert not model_differs(name, "nan_large"), name
    assert n_nan > 30
    rng = np.random.default_rng(C.SEED + 2)
    for _ in range(1500):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        step = rng.choice([0.01, 0.1, 0.2, 0.5, 1.0])
        v = np.round(rng.uniform(-1.5, 2.5, size=(int(rng.integers(1, 7)), 2)) * np.array([w, h]) / step) * step
        v = np.repeat(v, rng.integers(1, 4, size=len(v)), axis=0)
        if rng.random() < 0.3:
            v = np.concatenate([v, v[:1]])
        assert same(v.ravel(), h, w), v.ravel().tolist()
