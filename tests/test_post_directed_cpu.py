"""CPU: the directed postprocess cases (tests/post_cases.py) plant what they claim, the tie-rule restatement equals the oracle
wherever no tie touches a cut, and every deliberate error in a restatement changes the expectation of at least one case.
Every precondition and every tooth is printed (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import post_cases as K

_CACHE = {}


def _oracle_of(c):
    return K.make_oracle(K.SIZE, **c.cfg)


def _stable(cid, mutate=()):
    key = (cid, tuple(mutate))
    if key not in _CACHE:
        c = K.select_cases()[cid]
        _CACHE[key] = K.expected_stable(_oracle_of(c), c.predict, 0, mutate)
    return _CACHE[key]


def _scores(c):
    """(pair indices, float32 scores) of the passing pairs, row-major."""
    oracle = _oracle_of(c)
    conf = K.decode_conf(oracle, c.predict, 0).view(-1)
    idx = torch.nonzero(conf > oracle.conf_thresh).view(-1)
    return idx.numpy(), conf[idx].numpy()


def _same(a, b, keys=("bbox", "cls", "keep", "mask")):
    return all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("cid", list(K.select_cases()))
def test_select_case_plants_what_it_claims(built, cid):
    c = K.select_cases()[cid]
    cl = c.claims
    oracle = _oracle_of(c)
    pairs, score = _scores(c)
    bits = score.view(np.uint32)
    exp = _stable(cid)
    nms_pre = oracle.nms_pre
    facts = dict(total=int(pairs.size), n=int(min(pairs.size, nms_pre)), kept=exp["kept"])
    assert facts["total"] == cl["total"] == exp["total"] and facts["n"] == cl["n"], (cid, facts)
    if "kept" in cl:
        assert exp["kept"] == cl["kept"], (cid, exp["kept"])
    order = np.argsort(-score.astype(np.float64), kind="stable")          # visiting order: score descending, ties by pair index
    if "on_thresh" in cl:
        conf = K.decode_conf(oracle, c.predict, 0).view(-1).numpy()
        assert int((conf == np.float32(oracle.conf_thresh)).sum()) == cl["on_thresh"]
        facts["pairs_on_conf_thresh"] = cl["on_thresh"]
    if "tie_pairs" in cl:                                  # S5: a group of g equal keys of which r are inside the nms_pre cut
        T = bits[order[nms_pre - 1]]
        group = np.sort(pairs[bits == T])
        r = nms_pre - int((bits > T).sum())
        waves = sorted({K.wave_of_pair(int(p), 756 * K.C) for p in group})
        rows = sorted({int(p) // 256 for p in group})
        assert group.tolist() == cl["tie_pairs"] and len(group) == cl["g"] and r == cl["r"] and 1 < r < len(group), (cid, group, r)
        assert waves == cl["waves"] and rows == cl["rows"]
        assert (len(waves) >= 3) if cid.endswith("spread") else (len(rows) == 1), (cid, waves, rows)
        assert (cl["total"] > K.SEL_LIST_MAX) == ("radix" in cid)
        assert sorted(exp["pairs"].tolist())[:0] == [] and set(group[:r].tolist()) <= set(_selected_pairs(c)) and \
            not set(group[r:].tolist()) & set(_selected_pairs(c))
        facts.update(g=len(group), r=r, waves=waves, rows=rows)
    if cl.get("all_equal"):                                # S6
        assert len(set(bits.tolist())) == 1 and cl["total"] > K.SEL_LIST_MAX
        assert _selected_pairs(c) == sorted(pairs.tolist())[:nms_pre]
        facts.update(distinct_keys=1, r=nms_pre, above=0)
    if "shared_bits" in cl:                                # S7
        lo, hi = cl["around"]
        around = bits[order[lo:hi]]
        assert lo < nms_pre < hi and cl["total"] > K.SEL_LIST_MAX and len(set(bits.tolist())) == bits.size
        assert len(set((around >> 19).tolist())) == 1
        outside = np.concatenate([bits[order[:lo]], bits[order[hi:]]])
        if cl["shared_bits"] == 13:
            assert not (outside >> 19 == around[0] >> 19).any()                   # the level-1 bin holds these keys only ...
            assert len(set((around >> 8).tolist())) == around.size                 # ... and level 2 separates them
        else:
            assert around.tolist() == cl["keys"] and len(set((around >> 8).tolist())) == 1
            assert not (outside >> 8 == around[0] >> 8).any()
            assert int(bits[order[nms_pre - 1]]) - int(bits[order[nms_pre]]) == 1      # the cut: two keys one ulp apart
        facts.update(shared_bits=cl["shared_bits"], keys_sharing=int(around.size))
    if "post_ties" in cl:                                  # S8
        ks = exp["bbox"][:, 4].numpy().view(np.uint32)
        T = ks[oracle.nms_post - 1]
        kept_scores = bits[np.isin(pairs, _selected_pairs(c))]
        assert exp["kept"] > oracle.nms_post and int((kept_scores == T).sum()) == cl["g"]
        assert int((ks == T).sum()) == cl["r"] and 1 < cl["r"] < cl["g"]
        assert sorted(pairs[bits == T].tolist()) == cl["post_ties"]
        assert exp["pairs"][ks == T].tolist() == cl["post_ties"][:cl["r"]]        # the lowest pair indices of the group
        facts.update(g=cl["g"], r=cl["r"])
    if "partners" in cl:                                   # S4
        rank_of = {int(p): k for k, p in enumerate(pairs[order])}
        kept_ranks = {rank_of[int(p)] for p in _kept_pairs(c)}
        assert set(range(cl["n"])) - kept_ranks == {j for _, j in cl["partners"]}, cid
        n = cl["n"]
        assert (n > K.SEL_LDS_MASK_N) == any(j >= 512 for _, j in cl["partners"])
        assert any(i // 64 != j // 64 for i, j in cl["partners"]) and any(i // 64 == j // 64 for i, j in cl["partners"])
        assert any(i < 448 <= j for i, j in cl["partners"]) and any(i >= 448 for i, _ in cl["partners"])
        facts.update(suppressed=sorted(j for _, j in cl["partners"]))
    if cid.startswith("S3"):
        s = exp["bbox"][:, 4].numpy()
        if exp["kept"] <= oracle.nms_post:
            assert (np.diff(s) > 0).any() and (np.diff(s) < 0).any()              # index order is not score order
            assert (np.diff(exp["pairs"].numpy()) > 0).all()
        else:
            assert (np.diff(s) < 0).all() and s.size == oracle.nms_post
    if not c.stable:
        assert len(set(bits.tolist())) == bits.size or cl["total"] <= nms_pre
        want = oracle(c.predict)[0]
        assert _same(exp, want), (cid, "expected_stable differs from the oracle although no tie touches a cut")
        facts["expected_stable_equals_oracle"] = True
    print("precondition %s: %s" % (cid, facts))


def _selected_pairs(c):
    """Pairs inside the nms_pre cut under the tie rule (before NMS)."""
    pairs, score = _scores(c)
    order = np.argsort(-score.astype(np.float64), kind="stable")
    return sorted(pairs[order[:_oracle_of(c).nms_pre]].tolist())


def _kept_pairs(c):
    """Pairs that survive NMS (nms_post = nms_pre, so that none is cut)."""
    cfg = dict(c.cfg)
    cfg["nms_post"] = cfg.get("nms_pre", 400)
    return K.expected_stable(K.make_oracle(K.SIZE, **cfg), c.predict, 0)["pairs"].tolist()


def test_s2_selections_are_identical(built):
    a, b, c = (_stable("S2_total%d" % t) for t in (4095, 4096, 4097))
    assert _same(a, b) and _same(b, c) and a["bbox"].shape[0] == 400
    assert (a["total"], b["total"], c["total"]) == (4095, 4096, 4097)
    print("precondition S2: 4095 / 4096 / 4097 passing pairs give the same 400 detections")


def test_s9_members_exist(built):
    for cid in K.S9_MEMBERS:
        assert cid is None or cid in K.select_cases()
    conf = K.decode_conf(K.make_oracle(K.SIZE), K.empty_predict(), 0)
    assert not (conf > K.CONF_THRESH).any()
    conf = K.decode_conf(K.make_oracle(K.SIZE), K.all_pass_predict(1), 0)
    assert (conf > K.CONF_THRESH).all() and conf.numel() == 756 * K.C


SELECT_TEETH = {"ge_thresh": ["S1t_pair_on_conf_thresh"], "highest_first": ["S5_list_spread", "S5_list_one_row", "S5_radix_spread",
                                                                          "S5_radix_one_row", "S6_all_keys_equal"],
                "caseB_sorted": ["S1_pre400_total399", "S1_pre400_total400", "S3_kept99", "S3_kept100"]}


@pytest.mark.parametrize("mutation", list(SELECT_TEETH))
def test_select_restatement_has_teeth(built, mutation):
    changed = [cid for cid in K.select_cases() if not _same(_stable(cid), _stable(cid, (mutation,)))]
    print("tooth %s changes the expectation of: %s" % (mutation, changed))
    assert set(SELECT_TEETH[mutation]) <= set(changed), (mutation, changed)


# ------------------------------------------------------------------------------------------------------------------------
# mask cases
# ------------------------------------------------------------------------------------------------------------------------
def _expected(cid):
    if ("m", cid) not in _CACHE:
        _CACHE[("m", cid)] = K.expected_masks(K.mask_cases()[cid])
    return _CACHE[("m", cid)]


def test_mask_case_table_covers_what_it_claims(built):
    cases = K.mask_cases()
    f1 = {(c.size, K.ANCHOR_MASKS.index(c.anchor_mask)) for c in cases.values() if c.id.startswith("F1")}
    assert f1 == {(s, m) for s in K.GEOMETRIES for m in range(3)}
    assert [len(K.field_table(m)) for m in K.ANCHOR_MASKS] == [9, 8, 6]
    for c in cases.values():
        assert not K.mask_launch_unchunked(c.size, c.oriens.shape[0], len(K.field_table(c.anchor_mask))), c.id      # chunks of 8
        assert c.dets.shape == (c.oriens.shape[0], c.nms_post, 5) and c.fields.dtype == torch.int32 and int(c.counts.max()) <= c.nms_post
        for b in range(c.oriens.shape[0]):
            assert torch.isnan(c.dets[b, int(c.counts[b]):]).all()
    u = K.UNCHUNKED
    assert K.mask_launch_unchunked(u["size"], u["batch"], 9) and not K.mask_launch_unchunked(u["size"], u["batch"] - 1, 9)
    assert (512 // 4 + 1) * (512 // K.MASK_PX) == 4128 and 17 * 14 * 9 == 2142 >= 2048 > 17 * 13 * 9
    assert not K.mask_launch_unchunked(u["size"], 1, 9)              # the first image alone: chunks of 8
    d3 = cases["D3_100_on_one_field"]
    assert (d3.fields[0] == 4).all() and int(d3.counts[0]) == 100 and 100 > 64 and -(-100 // 8) == 13      # two ballot rounds, 13 chunks
    d3 = cases["D3_65_and_35_interleaved"]
    f = d3.fields[0].numpy()
    assert (f == 1).sum() == 65 and (f == 8).sum() == 35 and K.field_table(d3.anchor_mask)[1][0] != K.field_table(d3.anchor_mask)[8][0]
    assert (np.diff(np.flatnonzero(f == 8)) > 1).any() and (np.diff(np.flatnonzero(f == 1)) > 1).any()          # interleaved slots
    assert cases["D3_counts_0_100_37"].counts.tolist() == [0, 100, 37]
    print("precondition masks: %d cases; unchunked form from 14 images of 512 x 512 on (2142 >= 2048), 13 images: 1989" % len(cases))


@pytest.mark.parametrize("cid", [c for c in K.mask_cases() if c.startswith("D1")])
def test_d1_thresholds_sit_on_the_distance(built, cid):
    c = K.mask_cases()[cid]
    oracle, P = K._pixel_field(c.size, c.anchor_mask, c.oriens[0].numpy())
    table = K.field_table(c.anchor_mask)
    for f, (s, aid) in enumerate(table):                      # F2: constant few-bit planes interpolate exactly -> closed form
        nH, nW = oracle.grids[s]
        for ch, n, npix in ((0, nW, c.size[1]), (1, nH, c.size[0])):
            v = K.F32(K.FEW_BIT[2 * f + ch])
            base = torch.arange(npix, dtype=torch.float) / npix * n
            closed = (v * oracle.grid_anchors[aid, ch]) / 2 + base
            got = P[aid, ch]
            assert torch.equal(got, closed.view(1, -1).expand_as(got) if ch == 0 else closed.view(-1, 1).expand_as(got)), (cid, f, ch)
    count = {(ax, kind): 0 for ax in "xy" for kind in ("eq", "lo", "hi")}
    want = _expected(cid)[0]
    for k, ax, kind, px in c.claims["kinds"]:
        s, aid = table[int(c.fields[0, k])]
        gs = oracle.grid_sizes[aid].numpy()
        ch = "xy".index(ax)
        d = np.abs(P[aid, ch].numpy() - gs[ch] * c.dets[0, k, ch].numpy())
        t = (K.F32(0.3) * c.dets[0, k, 2 + ch].numpy()) * gs[ch]
        target = {"eq": d, "lo": np.nextafter(d, K.F32(-np.inf)), "hi": np.nextafter(d, K.F32(np.inf))}[kind]
        on = t == target
        line = on[0, :] if ax == "x" else on[:, 0]
        assert line[px], (cid, k, ax, kind, px)
        count[(ax, kind)] += int(on.sum())
        # the strict < decides: on equality and one float below the pixel is outside, one float above it is inside
        assert (want[k][on] == (kind == "hi")).all(), (cid, k, kind)
    print("precondition %s: pixels with the threshold on / one float below / one float above |P - c|: %s" % (cid, count))
    assert min(count.values()) >= 32, count


@pytest.mark.parametrize("cid", list(K.mask_cases()))
def test_upsample_restatement_equals_torch(built, cid):
    """Both forms of torch's bilinear x4 (tests/post_cases.py:torch_small_output_form), bit for bit, NaNs in the same places."""
    c = K.mask_cases()[cid]
    up = torch.cat([torch.nn.functional.interpolate(o, scale_factor=4.0, mode="bilinear", align_corners=False)
                    for _, o in K.split_oriens(c.oriens, c.anchor_mask)], 1).numpy()
    small = K.torch_small_output_form(c.size)
    assert small == (c.size in ((32, 32), (96, 32)))
    for b in range(up.shape[0]):
        for ch in range(up.shape[1]):
            got = K.upsample_x4(c.oriens[b, ch].numpy(), small=small)
            nan = np.isnan(up[b, ch])
            assert np.array_equal(np.isnan(got), nan), (cid, b, ch)
            assert np.array_equal(got[~nan].view(np.uint32), up[b, ch][~nan].view(np.uint32)), (cid, b, ch)
    if small and cid.startswith("F1"):          # the two forms do differ: a kernel with one form only cannot pass both kinds of geometry
        other = K.upsample_x4(c.oriens[0, 0].numpy(), small=False)
        assert not np.array_equal(other, up[0, 0])


@pytest.mark.parametrize("cid", list(K.mask_cases()))
def test_mask_restatement_equals_the_oracle(built, cid):
    want = _expected(cid)
    got = K.restated_masks(K.mask_cases()[cid])
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (cid, b, int((g != w).sum()))


def test_special_boxes_are_never_inside(built):
    for cid in [c for c in K.mask_cases() if c.startswith("D2")]:
        c = K.mask_cases()[cid]
        want = _expected(cid)[0]
        empty = [k for k in c.claims["special"] if not want[k].any()]
        full = [k for k in c.claims["special"] if want[k].any()]
        sizes = c.dets[0, :, 2:4].numpy()
        for k in c.claims["special"]:
            bad = ~(sizes[k] > 0) | ~np.isfinite(c.dets[0, k, :2].numpy()).all()          # 0, -0, negative, NaN size; non-finite centre
            if bad.any():
                assert not want[k].any(), (cid, k, c.dets[0, k])
        assert len(empty) >= 20 and len(full) >= 4, (cid, len(empty), len(full))          # +inf and 3e38 sizes: infinite thresholds
        print("precondition %s: %d special detections with an empty mask, %d with pixels" % (cid, len(empty), len(full)))


MASK_TEETH = {"le": "D1", "left_unclamped": "F1", "top_unclamped": "F1", "neg_abs": "D2", "top_row0_twice": "F3"}


@pytest.mark.parametrize("mutation", K.MASK_MUTATIONS)
def test_mask_restatement_has_teeth(built, mutation):
    changed = []
    for cid, c in K.mask_cases().items():
        got = K.restated_masks(c, (mutation,))
        if any(not np.array_equal(g, w) for g, w in zip(got, _expected(cid))):
            changed.append(cid)
    print("tooth %s changes the expectation of: %s" % (mutation, changed))
    assert any(cid.startswith(MASK_TEETH[mutation]) for cid in changed), (mutation, changed)
    if mutation == "top_row0_twice":          # equal to the right form on finite data: only the non-finite plants can show it
        assert all(cid.startswith("F3") for cid in changed), changed
        c = K.mask_cases()["F3_nonfinite_32x32"]
        got = K.restated_masks(c, (mutation,))
        hit = {spot for (i, spot, ch, y, x) in c.claims["planted"] if not np.array_equal(got[i], _expected(c.id)[i])}
        assert hit == {"row1"}, hit


def _fused_oracle(c):
    from oracle import orienmask_ref as R
    cfg = dict(c.cfg)
    anchors = cfg.pop("anchors", K.ANCHORS_YOLOV4)
    return R.PostProcessOracle(K.grids_of(K.SIZE), list(K.SIZE), anchors, K.ANCHOR_MASK, K.C, conf_thresh=K.CONF_THRESH, **cfg)


def test_fused_d1_centres_sit_on_the_threshold(built):
    """The heads of D1_fused decode (tw = th = 0: the box is its anchor, exactly) to centres whose distance to a pixel's position
    equals the threshold in float32, and to the nearest centres on either side."""
    c = K.fused_cases()["D1_fused"]
    oracle = _fused_oracle(c)
    exp = K.expected_stable(oracle, c.predict, 0)
    assert _same(exp, oracle(c.predict)[0])
    P = oracle.orien_field(c.predict, 0)
    pairs = exp["pairs"].tolist()
    decided = {"x": 0, "y": 0}
    for pair, ax, kind, px in c.claims["kinds"]:
        k = pairs.index(pair)
        a = int(oracle.flat_anchor_idx[pair // K.C])
        ch = "xy".index(ax)
        gs = oracle.grid_sizes[a].numpy()
        box = exp["bbox"][k].numpy()
        assert box[2] == np.float32(32) / np.float32(128) and box[3] == np.float32(24) / np.float32(96)
        t = (np.float32(0.3) * box[2 + ch]) * gs[ch]
        line = P[a, ch, 0, :].numpy() if ax == "x" else P[a, ch, :, 0].numpy()
        d = np.abs(line[px] - gs[ch] * box[ch])
        assert {"eq": d == t, "lo": d > t, "hi": d < t}[kind], (pair, ax, kind, d, t)
        m = exp["mask"][k].numpy()
        at = m[:, px] if ax == "x" else m[px, :]
        assert not at.any() or kind == "hi"
        decided[ax] += int(kind == "hi" and at.any())
    print("precondition D1_fused: %d detections, triples decided by the strict < on x / y: %s" % (len(pairs), decided))
    assert decided["x"] >= 1 and decided["y"] >= 1


def test_fused_d2_heads_decode_to_special_boxes(built):
    c = K.fused_cases()["D2_fused"]
    want = _fused_oracle(c)(c.predict)[0]
    b = want["bbox"].numpy()
    assert b.shape[0] == c.claims["total"]
    facts = dict(zero=int((b[:, 2:4] == 0).sum()), inf=int(np.isinf(b[:, 2:4]).sum()), nan_size=int(np.isnan(b[:, 2:4]).sum()),
                 nan_centre=int(np.isnan(b[:, :2]).sum()), denormal=int(((b[:, 2:4] > 0) & (b[:, 2:4] < 1e-38)).sum()),
                 huge=int(((b[:, 2:4] > 1e37) & np.isfinite(b[:, 2:4])).sum()))
    print("precondition D2_fused: %s" % facts)
    assert facts["zero"] >= 2 and facts["inf"] == 2 and facts["nan_size"] == 2 and facts["nan_centre"] == 2 and facts["huge"] >= 1
    empty = [k for k in range(b.shape[0]) if not want["mask"][k].any()]
    assert len(empty) >= 6 and len(empty) < b.shape[0]
