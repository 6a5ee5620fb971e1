"""CPU checks of tests/kmeans_cases.py: the references are right, and every case reaches the edge of csrc/labels_kmeans.hip it names.
The claims are conditions, not measurements: a case that stops meeting one fails here, before the GPU file relies on it."""
import warnings

import numpy as np
import pytest
import torch

import kmeans_cases as kc
from kmeans_cases import HEAD, KMEANS_CASES, REP_CASES


def _ids(cases):
    return [c.name for c in cases]


K1_CASES = [c for c in KMEANS_CASES if c.name.startswith(("tail_", "fast_C", "mfma_K1_"))]


@pytest.mark.parametrize("case", K1_CASES, ids=_ids(K1_CASES))
def test_ordered_sum_is_the_oracles_k1_code_book(case):
    d = case.data()
    cen, lab, cnt, _ = case.reference()
    assert int(d["seg_k"][0]) == 1 and cnt[0, 0] == len(d["pool"]) and not lab.any()
    assert np.array_equal(cen[0, 0], kc.ordered_mean(d["pool"]))


@pytest.mark.parametrize("case", KMEANS_CASES + REP_CASES, ids=_ids(KMEANS_CASES + REP_CASES))
def test_reference_equals_scipy(case):
    vq = pytest.importorskip("scipy.cluster.vq")
    d = case.data()
    cen, lab, cnt, _ = case.reference()
    for s, k in enumerate(d["seg_k"]):
        if k == 0:
            continue
        beg, end = d["offs"][s], d["offs"][s + 1]
        x = d["pool"][d["rows"][beg:end]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cb, l = vq.kmeans2(x, x[kc.clamp_init(d["init"][s, :k], end - beg)].copy(), minit="matrix", iter=d["iters"])
        assert np.array_equal(l, lab[beg:end]) and np.array_equal(cb, cen[s, :k]), f"segment {s}"


CLAIMING = [c for c in KMEANS_CASES if c.claims]


@pytest.mark.parametrize("case", CLAIMING, ids=_ids(CLAIMING))
def test_case_reaches_the_paths_it_names(case):
    rep = kc.classify_case(case)
    assert rep is not None and rep["tailed_clusters"] > 0, "no cluster beyond its literal head"
    for claim in case.claims:
        assert rep[claim] >= 1, f"{case.name}: {claim} = {rep[claim]} ({ {k: v for k, v in rep.items() if k != 'counts'} })"


def test_tail_boundary_cases_sit_on_the_boundary():
    sizes = sorted(len(c.data()["pool"]) for c in kc.TAIL_CASES)
    assert sizes == [HEAD, HEAD + 1, HEAD + kc.CHUNK, HEAD + kc.CHUNK + 1, 12000, 12000, 12000]
    assert sorted(c.data()["iters"] for c in kc.TAIL_CASES if len(c.data()["pool"]) == 12000) == [1, 2, 20]


def test_moving_membership_crosses_the_head_both_ways():
    rep = kc.classify_case(kc.MOVING_CASE)
    counts = np.array(rep["counts"])
    assert counts.shape == (20, 2) and (counts.sum(1) == 20600).all()
    assert rep["count_up_through_head"] >= 1 and rep["count_down_through_head"] >= 1 and rep["chunk_binade_moved"] >= 1


def test_tie_cases_tell_wrong_summation_orders_apart():
    """On the dyadic column a pairwise sum, a float64 sum rounded once and a ties-away sum each miss the sequential sum by a bit."""
    x = kc.tail_columns(12000)[:, :1]
    want = np.add.accumulate(x, axis=0, dtype=np.float32)[-1]
    pairwise = np.sum(x, axis=0, dtype=np.float32)
    once = np.sum(x.astype(np.float64), axis=0).astype(np.float32)
    away = kc.sum_ties_away(x)
    assert not np.array_equal(pairwise, want)
    assert not np.array_equal(once, want)
    assert not np.array_equal(away, want)
    # the walk itself: 2^24 + 1 + 1 stays at 2^24 under ties-to-even and reaches 2^24 + 4 under ties-away; no tie, no difference
    hand = np.array([[2.0 ** 24], [1.0], [1.0]], np.float32)
    assert np.add.accumulate(hand, axis=0, dtype=np.float32)[-1] == 2.0 ** 24 and kc.sum_ties_away(hand) == 2.0 ** 24 + 4
    ints = np.random.RandomState(0).randint(0, 100, (500, 3)).astype(np.float32)
    assert np.array_equal(kc.sum_ties_away(ints), ints.sum(0))


def test_fast_and_generic_widths_are_what_the_entry_dispatches_on():
    assert [c.data()["C"] for c in kc.WIDTH_CASES] == list(kc.FAST_WIDTHS) and all(kc.is_fast(c) for c in kc.WIDTH_CASES + kc.MFMA_CASES)
    assert [(c.data()["C"] + 63) // 64 for c in kc.GENERIC_CASES] == [1, 2, 3, 4, 4] and not any(kc.is_fast(c) for c in kc.GENERIC_CASES)
    assert sorted({(c.data()["kmax"] + 15) // 16 for c in kc.MFMA_CASES}) == [1, 2, 3, 4]
    groups = lambda c, g: ((c + g - 1) // g, c % g)
    assert {groups(c, 28)[0] for c in kc.FAST_WIDTHS} == {1, 2, 3, 4, 5} and {groups(c, 20)[0] for c in kc.FAST_WIDTHS} >= {1, 2, 3, 5, 7}
    assert any(groups(c, 28)[1] for c in kc.FAST_WIDTHS) and any(groups(c, 20)[1] for c in kc.FAST_WIDTHS)


def test_stitch_cases_tail_the_last_cluster_of_a_partial_block():
    for case, n_clusters in zip(kc.STITCH_CASES, (7, 9)):
        d = case.data()
        _, _, cnt, _ = case.reference()
        assert cnt.size == n_clusters == d["kmax"] * len(d["seg_k"])
        assert cnt.reshape(-1)[-1] > HEAD and n_clusters % 8 != 0


def test_assignment_edge_cases():
    for case, n_seg in zip(kc.ASSIGN_CASES[:3], (128, 129, 180)):
        d = case.data()
        lens = np.diff(d["offs"])
        assert len(lens) == n_seg and lens.min() == 1 and lens.max() == 300 and (d["seg_k"][1:-1] == 0).sum() >= 3
        assert (d["seg_k"] <= lens).all()
    dup = kc.ASSIGN_CASES[3]
    d = dup.data()
    cen, lab, cnt, _ = dup.reference()
    first, rest = kc.DUP_SLOTS[0], list(kc.DUP_SLOTS[1:])
    assert cnt[0, first] == 34 and not cnt[0, rest].any() and not np.isin(lab, rest).any()
    assert np.array_equal(cen[0, rest], d["pool"][d["init"][0, rest]])              # an empty cluster keeps its centroid
    assert np.array_equal(cen[0, first], cen[0, rest[0]]), "the duplicated code words must stay equal for the tie to be a tie"
    assert all((np.array(t) == first).sum() == 34 and not np.isin(t, rest).any() for t in dup.reference(trace=True)[3][0])
    oor = kc.ASSIGN_CASES[4].data()
    assert oor["init"].min() < 0 and oor["init"].max() >= 500
    assert np.array_equal(kc.clamp_init(oor["init"][0], 500)[[0, 5, 15]], [0, 499, 499])


def test_proxy_reference_against_the_oracles_build_adaptive_proxies():
    from oracle import matching as om
    rng = np.random.RandomState(3)
    n, c, n_obj = 400, 12, 3
    pool = kc.relu_gauss(rng, n, c)
    ids = rng.randint(-1, n_obj, n)                                       # -1: unlabelled, not kept
    lab = (ids[:, None] == np.arange(n_obj)).astype(np.float32)
    keep = lab.sum(1) > 0.9
    rows = [rng.permutation(int((ids == o).sum()))[:5] for o in range(n_obj)]
    prox = om.build_adaptive_proxies(torch.from_numpy(pool[keep]), torch.from_numpy(lab[keep]), 5, init_rows=rows)
    prep = kc.label_prep_reference(lab)
    d = dict(pool=pool, fg_rows=prep["fg_rows"], offs=prep["obj_offsets"], seg_k=kc.plan_reference(prep["counts"][:n_obj], 5),
             labels=np.concatenate([p["labels"] for p in prox]), centroids=np.stack([p["centroid"].numpy() for p in prox]), kmax=5, C=c)
    got, cnt, sq, bound = kc.proxy_reference(d)
    for s, p in enumerate(prox):
        assert np.array_equal(got[s, 0], p["centroid"].numpy()) and np.array_equal(cnt[s], p["counts"])
        live = np.nonzero(p["counts"] > 0)[0]
        np.testing.assert_allclose(got[s, 1, live], p["centroid_avg"].numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(sq[s, 1, live], p["centroid_avg"].double().pow(2).sum(1).numpy(), rtol=1e-5)


def test_proxy_case_is_what_it_says():
    d = kc.proxy_case(100)
    _, cnt, sq, _ = kc.proxy_reference(d)
    assert cnt[0, 0] > HEAD and cnt[0, 1] == 0 and cnt[0, 2] > 0 and d["seg_k"].tolist() == [3, 2] and d["kmax"] == 4
    assert np.isinf(sq[0, 1, 1]) and np.isinf(sq[:, :, 3]).all() and np.isinf(sq[1, :, 2]).all() and np.isfinite(sq[0, 0, :3]).all()
    assert np.isinf(sq[0, 1, 0]) and np.isfinite(sq[0, 1, 2])    # the 1e31 column: its square overflows
    beg = d["offs"][1]
    members = d["pool"][d["fg_rows"][np.nonzero(d["labels"][:beg] == 0)[0]]]
    assert (np.abs(members[:, 7]) > 2.0 ** 101).all()
    assert (d["fg_rows"][:100] != d["obj_rows"][:100]).any() and (d["fg_rows"][:900] != d["obj_rows"][beg:beg + 900]).all()
    assert len(d["fg_rows"]) >= np.diff(d["offs"]).max() and d["fg_rows"].max() < len(d["pool"])
    members = d["pool"][d["fg_rows"][np.nonzero(d["labels"][:beg] == 0)[0]]]
    rep = kc.classify(members[:, :9], [np.zeros(len(members), np.int32)], 1)
    for claim in kc.ALL_TAIL_CLAIMS:
        assert rep[claim] >= 1, claim


@pytest.mark.parametrize("n_obj", kc.LABEL_OBJ)
def test_label_cases_hold_every_kind_of_row_and_exact_sums(n_obj):
    lab, kinds = kc.label_case(257, n_obj)
    assert set(kinds.tolist()) == set(range(len(kc.LABEL_KINDS)))
    s64 = lab.astype(np.float64).sum(1)
    fwd = np.add.accumulate(lab, axis=1, dtype=np.float32)[:, -1]
    bwd = np.add.accumulate(lab[:, ::-1], axis=1, dtype=np.float32)[:, -1]
    assert np.array_equal(fwd.astype(np.float64), s64) and np.array_equal(bwd, fwd), "a row sum depends on the order"
    assert np.array_equal(torch.from_numpy(lab).sum(1).numpy(), fwd)
    ref = kc.label_prep_reference(lab)
    kept = (ref["right_bits"] & np.uint32(kc.KEPT_BIT)) != 0
    right = ref["right_bits"] & np.uint32(kc.KEPT_BIT - 1)
    kind = lambda name: kinds == kc.LABEL_KINDS.index(name)
    assert not kept[kind("at_0.9")].any() and not right[kind("at_0.9")].any()          # float32(0.9) > 0.9 is false in float32
    assert kept[kind("above_0.9")].all() and (right[kind("above_0.9")] != 0).all()
    w = ref["wrong_bits"]
    assert (w[kind("at_0.1")] != 2 ** n_obj - 1).all() and (w[kind("below_0.1")] == 2 ** n_obj - 1).all()
    if n_obj >= 2:
        assert (right[kind("right_not_kept")] != 0).all() and not kept[kind("right_not_kept")].any()
        assert kept[kind("kept_right_for_none")].all() and not right[kind("kept_right_for_none")].any()
        assert all(bin(v).count("1") == 2 for v in right[kind("multi_hot")])
        absent = set(ref["fg_rows"].tolist()) & set(np.nonzero(kind("right_not_kept"))[0].tolist())
        assert not absent
    if n_obj >= 3:
        assert ref["counts"][n_obj - 1] == 0 and ref["counts"][:n_obj - 1].any()
    # the oracle's formulation (build_adaptive_proxies): object lists are positions in the kept-compacted arrays
    t = torch.from_numpy(lab)
    keep = t.sum(1) > 0.9
    for o in range(n_obj):
        idx = torch.nonzero((t[keep] > 0.9)[:, o]).squeeze(1).numpy()
        assert np.array_equal(ref["obj_rows"][ref["obj_offsets"][o]:ref["obj_offsets"][o + 1]], ref["fg_rows"][idx])


def test_nothing_kept_label_case():
    lab, _ = kc.label_case(300, 4, nothing_kept=True)
    ref = kc.label_prep_reference(lab)
    assert not ref["counts"].any() and not ref["obj_offsets"].any() and (ref["right_bits"] != 0).any()


def test_plan_and_replicate_references():
    counts = np.array([40, 0, 7, 90, 3], np.int32)
    for cluster_num, want in ((0, [0, 0, 0, 0, 0]), (1, [1, 0, 0, 0, 0]), (64, [40, 0, 0, 0, 0])):
        k, out = cluster_num, []
        for c in counts:                                                  # AEM:268, the loop variable is overwritten
            k = min(k, int(c))
            out.append(k)
        assert kc.plan_reference(counts, cluster_num).tolist() == out == want
    assert kc.plan_reference(np.array([40, 9, 7, 90], np.int32), 16).tolist() == [16, 9, 7, 7]
    offs = np.array([0, 3, 3, 10], np.int32)
    rows = np.arange(100, 110, dtype=np.int32)
    r, o, k = kc.replicate_reference(rows, offs, [2, 0, 2], 3)
    assert o.tolist() == [0, 3, 3, 10, 13, 13, 20, 23, 23, 30] and k.tolist() == [2, 0, 2] * 3 and np.array_equal(r[20:], rows)
    r, o, k = kc.replicate_levels_reference(rows, offs, 4, [8, 16, 32])
    assert k.tolist() == [3, 0, 0] * 4 and len(r) == 40 and o[-1] == 40
    r, o, k = kc.replicate_levels_reference(rows, np.array([0, 3, 10], np.int32), 2, [2, 64])
    assert k.tolist() == [2, 2, 3, 3]


# ------------------------------------------------------------------------------------------ assignment: ties, rounding order, replica plans
def lloyd_walk(case, s):
    """Segment s of a case along the oracle's own trajectory: per iteration (dot, |x|^2, |c|^2, code book, labels), the operands from
    oracle.kmeans.vq_parts and the labels held to the oracle's trace, so what a variant rule is compared with IS the oracle."""
    from oracle import kmeans as okm
    d = case.data()
    k, beg, end = int(d["seg_k"][s]), int(d["offs"][s]), int(d["offs"][s + 1])
    x = d["pool"][d["rows"][beg:end]]
    code = x[kc.clamp_init(d["init"][s, :k], end - beg)]
    trace = case.reference(trace=True)[3][s]
    for it in range(d["iters"]):
        dot, xs, cs = okm.vq_parts(x, code)
        lab = np.argmin(kc.distances(dot, xs, cs), 1).astype(np.int32)
        assert np.array_equal(lab, trace[it]), "the restated distance is not the oracle's"
        yield x, dot, xs, cs, code, lab
        code, _ = okm.update_means(x, lab, code)


def test_vq_parts_are_the_operands_of_vq():
    from oracle import kmeans as okm
    rng = np.random.RandomState(5)
    x, code = kc.relu_gauss(rng, 300, 100), kc.relu_gauss(rng, 40, 100)
    lab, low = okm.vq(x, code)
    dist = kc.distances(*okm.vq_parts(x, code))
    assert dist.dtype == np.float32 and np.array_equal(np.argmin(dist, 1), lab) and np.array_equal(dist.min(1), low)
    new, cnt = okm.update_means(x, lab, code)
    want = okm.kmeans2_matrix(x, code, 1)
    assert np.array_equal(new, want[0]) and np.array_equal(cnt, want[2])


def test_slot_layout_of_the_planted_pairs():
    """What the pairs are chosen for, from slot = kt * 16 + g * 4 + r alone."""
    g = lambda slot: kc.slot_lane(slot)[1]
    kt = lambda slot: kc.slot_lane(slot)[0]
    p16, p64 = kc.TIE_PAIRS[16], kc.TIE_PAIRS[64]
    assert [g(a) ^ g(b) for a, b in p16] == [0, 1, 2, 3, 2] and [(g(a), g(b)) for a, b in p16[3:]] == [(1, 2), (1, 3)]
    assert all(a < b < k for k in (16, 64) for a, b in kc.TIE_PAIRS[k])
    inverted = {(g(a), g(b)) for a, b in p64 if kt(a) < kt(b) and g(a) > g(b)}
    assert inverted == {(hi, lo) for hi in range(4) for lo in range(hi)}, "every pair of lane groups, the lower index in the higher group"
    assert {(g(a), g(b)) for a, b in p64 if g(a) < g(b)} == {(1, 2), (1, 3)}
    assert {(kt(a), kt(b)) for a, b in p64} == {(0, 1), (0, 2), (1, 2), (1, 3)}
    assert kc.REP_TIE_PAIRS == ((5, 18), (9, 16), (13, 17), (14, 22), (31, 32), (9, 20), (13, 24))


def _sensitive(a, b):
    """Which wrong rules move the tie of slots a < b off a, from the lane layout: `<=` in the lane scan needs both in one lane; a merge that
    prefers the higher index needs two lanes; a merge without the `d2 == low` clause leaves the value of the lower lane group in lane group 0
    (g0 keeps its own over g1's, g2 over g3's, then g0's over g2's), which is wrong when b sits in a lower lane group than a."""
    ga, gb = kc.slot_lane(a)[1], kc.slot_lane(b)[1]
    return {"highest": True, "le_in_lane": ga == gb, "merge_highest": ga != gb, "merge_keep": gb < ga}


TIE_RULES = {"highest": ("<=", "highest"), "le_in_lane": ("<=", "lowest"), "merge_highest": ("<", "highest"), "merge_keep": ("<", "keep")}
TIE_CASES = kc.TIE_PAIR_CASES + [c for c in REP_CASES if c.name == "rep_tie_pairs"]


@pytest.mark.parametrize("case", TIE_CASES, ids=_ids(TIE_CASES))
def test_tie_pairs_are_decided_by_the_tie_rule(case):
    """Every (replica,) segment: the lower slot of the planted pair takes all copies in every iteration, the higher one stays empty and
    keeps its initial code word bit for bit, the two code words stay equal.  The lane restatement with the kernel's own rule is scipy's
    first minimum; with ties to the highest index it moves a label in every segment and every iteration, and each single wrong rule does so
    exactly in the segments whose pair it can see (_sensitive) -- at one tile of clusters the `d2 == low` clause of the merge decides nothing,
    lane group order being index order there, so "merge_keep" is told apart at K > 16 only."""
    d = case.data()
    cen, lab, cnt, traces = case.reference(trace=True)
    seen = {rule: 0 for rule in TIE_RULES}
    assert len(d["pairs"]) == len(d["seg_k"])
    for s, (a, b) in enumerate(d["pairs"]):
        beg, end = d["offs"][s], d["offs"][s + 1]
        x = d["pool"][d["rows"][beg:end]]
        first = x[d["init"][s]]
        assert np.array_equal(first[a], first[b]) and d["init"][s, a] != d["init"][s, b]
        assert (first == first[a]).all(1).sum() == 2, "a third copy among the initial code words"
        assert cnt[s, a] == kc.TIE_COPIES and cnt[s, b] == 0
        assert np.array_equal(cen[s, b], first[b]) and np.array_equal(cen[s, a], first[a])
        assert all(((t == a).sum() == kc.TIE_COPIES) and not (t == b).any() for t in traces[s])
        want = _sensitive(a, b)
        for x_, dot, xs, cs, code, oracle_lab in lloyd_walk(case, s):
            dist = kc.distances(dot, xs, cs)
            assert np.array_equal(kc.lane_argmin(dist), oracle_lab)
            assert np.array_equal(kc.lane_argmin(dist, "<=", "highest"), d["kmax"] - 1 - np.argmin(dist[:, ::-1], 1))
            for rule, (in_lane, merge) in TIE_RULES.items():
                moved = kc.lane_argmin(dist, in_lane, merge) != oracle_lab
                assert moved.any() == want[rule], f"segment {s}, pair {(a, b)}, {rule}"
                assert not moved.any() or (oracle_lab[moved] == a).all()
                seen[rule] += int(moved.any())
    assert seen["highest"] >= len(d["pairs"]) * d["iters"] and seen["merge_highest"] > 0
    assert (seen["merge_keep"] > 0) == (d["kmax"] > 16) and (seen["le_in_lane"] > 0) == (d["kmax"] == 16)


def _tie_classes(dist):
    """Rows whose minimum is shared by several slots, counted by where the lowest slot a and another tied slot b sit."""
    n = dict(rows=0, same_lane=0, xor16=0, xor32=0, two_step=0, later_tile_lower_group=0)
    for row in dist:
        tied = np.nonzero(row == row.min())[0]
        if len(tied) < 2:
            continue
        n["rows"] += 1
        (ta, ga, _), a = kc.slot_lane(tied[0]), tied[0]
        for b in tied[1:]:
            tb, gb, _ = kc.slot_lane(b)
            n[("same_lane", "xor16", "xor32", "two_step")[ga ^ gb]] += 1
            n["later_tile_lower_group"] += int(tb > ta and gb < ga)
    return n


@pytest.mark.parametrize("case", kc.LATTICE_CASES, ids=_ids(kc.LATTICE_CASES))
def test_lattice_ties_fall_into_every_class(case):
    """Distances in int64 from the integer rows: equal to the float32 ones (so every float32 tie is a true tie), and the tied minima of each
    case hold every class of the lane layout; the rule variants each miss the oracle.  The one-row segment ties all 33 slots."""
    d = case.data()
    assert d["iters"] == 1 and d["seg_k"].tolist() == [kc.LATTICE_K] * 5 and np.diff(d["offs"]).tolist() == list(kc.LATTICE_LENS)
    assert np.isin(d["pool"], (0.0, 1.0, 2.0)).all()
    total = None
    missed = {rule: 0 for rule in TIE_RULES}
    for s in range(len(d["seg_k"])):
        (x, dot, xs, cs, code, lab), = lloyd_walk(case, s)
        xi, ci = x.astype(np.int64), code.astype(np.int64)
        exact = ((xi[:, None, :] - ci[None, :, :]) ** 2).sum(-1)
        dist = kc.distances(dot, xs, cs)
        assert np.array_equal(dist.astype(np.int64), exact) and np.array_equal(dist, exact.astype(np.float32))
        assert np.array_equal(kc.lane_argmin(dist), lab)
        rep = _tie_classes(exact)
        total = rep if total is None else {key: total[key] + v for key, v in rep.items()}
        for rule, (in_lane, merge) in TIE_RULES.items():
            missed[rule] += int((kc.lane_argmin(dist, in_lane, merge) != lab).sum())
        if s == 0:
            assert (exact == 0).all() and lab.tolist() == [0]
        if len(x) >= kc.LATTICE_K:
            assert len(np.unique(code, axis=0)) == kc.LATTICE_K, "ties between DISTINCT code words"
    assert all(v >= 1 for v in total.values()), total
    assert total["rows"] >= 100 and all(v >= 1 for v in missed.values()), (total, missed)


@pytest.mark.parametrize("case", kc.NEAR_TIE_CASES, ids=_ids(kc.NEAR_TIE_CASES))
def test_near_tie_rows_pin_the_order_of_the_distance_expression(case):
    """In every iteration some row's label differs from (a) the float64 argmin of |x - c|^2, (b) the argmin of -2 dot + (|x|^2 + |c|^2) and
    (c) `<=` (the last minimum) -- each from the SAME float32 operands (dot the oracle's own fmaf chain, out of aoc_oracle.c; every further step
    one numpy float32 operation, rounded once), so only the named change moves the label."""
    d = case.data()
    x = d["pool"]
    assert 9 * d["C"] < float((x.astype(np.float64) ** 2).sum(1).min()) and np.abs(x - x.mean(0)).max() < 6e-3
    for it, (x, dot, xs, cs, code, lab) in enumerate(lloyd_walk(case, 0)):
        x64, c64 = x.astype(np.float64), code.astype(np.float64)
        exact = ((x64[:, None, :] - c64[None, :, :]) ** 2).sum(-1)
        regrouped = np.float32(-2.0) * dot + (xs[:, None] + cs[None, :])
        assert regrouped.dtype == np.float32
        dist = kc.distances(dot, xs, cs)
        n_a, n_b = int((np.argmin(exact, 1) != lab).sum()), int((np.argmin(regrouped, 1) != lab).sum())
        n_c = int((d["kmax"] - 1 - np.argmin(dist[:, ::-1], 1) != lab).sum())
        assert n_a >= 1 and n_b >= 1 and n_c >= 1, f"iteration {it}: float64 {n_a}, regrouped {n_b}, <= {n_c} rows differ"


def _rep_case(name):
    return next(c for c in REP_CASES if c.name == name)


def test_replica_plan_constants_are_those_of_the_source():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robust-video-object-segmentation_amd", "csrc",
                            "labels_kmeans.hip")).read()
    assert re.search(r"KM_REP_LDS_BUDGET = \(size_t\)78 \* 1024;", src) and kc.KM_REP_LDS_BUDGET == 78 * 1024
    assert re.search(r"KM_ASSIGN_GRID_CAP = 512;", src) and kc.KM_ASSIGN_GRID_CAP == 512
    assert src.count("constexpr int SEG_LDS = 32;") == 1 and kc.KM_REP_SEG_LDS == 32
    assert "const int fit = (int)std::min<size_t>(16, (KM_REP_LDS_BUDGET - fixed) / per);" in src


def test_replica_plan_by_cluster_count():
    """Code books per group: 6 / 3 / 2 / 1 at kmax <= 16 / 32 / 48 / 64.  One means the single-replica kernel: kmax 49 .. 64 never takes the
    replica kernel, so its <25, 4> instantiation cannot be launched; K = 40 with two or more replicas takes <25, 3> in groups of two."""
    fit = [kc.rep_plan(k, 2)["fit"] for k in range(1, 65)]
    assert fit == [6] * 16 + [3] * 16 + [2] * 16 + [1] * 16
    for kmax in range(1, 65):
        for n_rep in (1, 2, 3, 7, 16, 40):
            p = kc.rep_plan(kmax, n_rep, 4, 3000)
            if n_rep == 1 or kmax >= 49:
                assert p["kernel"] == "km_assign_mfma_kernel" and p["kt"] == (kmax + 15) // 16
            else:
                assert p["kernel"] == "km_assign_mfma_rep_kernel" and p["kt"] <= 3 and sum(p["groups"]) == n_rep
                assert max(p["groups"]) == p["n_grp"] <= p["fit"] and min(p["groups"]) >= 1 and p["grid"] <= p["gcap"]
    for n_rep in range(2, 12):
        p = kc.rep_plan(40, n_rep, 3, 1000)
        assert (p["kernel"], p["kt"], p["n_grp"]) == ("km_assign_mfma_rep_kernel", 3, 2)
        assert p["groups"] == [2] * (n_rep // 2) + [1] * (n_rep % 2)
    assert kc.rep_plan(32, 7, 3, 1000)["groups"] == [3, 3, 1] and kc.rep_plan(16, 3, 3, 1000)["gcap"] == 768


REP_PLANS = {"rep_K40_n2": (3, [2]), "rep_K40_n3": (3, [2, 1]), "rep_K40_n5": (3, [2, 2, 1]), "rep_levels_40_8_48": (3, [2, 1]),
             "rep_K16_n13": (1, [5, 5, 3]), "rep_K24_n7": (2, [3, 3, 1]), "rep_base40": (3, [2, 1]), "rep_level_zero": (1, [4]), "rep_over_grid_cap": (3, [2] * 11),
             "rep_tie_pairs": (3, [2, 1])}


@pytest.mark.parametrize("case", REP_CASES, ids=_ids(REP_CASES))
def test_replicated_case_takes_the_plan_it_is_named_for(case):
    d = case.data()
    p = kc.rep_case_plan(case)
    n_rep, n_base = d["n_rep"], len(d["seg_k"]) // d["n_rep"]
    assert d["C"] == 100 and n_rep > 1 and len(d["seg_k"]) == n_rep * n_base and d["offs"][n_base] <= 20000
    assert (p["kernel"], p["kt"], p["groups"]) == ("km_assign_mfma_rep_kernel",) + REP_PLANS[case.name]
    # the lists are replicas: the same rows, offsets shifted by the base total, initial rows of their own
    total = int(d["offs"][n_base])
    assert np.array_equal(d["rows"], np.tile(d["rows"][:total], n_rep))
    assert np.array_equal(d["offs"][:-1].reshape(n_rep, n_base), d["offs"][:n_base][None] + total * np.arange(n_rep)[:, None])
    assert any(not np.array_equal(d["init"][:n_base], d["init"][f * n_base:(f + 1) * n_base]) for f in range(1, n_rep))
    over = len(p["items"]) > p["grid"]
    assert over == (case.name == "rep_over_grid_cap") and (n_base > kc.KM_REP_SEG_LDS) == (case.name == "rep_base40")


def test_replicated_cases_hold_the_edges_they_name():
    k = lambda name: (lambda d: d["seg_k"].reshape(d["n_rep"], -1))(_rep_case(name).data())
    assert k("rep_levels_40_8_48").tolist() == [[40] * 3, [8] * 3, [48] * 3]          # group 0 = replicas 0, 1: one and three cluster tiles
    assert k("rep_level_zero").tolist() == [[16, 16, 5, 0, 0], [0] * 5, [8, 8, 5, 0, 0], [16, 16, 5, 0, 0]]
    assert np.diff(_rep_case("rep_level_zero").data()["offs"][:6]).tolist() == [500, 300, 5, 0, 400]
    d = _rep_case("rep_base40").data()
    kk, lens = k("rep_base40"), np.diff(d["offs"][:41])
    assert lens[:4].tolist() == [1, 255, 256, 257] and (kk[:, :4] == np.minimum(40, lens[:4])).all()
    assert not kk[:, list(kc.REP_BASE40_DEAD)].any()
    for s, f in kc.REP_BASE40_ONLY.items():
        assert (kk[:, s] > 0).tolist() == [g == f for g in range(3)]
    # group 0 = replicas 0 and 1, group 1 = replica 2: a group with one dead replica (7, 9), a group that walks a segment none of its replicas
    # clusters (39 for group 0; 7 and 9 for group 1), and the list's last segment live in the last replica only
    assert max(kc.REP_BASE40_ONLY) == 39 == len(lens) - 1
    d = _rep_case("rep_over_grid_cap").data()
    assert len(d["seg_k"]) // d["n_rep"] == kc.KM_REP_SEG_LDS and d["iters"] == 2
    assert (np.diff(d["offs"][:33]) < 40).sum() == 22 and d["seg_k"].min() >= 1 and (d["seg_k"] < 40).any()


def test_over_grid_cap_workgroups_change_group_and_segment():
    p = kc.rep_case_plan(_rep_case("rep_over_grid_cap"))
    items, grid = p["items"], p["grid"]
    assert grid == kc.KM_ASSIGN_GRID_CAP == 512 < len(items) < 2 * grid
    both = [b for b in range(len(items) - grid) if items[b][0] != items[b + grid][0] and items[b][1] != items[b + grid][1]]
    same_group = [b for b in range(len(items) - grid) if items[b][0] == items[b + grid][0]]
    assert len(both) >= 1 and len(both) + len(same_group) == len(items) - grid, "a workgroup serves two groups and two segments"
    assert len({g for g, _, _ in items}) == 11
