"""CPU checks of tests/kmeans_cases.py: the references are right, and every case reaches the edge of csrc/labels_kmeans.hip it names.
The claims are conditions, not measurements: a case that stops meeting one fails here, before the GPU file relies on it."""
import warnings

import numpy as np
import pytest
import torch

import kmeans_cases as kc
from kmeans_cases import HEAD, KMEANS_CASES


def _ids(cases):
    return [c.name for c in cases]


K1_CASES = [c for c in KMEANS_CASES if c.name.startswith(("tail_", "fast_C", "mfma_K1_"))]


@pytest.mark.parametrize("case", K1_CASES, ids=_ids(K1_CASES))
def test_ordered_sum_is_the_oracles_k1_code_book(case):
    d = case.data()
    cen, lab, cnt, _ = case.reference()
    assert int(d["seg_k"][0]) == 1 and cnt[0, 0] == len(d["pool"]) and not lab.any()
    assert np.array_equal(cen[0, 0], kc.ordered_mean(d["pool"]))


@pytest.mark.parametrize("case", KMEANS_CASES, ids=_ids(KMEANS_CASES))
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
