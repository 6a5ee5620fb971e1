"""The sequences and sweeps of carried_state_cases.py checked without a GPU: each of them can fail.

From the float64 references alone (no kernel output is involved):
1. every step of every sequence meets global_match_bounds' conditions on a reference (at least a quarter of the outputs are real
   distances, the transformed ones do not saturate) and every slip of its family leaves the bound there, so compare() can run at every
   frame and no frame has to be left out;
2. a stale answer is caught: frame k answered with the reference of the frame before it leaves frame k's bound on at least STALE_SHARE of
   the outputs, and the first frame of pool state B answered from state A's rows and labels does too;
3. the named conditions hold: the absent object's count is zero, the seed rows are what the seeded sequence says, the take-over frame
   breaks a precondition and the frames after it do not;
4. the (m, budget) pairs reach the split counts and the correlation shapes reach the grid edges the sweep is there for;
5. the entries reject what they must before any launch (return codes only)."""
import ctypes

import numpy as np
import pytest

import carried_state_cases as cs
import global_match_bounds as gb

OK, INVALID_ARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
SEQS = [s for s in cs.SEQUENCES]


def _outside(a, want, tol):
    with np.errstate(invalid="ignore"):
        return (np.abs(a - want) > tol) | (np.isfinite(a) != np.isfinite(want))


# ------------------------------------------------------------------------------------------ 1. every frame can be compared
@pytest.mark.parametrize("seq", SEQS)
def test_every_step_meets_the_conditions_and_sheds_its_slips(seq):
    for k, step in enumerate(cs.SEQUENCES[seq]):
        ref = cs.step_ref(seq, k)
        inp = cs.state_inputs(step.state)
        case = cs.STATES[step.state].case
        if step.expect == "empty":
            assert case.n_fg == 0 and int(inp["counts"].sum()) == 0
            assert np.isposinf(ref["raw"][0]).all() and (ref["transformed"][0] == 1.0).all()
            continue
        has_absent = bool((inp["counts"][:case.n_obj] == 0).any())
        gb.check_conditions(f"{seq} step {k}", ref["raw"][0], ref["transformed"][0], has_absent)
        kinds = gb.split_dense_slips(case) if step.expect == "split" else gb.dense_slips(case)
        assert set(ref["raw"][2]) == set(kinds) and ref["transformed"][2]
        for key in ("raw", "transformed"):          # the reference itself is inside its bound; every slip is not
            gb.compare(ref[key][0], ref[key], f"{seq} step {k} {key}")
        if step.expect == "split":                  # the inputs are what split_plan_kernel demands
            rows = inp["fg_rows"][:case.n_fg]
            mask = (1 << case.n_obj) - 1
            r, w = inp["right"][rows].astype(np.int64), inp["wrong"][rows].astype(np.int64)
            assert ((r >> 31) & 1 == 1).all() and all(bin(v & mask).count("1") == 1 for v in r) and ((~w & mask) == (r & mask)).all()
            assert int(inp["counts"][:case.n_obj].sum()) == case.n_fg == int(inp["obj_offsets"][case.n_obj])
            q = cs.step_query(seq, k)
            assert np.abs(q).max() * 1024 <= 65000 and (q.astype(np.float64) ** 2).sum(1).max() <= 4000


# ------------------------------------------------------------------------------------------ 2. a stale answer leaves the bound
@pytest.mark.parametrize("seq", SEQS)
def test_the_frame_before_does_not_answer_a_frame(seq):
    steps = cs.SEQUENCES[seq]
    checked = 0
    for k in range(1, len(steps)):
        step = steps[k]
        if step.expect == "empty":
            continue
        j = k - 2 if step.same else k - 1        # frame k is frame k - 1 again: the stale answer that could show is the one before both
        if j < 0 or steps[j].state != step.state:
            continue
        for key in ("raw", "transformed"):
            want, tol, _ = cs.step_ref(seq, k)[key]
            stale = cs.step_ref(seq, j)[key][0]
            share = _outside(stale, want, tol).mean()
            assert share >= cs.STALE_SHARE, f"{seq} step {k} {key}: only {share:.3f} of the outputs tell it from step {j}"
        checked += 1
    if steps[0].expect != "empty":
        assert checked >= len([s for s in steps[1:] if s.state == steps[0].state]) - 1


@pytest.mark.parametrize("seq", ["A_then_B", "B_then_A"])
def test_the_state_before_does_not_answer_the_next_state(seq):
    steps = cs.SEQUENCES[seq]
    first = steps[0].state
    seen = 0
    for k, step in enumerate(steps):
        if step.state == first:
            continue
        seen += 1
        raw, tr = cs.other_state_ref(step.state, first, cs.step_query(seq, k))
        n = min(raw.shape[0], cs.STATES[step.state].case.n_obj)
        for key, stale in (("raw", raw), ("transformed", tr)):
            want, tol, _ = cs.step_ref(seq, k)[key]
            share = _outside(stale[:n], want[:n], tol[:n]).mean()
            assert share >= cs.STALE_SHARE, f"{seq} step {k} {key}: only {share:.3f} of the outputs tell state {step.state} from {first}"
    assert seen == 3
    a, b = cs.state_inputs("cs_A"), cs.state_inputs("cs_B")
    assert a["pool"].shape[0] != b["pool"].shape[0] and cs.STATES["cs_A"].case.n_obj != cs.STATES["cs_B"].case.n_obj


# ------------------------------------------------------------------------------------------ 3. the named conditions
def test_sequences_hold_what_they_are_named_for():
    assert all(len(cs.SEQUENCES[s]) == 5 and [x.reuse for x in cs.SEQUENCES[s]] == [0, 1, 1, 1, 1] for s in ("plain_O3", "plain_O16", "C36", "C4"))
    assert cs.STATES["cs_O3"].case.n_obj == 3 and cs.STATES["cs_O16"].case.n_obj == 16
    for name, absent in (("cs_absent3", 3), ("cs_absent0", 0), ("cs_absent4", 4)):
        inp = cs.state_inputs(name)
        counts = inp["counts"]
        assert counts[absent] == 0 and (np.delete(counts[:5], absent) > 0).all() and counts[5] == 400
        assert inp["obj_offsets"][absent] == inp["obj_offsets"][absent + 1]
    assert (cs.state_inputs("cs_empty")["counts"] == 0).all()
    for name in ("A_then_B", "B_then_A"):
        assert [(s.state, s.reuse) for s in cs.SEQUENCES[name]][3][1] == 0 and [s.reuse for s in cs.SEQUENCES[name]] == [0, 1, 1, 0, 1, 1]
    inp = cs.state_inputs("cs_soft")
    rows = inp["fg_rows"][:400]
    assert ((inp["right"][rows].astype(np.int64) & 31) == 0).any(), "no soft row: the plan's gate would not be set"
    assert all(s.expect == "takeover" for s in cs.SEQUENCES["soft_gate"])


@pytest.mark.parametrize("state,seeds", [("cs_seeded", True), ("cs_unseeded", False)])
def test_seeded_sequence_has_the_rows_it_names(state, seeds):
    inp = cs.state_inputs(state)
    case = cs.STATES[state].case
    n, m = inp["pool"].shape[0], case.m
    assert (n >= m) == seeds and (seeds or n == m - 1)
    right = inp["right"].astype(np.int64)
    kept, mask = (right >> 31) & 1 == 1, (1 << case.n_obj) - 1
    last = np.arange(max(0, n - m), n)
    assert (~kept[last]).any(), "no unkept row among the last m"
    lone, (pix, row) = inp["seed"]["lone"], inp["seed"]["exact"]
    mine = np.nonzero(kept & ((right >> cs.SEED_OBJECT) & 1 == 1))[0]
    assert list(mine[mine >= n - m]) == [lone] and inp["counts"][cs.SEED_OBJECT] == mine.size
    if seeds:
        assert (mine < n - m).sum() >= 10, "the seed object's other rows are all older, and there are some"
    assert row == n - m + pix and kept[row] and bin(right[row] & mask).count("1") == 1 and row in last
    seq = "seeded" if seeds else "unseeded"
    owner = int(np.log2(right[row] & mask))
    for k, step in enumerate(cs.SEQUENCES[seq]):
        q = cs.step_query(seq, k)
        assert np.array_equal(q[pix], inp["pool"][row])
        d = ((q[pix].astype(np.float64)[None, :] - inp["pool"][inp["fg_rows"][:case.n_fg]].astype(np.float64)) ** 2).sum(1)
        assert inp["fg_rows"][d.argmin()] == row and d.min() == 0.0 and np.sort(d)[1] > 1e-3
        assert abs(cs.step_ref(seq, k)["raw"][0][owner, pix]) <= cs.step_ref(seq, k)["raw"][1][owner, pix]
    steps = cs.SEQUENCES[seq]
    assert [s.same for s in steps] == [False, False, True, False] and np.array_equal(cs.step_query(seq, 2), cs.step_query(seq, 1))
    assert not np.array_equal(cs.step_query(seq, 3), cs.step_query(seq, 2))


def test_takeover_in_the_middle_is_only_the_sticky_flag_afterwards():
    steps = cs.SEQUENCES["takeover_mid"]
    assert [s.expect for s in steps] == ["split"] * 2 + ["takeover"] * 4 + ["split"] * 3
    assert [s.reuse for s in steps] == [0, 1, 1, 1, 1, 1, 0, 1, 1] and [s.zero_flag for s in steps] == [False] * 5 + [True, True] + [False] * 2
    for k, step in enumerate(steps):
        q = cs.step_query("takeover_mid", k)
        breaks = np.abs(q).max() * 1024 > 65000 and (q.astype(np.float64) ** 2).sum(1).max() > 4000
        assert breaks == (k == 2) and (not breaks or q[100, 7] == 80.0)


# ------------------------------------------------------------------------------------------ 4. what the budget sweeps reach
def test_budget_pairs_reach_the_split_counts():
    counts = {(m, b): cs.split_nsplit(m, b) for m in cs.BUDGET_M for b in cs.BUDGETS}
    got = set(counts.values())
    assert {1, 2, 64} <= got and got & set(range(3, 9)) and all(1 <= v <= 64 for v in got)
    assert [(m + 511) // 512 for m in cs.BUDGET_M] == [1, 2, 3]
    assert cs.split_nsplit(150, 0) == cs.split_nsplit(513, 0) == cs.split_nsplit(1100, 0) == 64          # the default the suite always ran
    assert cs.split_nsplit(1100, 64) == 42 and cs.split_nsplit(150, 7) == 14 and cs.split_nsplit(513, 1) == 1
    more = fewer = 0
    for m in cs.BUDGET_M:
        for pool, (n_fg, n_obj) in cs.BUDGET_POOLS.items():
            inp = cs.state_inputs(cs.budget_case(m, pool).name)
            tiles = cs.plan_tiles(inp["counts"], n_obj)
            assert (tiles <= 3) if pool == "small" else (tiles > 64)
            for b in cs.BUDGETS:
                more += counts[(m, b)] > tiles
                fewer += counts[(m, b)] < tiles
            assert (inp["pool"].shape[0] >= m) == (pool == "large")         # the large pools are seeded, the small ones are not
    assert more and fewer


def test_corr_shapes_reach_the_grid_edges_at_budget_one():
    items = sorted(cs.corr_items(m, f) for m, f in cs.CORR_SHAPES)
    assert items == [2, 3, 4, 6, 21, 63]
    for grid in (1, 2):                 # proxy_corr_batched_kernel: n_cu workgroups; the records kernels: 2 n_cu
        assert grid + 1 in items and 2 * grid in items and any(6 * grid <= i <= 11 * grid for i in items)      # 6 and 21: about ten rounds
    assert 2 * 2 - 1 in items
    for name, (levels, n_obj) in cs.LEVEL_CASES.items():
        inp = cs.levels_inputs(name, 33)
        assert len(inp["set_size"]) == (2 * len(levels) + 1) * n_obj and inp["proxies"].shape[0] == (2 * sum(levels) + 1) * n_obj + 1
        ref = cs.levels_ref(name, 33)
        for key in ("raw", "transformed"):
            gb.compare(ref[key][0], ref[key], f"{name} {key}")
    # the passes of the restated packing (corr_passes): four sets of up to 8 or two of up to 16 per tile, ceil(size / 32) tiles above that, one
    # column-wise tile for the run of single-proxy sets, five tiles per pass
    passes = {name: cs.corr_passes(*(cs.levels_inputs(name, 33)[k] for k in ("set_begin", "set_size", "set_off"))) for name in cs.LEVEL_CASES}
    assert all(1 <= t <= cs.CORR_MAX_TILES for p in passes.values() for t in p)
    assert sum(passes["levels_8_16_32_O6"]) == 12 // 4 + 12 // 2 + 12 + 1 == 22 and 2 <= len(passes["levels_8_16_32_O6"]) <= cs.CORR_MAX_PASSES
    assert sum(passes["levels_64_O24"]) == 48 * 2 + 1 == 97
    assert len(passes["levels_64_O24"]) == 24 > cs.CORR_MAX_PASSES       # two launches of all-passes-in-one: 16 passes, then 8, in one call
    assert cs.corr_passes([0, 1, 2, 3, 20], [1, 1, 1, 8, 33], [0, 10, 30, 40, 50]) == [1, 4]     # a changed output step ends the run of singles
    assert cs.corr_passes([0, 8, 16, 24, 32], [8, 8, 8, 8, 8], [0, 1, 2, 3, 4]) == [2] and cs.corr_passes([0] * 3, [64, 64, 64], [0, 1, 2]) == [4, 2]
    for m, f in cs.CORR_SHAPES:
        for records in (False, True):
            ref = cs.corr_ref(m, 0, records)
            gb.compare(ref["raw"][0], ref["raw"], f"corr m{m} raw")
    inp = cs.corr_takeover_inputs()
    assert np.abs(inp["query"]).max() == 80.0 and (inp["query"].astype(np.float64) ** 2).sum(1).max() > 4000
    ref = cs.corr_takeover_ref()
    gb.compare(ref["raw"][0], ref["raw"], "corr takeover raw")


# ------------------------------------------------------------------------------------------ 5. rejections, return codes only
def _lib():
    import aoc_amd
    return aoc_amd._lib.lib()


def test_set_stream_cus_rejects_a_negative_budget_and_recovers():
    L = _lib()
    assert L.aoc_set_stream_cus(-1) == INVALID_ARG
    assert L.aoc_set_stream_cus(0) == OK


def test_cached_split_entry_rejects_before_any_launch():
    """Without a device a launch attempt would report AOC_ERR_LAUNCH: these calls return their validation code."""
    L = _lib()
    vp = ctypes.c_void_p
    dummy = (ctypes.c_float * 64)()
    p = ctypes.cast(dummy, vp)

    def call(m=100, C=100, n=50, n_obj=3, short=0, null=None, reuse=1):
        ws = int(L.aoc_dense_match_split_workspace_bytes(ctypes.c_int64(max(m, 1)), ctypes.c_int64(n), min(n_obj, 16))) - short
        assert ws > 0
        a = [p, p, p, 1, ctypes.c_int64(m), C, p, p, p, ctypes.c_int64(n), p, p, p, p, p, p, None, n_obj, p, ctypes.c_int64(1), ctypes.c_int64(m), 0, p,
             ctypes.c_size_t(ws), reuse, None]
        if null is not None:
            a[null] = None
        return L.aoc_dense_match_min_split_cached(*a)

    for reuse in (0, 1):
        for null in (0, 1, 2, 6, 7, 8, 10, 11, 12, 13, 14, 15, 18, 22):        # every pointer but obj_bias, which may be NULL
            assert call(null=null, reuse=reuse) == INVALID_ARG, null
        assert call(m=0, reuse=reuse) == INVALID_ARG
        assert call(n_obj=17, reuse=reuse) == UNSUPPORTED
        assert call(C=104, reuse=reuse) == UNSUPPORTED
        assert call(short=1, reuse=reuse) == WORKSPACE
