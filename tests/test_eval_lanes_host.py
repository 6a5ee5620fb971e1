"""The host side of test_gpu_eval_lanes.py (helpers: tests/lane_cases.py): the five sequences are not degenerate, run_interleaved's bookkeeping
takes every sequence once, and the lanes' draw workers do not disturb one another.

The clips.  lane_cases.oracle_sequence runs the backend's whole loop on the CPU oracle, once per sequence for the module (8 s for the five).
A lanes-against-alone comparison could pass for the wrong reason on a clip whose objects vanish, whose pool never changes or whose label maps
are constant: the conditions below rule that out on the oracle's maps, and test_gpu_eval_lanes.py asserts the same conditions on the device's own
one-lane record before it compares anything with it.

The bookkeeping.  eval_runner.round_robin is the loop of run_interleaved without a device (run_interleaved itself creates HIP streams and cannot
run here); RESTATED below is the same schedule worked out independently, from the rule in the function's docstring, and the totals are the
product's own sequence_steps / HostMetric over a stub backend."""
import contextlib
import itertools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import lane_cases as lc


@pytest.fixture(scope="module")
def oracle():
    return {s.name: lc.oracle_sequence(s) for s in lc.specs()}


# ------------------------------------------------------------------------------------------ the clips
def test_the_five_sequences_take_different_paths():
    A, B, C, D, E = lc.specs()
    assert [s.name for s in (A, B, C, D, E)] == list("ABCDE")
    assert (A.h, A.w, A.n_obj, A.levels, A.mem_every, A.frames) == (24, 40, 3, (16,), 2, 7)
    assert (B.h, B.w, B.n_obj, B.levels, B.mem_every, B.frames) == (23, 37, 4, (8, 16, 32), 3, 8)
    assert (C.h, C.w, C.n_obj, C.levels, C.mem_every, C.frames) == (29, 41, 6, (8, 16, 32), 2, 6)
    assert (D.h, D.w, D.n_obj, D.levels, D.mem_every, D.frames) == (A.h, A.w, A.n_obj, A.levels, A.mem_every, A.frames) and D.seed != A.seed
    assert len({(s.h, s.w) for s in (A, B, C, E)}) == 4
    assert [s.name for s in lc.cost_sorted([A, B, C, D, E])] == ["C", "B", "A", "D", "E"]       # the order eval_sharded hands to the lanes


def test_no_sequence_is_degenerate(oracle):
    for s in lc.specs():
        o = oracle[s.name]
        gt0 = [int((o["gt"][0] == k).sum()) for k in range(s.n_obj)]
        assert min(gt0) > 0, f"{s.name}: an object has no labelled pixel in frame 0: {gt0}"
        assert len(o["R"]) == s.frames - 1 and o["R"][0] == 1
        changes = sum(a != b for a, b in zip(o["R"], o["R"][1:]))
        assert changes >= 2, f"{s.name}: the pool changes {changes} times (frames see {o['R']})"
        labels = o["labels"]
        assert labels.shape == (s.frames - 1, 4 * s.h, 4 * s.w)
        for t, lab in enumerate(labels, start=1):
            n = [int((lab == k).sum()) for k in range(s.n_obj)]
            assert min(n) > 0 and sum(n) == lab.numel(), f"{s.name}, frame {t}: an object is lost, or a label is none of the objects': {n}"
        moved = [int((a != b).sum()) for a, b in zip(labels, labels[1:])]
        assert min(moved) > 0, f"{s.name}: two consecutive label maps are equal ({moved})"


def test_no_two_sequences_have_equal_label_maps(oracle):
    for a, b in itertools.combinations(lc.specs(), 2):
        la, lb = oracle[a.name]["labels"], oracle[b.name]["labels"]
        assert la.shape != lb.shape or int((la != lb).sum()) > 50, f"{a.name} and {b.name}: the label maps (nearly) coincide"
        ga, gb = oracle[a.name]["gt"], oracle[b.name]["gt"]
        assert ga.shape != gb.shape or int((ga != gb).sum()) > 50


# ------------------------------------------------------------------------------------------ the bookkeeping
def _restated(steps, n_lanes, stagger):
    """When does which lane take which item?  Worked out lane by lane from the rule: a lane is free from pass 1 + lane x stagger on; an item of
    n steps (n calls that yield; the n + 1st says "ended") taken in pass p is advanced in the passes p .. p + n - 1, found ended in pass p + n,
    and the lane is free again in pass p + n + 1; in a pass the free lanes take the list's next items in lane order."""
    free = [1 + l * stagger for l in range(n_lanes)]
    todo, taken, p = list(range(len(steps))), [], 0
    while todo:
        p += 1
        for l in range(n_lanes):
            if todo and free[l] <= p:
                i = todo.pop(0)
                taken.append((p, l, i))
                free[l] = p + steps[i] + 1
    return taken


STEPS = {"five": [7, 8, 6, 7, 6], "sorted": [6, 8, 7, 7, 6], "two": [3, 1], "one": [4], "uneven": [1, 9, 1, 1, 2, 5, 1]}


@pytest.mark.parametrize("stagger", [0, 1, 2])
@pytest.mark.parametrize("lanes", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("case", list(STEPS))
def test_round_robin_takes_every_item_once(case, lanes, stagger):
    from aoc_amd import eval_runner as er
    steps = STEPS[case]
    n_lanes = max(1, min(lanes, len(steps)))                      # run_interleaved: never more lanes than sequences
    turns, inside = [], []

    @contextlib.contextmanager
    def lane_context(l):
        inside.append(l)
        yield
        inside.pop()

    def begin(l, i):
        assert inside == [l]
        for k in range(steps[i]):
            turns.append((l, i, k))
            yield k

    taken = er.round_robin(range(len(steps)), n_lanes, stagger, begin, lane_context)
    assert sorted(i for _, _, i in taken) == list(range(len(steps))), "every item exactly once"
    assert [i for _, _, i in taken] == list(range(len(steps))), "in the list's order"
    assert taken == _restated(steps, n_lanes, stagger)
    assert sorted(turns) == sorted((l, i, k) for _, l, i in taken for k in range(steps[i])), "every step of every item, on the lane that took it"
    for _, l, i in taken:
        assert [k for ll, ii, k in turns if ii == i] == list(range(steps[i]))
    assert all(p >= 1 + l * stagger for p, l, _ in taken), "no lane takes anything before its staggered start"
    assert taken[0][:2] == (1, 0)
    assert not inside


def test_the_lane_that_finishes_A_takes_D():
    """The arrangement of the stalled tests: A, B, C in flight on three lanes, stagger 1; A (7 steps, from pass 1) is found ended in pass 8, so
    lane 0 takes D in pass 9, while C (6 steps, from pass 3) is found ended in pass 9 and lane 2 takes E in pass 10; lane 1 keeps B until pass 10."""
    from aoc_amd import eval_runner as er
    steps = STEPS["five"]
    taken = er.round_robin(range(5), 3, 1, lambda l, i: iter(range(steps[i])), lambda l: contextlib.nullcontext())
    assert taken == [(1, 0, 0), (2, 1, 1), (3, 2, 2), (9, 0, 3), (10, 2, 4)]


class _StubBackend:
    """test_host_logic.py's stand-in for the hot path: a deterministic label map from the embedding."""

    def start(self, spec):
        self.spec = spec

    def first_frame(self, emb, gt):
        pass

    def frame(self, emb):
        lab = (emb[..., :3].sum(-1) * 40.0).long() % self.spec.n_obj
        return lab.repeat_interleave(4, 0).repeat_interleave(4, 1).to(torch.int32)


@pytest.mark.parametrize("lanes,stagger", [(1, 1), (2, 0), (3, 1), (4, 2), (5, 1)])
def test_lane_totals_equal_the_per_sequence_sums(lanes, stagger):
    from aoc_amd import eval_runner as er
    cpu = torch.device("cpu")
    specs = lc.specs()
    data = [er.load_sequence(s, cpu) for s in specs]
    alone = []
    for s, d in zip(specs, data):
        r = er.run_sequence(s, _StubBackend(), cpu, er.HostMetric(), data=d)
        assert r["frames"] == s.frames - 1 and r["iou_count"] == r["objects"] == (s.frames - 1) * (s.n_obj - 1) and r["sum_iou"] > 0
        alone.append(r)
    backends, metrics = [_StubBackend() for _ in range(lanes)], [er.HostMetric() for _ in range(lanes)]
    taken = er.round_robin(list(zip(specs, data)), lanes, stagger, lambda l, item: er.sequence_steps(item[0], backends[l], metrics[l], item[1]),
                           lambda l: contextlib.nullcontext())
    assert [item[0].name for _, _, item in taken] == list("ABCDE")
    tot = [m.totals() for m in metrics]
    assert sum(t["frames"] for t in tot) == sum(r["frames"] for r in alone)
    assert sum(t["objects"] for t in tot) == sum(r["iou_count"] for r in alone)
    want = sum(r["sum_iou"] for r in alone)
    got = sum(t["sum_j"] for t in tot)
    n = sum(r["iou_count"] for r in alone)                          # HostMetric adds one float64 per (frame, object)
    assert abs(got - want) <= lc.sum_bound(n, 5, want), (got, want)
    for l in range(lanes):                                          # and lane by lane: the lane's sequences, whichever they were
        mine = [i for i, (_, ll, _) in enumerate(taken) if ll == l]
        want_l = sum(alone[i]["sum_iou"] for i in mine)
        assert abs(tot[l]["sum_j"] - want_l) <= lc.sum_bound(n, 5, want) and tot[l]["frames"] == sum(alone[i]["frames"] for i in mine)


# ------------------------------------------------------------------------------------------ the draw workers
def test_three_draw_workers_at_once_draw_what_they_draw_one_after_another():
    """HotPathBackend hands the later batches' draws of a pool state to a worker thread of its own; with three lanes three of them run
    ops.kmeans_init_rows_draw at once (the call releases the GIL), each on its own RandomState.  Same rows, same snapshots, same final states as
    the same calls made one after another."""
    import aoc_amd
    draw = aoc_amd.ops.kmeans_init_rows_draw
    jobs = [(33, [800, 40, 70], [16], [1, 4, 2]), (88, [2400, 90, 0, 130], [8, 16, 32], [2, 3, 3]), (5, [3000, 48, 38, 49, 80, 7], [8, 16, 32], [5, 1, 4])]

    def work(job, rng):
        _, counts, levels, batches = job
        return [draw(rng, np.asarray(counts), levels, b, max(levels)) for b in batches for _ in range(20)]

    serial_rngs = [np.random.RandomState(j[0]) for j in jobs]
    serial = [work(j, r) for j, r in zip(jobs, serial_rngs)]
    rngs = [np.random.RandomState(j[0]) for j in jobs]
    workers = [ThreadPoolExecutor(max_workers=1) for _ in jobs]     # one executor per lane, as the backends keep them
    try:
        futures = [w.submit(work, j, r) for w, j, r in zip(workers, jobs, rngs)]
        together = [f.result(timeout=120) for f in futures]
    finally:
        for w in workers:
            w.shutdown()
    for j, a, b, ra, rb in zip(jobs, serial, together, serial_rngs, rngs):
        assert len(a) == len(b) == 60
        for (rows_a, states_a), (rows_b, states_b) in zip(a, b):
            assert np.array_equal(rows_a, rows_b), j
            assert all(np.array_equal(x[1], y[1]) and x[2:] == y[2:] for x, y in zip(states_a, states_b)), j
        sa, sb = ra.get_state(), rb.get_state()
        assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
        assert ra.randint(0, 1 << 30) == rb.randint(0, 1 << 30)
