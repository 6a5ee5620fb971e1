"""eval_runner.run_interleaved's lanes against the one-lane result, frame by frame and stage by stage (helpers and the method: tests/lane_cases.py).

The reference of every test is each of the five sequences run alone through run_interleaved(..., lanes=1) with the recording backend, once per
module (`ref`); every arrangement is run once and every recorded tensor of every frame -- pool size, pre-head input, pre-head output, low-resolution
logits, label map -- must be torch.equal to it, so the first difference names its sequence, frame and stage.

  a  2, 3 and 4 lanes, eval_sharded's cost-sorted order and the listed one, stagger 0, 1 and 2; the totals against one ops.MaskJF per sequence over
     the recorded label maps; two runs on backends that carry on, so that a FrameRunner is evicted and built again (max_runners = 2)
  b  three lanes (A, B, C in flight, D and E following) with a stalled stream: each lane's side stream at every chain launch; each lane's own
     stream at the start of every frame the host does not wait for; the side stream of A's lane before A's last frame, so that D's start()
     runs while A's last chain has not begun.  Every stall goes through stream_order_cases.Ctx: the calibrated spin, its 500 ms refusal,
     "still stalled" and the overtaking probe
  c  the frame's tail -- ops.prehead, the einsum read-out, interpolate, softmax, ops.confident_labels, MaskJF.add -- each once on an idle device
     and once while three other streams run real frames of sequence C back to back: equal bits
  d  test_gpu_stream_order.py's pool_grows and ground_truth_early variants as the middle lane of three

No test repeats a run to wait for a failure.  profiles/eval_lanes_mutants.txt records four edits of eval_runner.py under these tests."""
import dataclasses

import pytest
import torch

import lane_cases as lc
import stream_order_cases as soc
from stream_order_cases import Ctx

pytestmark = pytest.mark.gpu

ORDERS = {"cost_sorted": "CBADE", "as_listed": "ABCDE"}


@pytest.fixture(scope="module")
def so():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    return soc.Env(aoc_amd)


class Ref:
    """The five sequences resident on the device, each one's record and totals alone, and its J / F sums from the recorded label maps."""

    def __init__(self, so):
        er, ops = so.aoc.eval_runner, so.ops
        self.er = er
        self.specs = {s.name: s for s in lc.specs()}
        assert [s.name for s in lc.cost_sorted(lc.specs())] == list(ORDERS["cost_sorted"])
        self.data = {n: er.load_sequence(s, so.dev) for n, s in self.specs.items()}
        self.want, self.totals, self.jf = {}, {}, {}
        for n, s in self.specs.items():
            run = lc.alone(er, so.dev, s, self.data[n])
            torch.cuda.synchronize()
            assert set(run.log) == {(n, t) for t in range(1, s.frames)} and run.backends[0].history == [n] and len(run.backends[0].built) == 1
            self.want.update(run.log)
            self.totals[n] = run.totals
            jf = ops.MaskJF(so.dev)
            for t in range(1, s.frames):
                jf.add(run.log[(n, t)]["label"], self.data[n][1][t], s.n_obj)
            self.jf[n] = jf.totals()
            # one lane, one sequence: the runner's own accumulator saw the same maps in the same order
            assert (run.totals["sum_iou"], run.totals["sum_f"], run.totals["iou_count"]) == (self.jf[n]["sum_j"], self.jf[n]["sum_f"], self.jf[n]["objects"])
            assert run.totals["frames"] == s.frames - 1 and run.totals["objects"] == run.totals["iou_count"] == (s.frames - 1) * (s.n_obj - 1)
        self._not_degenerate()

    def _not_degenerate(self):
        """test_eval_lanes_host.py's conditions on the device's own one-lane record."""
        for n, s in self.specs.items():
            labels = torch.stack([self.want[(n, t)]["label"] for t in range(1, s.frames)])
            R = [self.want[(n, t)]["R"] for t in range(1, s.frames)]
            assert R[0] == 1 and sum(a != b for a, b in zip(R, R[1:])) >= 2, (n, R)
            for t, lab in enumerate(labels, start=1):
                count = [int((lab == k).sum()) for k in range(s.n_obj)]
                assert min(count) > 0 and sum(count) == lab.numel(), (n, t, count)
            assert min(int((a != b).sum()) for a, b in zip(labels, labels[1:])) > 0, n
            assert 0.0 < self.jf[n]["sum_j"] < self.jf[n]["objects"]
        A, D = (torch.stack([self.want[(n, t)]["label"] for t in range(1, 7)]) for n in "AD")
        assert int((A != D).sum()) > 50

    def items(self, names):
        return [(self.specs[n], self.data[n]) for n in names]

    def check_totals(self, got, names, n_groups):
        frames = sum(self.specs[n].frames - 1 for n in names)
        count = sum((self.specs[n].frames - 1) * (self.specs[n].n_obj - 1) for n in names)
        assert got["frames"] == frames and got["objects"] == count and got["iou_count"] == count, got
        for mine, theirs in (("sum_iou", "sum_j"), ("sum_f", "sum_f")):
            want = sum(self.jf[n][theirs] for n in names)
            bound = lc.sum_bound(frames, max(n_groups, len(names)), want)
            print(f"{mine}: lanes {got[mine]!r}, per sequence {want!r}, difference {abs(got[mine] - want):.3e}, bound {bound:.3e}")
            assert abs(got[mine] - want) <= bound, f"{mine}: {got[mine]!r} against {want!r} from the recorded label maps (bound {bound:.3e})"


@pytest.fixture(scope="module")
def ref(so):
    return Ref(so)


def _held(run, ref, names, what):
    bad = lc.first_mismatch(run.log, {k: v for k, v in ref.want.items() if k[0] in names}, what)
    assert bad is None, bad
    ref.check_totals(run.totals, names, len(run.backends))


# ------------------------------------------------------------------------------------------ a. lanes against alone
def _lanes_against_alone(so, ref, lanes, order, stagger):
    run = lc.run_lanes(ref.er, so.dev, ref.items(ORDERS[order]), lanes, stagger)
    assert len(run.backends) == lanes and sorted(n for b in run.backends for n in b.history) == list("ABCDE")
    _held(run, ref, "ABCDE", f"{lanes} lanes, {order} order, stagger {stagger}")
    if (lanes, order, stagger) == (3, "as_listed", 1):
        # the arrangement of b: the lane that finishes A takes D, and A's FrameRunner comes back from the LRU
        assert [b.history for b in run.backends] == [["A", "D"], ["B"], ["C", "E"]]
        assert len(run.backends[0].built) == 1 and len(run.backends[0].reused) == 1


@pytest.mark.parametrize("stagger", [0, 1, 2])
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("lanes", [2, 3, 4])
def test_lanes_equal_each_sequence_alone(so, ref, lanes, order, stagger):
    _, failure = lc.contained(_lanes_against_alone, so, ref, lanes, order, stagger)
    assert failure is None, failure


def _carry_on(so, ref):
    first = lc.run_lanes(ref.er, so.dev, ref.items("ABCDE"), 2, 1)
    assert [b.history for b in first.backends] == [["A", "C", "E"], ["B", "D"]]
    _held(first, ref, "ABCDE", "two lanes, first run")
    assert len(first.backends[0].built) == 3 and len(first.backends[0]._runners) == 2, "E's workspace evicted A's"
    second = lc.run_lanes(ref.er, so.dev, ref.items("ABCDE"), 2, 1, backends=first.backends)
    _held(second, ref, "ABCDE", "two lanes, second run on the first run's backends")
    assert len(second.backends[0].built) == 6, "A, C and E each evicted and built again"
    assert len(second.backends[1].built) == 2 and len(second.backends[1].reused) == 2, "B's and D's came back from the LRU"


def test_a_frame_runner_evicted_and_built_again_gives_the_same_frames(so, ref):
    """max_runners = 2: lane 0 sees three map sizes (A, C, E), so E's workspace evicts A's; a second run on the same backends builds A's again
    (evicting C's), then C's, then E's, while lane 1's two (B, D) come back from its LRU."""
    _, failure = lc.contained(_carry_on, so, ref)
    assert failure is None, failure


# ------------------------------------------------------------------------------------------ b. stalled streams, three lanes
def _lane_streams(so, n=3):
    return [so.aoc.eval_runner._cached_stream(so.dev, "lane", l) for l in range(n)]


def _stalled_three_lanes(so, ref, make_plan, sides, min_stalls):
    """A, B, C, D, E over three lanes, stagger 1: once with a plan that only measures, then with the spin."""
    items = ref.items("ABCDE")
    warm = make_plan(None)
    lc.run_lanes(ref.er, so.dev, items, 3, 1, plan=warm, sides=sides)
    torch.cuda.synchronize()
    assert warm.t > 0.0
    # a block a stalled stream still reads cannot be handed out again, so the stalled run asks for more memory than the measuring run did; a free
    # cached block per lane keeps that from becoming a hipMalloc, which waits for the device (and with it for the spin: "still stalled" would fail)
    for s in _lane_streams(so):
        with torch.cuda.stream(s):
            torch.empty(32 << 20, dtype=torch.uint8, device=so.dev)
    ctx = Ctx(so, "stalled", so.stall_cycles(warm.t))
    plan = make_plan(ctx)
    run = lc.run_lanes(ref.er, so.dev, items, 3, 1, plan=plan, sides=sides)
    ctx.finish()
    assert ctx.n_stalls >= min_stalls and plan.n_real >= min_stalls, (ctx.n_stalls, plan.n_real)
    assert [b.history for b in run.backends] == [["A", "D"], ["B"], ["C", "E"]]
    print(f"{ctx.n_stalls} stalls of {ctx.cycles / so.cycles_per_ms:.0f} ms (host interval {warm.t * 1e3:.2f} ms), {plan.n_real} settled by a lane's frame")
    return run


def _side_stalled(so, ref, lane):
    side = so.partner_of(_lane_streams(so)[lane])                # a side stream that the lane's own stream overtakes
    run = _stalled_three_lanes(so, ref, lambda ctx: lc.SideStall(lane, ctx), {lane: side}, 3)
    _held(run, ref, "ABCDE", f"three lanes, lane {lane}'s side stream late at every chain launch")


@pytest.mark.parametrize("lane", [0, 1, 2])
def test_three_lanes_with_one_lanes_side_stream_late(so, ref, lane):
    _, failure = lc.contained(_side_stalled, so, ref, lane)
    assert failure is None, failure


def _own_stalled(so, ref, lane):
    streams = _lane_streams(so)
    others = {l: so.overtakes(streams[lane], streams[l]) for l in range(3) if l != lane}
    assert any(others.values()), f"neither of the other lanes' streams runs while lane {lane}'s stream spins (shared hardware queue): a missing wait could not show"
    spare = next((s for s in so.streams if so.overtakes(streams[lane], s)), None)
    assert spare is not None, f"none of the module's streams runs while lane {lane}'s stream spins"
    run = _stalled_three_lanes(so, ref, lambda ctx: lc.OwnStall(lane, others, spare, ctx), None, 3)
    _held(run, ref, "ABCDE", f"three lanes, lane {lane}'s own stream late at the start of its frames")


@pytest.mark.parametrize("lane", [0, 1, 2])
def test_three_lanes_with_one_lanes_own_stream_late(so, ref, lane):
    _, failure = lc.contained(_own_stalled, so, ref, lane)
    assert failure is None, failure


def _next_sequence_starts_under_a_late_chain(so, ref):
    side = so.partner_of(_lane_streams(so)[0])
    run = _stalled_three_lanes(so, ref, lambda ctx: lc.LastFrameStall("A", "D", ctx), {0: side}, 1)
    assert run.backends[0].reused and not run.backends[0].built[1:], "D runs in A's FrameRunner"
    _held(run, ref, "ABCDE", "three lanes, A's last chain late while its lane starts D")


def test_the_next_sequence_starts_while_the_last_chain_has_not_begun(so, ref):
    _, failure = lc.contained(_next_sequence_starts_under_a_late_chain, so, ref)
    assert failure is None, failure


# ------------------------------------------------------------------------------------------ c. the tail under busy neighbours
TAIL = ("prehead", "readout", "interpolate", "softmax", "confident_label", "confident_confident", "confident_entropy", "jf")


def _tail_inputs(so, ref):
    """The inputs of the six operations, each the output of the one before on an idle device, from the last frame of C (the largest map)."""
    C = ref.specs["C"]
    rec = ref.want[("C", C.frames - 1)]
    pre, wv = ref.er.HotPathBackend(so.dev)._head(rec["feat"].shape[1])
    up = torch.nn.functional.interpolate(rec["logits"][None], size=(4 * C.h, 4 * C.w), mode="bilinear", align_corners=True)[0]
    probs = torch.softmax(up, dim=0)
    label = so.ops.confident_labels(probs.reshape(C.n_obj, -1), (1 << C.n_obj) - 1, None, 1.0)[0]
    inp = dict(pre=pre, wv=wv, feat=rec["feat"], y=rec["y"], logits=rec["logits"], up=up, probs=probs, label=label.view(4 * C.h, 4 * C.w),
               gt=ref.data["C"][1][C.frames - 1], spec=C)
    torch.cuda.synchronize()
    assert torch.equal(pre(inp["feat"]), rec["y"]) and torch.equal(label.view(4 * C.h, 4 * C.w), rec["label"])
    return inp


def _tail(so, inp):
    """Each operation once, on the current stream, from its fixed input."""
    C = inp["spec"]
    out = dict(prehead=inp["pre"](inp["feat"]), readout=torch.einsum("ochw,c->ohw", inp["y"], inp["wv"]),
               interpolate=torch.nn.functional.interpolate(inp["logits"][None], size=(4 * C.h, 4 * C.w), mode="bilinear", align_corners=True)[0],
               softmax=torch.softmax(inp["up"], dim=0))
    lab, conf, ent = so.ops.confident_labels(inp["probs"].reshape(C.n_obj, -1), (1 << C.n_obj) - 1, None, 1.0)
    out.update(confident_label=lab, confident_confident=conf, confident_entropy=ent)
    jf = so.ops.MaskJF(so.dev)
    jf.add(inp["label"], inp["gt"], C.n_obj)
    out["jf"] = jf.accum
    assert tuple(out) == TAIL
    return out


def _tail_beside_three_busy_streams(so, ref, inp, ctx):
    """Three backends, each on a lane's stream with a side stream of its own, have run C's first two frames; behind one gate (a spin on a stream
    of the module's) each enqueues the four frames that follow back to back -- C with MEM_EVERY 5: none of them waits for the device -- and the
    operations go to a fourth stream after the second round, so that each neighbour has frames in front of them and behind them whichever
    hardware queue the fourth stream shares.  -> (outputs, per neighbour: did its four frames' interval overlap the operations', the four times)."""
    er = ref.er
    busy = dataclasses.replace(ref.specs["C"], name="C-busy", mem_every=5)
    emb, gt = ref.data["C"]
    streams, op_stream = _lane_streams(so), er._cached_stream(so.dev, "lane", 3)
    backends = [er.HotPathBackend(so.dev, lane=l) for l in range(3)]
    for b, s in zip(backends, streams):
        with torch.cuda.stream(s):
            b.start(busy)
            b.first_frame(emb[0], gt[0])
            b.frame(emb[1])
    torch.cuda.synchronize()
    event = lambda: torch.cuda.Event(enable_timing=True)
    n_start, n_end, op_start, op_end = [event() for _ in streams], [event() for _ in streams], event(), event()
    with ctx.timed():
        if ctx.stalled:
            ctx.stall(so.partner_of(op_stream))
            ctx.probe(op_stream)
            for s in streams + [op_stream]:
                s.wait_event(ctx.events[-1])
        for s, e in zip(streams, n_start):
            e.record(s)
        for t in range(2, 6):
            for b, s in zip(backends, streams):
                with torch.cuda.stream(s):
                    b.frame(emb[t])
            if t == 3:
                with torch.cuda.stream(op_stream):
                    op_start.record(op_stream)
                    out = _tail(so, inp)
                    op_end.record(op_stream)
        for s, e in zip(streams, n_end):
            e.record(s)
        ctx.still_stalled()
    ctx.finish()
    times = [(a.elapsed_time(op_end), op_start.elapsed_time(b)) for a, b in zip(n_start, n_end)]      # ms: start -> operations' end, operations' start -> end
    return out, [x > 0.0 and y > 0.0 for x, y in times], times


def _tail_case(so, ref):
    inp = _tail_inputs(so, ref)
    op_stream = ref.er._cached_stream(so.dev, "lane", 3)
    with torch.cuda.stream(op_stream):
        idle = _tail(so, inp)
    torch.cuda.synchronize()
    with torch.cuda.stream(op_stream):
        again = _tail(so, inp)
    soc.assert_same(again, idle, "the tail twice on an idle device")
    warm = Ctx(so, "plain")
    _tail_beside_three_busy_streams(so, ref, inp, warm)
    ctx = Ctx(so, "stalled", so.stall_cycles(warm.t_enq))
    got, overlapped, times = _tail_beside_three_busy_streams(so, ref, inp, ctx)
    print(f"neighbours whose frames ran around the operations: {overlapped} (ms from a neighbour's start to the operations' end, from their start to its end: {times})")
    # which streams share a hardware queue is the runtime's choice: one neighbour running around the operations is the least that makes the run mean
    # something, and the figures of all three are printed
    assert any(overlapped), f"the operations ran while none of the three streams' frames ran: {times}"
    soc.assert_same(got, idle, "the tail beside three busy streams != the tail on an idle device")
    print(f"gate of {ctx.cycles / so.cycles_per_ms:.0f} ms over an enqueue of {warm.t_enq * 1e3:.2f} ms")


def test_the_tail_gives_the_same_bits_beside_three_busy_streams(so, ref):
    """Separates "our ordering" from "an operation whose result depends on scheduling": the stand-in tail's torch operations and the library's
    three, from fixed inputs, idle against busy."""
    _, failure = lc.contained(_tail_case, so, ref)
    assert failure is None, failure


# ------------------------------------------------------------------------------------------ d. pool growth and ground truth early, as the middle lane
def _variant_in_the_middle(so, ref, variant):
    er = ref.er
    A, gt = ref.specs["A"], ref.data["A"][1]
    kw = dict(pool_capacity=1) if variant == "pool_grows" else dict(chain_plan=[2], gt_frames={1: gt[1], 3: gt[3]})
    want = lc.alone(er, so.dev, A, ref.data["A"], **kw)
    torch.cuda.synchronize()
    if variant == "pool_grows":
        bad = lc.first_mismatch(want.log, {k: v for k, v in ref.want.items() if k[0] == "A"}, "a pool tensor that has to grow, alone")
        assert bad is None, bad
    else:
        R = [want.log[("A", t)]["R"] for t in range(1, A.frames)]
        assert R == [1, 2, 3, 4, 5, 5], f"ground truth on frames 1 and 3 joins the pool at once: the frames saw {R}"
    reference = {k: v for k, v in ref.want.items() if k[0] in "BC"}
    reference.update(want.log)
    side = so.partner_of(_lane_streams(so)[1])
    items = ref.items("BAC")
    warm = lc.SideStall(1)
    lc.run_lanes(er, so.dev, items, 3, 1, plan=warm, sides={1: side}, backend_kw={1: kw})
    torch.cuda.synchronize()
    ctx = Ctx(so, "stalled", so.stall_cycles(warm.t))
    plan = lc.SideStall(1, ctx)
    run = lc.run_lanes(er, so.dev, items, 3, 1, plan=plan, sides={1: side}, backend_kw={1: kw})
    ctx.finish()
    assert ctx.n_stalls >= 3 and [b.history for b in run.backends] == [["B"], ["A"], ["C"]]
    bad = lc.first_mismatch(run.log, reference, f"{variant} as the middle lane of three, its side stream late")
    assert bad is None, bad
    assert run.totals["frames"] == sum(ref.specs[n].frames - 1 for n in "BAC")


@pytest.mark.parametrize("variant", ["pool_grows", "ground_truth_early"])
def test_runner_variants_as_the_middle_lane_of_three(so, ref, variant):
    """test_gpu_stream_order.py::test_runner_with_a_late_side_stream's variants with a lane on either side: the resident pool starts with room for
    one frame (torch.cat replaces the tensor chains were given); two frames per chain and ground truth on frames 1 and 3 (a chain launched
    ahead is dropped and its draws are handed back)."""
    _, failure = lc.contained(_variant_in_the_middle, so, ref, variant)
    assert failure is None, failure
