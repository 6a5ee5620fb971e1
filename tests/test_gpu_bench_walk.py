"""bench.py's arrangement held to serial and oracle results at every step of its walk (helpers and the method: tests/bench_walk_cases.py).

The benchmark steps two sequences on two CU-masked streams, one aoc_frame_enqueue and one aoc_gates_enqueue call per frame, the k-means chains
enqueued ahead on side streams in batches, over a walk that jumps between pool states, so the pool shrinks as well as grows under cached split
records, pooled heads and dense plans.  test_walk_equals_serial_twin_and_oracle runs that arrangement -- the bench's own ClipWorkload / frame_step
under real hipExtStreamCreateWithCUMask streams -- for 20 steps on a 23 x 37 clip of 17 frames, once per command line of
bench_walk_cases.ARRANGEMENTS, and demands of every step and sequence

  serial twin   feat, head and the 14 gate outputs torch.equal to the same frame through hotpath.proto_mask_features with the chain inline and the
                gates module by module, on the idle default stream at budget 0 (frame call = Python orchestration, chains ahead = inline, batched
                chains = single chains, every budget and share = the same bits, cached records = uncached);
  oracle        feat within 5e-6 and head within rtol 1e-5 / atol 1e-6 of oracle.hotpath.proto_mask_features on the CPU with the frame's host rows.

That test waits for the device after every step, to compare; test_walk_enqueued_without_a_host_wait_equals_the_serial_twins enqueues every
arrangement's 20 steps as the timed region does, with no host wait in between, and compares the cloned outputs with the serial twins afterwards.
Both keep their arrangement inside one function call (_contained): the masked streams are destroyed at the module's teardown, and nothing that
was recorded on them may be freed after that, a failed test's traceback included.

test_bench_process_dumps_its_serial_twin runs the real process at the real size once (`--steps 7 --warmup 1 --dump-outputs`): the one thing that
knows main()'s wiring without restating it.  Its eighth step is t = 58 at R = 12 and t = 51 at R = 11 (first of its group: no chain ahead); every
dumped file must equal the serial twin of those two frames computed here, sampled as bench.dump_outputs samples.

tests/test_bench_walk_host.py shows without a GPU that a chain handed to the wrong frame of its group, or a stale output, cannot stay inside these
bounds; profiles/bench_walk_mutants.txt records four edits of bench.py under the default arrangement."""
import gc
import os
import time
import traceback

import numpy as np
import pytest
import torch

import bench_walk_cases as bw
from stream_order_cases import first_difference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    return aoc_amd


@pytest.fixture(scope="module")
def masked(aoc):
    """The CU-masked streams of the module (at most four: two of 224 CUs, two of 64), destroyed at teardown."""
    m = bw.MaskedStreams(torch.device("cuda", torch.cuda.current_device()))
    yield m
    m.close()


@pytest.fixture(autouse=True)
def default_budget_and_share(aoc):
    """Whatever an arrangement sets, budget 0 and the share the process started with are in force again afterwards."""
    before = aoc._lib.lib().aoc_dense_share()
    yield
    aoc.ops.set_stream_cus(0, dense_share=before)


def _same(got, want, what):
    diff = first_difference(got, want)
    assert diff is None, f"{what}: {diff}"


def _contained(body, *args):
    """body(*args) -> (its result, None), or (None, the failure as text).  A failure that pytest reported itself would keep the arrangement
    alive in its traceback until the session ends -- tensors that a masked stream was recorded on (record_stream) among them, freed only after
    the module's teardown has destroyed that stream.  So the body's failure becomes text here, where its frames end, and the test asserts on
    the text; `body` returns plain Python values only."""
    result = failure = None
    try:
        result = body(*args)
    except Exception:
        failure = traceback.format_exc()
    gc.collect()
    torch.cuda.synchronize()
    return result, failure


def _compare_with_twin(aoc, a, wl, names, at, t, R, feat, head, outs):
    t_feat, t_head, t_outs = bw.serial_twin(aoc, wl, a.gates, a.acts, t, R, a.budget)
    _same(feat, t_feat, f"{at}: feat != serial twin")
    _same(head, t_head, f"{at}: head != serial twin")
    for name, o, w in zip(names, outs, t_outs):
        _same(o, w, f"{at}: gate {name} != serial twin")


def _walk(aoc, masked, arr):
    import bench
    syn = aoc.synthetic
    aoc.ops.set_stream_cus(0)
    a = bw.arrange(aoc, bench, arr, masked)
    assert len(a.workloads) == arr.n_streams and all(wl.pool_gen > 0 for wl in a.workloads)
    if arr.reserve:
        assert a.budget == (64 if arr.reserve == "narrow" else masked.n_cu - arr.reserve) and len(masked._made) <= bw.MaskedStreams.MAX
    names = [p[0] for p in a.gates.plan(0, 0)]
    worst_feat = 0.0
    for i in range(bw.STEPS):
        results = bw.step(bench, a)
        torch.cuda.synchronize()
        for s, (wl, (t, R, feat, head, outs)) in enumerate(zip(a.workloads, results)):
            at = f"{arr.name}, step {i}, sequence {s}, t = {t}, R = {R}"
            assert t == bw.WALKS[s][i] and R == bw.pool_frames(t), f"{at}: the walk is {bw.WALKS[s][i]} here"
            assert feat.shape == (arr.n_obj, a.mc.proto_channels, bw.H, bw.W) and len(outs) == len(names) == 14
            _compare_with_twin(aoc, a, wl, names, at, t, R, feat, head, outs)
            rows = wl.init_rows[t][1]
            mine = bw.host_rows(syn, 1 + s, arr.n_obj, arr.levels, t)
            assert len(rows) == len(mine) and all(np.array_equal(x, y) for lr, lm in zip(rows, mine) for x, y in zip(lr, lm)), f"{at}: host rows"
            o_feat, o_head = bw.oracle_frame(syn, 1 + s, arr.n_obj, arr.levels, t, rows=rows)
            err = float((feat.cpu() - o_feat).abs().max())
            worst_feat = max(worst_feat, err)
            assert err <= bw.FEAT_ATOL, f"{at}: |feat - oracle| = {err:.3e} > {bw.FEAT_ATOL}"
            np.testing.assert_allclose(head.cpu().numpy(), o_head.numpy(), rtol=bw.HEAD_RTOL, atol=bw.HEAD_ATOL, err_msg=f"{at}: head != oracle")
    return worst_feat


@pytest.mark.parametrize("arr", bw.ARRANGEMENTS, ids=[a.name for a in bw.ARRANGEMENTS])
def test_walk_equals_serial_twin_and_oracle(aoc, masked, arr):
    worst_feat, failure = _contained(_walk, aoc, masked, arr)
    assert failure is None, failure
    print(f"bench walk [{arr.name}]: largest |feat - oracle| over {bw.STEPS} steps x {arr.n_streams} sequences = {worst_feat:.3e} (bound {bw.FEAT_ATOL})")


def _walk_without_host_wait(aoc, masked, arr):
    import bench
    aoc.ops.set_stream_cus(0)
    a = bw.arrange(aoc, bench, arr, masked)
    names = [p[0] for p in a.gates.plan(0, 0)]
    steps = [bw.step(bench, a) for _ in range(bw.STEPS)]
    torch.cuda.synchronize()
    for i, results in enumerate(steps):
        for s, (wl, (t, R, feat, head, outs)) in enumerate(zip(a.workloads, results)):
            at = f"no host wait, step {i}, sequence {s}, t = {t}, R = {R}"
            assert t == bw.WALKS[s][i] and R == bw.pool_frames(t), at
            _compare_with_twin(aoc, a, wl, names, at, t, R, feat, head, outs)
    return len(steps)


@pytest.mark.parametrize("arr", bw.ARRANGEMENTS, ids=[a.name for a in bw.ARRANGEMENTS])
def test_walk_enqueued_without_a_host_wait_equals_the_serial_twins(aoc, masked, arr):
    """Every arrangement as the timed region runs it: all 20 steps enqueued with no host synchronisation in between (the test above waits
    after every step to compare, so there a chain enqueued ahead has always finished before its frame starts).  Every step's outputs are cloned
    on the frame's stream and compared with the serial twins once the device is idle."""
    n, failure = _contained(_walk_without_host_wait, aoc, masked, arr)
    assert failure is None, failure
    assert n == bw.STEPS


def test_bench_process_dumps_its_serial_twin(aoc, tmp_path):
    import bench
    from test_gpu_bench import _bench
    hot, syn = aoc.hotpath, aoc.synthetic
    dump = tmp_path / "dump"
    t0 = time.perf_counter()
    line = _bench("--steps", "7", "--warmup", "1", "--dump-outputs", str(dump))
    t_bench = time.perf_counter() - t0
    assert line["steps"] == 7 and line["warmup"] == 1 and line["timed_regions"] == 1 and line["config"]["sequences_per_gpu"] == 2
    # the two cfg2 workloads of that process, constructed only (no pretouch, no step)
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = syn.CONFIGS["cfg2"]
    mc = hot.MatchingConfig(CLUSTER_NUM=cfg.k, CLUSTER_LEVELS=bench.CONFIG_LEVELS.get("cfg2"))
    torch.manual_seed(0)
    gates = hot.CalibrationGates(mc).to(dev)
    workloads = [bench.ClipWorkload(cfg, seed=1 + s, device=dev, mc=mc, phase=s, start=(s * mc.MEM_EVERY) // 2) for s in range(2)]
    acts = bench.make_activations(gates, cfg.n_obj, cfg.h, cfg.w, dev, seed=7)
    named = []
    for s, wl in enumerate(workloads):
        t = wl.order[(wl.start + 7) % len(wl.order)]                     # 1 warm-up step + 7 timed steps: the eighth
        assert (t, wl.R_of(t)) == ((58, 12), (51, 11))[s] and (t in wl.group_first) == (s == 1)
        feat, head, outs = bw.serial_twin(aoc, wl, gates, acts, t, wl.R_of(t))
        exact = bw.serial_twin(aoc, wl, gates, acts, t, wl.R_of(t), dense_precision="fp32")[0]
        err = float((feat - exact).abs().max())
        print(f"bench process, sequence {s}, t = {t}: |feat - exact-fp32 feat| = {err:.3e} (bound {bw.FEAT_ATOL})")
        assert err <= bw.FEAT_ATOL, f"sequence {s}, t = {t}: |feat - exact-fp32 feat| = {err:.3e}"
        named += [(f"seq{s}_features", feat), (f"seq{s}_attention_head", head)]
        named += [(f"seq{s}_{plan[0]}", x) for plan, x in zip(gates.plan(0, 0), outs)]
    # bench.dump_outputs' sampling, applied to the same ordered list
    keep = bench.dump_sample_sizes([x.numel() * 4 for _, x in named], bench.DUMP_LIMIT_BYTES - 128 * len(named))
    assert sorted(os.listdir(dump)) == sorted(n + ".npy" for n, _ in named)
    sampled = 0
    for (name, x), k in zip(named, keep):
        idx = bench.dump_sample_index(name, x.numel(), max(1, k // 4))
        want = x.reshape(-1)[torch.from_numpy(idx).to(dev)] if idx is not None else x
        sampled += idx is not None
        got = np.load(dump / (name + ".npy"))
        want = want.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape, f"{name}: {got.dtype} {got.shape} against {want.shape}"
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {got.size} dumped elements differ from the serial twin"
    assert 0 < sampled < len(named)             # the dump holds whole arrays and samples: both ways of writing were compared
    print(f"bench process: {t_bench:.1f} s in the subprocess, {time.perf_counter() - t0:.1f} s in all")
