"""What the matching entries keep between calls, how they size persistent grids, and what they assume of a workspace, on the MI355X.

1. aoc_dense_match_min_split_cached over the sequences of carried_state_cases.py: a build (reuse_plan = 0) and reusing calls in ONE
   workspace (every 32-bit word 1 before the first call), every frame a new query.  After every frame the output is array_equal to
   aoc_dense_match_min_split on the same inputs in a fresh zeroed workspace and inside the float64 bound of global_match_bounds
   (split_dense_ref; dense_ref on a take-over frame, which is also array_equal to aoc_dense_match_min), and aoc_dense_prune_stats, reset
   before the frame, says which kernels ran: counters above zero where the split kernels must have answered, zero on a take-over frame.
   Outputs go into an oversized NaN-filled buffer (check_layout), both transform values.
2. The CU budget (aoc_set_stream_cus, aoc_frame_desc.stream_cus): the same bits at every budget of carried_state_cases.BUDGETS.  The
   budget-0 run is checked against the float64 bound, every other run is array_equal to it.  No test leaves the process-wide value set.
3. Every workspace-taking entry whose header text does not ask for a cleared workspace, run in a fresh zeroed workspace, in one whose
   every 32-bit word is 1, and in one a larger case of the same entry has just used: the same bits.  (Word 1, not all-ones bytes or NaN: a
   flag, ticket, counter or min / max slot read before it is written shows as wrong bits, and an index read from an unwritten word stays
   in range.)  ops hands every such workspace out through ops._ws; the sweep replaces that allocator.  The small case of an entry is
   the smallest of its own test module's list, built by that module's input builder; the larger one comes from the same list.

test_carried_state_host.py proves without a GPU that every sequence can fail: a stale answer leaves the bound."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import carried_state_cases as cs
import global_match_bounds as gb

pytestmark = pytest.mark.gpu
RATIOS = []         # worst error / bound of the budget-0 and sequence runs against the float64 references (printed when the module ends)


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    yield aoc_amd
    if RATIOS:              # whichever tests of the module ran: the figure STATUS.md quotes
        print(f"\ncarried state: {len(RATIOS)} comparisons with a float64 reference, largest error / bound {max(RATIOS):.3f}")


def teardown_module(module):
    import aoc_amd
    assert aoc_amd._lib.lib().aoc_set_stream_cus(0) == 0, "the final aoc_set_stream_cus(0) failed"


@contextlib.contextmanager
def cu_budget(aoc, k):
    """The process-wide CU budget for the calls inside; 0 again afterwards, whatever happens."""
    aoc.ops.set_stream_cus(k)
    try:
        yield
    finally:
        aoc.ops.set_stream_cus(0)


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def nan_buffer(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


def ones_words(nbytes):
    """A device buffer of nbytes whose every 32-bit word is 1."""
    nbytes = max(int(nbytes), 16)
    return torch.ones((nbytes + 3) // 4, dtype=torch.int32, device="cuda").view(torch.uint8)[:nbytes]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------------------ 1. the reused dense plan
class DevState:
    """A pool state of carried_state_cases on the device: the label prep filled by hand, the pool, its row-major records."""

    def __init__(self, aoc, name, flag):
        self.case = cs.STATES[name].case
        inp = cs.state_inputs(name)
        p = self.prep = aoc.ops.LabelPrep()
        p.n, p.n_obj = inp["pool"].shape[0], self.case.n_obj
        p.wrong_bits, p.fg_rows, p.counts = dev(inp["wrong"]), dev(inp["fg_rows"]), dev(inp["counts"])
        p.right_bits, p.obj_rows, p.obj_offsets = dev(inp["right"]), dev(inp["obj_rows"]), dev(inp["obj_offsets"])
        self.pool, self.bias = dev(inp["pool"]), dev(inp["bias"])
        self.rec = aoc.ops.split_rows(self.pool, overflow=flag)
        self.ws_bytes = int(aoc._lib.lib().aoc_dense_match_split_workspace_bytes(self.case.m, p.n, p.n_obj))
        assert self.ws_bytes > 0


def split_call(aoc, st, q, qs, flag, transform, ws, reuse):
    """aoc_dense_match_min_split_cached (reuse = 0 / 1) or, reuse = None, aoc_dense_match_min_split, into an oversized NaN buffer.
    -> the named outputs [n_obj, m]."""
    case, p = st.case, st.prep
    ps, os_, length, named = gb.dense_layout(case)
    buf = nan_buffer(length)
    out = buf[2:]
    L = aoc._lib.lib()
    assert ws.numel() >= st.ws_bytes and qs.records.shape[0] >= case.m and st.rec.records.shape[0] >= p.n
    head = (_p(q), _p(qs.records), _p(qs.sqnorm), int(qs.tiled), case.m, case.C, _p(st.pool), _p(st.rec.records), _p(flag), p.n, _p(p.right_bits),
            _p(p.wrong_bits), _p(p.fg_rows), _p(p.obj_rows), _p(p.counts), _p(p.obj_offsets), _p(st.bias) if transform else None, p.n_obj, _p(out),
            ps, os_, int(transform), _p(ws), ws.numel())
    if reuse is None:
        aoc._lib.check(L.aoc_dense_match_min_split(*head, aoc.ops._stream()), "aoc_dense_match_min_split")
    else:
        aoc._lib.check(L.aoc_dense_match_min_split_cached(*head, int(reuse), aoc.ops._stream()), "aoc_dense_match_min_split_cached")
    torch.cuda.synchronize()
    return gb.check_layout(buf.cpu().numpy(), named, f"{case.name} transform={transform} reuse={reuse}")


def fp32_call(aoc, st, q, transform):
    ps, os_, length, named = gb.dense_layout(st.case)
    buf = nan_buffer(length)
    aoc.ops.dense_match_min(q, st.pool, st.prep, st.bias if transform else None, buf[2:], ps, os_, transform=transform)
    return gb.check_layout(buf.cpu().numpy(), named, f"{st.case.name} fp32 entry")


def run_sequence(aoc, seq, tiled, transform, check=True):
    """Every step of the sequence in one workspace.  -> the outputs per step.  check: the three comparisons of the module docstring."""
    steps = cs.SEQUENCES[seq]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    states = {name: DevState(aoc, name, flag) for name in cs.sequence_workspace_states(seq)}
    ws = ones_words(max(s.ws_bytes for s in states.values()))
    assert int(flag.item()) == 0, "the pools meet the split preconditions"
    key = "transformed" if transform else "raw"
    outs = []
    for k, step in enumerate(steps):
        st = states[step.state]
        if step.zero_flag:
            flag.zero_()
        q = dev(cs.step_query(seq, k))
        qs = aoc.ops.split_rows(q, overflow=flag, tiled=tiled)
        aoc.ops.dense_prune_stats(reset=True)
        got = split_call(aoc, st, q, qs, flag, transform, ws, step.reuse)
        stats = aoc.ops.dense_prune_stats(reset=True)
        outs.append(got)
        what = f"{seq} step {k} ({step.state}, reuse={step.reuse}, {'tiled' if tiled else 'rows'}, {key})"
        print(what, "flag", int(flag.item()), "tested", stats["tested"], "rescored", stats["rescored"])
        if step.expect == "split":
            assert int(flag.item()) == 0, what
            assert stats["tested"] > 0, f"{what}: the split kernels did not run"
        elif step.expect == "takeover":
            assert stats["tested"] == 0 and stats["rescored"] == 0, f"{what}: the split kernels ran on a take-over frame"
        if not check:
            continue
        if not (step.expect == "takeover" and step.zero_flag):
            # (the one frame a fresh call answers otherwise: the flag is zero again but the gate in the kept workspace is still set, so the
            # reusing call is the fp32 entry's, bit for bit, where a call that builds its plan runs the split kernels)
            fresh = split_call(aoc, st, q, qs, flag, transform, torch.zeros(st.ws_bytes, dtype=torch.uint8, device="cuda"), None)
            assert np.array_equal(got, fresh), f"{what}: {int((got != fresh).sum())} outputs differ from the call in a fresh zeroed workspace"
        ref = cs.step_ref(seq, k)[key]
        if step.expect == "empty":
            assert (got == 1.0).all() if transform else np.isposinf(got).all(), what
            continue
        if step.expect == "takeover":
            assert np.array_equal(got, fp32_call(aoc, st, q, transform)), f"{what}: the take-over is not bit-equal to the fp32 entry"
        gb.compare(got, ref, what, report=RATIOS)
    return outs


SEQ_PARAMS = [(s, t) for s in cs.SEQUENCES if not s.startswith("cs_budget") for t in ((False, True) if s in cs.BOTH_RECORD_ORDERS else (True,))]


@pytest.mark.parametrize("transform", [False, True], ids=["raw", "transformed"])
@pytest.mark.parametrize("seq,tiled", SEQ_PARAMS, ids=[f"{s}-{'tiled' if t else 'rows'}" for s, t in SEQ_PARAMS])
def test_reused_plan_sequence(aoc, seq, tiled, transform):
    """aoc_dense_match_min_split_cached(reuse_plan = 1) after a build, after an absent object's untouched bound column, with and without
    the seed launch, through a take-over in the middle and out of it again, on a gate that soft labels set, with nothing labelled, and
    after another pool state's plan in the same bytes."""
    outs = run_sequence(aoc, seq, tiled, transform)
    assert len(outs) == len(cs.SEQUENCES[seq])          # no frame left out
    steps = cs.SEQUENCES[seq]
    for k, step in enumerate(steps):
        if step.same:
            assert np.array_equal(outs[k], outs[k - 1]), f"{seq} step {k}: the same frame again gave other bits"


# ------------------------------------------------------------------------------------------ 2. the CU budget
@pytest.mark.parametrize("pool", list(cs.BUDGET_POOLS))
@pytest.mark.parametrize("m", cs.BUDGET_M)
def test_cu_budget_split_dense(aoc, m, pool):
    """split_nsplit (grid.y of dense_prune_kernel) from 1 to 64, with more splits than the plan has tiles and with fewer: a build and one
    reusing frame per budget, raw and transformed."""
    seq = cs.budget_case(m, pool).name
    base = {}
    for transform in (False, True):
        base[transform] = run_sequence(aoc, seq, True, transform)                   # budget 0, held to the float64 bound
    for budget in cs.BUDGETS[1:]:
        for transform in (False, True):
            with cu_budget(aoc, budget):
                outs = run_sequence(aoc, seq, True, transform, check=False)
            for k, (a, b) in enumerate(zip(outs, base[transform])):
                assert np.array_equal(a, b), f"{seq} budget {budget} step {k} transform={transform}: {int((a != b).sum())} outputs differ from budget 0"


def _corr_run(aoc, entry, inps, transform):
    """One call of a split proxy entry over len(inps) frames, each with its own inputs.  -> per frame the named outputs [n_set, m]."""
    held = [tuple(dev(i[k]) for k in ("query", "proxies", "sqnorm", "bias")) for i in inps]
    outs = [nan_buffer(inps[0]["out_len"]) for _ in inps]
    sets = (inps[0]["set_begin"], inps[0]["set_size"], inps[0]["set_off"])
    if entry == "batched":
        frames = [(*h[:3], h[3] if transform else None, o) for h, o in zip(held, outs)]
        aoc.ops.proxy_corr_min_batched(frames, *sets, transform=transform, precision="split")
    else:
        recs = [aoc.ops.split_rows(h[0], tiled=True) for h in held]
        frames = [(h[0], r, *h[1:3], h[3] if transform else None, o) for h, r, o in zip(held, recs, outs)]
        cache = aoc.ops.CorrTableCache(held[0][0].device) if entry == "cached" else None
        aoc.ops.proxy_corr_min_records(frames, *sets, transform=transform, cache=cache)
    torch.cuda.synchronize()
    return [gb.check_layout(o.cpu().numpy(), inps[0]["named"], f"{entry} frame {f} transform={transform}") for f, o in enumerate(outs)]


def _budget_sweep(aoc, entry, inps, refs, what, budgets=cs.BUDGETS):
    """Budget 0 against the float64 bound (refs per frame, or None), every other budget array_equal to budget 0."""
    for transform in (False, True):
        base = _corr_run(aoc, entry, inps, transform)
        for f, got in enumerate(base):
            if refs is not None:
                gb.compare(got, refs[f]["transformed" if transform else "raw"], f"{what} {entry} frame {f} transform={transform}", report=RATIOS)
        for budget in budgets[1:]:
            with cu_budget(aoc, budget):
                outs = _corr_run(aoc, entry, inps, transform)
            for f, (a, b) in enumerate(zip(outs, base)):
                assert np.array_equal(a, b), f"{what} {entry} budget {budget} frame {f} transform={transform}: {int((a != b).sum())} outputs differ"
    return base


@pytest.mark.parametrize("entry", ["batched", "records", "cached"])
@pytest.mark.parametrize("m,frames", cs.CORR_SHAPES, ids=[f"m{m}x{f}" for m, f in cs.CORR_SHAPES])
def test_cu_budget_proxy_corr(aoc, entry, m, frames):
    """proxy_corr_batched_kernel, proxy_corr_records_kernel and proxy_corr_records_multi_kernel striding over more item tiles than they
    have workgroups: at budget 1 the items are grid + 1, 2 grid - 1, 2 grid and about 10 grid and more."""
    case = cs.corr_case(m)
    inps = [gb.proxy_inputs(case, f) for f in range(frames)]
    refs = [cs.corr_ref(m, f, entry != "batched") for f in range(frames)]
    _budget_sweep(aoc, entry, inps, refs, f"corr m{m}x{frames}")


@pytest.mark.parametrize("name", list(cs.LEVEL_CASES))
@pytest.mark.parametrize("m,frames", [(33, 1), (97, 3)])
def test_cu_budget_cached_passes(aoc, name, m, frames):
    """aoc_proxy_corr_min_records_cached with several passes in one launch (five: 2 n_cu / n_pass workgroups per pass, a quotient that
    budget 1 and 2 take to 0, which the entry lifts to 1) and with 24 passes, more than the 16 one table array holds: the call goes out as
    two such launches whose tables replace each other in the workspace (test_carried_state_host.py derives both counts)."""
    inps = [cs.levels_inputs(name, m, f) for f in range(frames)]
    refs = [cs.levels_ref(name, m, f) for f in range(frames)]
    base = _budget_sweep(aoc, "cached", inps, refs, f"{name} m{m}x{frames}")
    plain = _corr_run(aoc, "records", inps, True)       # one launch per pass: the same bits as all passes in one
    for a, b in zip(plain, base):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("entry", ["batched", "records", "cached"])
def test_cu_budget_proxy_takeover(aoc, entry):
    """One query value of 80.0: the exact-fp32 kernel recomputes the launch, at budget 1 as at budget 0, bit-equal to the fp32 entry."""
    inp = cs.corr_takeover_inputs()
    ref = cs.corr_takeover_ref()
    for transform in (False, True):
        held = tuple(dev(inp[k]) for k in ("query", "proxies", "sqnorm", "bias"))
        out32 = nan_buffer(inp["out_len"])
        aoc.ops.proxy_corr_min(*held[:3], inp["set_begin"], inp["set_size"], inp["set_off"], held[3] if transform else None, out32, 1, transform=transform)
        want32 = gb.check_layout(out32.cpu().numpy(), inp["named"], "fp32 entry")
        for budget in (0, 1):
            with cu_budget(aoc, budget):
                got, = _corr_run(aoc, entry, [inp], transform)
            assert np.array_equal(got, want32), f"{entry} budget {budget}: the take-over is not bit-equal to the fp32 entry"
        gb.compare(got, ref["transformed" if transform else "raw"], f"corr takeover {entry} transform={transform}")


def _init_rows_dev(syn, seed, counts, levels, n_obj):
    kmax = max(levels)
    rows = np.zeros((len(levels) * n_obj, kmax), np.int32)
    for li, k in enumerate(levels):
        for o, r in enumerate(syn.kmeans_init_rows(seed + li, counts, k)):
            if r is not None:
                rows[li * n_obj + o, :len(r)] = r
    return torch.from_numpy(rows).cuda()


def _tiny_frames(aoc, stream_cus=0):
    """The `tiny` configuration of test_gpu_frame.py over a growing pool through aoc_frame_enqueue.  -> [(feat, head)] per frame."""
    syn, hot = aoc.synthetic, aoc.hotpath
    cfg = syn.CONFIGS["tiny"]
    T = 6
    clip = syn.make_clip(cfg, 21, frames=T)
    O, h, w, C = cfg.n_obj, cfg.h, cfg.w, cfg.c
    mc = hot.MatchingConfig(MEM_EVERY=3)
    emb = torch.from_numpy(clip["emb"]).cuda()
    lab = torch.from_numpy(np.stack([syn.one_hot(l, O) for l in clip["lab"]])).cuda()
    bias = torch.tensor([0.25, -0.5, 0.125, 0.0, 0.3, -0.1][:O]).cuda()
    runner = hot.FrameRunner(mc, h, w, C, O, capacity_frames=4, device=emb.device)
    pool_ids, outs = [0], []
    for t in range(1, T):
        ref_emb, ref_lab = emb[pool_ids].contiguous(), lab[pool_ids].contiguous()
        counts = [int(ref_lab[..., o].sum().item()) for o in range(O)]
        a = hot.launch_cluster_proxies(mc, ref_emb, ref_lab, _init_rows_dev(syn, 100 + t, counts, mc.cluster_levels, O))
        torch.cuda.synchronize()
        feat, head = runner.call(ref_emb, ref_lab, emb[t - 1], lab[t - 1], emb[t], bias, a.prep, a.table, a.sqn, a.prep_event, a.done_event,
                                 len(pool_ids), stream_cus=stream_cus)
        torch.cuda.synchronize()
        outs.append((feat.cpu().numpy().copy(), head.cpu().numpy().copy()))
        if t % 3 == 0:
            pool_ids.append(t)
    assert len(pool_ids) == 2
    return outs


def _same_frames(a, b, what):
    assert len(a) == len(b)
    for t, ((fa, ha), (fb, hb)) in enumerate(zip(a, b)):
        assert np.array_equal(fa, fb), f"{what}: frame {t + 1}: {int((fa != fb).sum())} proto-mask values differ"
        assert np.array_equal(ha, hb), f"{what}: frame {t + 1}: the attention head differs"


def test_cu_budget_frame_call(aoc):
    """aoc_frame_desc.stream_cus = 1, and stream_cus = 0 under a process-wide budget of 7, against the budget-0 run; then budget 0 again:
    the descriptor's scope does not leak into the next call."""
    base = _tiny_frames(aoc)
    _same_frames(_tiny_frames(aoc, stream_cus=1), base, "stream_cus = 1 in the descriptor")
    with cu_budget(aoc, 7):
        _same_frames(_tiny_frames(aoc), base, "process-wide budget 7")
    _same_frames(_tiny_frames(aoc), base, "budget 0 again")


# ------------------------------------------------------------------------------------------ 3. workspace hygiene
class WsAllocator:
    """Stands in for ops._ws while an entry runs.  zero: fresh zeroed buffers; ones: every 32-bit word 1; record: fresh buffers that are
    kept, in call order; replay: the recorded buffers of a larger case again, in call order, cut to the size the call asks for."""

    def __init__(self, ops, mode, arena=None):
        self.ops, self.mode, self.arena, self.count = ops, mode, [] if arena is None else arena, 0

    def __call__(self, nbytes, device):
        n = max(int(nbytes), 16)
        if self.mode == "ones":
            buf = ones_words(n)
        elif self.mode == "replay":
            assert self.count < len(self.arena), "the larger case took fewer workspaces than the small one"
            assert self.arena[self.count].numel() >= n, "the larger case's workspace is smaller than the small case's"
            buf = self.arena[self.count][:n]
        else:
            buf = torch.zeros(n, dtype=torch.uint8, device=device)
            if self.mode == "record":
                self.arena.append(buf)
        self.count += 1
        return buf

    def __enter__(self):
        self.saved = self.ops._ws
        self.ops._ws = self
        return self

    def __exit__(self, *exc):
        self.ops._ws = self.saved


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype
        if a.tobytes() != b.tobytes():
            diff = int((a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)).sum())
            raise AssertionError(f"{what}: output {i} differs in {diff} bytes of {a.nbytes} from the run in a fresh zeroed workspace")


def sweep(aoc, run, what):
    """run(size) -> outputs.  (a) zeroed, (b) every word 1, (c) after the larger case in the same bytes."""
    with WsAllocator(aoc.ops, "zero") as a:
        base = run("small")
    assert a.count >= 1, f"{what}: no workspace was taken through ops._ws"
    with WsAllocator(aoc.ops, "ones"):
        same_bits(run("small"), base, f"{what}, workspace words all 1")
    with WsAllocator(aoc.ops, "record") as rec:
        run("large")
    with WsAllocator(aoc.ops, "replay", rec.arena) as rep:
        same_bits(run("small"), base, f"{what}, workspace used by a larger case")
    assert rep.count == a.count


def _tiny_pool(aoc, R):
    syn = aoc.synthetic
    cfg = syn.CONFIGS["tiny"]
    clip = syn.make_clip(cfg, 4, frames=3)
    emb = torch.from_numpy(clip["emb"][:R].copy()).cuda()
    lab = torch.from_numpy(np.stack([syn.one_hot(l, cfg.n_obj) for l in clip["lab"][:R]])).cuda()
    return cfg, emb, lab


def run_label_kmeans_proxies(aoc, size):
    """aoc_label_prep, aoc_kmeans_segmented_rep and aoc_build_proxies, the three calls of a cluster frame."""
    syn, ops = aoc.synthetic, aoc.ops
    R, levels, F = (1, [16], 1) if size == "small" else (2, [8, 16, 32], 2)
    cfg, emb, lab = _tiny_pool(aoc, R)
    O, C, L, kmax = cfg.n_obj, cfg.c, len(levels), max(levels)
    pool = emb.reshape(-1, C)
    prep = ops.label_prep(lab.reshape(-1, O))
    counts = host(prep.counts)
    cnt_list = [int(c) for c in counts[:O]]
    cap = prep.obj_rows.numel()
    rows_f, off_f, k_f = ops.kmeans_replicate_levels(prep.obj_rows, prep.obj_offsets, O, F * L, levels, rows_capacity=cap)
    init = torch.cat([_init_rows_dev(syn, 40 + f, cnt_list, levels, O) for f in range(F)], dim=0)
    cen, labels, cnt = ops.kmeans_segmented(pool, rows_f, off_f, k_f, init, kmax, 20, rows_capacity=F * L * cap, n_rep=F * L)
    proxies, psq = ops.build_proxies(pool, prep.fg_rows, off_f, k_f, labels, cen)
    kk, n_rows = host(k_f), int(host(off_f)[-1])
    live = np.arange(kmax)[None, :] < kk[:, None]
    outs = [host(prep.right_bits), host(prep.wrong_bits), counts, host(prep.obj_offsets), host(prep.fg_rows)[:counts[O]],
            host(prep.obj_rows)[:int(counts[:O].sum())], host(labels)[:n_rows], np.where(live[:, :, None], host(cen), 0), np.where(live, host(cnt), 0),
            host(proxies), host(psq)]
    return outs


def run_cluster_chain(aoc, size):
    syn, hot = aoc.synthetic, aoc.hotpath
    R, levels, F = (1, None, 1) if size == "small" else (2, [8, 16, 32], 3)
    cfg, emb, lab = _tiny_pool(aoc, R)
    O = cfg.n_obj
    mc = hot.MatchingConfig(CLUSTER_LEVELS=levels)
    counts = [int(lab[..., o].sum().item()) for o in range(O)]
    inits = [_init_rows_dev(syn, 40 + f, counts, mc.cluster_levels, O) for f in range(F)]
    outs = hot.launch_cluster_proxies_batch(mc, emb, lab, inits)
    n_ad = len(mc.cluster_levels) * O * 2 * max(mc.cluster_levels)
    return [host(t) for o in outs for t in (o.table[:n_ad], o.sqn[:n_ad])]


def _dense_prep(aoc, case, inp):
    prep = aoc.ops.LabelPrep()
    prep.n, prep.n_obj = inp["pool"].shape[0], case.n_obj
    prep.wrong_bits, prep.fg_rows, prep.counts = dev(inp["wrong"]), dev(inp["fg_rows"]), dev(inp["counts"])
    prep.right_bits = prep.obj_rows = prep.obj_offsets = None
    return prep


def run_dense(aoc, size, mode):
    """aoc_dense_match_min, aoc_dense_match_min_f16 and aoc_dense_match_argmin on the smallest five-object case and on the 9 001-row one."""
    case = gb.DENSE_BY_NAME["C100_O5" if size == "small" else "rows9001"]
    inp = gb.dense_inputs(case)
    prep = _dense_prep(aoc, case, inp)
    ps, os_, length, named = gb.dense_layout(case)
    q, pool, bias = dev(inp["query"]), dev(inp["pool"]), dev(inp["bias"])
    outs = []
    for transform in (False, True):
        buf = nan_buffer(length)
        if mode == "argmin":
            arg = torch.full((length,), -7, dtype=torch.int32, device="cuda")
            aoc.ops.dense_match_argmin(q, pool, prep, bias if transform else None, buf[2:], arg[2:], ps, os_, transform=transform)
            outs.append(host(arg))
        else:
            aoc.ops.dense_match_min(q, pool, prep, bias if transform else None, buf[2:], ps, os_, transform=transform, float16=mode == "f16")
        outs.append(host(buf))
    return outs


def run_dense_grad(aoc, size):
    """aoc_label_prep, aoc_dense_match_argmin and aoc_dense_match_grad on match_grad_bounds' smallest case and on its 17 001-row one."""
    import match_grad_bounds as mgb
    ops = aoc.ops
    case = mgb.DENSE_BY_NAME["C4_m17_O3" if size == "small" else "rows17001"]
    inp = mgb.grad_case_inputs(case)
    m, n_obj = case.m, case.n_obj
    q, p, bias = dev(inp["query"]), dev(inp["pool"]), dev(inp["bias"])
    prep = ops.label_prep(dev(inp["labels"]))
    n = m * n_obj + 10
    out, arg = nan_buffer(n), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ops.dense_match_argmin(q, p, prep, bias, out[2:], arg[2:], 1, m, True)
    go = nan_buffer(n)
    go[2:2 + m * n_obj] = dev(inp["grad_out"]).reshape(-1)
    grads = ops.dense_match_backward(go[2:], out[2:], arg[2:], 1, m, q, p, n_obj)
    return [host(out), host(arg)] + [host(t) for t in grads]


def run_proxy_grad(aoc, size):
    import match_grad_bounds as mgb
    ops = aoc.ops
    name, C, m, n_obj = ("p_C4_m1_O1", 4, 1, 1) if size == "small" else ("p_C128_m257_O30", 128, 257, 30)
    inp = mgb.proxy_case_inputs(name, C, m, n_obj)
    q, p, bias = dev(inp["query"]), dev(inp["proxies"]), dev(inp["bias"])
    n = m * n_obj + 10
    out = nan_buffer(n)
    ops.proxy_corr_min(q, p, None, list(range(n_obj)), [1] * n_obj, [2 + o * m for o in range(n_obj)], bias, out, 1, True)
    go = nan_buffer(n)
    go[2:2 + m * n_obj] = dev(inp["grad_out"]).reshape(-1)
    return [host(out)] + [host(t) for t in ops.proxy_match_backward(go[2:], out[2:], 1, m, q, p)]


def _by_workspace(cases, nbytes):
    """-> (the first, i.e. smallest, case of an entry's own list; the case of that list with the largest workspace)."""
    return {"small": cases[0], "large": max(cases, key=nbytes)}


def run_masked_mean_pool(aoc, size):
    """POOL_CASES and _pool_inputs of test_gpu_stream_kernels.py: one pixel of four channels; the largest workspace below the full map."""
    import test_gpu_stream_kernels as tsk
    L = aoc._lib.lib()
    cases = [c for c in tsk.POOL_CASES if c[2] < 1000]
    C, n_obj, hw, F, pixel_major = _by_workspace(cases, lambda c: L.aoc_masked_mean_pool_workspace_bytes(c[3], c[2], c[1], c[0]))[size]
    emb, lab = tsk._pool_inputs(np.random.RandomState(C * 1000 + n_obj * 10 + F), C, n_obj, hw, F)
    sq = torch.empty(n_obj, dtype=torch.float32, device="cuda")
    pos, neg = aoc.ops.masked_mean_pool(dev(emb), dev(lab.transpose(0, 2, 1)) if pixel_major else dev(lab), 1e-5, pixel_major=pixel_major, out_pos_sqnorm=sq)
    return [host(pos), host(neg), host(sq)]


def run_cond_gate_pool(aoc, size):
    """CG_EXACT of test_gpu_decoder_kernels.py with the inputs of test_cond_gate_pool_exact_scores (tied scores at the threshold)."""
    import test_gpu_decoder_kernels as tdk
    L = aoc._lib.lib()
    cases = [c for c in tdk.CG_EXACT if c[2] < 10000]
    N, C, hw = _by_workspace(cases, lambda c: L.aoc_cond_gate_pool_workspace_bytes(*c))[size]
    rng = np.random.RandomState(N * 1000 + C + hw)
    period = max(1, hw // 3)
    z = (rng.randint(-8, 9, (N, C, period)) / 16.0).astype(np.float32)
    z[:, :, 0][z[:, :, 0] == 0] = 1 / 16.0
    z = np.tile(z, (1, 1, -(-hw // period)))[:, :, :hw]
    phi_w = (rng.choice([-1.0, 1.0], C) * 2.0 ** rng.randint(-2, 3, C)).astype(np.float32)
    outs = aoc.ops.cond_gate_pool(dev(z).view(N, C, hw, 1), dev(phi_w), dev(np.array([0.25], np.float32)), max(1, int(0.3 * hw)), want_debug=True,
                                  want_plane_mean=True)
    return [host(t) for t in outs]


def run_prehead(aoc, size):
    """PH_CASES of test_gpu_decoder_kernels.py with float64_bounds.ph_inputs: the one-pixel generic case; the full map."""
    import float64_bounds as fb
    import test_gpu_decoder_kernels as tdk
    L = aoc._lib.lib()
    picks = _by_workspace(tdk.PH_CASES, lambda c: L.aoc_prehead_workspace_bytes(c[0], c[2], c[2] // c[3], c[4]))
    picks["small"] = min(tdk.PH_CASES, key=lambda c: c[0] * c[1] * c[4])
    n_obj, n_in, n_out, n_groups, hw, C = picks[size]
    rng = np.random.RandomState(n_in * 100 + n_groups + hw)
    feat, w, b, gw, gb_ = fb.ph_inputs(rng, n_obj, n_in, n_out, hw)
    emb = rng.standard_normal((hw, C)).astype(np.float32) if C else None
    return [host(aoc.ops.prehead(dev(feat).view(n_obj, n_in, hw, 1), dev(w), dev(b), n_groups, dev(gw), dev(gb_), 1e-5, emb_hwc=dev(emb)))]


SHORTCUT_RANDOM = [(1, 5, 3, 7, 5, 7, 9, 14), (3, 6, 2, 70, 9, 6, 17, 11), (30, 4, 3, 9, 3, 4, 6, 7)]       # test_gpu_decoder_tail.py::test_shortcut_stage_random


def run_shortcut_stage(aoc, size):
    import decoder_tail_bounds as tb
    L = aoc._lib.lib()
    N, Ce, Cr, D, h, w, H, W = _by_workspace(SHORTCUT_RANDOM, lambda c: L.aoc_shortcut_stage_workspace_bytes(*c[:4]))[size]
    rng = np.random.RandomState(N * 10 + D)
    x, low, _ = tb.resize_inputs(rng, N, Ce, Cr, h, w, H, W)
    head = (0.5 * rng.standard_normal((N, D))).astype(np.float32)
    weight = (rng.standard_normal((Ce + Cr, D + Ce + Cr)) / np.sqrt(D + Ce + Cr)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(Ce + Cr)).astype(np.float32)
    return [host(t) for t in aoc.ops.shortcut_stage(dev(x), dev(low), dev(head), dev(weight), dev(bias), want_debug=True)]


def run_groupnorm(aoc, size, mode):
    """relu: GN_CASES of test_gpu_decoder_kernels.py with float64_bounds.gn_inputs (one element per group; the bottleneck's shape).
    relu_scale: GN_CASES and gate_inputs of test_gpu_decoder_memory.py.  cat: GN_CASES, the smallest map and the first / second variant of
    test_gpu_aspp.py::test_groupnorm_cat_relu_bits_and_plane_sumsq."""
    import float64_bounds as fb
    L = aoc._lib.lib()
    if mode == "relu":
        import test_gpu_decoder_kernels as tdk
        cases = [c for c in tdk.GN_CASES if c[3] < 10000]
        N, C, G, hw = {"small": min(cases, key=lambda c: c[0] * c[1] * c[3]), "large": _by_workspace(cases, lambda c: L.aoc_groupnorm_relu_workspace_bytes(c[0], c[2]))["large"]}[size]
        x, w, b, res = fb.gn_inputs(np.random.RandomState(N * 1000 + C + hw), N, C, G, hw, 0.0)
        return [host(aoc.ops.groupnorm_relu(dev(x), G, dev(w), dev(b), 1e-5, dev(res), True))]
    if mode == "relu_scale":
        import test_gpu_decoder_memory as tdm
        N, C, G, hw, D = _by_workspace(tdm.GN_CASES, lambda c: L.aoc_groupnorm_relu_workspace_bytes(c[0], c[2]))[size]
        rng = np.random.RandomState(C * 100 + hw)
        x = dev((rng.standard_normal((N, C, hw, 1)) * 2 + 0.5).astype(np.float32))
        res = dev(rng.standard_normal((N, C, hw, 1)).astype(np.float32))
        gam, bet = dev(rng.uniform(0.5, 1.5, C).astype(np.float32)), dev((0.5 * rng.standard_normal(C)).astype(np.float32))
        head, weight, gbias = tdm.gate_inputs(rng, N, C, D)
        return [host(aoc.ops.groupnorm_relu_scale(x, G, gam, bet, 1e-5, res, True, head, weight, gbias))]
    import test_gpu_aspp as tga
    hw = min(tga.HW) if size == "small" else 257
    (n_src, C_src, G), (C_tail, N, relu, _, _) = {"small": (tga.GN_CASES[0], tga.GN_VARIANTS[0]), "large": (tga.GN_CASES[1], tga.GN_VARIANTS[1])}[size]
    rng = np.random.RandomState(hw * 10 + n_src + C_tail)
    xs = [dev((rng.standard_normal((N, C_src, hw, 1)) * 2 + 0.5).astype(np.float32)) for _ in range(n_src)]
    gam = dev(rng.uniform(0.5, 1.5, (n_src, C_src)).astype(np.float32))
    bet = dev((0.5 * rng.standard_normal((n_src, C_src))).astype(np.float32))
    tail = dev(rng.standard_normal((N, C_tail)).astype(np.float32)) if C_tail else None
    y, sq = aoc.ops.groupnorm_cat_relu(xs, G, gam, bet, 1e-5, tail, relu, want_plane_sumsq=True)
    return [host(y), host(sq)]


SWEEP = {
    "label_prep+kmeans+build_proxies": run_label_kmeans_proxies,
    "cluster_chain": run_cluster_chain,
    "dense_match_min": lambda aoc, size: run_dense(aoc, size, "fp32"),
    "dense_match_min_f16": lambda aoc, size: run_dense(aoc, size, "f16"),
    "dense_match_argmin": lambda aoc, size: run_dense(aoc, size, "argmin"),
    "dense_match_grad": run_dense_grad,
    "proxy_match_grad": run_proxy_grad,
    "masked_mean_pool": run_masked_mean_pool,
    "cond_gate_pool": run_cond_gate_pool,
    "prehead": run_prehead,
    "shortcut_stage": run_shortcut_stage,
    "groupnorm_relu": lambda aoc, size: run_groupnorm(aoc, size, "relu"),
    "groupnorm_relu_scale": lambda aoc, size: run_groupnorm(aoc, size, "relu_scale"),
    "groupnorm_cat_relu": lambda aoc, size: run_groupnorm(aoc, size, "cat"),
}


@pytest.mark.parametrize("entry", list(SWEEP))
def test_workspace_content_changes_no_bit(aoc, entry):
    """The entries that take their workspace through ops._ws.  (The k-means entry already runs after a larger case in
    test_gpu_kmeans_paths.py; here it also meets a workspace of ones.)"""
    sweep(aoc, lambda size: SWEEP[entry](aoc, size), entry)


def _three_workspaces(small_bytes, large_bytes, run_large):
    """-> the three workspaces of a sweep for an entry that is handed its workspace directly; run_large(ws) uses the third one first."""
    used = torch.zeros(max(large_bytes, small_bytes), dtype=torch.uint8, device="cuda")
    run_large(used)
    return torch.zeros(small_bytes, dtype=torch.uint8, device="cuda"), ones_words(small_bytes), used


def test_workspace_content_split_dense_build(aoc):
    """aoc_dense_match_min_split (reuse_plan = 0): the 400-row, three-object state, after the 2 100-row, five-object one at m = 1 100."""
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    small, large = DevState(aoc, "cs_O3", flag), DevState(aoc, cs.budget_case(1100, "large").name, flag)

    def call(st, seq, ws, transform):
        q = dev(cs.step_query(seq, 0))
        return split_call(aoc, st, q, aoc.ops.split_rows(q, overflow=flag, tiled=True), flag, transform, ws, None)

    for transform in (False, True):
        zero, ones, used = _three_workspaces(small.ws_bytes, large.ws_bytes, lambda ws: call(large, large.case.name, ws, transform))
        base = call(small, "plain_O3", zero, transform)
        assert np.array_equal(call(small, "plain_O3", ones, transform), base), "workspace words all 1"
        assert np.array_equal(call(small, "plain_O3", used, transform), base), "workspace used by a larger case"
    assert int(flag.item()) == 0


def test_workspace_content_mask_jf_unclean(aoc):
    """aoc_mask_jf_accumulate with workspace_is_clean = 0."""
    L, ops = aoc._lib.lib(), aoc.ops

    def call(H, W, n_obj, ws):
        rng = np.random.RandomState(H * W)
        pred, gt = (dev(rng.randint(0, n_obj + 1, (H, W)).astype(np.int32)) for _ in range(2))
        accum = torch.zeros(4, dtype=torch.float64, device="cuda")
        bound = int(np.ceil(0.008 * np.hypot(H, W)))
        aoc._lib.check(L.aoc_mask_jf_accumulate(_p(pred), _p(gt), H, W, n_obj, bound, _p(ws), ws.numel(), 0, _p(accum), ops._stream()), "aoc_mask_jf_accumulate")
        return host(accum)

    nb = lambda H, W: int(L.aoc_mask_jf_workspace_bytes(H, W))
    zero, ones, used = _three_workspaces(nb(9, 11), nb(120, 160), lambda ws: call(120, 160, 4, ws))
    base = call(9, 11, 2, zero)
    assert base[3] == 1.0                       # one frame counted
    assert np.array_equal(call(9, 11, 2, ones), base), "workspace words all 1"
    assert np.array_equal(call(9, 11, 2, used), base), "workspace used by a larger case"


def test_workspace_content_gates(aoc):
    """aoc_gates_enqueue: the batch's own workspace replaced by the three."""
    hot = aoc.hotpath
    torch.manual_seed(5)
    gates = hot.CalibrationGates(hot.MatchingConfig()).cuda()

    def make(O, h, w, seed):
        g = torch.Generator().manual_seed(seed)
        acts = [torch.randn(O, c, hh, ww, generator=g).cuda() for (_, c, hh, ww, _) in gates.plan(h, w)]
        head = torch.randn(O, 400, generator=g).cuda()
        gates.forward_batched(acts, head, slot=(O, h, w))
        return acts, head, gates._batches[(O, h, w)][1]

    def call(acts, head, batch, ws):
        assert ws.numel() >= need[id(batch)]
        batch.ws = ws
        return [host(t) for t in batch(head)]

    s_acts, s_head, s_batch = make(1, 9, 11, 9)
    l_acts, l_head, l_batch = make(3, 33, 45, 10)
    need = {id(s_batch): s_batch.ws.numel(), id(l_batch): l_batch.ws.numel()}
    zero, ones, used = _three_workspaces(need[id(s_batch)], need[id(l_batch)], lambda ws: call(l_acts, l_head, l_batch, ws))
    base = call(s_acts, s_head, s_batch, zero)
    same_bits(call(s_acts, s_head, s_batch, ones), base, "gates, workspace words all 1")
    same_bits(call(s_acts, s_head, s_batch, used), base, "gates, workspace used by a larger case")
