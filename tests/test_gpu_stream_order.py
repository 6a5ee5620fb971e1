"""The ordering between the hot path's streams, one stalled dependency edge per test (the method: tests/stream_order_cases.py).

  a  main -> side stream       the pool's newest frame is written late; the k-means chain joins through wait_stream(main) / a caller's event
  b  chain -> proto_mask_features   (prep_event, done_event; with the cached pooled heads the main stream writes the k = 1 rows of the table)
  c  chain -> FrameRunner           (aoc_frame_desc.prep_ready / proxies_ready), three frames of a growing pool
  d  dense_stream              first tests of the option: equal bits with the plain call; main late (the fork waits), dense late (the join waits)
  e  defer_correlation + launch_correlations   first tests of the path: equal bits with the plain call; a frame's `ready` late; the batch late
  f  IncrementalProxyBank.append on a late side stream, appending and re-writing a slot
  g  buffer lifetimes          every tensor handed to record_stream: dropped while the using stream is late, its block asked for again at once
  h  eval_runner.HotPathBackend with a late side stream: label maps against a backend whose side stream IS the main stream

Every comparison is torch.equal against the same kernels run with a device synchronisation after every step.  The prep_event / prep_ready waits
are covered by b and c on the library as it is; nobody should run them REMOVED on a GPU: the arrays behind them are row indices allocated inside
the library's wrappers, and an early read of an unwritten list can address outside the pool."""
import pytest
import torch

import lane_cases
import stream_order_cases as soc
from stream_order_cases import H, W, C, Ctx, assert_same, snapshot, stalled_equals_serial

pytestmark = pytest.mark.gpu

REAL, OTHER = 33, 71             # synthetic.make_clip seeds: the inputs of the answer, and the other frame's


@pytest.fixture(scope="module")
def so():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()
    return soc.Env(aoc_amd)


def _pool(inp, ids):
    return inp.emb[ids].contiguous(), inp.lab[ids].contiguous()


def _ahead_on_this_stream(so, mc, ref_emb, ref_lab, seed):
    """The k-means chain of a pool on the CURRENT stream (no side stream: not the edge under test)."""
    return so.hot.launch_cluster_proxies(mc, ref_emb, ref_lab, so.init_rows(mc, [ref_lab], seed)[0])


# ------------------------------------------------------------------------------------------ a. main into the side stream
@pytest.mark.parametrize("join", ["wait_stream", "event_and_callers_prep"])
def test_chain_waits_for_the_pool_written_late_on_main(so, join):
    """The copy that writes the newest pool frame and its labels into the resident pool is behind a spin on main.  wait_event=None makes the
    side stream wait for main as it stands at the launch; the other variant hands over an event recorded after the write and the label prep
    main computed (eval_runner._launch_ahead).  The pool slot and the caller's prep hold the other frame's data first."""
    main, side = so.roles(2, [(0, 1)])
    mc = so.hot.MatchingConfig()
    real, other = so.clip(REAL), so.clip(OTHER)
    O = real.lab.shape[-1]
    labellings = [torch.stack([a.lab[0], b.lab[2]]) for a in (real, other) for b in (real, other)]
    rows = so.init_rows(mc, labellings, 11)[0]

    def run(ctx, inp, oth):
        with torch.cuda.stream(main):
            pool_emb, pool_lab = torch.stack([inp.emb[0], oth.emb[2]]), torch.stack([inp.lab[0], oth.lab[2]])
            prep = so.ops.label_prep(pool_lab.reshape(-1, O)) if join != "wait_stream" else None
            init = rows.clone()
            ctx.begin()
            with ctx.timed():
                ctx.stall(main)
                pool_emb[1].copy_(inp.emb[2])
                pool_lab[1].copy_(inp.lab[2])
                ready = None
                if prep is not None:
                    so.prep_into(prep, pool_lab)
                    ready = torch.cuda.Event()
                    ready.record(main)
                ctx.step()
                ctx.probe(side)
                a = so.hot.launch_cluster_proxies(mc, pool_emb, pool_lab, init, side, wait_event=ready, prep=prep)
                ctx.still_stalled()
            ctx.step()
            return dict(table=a.table[:-O], sqn=a.sqn[:-O], centroids=a.aux["centroids"])      # (the k = 1 rows belong to the frame call)

    stalled_equals_serial(so, run, real, other)


# ------------------------------------------------------------------------------------------ b. chain into proto_mask_features
@pytest.mark.parametrize("state", ["no_dense_state", "cached_pooled_heads", "float16_no_chain"])
def test_proto_mask_features_waits_for_a_late_chain(so, state):
    """The side stream is stalled in front of the chain (label prep included): main must wait at prep_event before it reads the lists and at
    done_event before the correlation launch.  With the pooled heads cached in dense_state, main's local-prep launch writes the k = 1 rows of
    the table the chain is still writing.  float16 matching has no chain: the control, pipelined against serial."""
    main, side = so.roles(2, [(0, 1)])
    f16 = state == "float16_no_chain"
    mc = so.hot.MatchingConfig(MODEL_FLOAT16_MATCHING=f16)
    real, other = so.clip(REAL), so.clip(OTHER)
    bias = so.bias()
    rows = {id(c): so.init_rows(mc, [c.lab[:1]], 12)[0] for c in (real, other)}

    def run(ctx, inp, oth):
        with torch.cuda.stream(main):
            ref_emb, ref_lab = _pool(inp, [0])
            init = rows[id(inp)].clone()
            ds = None
            if state == "cached_pooled_heads":
                ds = {}
                a0 = so.hot.launch_cluster_proxies(mc, ref_emb, ref_lab, init)
                so.hot.proto_mask_features(mc, ref_emb, ref_lab, inp.emb[0], inp.lab[0], inp.emb[1], bias, cluster_ahead=a0, dense_state=ds)
                assert ds["ref_pool"][0] == 1
            ctx.begin()
            with ctx.timed():
                if f16:
                    a = so.hot.prepare_without_clustering(mc, ref_emb, ref_lab)
                else:
                    ctx.stall(side)
                    a = so.hot.launch_cluster_proxies(mc, ref_emb, ref_lab, init, side)
                ctx.step()
                if not f16:
                    ctx.probe(main)
                feat, head, _ = so.hot.proto_mask_features(mc, ref_emb, ref_lab, inp.emb[1], inp.lab[1], inp.emb[2], bias, cluster_ahead=a, dense_state=ds)
                if not f16:
                    ctx.still_stalled()
            ctx.step()
            return dict(feat=feat, head=head)

    stalled_equals_serial(so, run, real, other, stalled=not f16)


# ------------------------------------------------------------------------------------------ c. chain into FrameRunner
@pytest.mark.parametrize("levels", [None, [8, 16, 32]])
def test_frame_runner_waits_for_a_late_chain_over_a_growing_pool(so, levels):
    """b through aoc_frame_enqueue (prep_ready, proxies_ready), three frames, the pool growing from one frame to two.  Every frame's chain is
    stalled; frame i's outputs are compared on the host (on a stream of its own) while frame i + 1's chain is still spinning."""
    main, side, cmp = so.roles(3, [(0, 1), (2, 1)])
    mc = so.hot.MatchingConfig(CLUSTER_LEVELS=levels)
    real, other = so.clip(REAL), so.clip(OTHER)
    bias = so.bias()
    O = real.lab.shape[-1]
    frames = [(1, 1), (2, 1), (3, 2)]                               # (frame, pool frames): the pool is frames [0, 2][:R]
    rows = {id(c): [so.init_rows(mc, [c.lab[[0, 2]][:R]], 20 + t)[0] for t, R in frames] for c in (real, other)}

    def run(ctx, inp, oth):
        with torch.cuda.stream(main):
            runner = so.hot.FrameRunner(mc, H, W, C, O, capacity_frames=2, device=so.dev)
            pool_emb, pool_lab = _pool(inp, [0, 2])
            init = [r.clone() for r in rows[id(inp)]]
            out, last = {}, None
            ctx.begin()
            for i, (t, R) in enumerate(frames):
                with ctx.timed():
                    ctx.stall(side)
                    a = so.hot.launch_cluster_proxies(mc, pool_emb[:R], pool_lab[:R], init[i], side)
                    ctx.step()
                    ctx.probe(main)
                    feat, head = runner(pool_emb[:R], pool_lab[:R], inp.emb[t - 1], inp.lab[t - 1], inp.emb[t], bias, a, pool_key=R)
                    ctx.still_stalled()
                done = torch.cuda.Event()
                done.record(main)
                if ctx.want is not None and last is not None:
                    with torch.cuda.stream(cmp):
                        cmp.wait_event(last[2])
                        for k, v in ((f"feat{i - 1}", last[0]), (f"head{i - 1}", last[1])):
                            diff = soc.first_difference(v, ctx.want[k])
                            if diff is not None:
                                ctx.errors.append(f"{k}, compared under the next frame's stall: {diff}")
                last = (feat, head, done)
                out[f"feat{i}"], out[f"head{i}"] = feat, head
                ctx.step()
            return out

    stalled_equals_serial(so, run, real, other)


# ------------------------------------------------------------------------------------------ d. dense stream
def _dense_case(so, main, dense, stall, with_state, use_dense_stream=True):
    mc = so.hot.MatchingConfig()
    bias = so.bias()

    def run(ctx, inp, oth):
        with torch.cuda.stream(main):
            ref_emb, ref_lab = _pool(inp, [0, 2])
            a = _ahead_on_this_stream(so, mc, ref_emb, ref_lab, 31)
            cur = oth.emb[4].clone()                      # the query buffer: the other frame's until main writes it
            ds = {} if with_state else None
            ctx.begin()
            with ctx.timed():
                if stall == "main":
                    ctx.stall(main)
                    ctx.probe(dense)
                cur.copy_(inp.emb[4])
                if stall == "dense":
                    ctx.stall(dense)
                    ctx.probe(main)
                ctx.step()
                feat, head, _ = so.hot.proto_mask_features(mc, ref_emb, ref_lab, inp.emb[3], inp.lab[3], cur, bias, cluster_ahead=a, dense_state=ds,
                                                           dense_stream=dense if use_dense_stream else None)
                ctx.still_stalled()
            ctx.step()
            return dict(feat=feat, head=head)
    return run


@pytest.mark.parametrize("with_state", [False, True], ids=["no_dense_state", "dense_state"])
def test_dense_stream_equals_the_plain_call(so, with_state):
    """proto_mask_features(dense_stream=s), nothing stalled, against the call without the option: equal bits (pool split records absent / present)."""
    main, dense = so.roles(2, [(0, 1)])
    real, other = so.clip(REAL), so.clip(OTHER)
    want = snapshot(_dense_case(so, main, dense, None, with_state, use_dense_stream=False)(Ctx(so, "serial"), real, other))
    got = _dense_case(so, main, dense, None, with_state)(Ctx(so, "plain"), real, other)
    assert_same(got, want, "dense_stream != plain call")


@pytest.mark.parametrize("with_state", [False, True], ids=["no_dense_state", "dense_state"])
@pytest.mark.parametrize("stall", ["main", "dense"])
def test_dense_stream_fork_and_join(so, stall, with_state):
    """main stalled in front of the query's write (and so of its split records): the dense stream must wait for main at the fork.
    dense stream stalled: proto_finish on main must wait for dense_done at the join."""
    main, dense = so.roles(2, [(0, 1)])
    real, other = so.clip(REAL), so.clip(OTHER)
    want = stalled_equals_serial(so, _dense_case(so, main, dense, stall, with_state), real, other)
    plain = snapshot(_dense_case(so, main, dense, None, with_state, use_dense_stream=False)(Ctx(so, "serial"), real, other))
    assert_same(want, plain, "dense_stream (serial) != plain call")


# ------------------------------------------------------------------------------------------ e. deferred correlations
def _deferred_case(so, streams, corr, main, precision, n_obj, stall, deferred=True):
    """len(streams) frames of different sequences, each on its own stream, their correlations in ONE launch on `corr`; `main` is the consumer.
    Returns every frame's feat / head, and `seen` = the cluster and proxy channels as a stream that waited ONLY for the returned event sees them."""
    hot = so.hot
    mc = hot.MatchingConfig()
    bias = so.bias(n_obj)
    ch = hot.channel_slices(mc)
    cl = slice(ch["cluster"], ch["proxy"] + 1)

    def run(ctx, inp, oth):
        clips = [inp] + [so.clip(s, n_obj) for s in (101, 102)][:len(streams) - 1]
        clips = clips[1:] + clips[:1]                      # `inp` is the LAST frame of the batch: the one whose stream is stalled
        pend, feats, heads = [], [], []
        pools = [_pool(clip, [0, 2]) for clip in clips]
        inits = [so.init_rows(mc, [lab], 40 + i)[0] for i, (_, lab) in enumerate(pools)]
        ctx.begin()
        with ctx.timed():
            for i, (clip, s) in enumerate(zip(clips, streams)):
                with torch.cuda.stream(s):
                    ref_emb, ref_lab = pools[i]
                    a = hot.launch_cluster_proxies(mc, ref_emb, ref_lab, inits[i])
                    if stall == "frame" and i == len(streams) - 1:
                        ctx.stall(s)
                        ctx.probe(corr)
                    feat, head, aux = hot.proto_mask_features(mc, ref_emb, ref_lab, clip.emb[3], clip.lab[3], clip.emb[4], bias, cluster_ahead=a,
                                                              dense_precision=precision, defer_correlation=deferred)
                    if deferred:
                        pend.append(aux["pending_correlation"])
                        assert pend[-1].stream == s and (pend[-1].query_split is None) == (precision != "split" or n_obj > 16)
                    else:
                        assert aux["pending_correlation"] is None
                    feats.append(feat)
                    heads.append(head)
                ctx.step()
            out = {}
            with torch.cuda.stream(main):
                if deferred:
                    if stall == "corr":
                        ctx.stall(corr)
                        ctx.probe(main)
                    done = hot.launch_correlations(pend, stream=corr, precision=precision)
                    main.wait_event(done)
                    for i, f in enumerate(feats):
                        out[f"seen{i}"] = f[:, cl].clone()
                ctx.still_stalled()
                for s in streams:
                    main.wait_stream(s)                    # the rest of a frame (proto_finish) is on the frame's own stream
                for i, (f, hd) in enumerate(zip(feats, heads)):
                    out[f"feat{i}"], out[f"head{i}"] = f.clone(), hd.clone()
                    if not deferred:
                        out[f"seen{i}"] = f[:, cl].clone()
        ctx.step()
        return out
    return run


@pytest.mark.parametrize("n_frames,precision,n_obj", [(1, "split", 3), (2, "split", 3), (3, "split", 3), (1, "fp32", 3), (2, "fp32", 3), (3, "fp32", 3),
                                                      (2, "split", 18)])
def test_deferred_correlations_equal_the_plain_call(so, n_frames, precision, n_obj):
    """defer_correlation=True + launch_correlations for 1..3 frames of different sequences on different streams: every frame's feat (and what a
    consumer that waits for the returned event alone sees of the cluster / proxy channels) equals the non-deferred call's.  At 18 objects
    query_split is None and the batched entry is taken."""
    streams = so.roles(n_frames + 2, [])
    frames, corr, main = streams[:n_frames], streams[n_frames], streams[n_frames + 1]
    real, other = so.clip(REAL, n_obj), so.clip(OTHER, n_obj)
    want = snapshot(_deferred_case(so, frames, corr, main, precision, n_obj, None, deferred=False)(Ctx(so, "serial"), real, other))
    got = _deferred_case(so, frames, corr, main, precision, n_obj, None)(Ctx(so, "plain"), real, other)
    assert_same(got, want, "deferred correlations != plain call")


@pytest.mark.parametrize("stall", ["frame", "corr"])
def test_deferred_correlations_wait_for_ready_and_signal_done(so, stall):
    """One frame's stream stalled in front of its `ready` event: the batched launch must wait for it.  The correlation stream stalled: a consumer
    that waits for the returned event sees complete cluster and proxy channels."""
    f0, f1, corr, main = so.roles(4, [(1, 2), (2, 3)])
    real, other = so.clip(REAL), so.clip(OTHER)
    stalled_equals_serial(so, _deferred_case(so, [f0, f1], corr, main, "split", 3, stall), real, other)


# ------------------------------------------------------------------------------------------ f. IncrementalProxyBank
def test_incremental_bank_appends_on_a_late_side_stream(so):
    """append (twice), then slot=0 re-written with other initial rows, all on a stalled side stream behind a caller's event; then handle() and a
    frame on main, which joins through the bank's done_event."""
    main, side = so.roles(2, [(0, 1)])
    hot = so.hot
    mc = hot.MatchingConfig()
    real, other = so.clip(REAL), so.clip(OTHER)
    bias = so.bias()
    O = real.lab.shape[-1]
    rows = {id(c): [so.init_rows(mc, [c.lab[f:f + 1]], s)[0] for f, s in ((0, 50), (2, 51), (0, 52))] for c in (real, other)}

    def run(ctx, inp, oth):
        with torch.cuda.stream(main):
            bank = hot.IncrementalProxyBank(mc, O, C, 2, so.dev)
            ref_emb, ref_lab = _pool(inp, [0, 2])
            init = [r.clone() for r in rows[id(inp)]]
            ready = torch.cuda.Event()
            ready.record(main)
            ctx.begin()
            with ctx.timed():
                ctx.stall(side)
                bank.append(ref_emb[0], ref_lab[0], init[0], side, wait_event=ready)
                bank.append(ref_emb[1], ref_lab[1], init[1], side, wait_event=ready)
                bank.append(ref_emb[0], ref_lab[0], init[2], side, wait_event=ready, slot=0)
                assert bank.R == 2
                ctx.step()
                ctx.probe(main)
                feat, head, _ = hot.proto_mask_features(mc, ref_emb, ref_lab, inp.emb[3], inp.lab[3], inp.emb[4], bias, cluster_ahead=bank.handle(ref_lab))
                ctx.still_stalled()
            ctx.step()
            return dict(feat=feat, head=head, table=bank.table, sqn=bank.sqn)

    stalled_equals_serial(so, run, real, other)


# ------------------------------------------------------------------------------------------ g. buffer lifetimes
N_REPLACEMENTS = 4


def _ask_again(tensors):
    """Several new tensors per given one, same size and dtype, holding its content: allocated under the current stream, the first of them gets the
    block a tensor of that size has just given back -- unless a record_stream keeps it."""
    return [t.clone() for t in tensors for _ in range(N_REPLACEMENTS)]


@pytest.mark.parametrize("callers_prep", [False, True], ids=["pool_labels_init_rows", "callers_prep"])
def test_chain_inputs_outlive_the_callers_references(so, callers_prep):
    """The pool, its labels and the initial rows (and a caller's prep lists) are allocated under main and read by the chain on the side stream.
    The side stream is stalled, the caller drops them, and main at once allocates tensors of the same sizes filled with the other frame's pool,
    labels, rows (in range for both labellings) and prep lists."""
    main, side = so.roles(2, [(0, 1)])
    mc = so.hot.MatchingConfig()
    real, other = so.clip(REAL), so.clip(OTHER)
    O = real.lab.shape[-1]
    both = [c.lab[[0, 2]] for c in (real, other)]
    rows, rows_other = so.init_rows(mc, both, 60)[0], so.init_rows(mc, both, 61)[0]

    def run(ctx, inp, oth):
        with torch.cuda.stream(main):
            ref_emb, ref_lab, init = inp.emb[[0, 2]].clone(), inp.lab[[0, 2]].clone(), rows.clone()
            fill = [oth.emb[[0, 2]].clone(), oth.lab[[0, 2]].clone(), rows_other.clone()]
            prep = ready = None
            if callers_prep:
                prep = so.ops.label_prep(ref_lab.reshape(-1, O))
                theirs = so.ops.label_prep(fill[1].reshape(-1, O))
                fill += [getattr(theirs, f) for f in soc.PREP_LISTS]
                ready = torch.cuda.Event()
                ready.record(main)
            ctx.begin()
            with ctx.timed():
                ctx.stall(side)
                a = so.hot.launch_cluster_proxies(mc, ref_emb, ref_lab, init, side, wait_event=ready, prep=prep)
                out = dict(table=a.table[:-O], sqn=a.sqn[:-O], centroids=a.aux["centroids"])
                ctx.step()
                ctx.probe(main)
                del a, ref_emb, ref_lab, init, prep                # (a.aux["chain"]["keep"] held the pool and the rows, a.prep the lists)
                junk = _ask_again(fill)
                ctx.still_stalled()
            ctx.step()
            del junk
            return out

    stalled_equals_serial(so, run, real, other)


@pytest.mark.parametrize("entry", ["proto_mask_features", "FrameRunner"])
def test_proxy_table_and_prep_outlive_the_chain_handle(so, entry):
    """The proxy table, its norms and the prep lists are allocated under the side stream and read by the frame on main.  main is stalled in front of
    the frame, the caller drops the ClusterProxiesAhead (and aux, which names it), and the side stream at once allocates tensors of those sizes
    filled with the other frame's table, norms and lists."""
    main, side = so.roles(2, [(0, 1)])
    hot = so.hot
    mc = hot.MatchingConfig()
    real, other = so.clip(REAL), so.clip(OTHER)
    bias = so.bias()
    O = real.lab.shape[-1]
    rows = {id(c): so.init_rows(mc, [c.lab[[0, 2]]], 70)[0] for c in (real, other)}

    def run(ctx, inp, oth):
        with torch.cuda.stream(main):
            ref_emb, ref_lab = _pool(inp, [0, 2])
            runner = hot.FrameRunner(mc, H, W, C, O, capacity_frames=2, device=so.dev) if entry == "FrameRunner" else None
            with torch.cuda.stream(side):
                b = hot.launch_cluster_proxies(mc, *_pool(oth, [0, 2]), rows[id(oth)].clone())
                fill = [b.table.clone(), b.sqn.clone()] + [getattr(b.prep, f).clone() for f in soc.PREP_LISTS]
                del b
            ready = torch.cuda.Event()
            ready.record(main)
            ctx.begin()
            with ctx.timed():
                a = hot.launch_cluster_proxies(mc, ref_emb, ref_lab, rows[id(inp)].clone(), side, wait_event=ready)
                ctx.step()
                ctx.stall(main)
                ctx.probe(side)
                if runner is not None:
                    feat, head = runner(ref_emb, ref_lab, inp.emb[3], inp.lab[3], inp.emb[4], bias, a, pool_key=2)
                else:
                    feat, head, aux = hot.proto_mask_features(mc, ref_emb, ref_lab, inp.emb[3], inp.lab[3], inp.emb[4], bias, cluster_ahead=a)
                    del aux
                del a
                with torch.cuda.stream(side):
                    junk = _ask_again(fill)
                ctx.still_stalled()
            ctx.step()
            del junk
            return dict(feat=feat, head=head)

    stalled_equals_serial(so, run, real, other)


def test_query_split_records_outlive_the_call_under_dense_stream(so):
    """The query's split records are allocated under main inside the call, read by the dense kernel on the (stalled) dense stream and dropped when
    the call returns; main then allocates tensors of their sizes filled with the other query's records.  `feat` itself is the caller's result:
    the same is done for it in a second call whose result is dropped, where the REPLACEMENTS must stay what they were filled with."""
    main, dense = so.roles(2, [(0, 1)])
    hot, ops = so.hot, so.ops
    mc = hot.MatchingConfig()
    real, other = so.clip(REAL), so.clip(OTHER)
    bias = so.bias()

    def run(ctx, inp, oth):
        with torch.cuda.stream(main):
            ref_emb, ref_lab = _pool(inp, [0, 2])
            a = _ahead_on_this_stream(so, mc, ref_emb, ref_lab, 80)
            theirs = ops.split_rows(oth.emb[4].reshape(-1, C), tiled=True)
            fill = [theirs.records, theirs.sqnorm]
            filler = torch.full((ref_lab.shape[-1], mc.proto_channels, H, W), 0.25, device=so.dev)
            ctx.begin()
            with ctx.timed():
                ctx.stall(dense)
                ctx.probe(main)
                feat, head, _ = hot.proto_mask_features(mc, ref_emb, ref_lab, inp.emb[3], inp.lab[3], inp.emb[4], bias, cluster_ahead=a, dense_stream=dense)
                junk = _ask_again(fill)
                ctx.still_stalled()
                ctx.step()
                ctx.stall(dense)
                ctx.probe(main)
                hot.proto_mask_features(mc, ref_emb, ref_lab, inp.emb[3], inp.lab[3], inp.emb[4], bias, cluster_ahead=a, dense_stream=dense)   # result dropped
                kept = _ask_again([filler])
                ctx.still_stalled()
            ctx.step()
            del junk
            return dict(feat=feat, head=head, replacements=torch.stack(kept))

    want = stalled_equals_serial(so, run, real, other)
    assert bool((want["replacements"] == 0.25).all())


def test_pending_correlation_tensors_outlive_the_frame(so):
    """The query, table, norms, per-set bias, feat and split records of a PendingCorrelation are allocated under the frame's stream and used by the
    batched launch on the (stalled) correlation stream.  The caller drops everything but feat; the frame's stream at once allocates tensors of
    those sizes with the other frame's content.  For feat: a second frame whose result is dropped, and replacements that must stay intact."""
    frame, corr = so.roles(2, [(0, 1)])
    hot, ops = so.hot, so.ops
    mc = hot.MatchingConfig()
    real, other = so.clip(REAL), so.clip(OTHER)
    bias = so.bias()
    ch = hot.channel_slices(mc)

    rows = {id(c): so.init_rows(mc, [c.lab[[0, 2]]], 90)[0] for c in (real, other)}

    def one(clip, cur):
        ref_emb, ref_lab = _pool(clip, [0, 2])
        a = hot.launch_cluster_proxies(mc, ref_emb, ref_lab, rows[id(clip)])
        feat, head, aux = hot.proto_mask_features(mc, ref_emb, ref_lab, clip.emb[3], clip.lab[3], cur, bias.clone(), cluster_ahead=a, defer_correlation=True)
        return feat, aux["pending_correlation"]

    def run(ctx, inp, oth):
        with torch.cuda.stream(frame):
            _, p = one(oth, oth.emb[4].clone())
            fill = [p.query.clone(), p.table.clone(), p.sqn.clone(), p.set_bias.clone(), p.query_split.records.clone(), p.query_split.sqnorm.clone()]
            filler = torch.full((inp.lab.shape[-1], mc.proto_channels, H, W), 0.25, device=so.dev)
            del p
            ctx.begin()
            with ctx.timed():
                cur = inp.emb[4].clone()
                feat, p = one(inp, cur)
                ctx.stall(corr)
                ctx.probe(frame)
                done = hot.launch_correlations([p], stream=corr)
                del p, cur
                junk = _ask_again(fill)
                ctx.still_stalled()
                frame.wait_event(done)
                ctx.step()
                dropped, p = one(inp, inp.emb[4])
                ctx.stall(corr)
                ctx.probe(frame)
                done2 = hot.launch_correlations([p], stream=corr)
                del p, dropped
                kept = _ask_again([filler])
                ctx.still_stalled()
                frame.wait_event(done2)
            ctx.step()
            del junk
            return dict(feat=feat, replacements=torch.stack(kept))

    want = stalled_equals_serial(so, run, real, other)
    assert bool((want["replacements"] == 0.25).all())


# ------------------------------------------------------------------------------------------ h. the evaluation runner
_backend_class = lane_cases.stalled_backend_class          # StalledBackend: shared with test_gpu_eval_lanes.py


def _label_maps(be, spec, data, gt_frames=()):
    emb, gt = data
    be.start(spec)
    be.first_frame(emb[0], gt[0])
    out = [(be.frame_with_gt(emb[t], gt[t]) if t in gt_frames else be.frame(emb[t])).clone() for t in range(1, emb.shape[0])]
    torch.cuda.synchronize()
    return torch.stack(out)


@pytest.mark.parametrize("variant", ["plain", "pool_grows", "ground_truth_early"])
def test_runner_with_a_late_side_stream(so, variant):
    """One sequence, mem_every = 2, 7 frames, every chain launch stalled; against a backend whose side stream IS the main stream.
    pool_grows: the resident pool starts with room for one frame, so _reference_pool's torch.cat replaces the tensor chains were given.
    ground_truth_early: two frames per chain (chain_plan [2]) and ground truth on frames 1 and 3: the pool changes before the second frame
    of a chain launched ahead is used, so that chain's tables are dropped and the draws handed back."""
    er = so.aoc.eval_runner
    main, side = so.roles(2, [(0, 1)])
    cls = _backend_class(er)
    kw = dict(pool_capacity=1 if variant == "pool_grows" else None, chain_plan=[2] if variant == "ground_truth_early" else None)
    gt_frames = (1, 3) if variant == "ground_truth_early" else ()
    spec = er.SequenceSpec("stream-order", H, W, 3, 7, seed=REAL, levels=(16,), mem_every=2)
    other = er.SequenceSpec("stream-order-other", H, W, 3, 7, seed=OTHER, levels=(16,), mem_every=2)
    data, data_other = er.load_sequence(spec, so.dev), er.load_sequence(other, so.dev)
    with torch.cuda.stream(main):
        _label_maps(cls(so.dev, side, **kw), other, data_other, gt_frames)
        want = _label_maps(cls(so.dev, main, **kw), spec, data, gt_frames)
        want_other = _label_maps(cls(so.dev, main, **kw), other, data_other, gt_frames)
        assert not torch.equal(want, want_other)
        warm = cls(so.dev, side, **kw)
        _label_maps(warm, other, data_other, gt_frames)
        ctx = Ctx(so, "stalled", so.stall_cycles(warm.t_frame))
        got = _label_maps(cls(so.dev, side, ctx=ctx, **kw), spec, data, gt_frames)
        ctx.finish()
        assert ctx.n_stalls >= 3
    assert_same(dict(labels=got), dict(labels=want), "late side stream != serial backend")


def test_two_lanes_with_lane_ones_side_stream_late(so):
    """run_interleaved with two lanes, lane 1's side stream stalled at every chain launch: the per-sequence sums equal the one-lane runs' exactly."""
    er = so.aoc.eval_runner
    cls = _backend_class(er)
    lane_streams = [er._cached_stream(so.dev, "lane", l) for l in range(2)]
    side = so.partner_of(lane_streams[1])                    # a side stream that lane 1's own stream overtakes
    specs = [er.SequenceSpec(f"lane{l}", H, W, 3, 7, seed=s, levels=(16,), mem_every=2) for l, s in enumerate((REAL, OTHER))]
    data = [er.load_sequence(s, so.dev) for s in specs]
    single = [er.run_interleaved([(s, d)], so.dev, 1) for s, d in zip(specs, data)]
    er.run_interleaved(list(zip(specs, data)), so.dev, 2)                      # every kernel loaded, the allocator warm
    made = []

    def factory(ctx=None):
        l = len(made)
        made.append(cls(so.dev, side, ctx=ctx, consumer=lane_streams[1]) if l == 1 else er.HotPathBackend(so.dev))
        return made[-1]
    er.run_interleaved(list(zip(specs, data)), so.dev, 2, backend_factory=factory)
    t_frame = made[1].t_frame
    made.clear()
    ctx = Ctx(so, "stalled", so.stall_cycles(t_frame))
    got = er.run_interleaved(list(zip(specs, data)), so.dev, 2, backend_factory=lambda: factory(ctx))
    ctx.finish()
    assert ctx.n_stalls >= 3
    for k in ("sum_iou", "sum_f", "iou_count", "frames", "objects"):
        assert got[k] == single[0][k] + single[1][k], (k, got[k], single[0][k], single[1][k])
