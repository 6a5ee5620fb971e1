"""Helpers of test_gpu_bench_walk.py and test_bench_walk_host.py: bench.py's arrangement restated once, its walk, and the references.

The arrangement.  ``arrange`` builds what ``bench.main()`` builds between ``cfg = syn.CONFIGS[...]`` and ``run_steps`` out of the bench's own
objects (ClipWorkload, frame_step, make_activations; CalibrationGates under torch.manual_seed(0)): seeds 1 + s, phase s, start
(s * MEM_EVERY) // n_streams, chains / chain_plan / chain_lead / runner / batch_gates as main() sets them, one CU-masked main stream per sequence
(hipExtStreamCreateWithCUMask, a contiguous mask of n_cu - reserve CUs, next to ops.set_stream_cus(n_cu - reserve)) or, for --dense-stream, the
mask on a stream for the dense kernel alone, then ``pretouch`` per sequence under its stream.  ``make_main_stream`` is nested in main() and is
restated here (MaskedStreams); a mask call that fails FAILS the test with its return code, there is no unmasked stand-in.

The clip is 23 x 37 with 17 frames: 851 pixels are two 512-pixel query blocks (the second partial) and a partial last 32-row tile, both edges are
odd (the local matching's 12 x 19 down-sampled map, the gates' 12 x 19 half-size maps), hw is no multiple of 4, and 17 frames give the pool
states R = 1..4 in groups of 5, 5, 5 and 1 frames -- the one-frame group has no "rest" to batch.  WALKS are the first 20 steps of both sequences,
worked out by hand from bench.group_order; walk_of restates ClipWorkload's order logic (the class needs a device) and the host test holds the two
together.

The references.  ``serial_twin``: the same frame through hotpath.proto_mask_features with the chain inline and the gates module by module, on the
default stream, synchronised, budget 0 -- the project's contract says every arrangement gives ITS bits.  ``oracle_frame``: the CPU oracle with the
frame's host rows, cached by (seed, n_obj, levels, t) because the arrangements share clips.
"""
import ctypes
import gc
from collections import namedtuple

import numpy as np
import torch

H, W, FRAMES, K = 23, 37, 17, 16
STEPS = 20
FEAT_ATOL = 5e-6                           # every matching branch against the oracle (test_gpu_corr_batched.py, test_gpu_frame.py)
HEAD_RTOL, HEAD_ATOL = 1e-5, 1e-6          # test_frame_call_vs_reference_golden
SWAP_MOVES = 1e-4                          # 20 x FEAT_ATOL: what a chain of the wrong frame must move the cluster channels by
LEVELS3 = (8, 16, 32)

# the first 20 steps of sequence 0 and sequence 1 (phase 1, start 2: inside its first group), t and the pool frames R(t) = 1 + (t - 1) // 5
WALKS = (
    [1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 1, 2, 3, 4],
    [2, 3, 4, 5, 11, 12, 13, 14, 15, 6, 7, 8, 9, 10, 16, 1, 2, 3, 4, 5],
)

# one arrangement = one bench command line.  reserve: CUs kept off the main streams ("narrow" = all but 64); mask_main False = --dense-stream
Arrangement = namedtuple("Arrangement", "name n_obj levels chain_plan python_frames mask_main reserve n_streams")
ARRANGEMENTS = [
    Arrangement("default", 4, None, (2, 3), False, True, 32, 2),
    Arrangement("dense_stream", 4, None, (2, 3), False, False, 32, 2),
    Arrangement("python_frames", 4, None, (2, 3), True, True, 32, 2),
    Arrangement("cfg3_like_levels", 3, LEVELS3, None, False, True, 32, 2),                 # no plan: the --chains 3 schedule of cfg3 / cfg4
    Arrangement("narrow_mask_64", 4, None, (2, 3), False, True, "narrow", 2),
    Arrangement("one_stream_no_reserve", 4, None, (2, 3), False, True, 0, 1),
]
CHAINS = 3                                 # bench --chains default


def clip_config(syn, n_obj):
    return syn.ClipConfig("walk", H, W, n_obj, K, frames=FRAMES)


# ------------------------------------------------------------------------------------------ the walk, without a device
def walk_of(bench, frames, mem_every, phase, start):
    """ClipWorkload's visiting order (bench.py, ClipWorkload.__init__) from bench.group_order: (order, groups)."""
    me = mem_every
    groups = [list(range(g * me + 1, min(g * me + me, frames - 1) + 1)) for g in range((frames - 2) // me + 1)]
    order = bench.group_order(len(groups))
    if phase % 2:
        order = [g for i in range(0, len(order), 2) for g in reversed(order[i:i + 2])]
    rot = (phase // 2) * 2 % len(order)
    order = order[rot:] + order[:rot]
    ts = [t for g in order for t in groups[g]]
    start = start % len(ts)
    return ts[start:] + ts[:start], groups


def first_steps(bench, frames, mem_every, n_streams, s, n):
    order, _ = walk_of(bench, frames, mem_every, s, (s * mem_every) // n_streams)
    return [order[i % len(order)] for i in range(n)]


def pool_frames(t, mem_every=5):
    return 1 + (t - 1) // mem_every


def in_group_pairs(groups):
    """Frames whose successor in the walk sees the same pool: the frames a chain enqueued ahead could be swapped between."""
    return [t for g in groups for t in g[:-1]]


# ------------------------------------------------------------------------------------------ the oracle
_HOST_CLIPS, _ORACLE = {}, {}


def host_clip(syn, seed, n_obj):
    key = (seed, n_obj)
    if key not in _HOST_CLIPS:
        clip = syn.make_clip(clip_config(syn, n_obj), seed)
        lab = np.stack([syn.one_hot(l, n_obj) for l in clip["lab"]])
        _HOST_CLIPS[key] = (torch.from_numpy(clip["emb"]), torch.from_numpy(lab), clip["lab"])
    return _HOST_CLIPS[key]


def host_rows(syn, seed, n_obj, levels, t, mem_every=5):
    """The k-means initial rows of frame t as ClipWorkload draws them (init_rows[t][1]): one list per level."""
    lab_ids = host_clip(syn, seed, n_obj)[2]
    R = pool_frames(t, mem_every)
    counts = [int(sum((lab_ids[i * mem_every] == o).sum() for i in range(R))) for o in range(n_obj)]
    return [syn.kmeans_init_rows(seed * 100003 + t * 7 + li, counts, k) for li, k in enumerate(levels or (K,))]


def oracle_call(syn, seed, n_obj, levels, t, rows, mem_every=5):
    """oracle.hotpath.proto_mask_features of frame t of the clip with the given host rows (one list per level) -> (feat, head)."""
    from oracle import hotpath as ohot
    emb, lab, _ = host_clip(syn, seed, n_obj)
    R = pool_frames(t, mem_every)
    pool = slice(0, (R - 1) * mem_every + 1, mem_every)
    bias = torch.zeros(n_obj)
    if levels is None:
        return ohot.proto_mask_features(emb[pool], lab[pool], emb[t - 1], lab[t - 1], emb[t], bias, init_rows=rows[0])
    return ohot.proto_mask_features(emb[pool], lab[pool], emb[t - 1], lab[t - 1], emb[t], bias, init_rows=list(rows), cluster_levels=tuple(levels))


def oracle_frame(syn, seed, n_obj, levels, t, rows=None):
    """Cached by (seed, n_obj, levels, t).  rows: the workload's own host rows (wl.init_rows[t][1]); None = host_rows' restatement."""
    key = (seed, n_obj, tuple(levels) if levels else None, t)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_call(syn, seed, n_obj, levels, t, rows if rows is not None else host_rows(syn, seed, n_obj, levels, t))
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------ CU-masked streams
class MaskedStreams:
    """bench.main()'s make_main_stream: streams whose workgroups stay on the first n CUs (contiguous mask).  Created once per module, by width, and
    destroyed at teardown; a mask call that fails is an AssertionError that carries the return code."""

    MAX = 4

    def __init__(self, dev):
        self.dev = dev
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        self.n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        self._made = {}                                     # (CUs, index) -> (handle, ExternalStream)

    def get(self, cus, index):
        key = (int(cus), int(index))
        if key not in self._made:
            assert len(self._made) < self.MAX, f"more than {self.MAX} masked streams asked for"
            assert 0 < cus <= self.n_cu
            words = (self.n_cu + 31) // 32
            mask = [0] * words
            for cu in range(cus):
                mask[cu // 32] |= 1 << (cu % 32)
            arr = (ctypes.c_uint32 * words)(*mask)
            handle = ctypes.c_void_p()
            rc = self.hip.hipExtStreamCreateWithCUMask(ctypes.byref(handle), ctypes.c_uint32(words), arr)
            assert rc == 0 and handle.value, f"hipExtStreamCreateWithCUMask({cus} of {self.n_cu} CUs) returned {rc}"
            self._made[key] = (handle, torch.cuda.ExternalStream(handle.value, device=self.dev))
        return self._made[key][1]

    def close(self):
        """Only once nothing that was recorded on these streams is alive any more (the tests keep their arrangements inside one function
        call): a tensor freed later would have the allocator record an event on a destroyed stream."""
        gc.collect()
        torch.cuda.synchronize()
        for handle, _ in self._made.values():
            rc = self.hip.hipStreamDestroy(handle)
            assert rc == 0, f"hipStreamDestroy returned {rc}"
        self._made.clear()


# ------------------------------------------------------------------------------------------ the arrangement
class Arranged:
    """What arrange() hands back: the workloads, their streams, gates and activations, and the CU budget in force."""

    def __init__(self, arr, cfg, mc, gates, acts, workloads, streams, in_stream_ctx, budget):
        self.arr, self.cfg, self.mc, self.gates, self.acts = arr, cfg, mc, gates, acts
        self.workloads, self.streams, self.in_stream_ctx, self.budget = workloads, streams, in_stream_ctx, budget


def arrange(aoc, bench, arr, masked):
    hot, ops, syn = aoc.hotpath, aoc.ops, aoc.synthetic
    dev = masked.dev
    n_cu = masked.n_cu
    reserve = n_cu - 64 if arr.reserve == "narrow" else int(arr.reserve)
    assert 0 <= reserve < n_cu
    if reserve > 0:
        ops.set_stream_cus(n_cu - reserve)
    cfg = clip_config(syn, arr.n_obj)
    mc = hot.MatchingConfig(CLUSTER_NUM=cfg.k, CLUSTER_LEVELS=list(arr.levels) if arr.levels else None)
    torch.manual_seed(0)
    gates = hot.CalibrationGates(mc).to(dev)
    n_streams = arr.n_streams
    workloads = [bench.ClipWorkload(cfg, seed=1 + s, device=dev, mc=mc, overlap=True, phase=s, start=(s * mc.MEM_EVERY) // n_streams)
                 for s in range(n_streams)]
    for wl in workloads:
        wl.chains = max(1, min(CHAINS, mc.MEM_EVERY))
        wl.chain_plan = list(arr.chain_plan) if arr.chain_plan else None
        wl.chain_lead = 1
        wl.reuse_proxies = False
        if not arr.python_frames and hot.FrameRunner.supported(mc, cfg.c, cfg.n_obj):
            wl.runner = hot.FrameRunner(mc, cfg.h, cfg.w, cfg.c, cfg.n_obj, wl.rmax, dev)
        wl.batch_gates = not arr.python_frames
    assert arr.python_frames or all(wl.runner is not None for wl in workloads), "the frame call does not cover the walk's configuration"
    acts = bench.make_activations(gates, cfg.n_obj, cfg.h, cfg.w, dev, seed=7)

    def main_stream(i):
        return masked.get(n_cu - reserve, i) if reserve > 0 else torch.cuda.Stream(device=dev)

    if arr.mask_main:
        streams = [main_stream(i) for i in range(n_streams)] if (n_streams > 1 or reserve > 0) else [torch.cuda.current_stream()]
        dense_streams = [None] * n_streams
    else:
        streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)] if n_streams > 1 else [torch.cuda.current_stream()]
        dense_streams = [main_stream(i) if reserve > 0 else None for i in range(n_streams)]
    for wl, ds in zip(workloads, dense_streams):
        wl.dense_stream = ds
    for wl, st in zip(workloads, streams):
        with torch.cuda.stream(st):
            wl.pretouch(gates, acts, "split", True)
    torch.cuda.synchronize()
    return Arranged(arr, cfg, mc, gates, acts, workloads, streams, n_streams > 1 or (reserve > 0 and arr.mask_main), n_cu - reserve if reserve > 0 else 0)


def _kept(feat, outs, head):
    return feat.clone(), head.clone(), [o.clone() for o in outs]


def step(bench, a):
    """One bench step: bench.frame_step for each sequence in turn under its stream, as run_steps does.  The frame call and the batched gates hand
    back persistent buffers, so the results are cloned inside the stream context.  -> [(t, R, feat, head, gate outputs)], not yet synchronised."""
    out = []
    for wl, st in zip(a.workloads, a.streams):
        t, R = wl.t, wl.R
        if a.in_stream_ctx:
            with torch.cuda.stream(st):
                feat, outs, pending, head = bench.frame_step(wl, a.gates, a.acts, "split", True, False)
                kept = _kept(feat, outs, head)
        else:
            feat, outs, pending, head = bench.frame_step(wl, a.gates, a.acts, "split", True, False)
            kept = _kept(feat, outs, head)
        assert pending is None
        out.append((t, R) + kept)
    return out


def serial_twin(aoc, wl, gates, acts, t, R, budget=0, dense_precision=None):
    """Frame t of the workload's clip with nothing of the arrangement: default stream, device idle before and after, the k-means chain inline on the
    same stream, no dense_state, no runner, the gates module by module, CU budget 0 (put back to `budget` afterwards)."""
    hot, ops = aoc.hotpath, aoc.ops
    torch.cuda.synchronize()
    ops.set_stream_cus(0)
    try:
        feat, head, _ = hot.proto_mask_features(wl.mc, wl.pool_emb[:R], wl.pool_lab[:R], wl.emb[t - 1], wl.lab[t - 1], wl.emb[t], wl.bias,
                                                cluster_state=dict(init_rows=wl.init_rows[t][0]), dense_precision=dense_precision)
        outs = gates(acts, head)
        torch.cuda.synchronize()
    finally:
        ops.set_stream_cus(budget)
    return feat, head, outs
