"""Helpers of test_gpu_stream_order.py: one stalled dependency edge per test.

The method.  A case is a function ``run(ctx, inp, other)`` that enqueues a piece of the frame pipeline on the streams the test chose and returns the
tensors to compare.  ``inp`` are the inputs the answer is computed from, ``other`` inputs of the same shapes (another seed, another labelling): a
buffer of the test's that a late producer writes holds ``other``'s content first, so a read that comes too early sees valid data of another
frame (row indices in range, finite embeddings) and yields wrong numbers, never a bad address.  ``stalled_equals_serial`` runs a case

  1. on ``other``, unsynchronised (every kernel is loaded after this),
  2. on ``inp`` and on ``other`` with a device synchronisation after every step (``ctx.step()``): the SERIAL answers; they must differ,
  3. on ``other`` again, unsynchronised and timed: the host time of the part between stall and last enqueue is ``t_enq``, and the caching
     allocator's free blocks now hold the other frame's data (run after the serial pass on purpose: blocks that still held the serial run's
     right answers would hide a read that comes too early),
  4. on ``inp`` with a bounded spin (torch.cuda._sleep) of max(20 ms, 10 t_enq) in front of the producer, no host synchronisation between
     producer and consumer,

and demands torch.equal between 4 and the serial answer for every returned tensor.  No tolerance exists anywhere in this file.

Two conditions make a stalled run mean something; Ctx.finish asserts both, so a run in which either fails has not passed:

  still stalled     right after the consumer's enqueue returned, the event recorded behind the spin still answers query() == False (the
                    producer's own completion event lies behind that one in the same stream, so it cannot have happened either);
  overtaking probe  the stalled stream writes a sentinel right after its spin and the consumer's stream copies the sentinel with no wait at
                    all; the copy must hold the OLD value: the two streams do overlap on this machine (two streams that share a hardware
                    queue serialise, and then a missing wait is invisible).  The copy is enqueued on the consumer's stream right BEFORE the
                    consumer, not after it: the consumer's own (correct) wait for the producer orders everything behind it in that stream
                    after the sentinel's write, so a copy behind the consumer could only ever show the new value.

Env.roles picks streams for which the probe holds among a handful of fresh ones and FAILS (it does not skip) when there are none.
"""
import itertools
import time
from collections import namedtuple
from contextlib import contextmanager

import numpy as np
import pytest
import torch

H, W, C = 24, 40, 100
STALL_MIN_MS, STALL_MAX_MS, STALL_T_ENQ_FACTOR = 20.0, 500.0, 10.0
N_STREAMS = 8
PREP_LISTS = ("right_bits", "wrong_bits", "fg_rows", "obj_rows", "counts", "obj_offsets")

Clip = namedtuple("Clip", "emb lab")          # emb [T, h, w, C] float32, lab [T, h, w, O] one-hot float32, on the device


def _timed_sleep(cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(int(cycles))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate_cycles_per_ms():
    """Spin cycles per millisecond from two timed torch.cuda._sleep calls (the slope: launch overhead cancels), checked with a third call that
    asks for STALL_MIN_MS."""
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    c1, c2 = 200_000, 1_000_000
    t1, t2 = _timed_sleep(c1), _timed_sleep(c2)
    assert t2 > t1 > 0, f"torch.cuda._sleep does not scale with its argument ({c1}: {t1} ms, {c2}: {t2} ms)"
    cpm = (c2 - c1) / (t2 - t1)
    t3 = _timed_sleep(STALL_MIN_MS * cpm)
    assert 0.5 * STALL_MIN_MS <= t3 <= 2.0 * STALL_MIN_MS, f"calibration: asked for {STALL_MIN_MS} ms, measured {t3} ms"
    return cpm


class Env:
    """Per module: the library, the calibrated spin, a handful of streams and which pairs of them overlap."""

    def __init__(self, aoc):
        self.aoc, self.hot, self.ops, self.syn = aoc, aoc.hotpath, aoc.ops, aoc.synthetic
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.cycles_per_ms = calibrate_cycles_per_ms()
        self.streams = [torch.cuda.Stream() for _ in range(N_STREAMS)]
        self._overlap, self._clips = {}, {}

    # ---- the stall
    def stall_cycles(self, t_enq):
        ms = max(STALL_MIN_MS, STALL_T_ENQ_FACTOR * t_enq * 1e3)
        assert ms <= STALL_MAX_MS, f"the consumer's enqueue took {t_enq * 1e3:.1f} ms on the host: a stall of {ms:.0f} ms is refused"
        return int(ms * self.cycles_per_ms)

    # ---- streams
    def overtakes(self, stalled, consumer):
        """Does stream `consumer` run while stream `stalled` spins?  (The overtaking probe on its own, 5 ms.)"""
        sent = torch.zeros(1, device=self.dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stalled):
            torch.cuda._sleep(int(5 * self.cycles_per_ms))
            sent.fill_(1.0)
        with torch.cuda.stream(consumer):
            snap = sent.clone()
        torch.cuda.synchronize()
        return float(snap) == 0.0

    def overlaps(self, i, j):
        key = (min(i, j), max(i, j))
        if key not in self._overlap:
            self._overlap[key] = self.overtakes(self.streams[i], self.streams[j])
        return self._overlap[key]

    def partner_of(self, consumer):
        """One of this module's streams that a stream from elsewhere (a runner's lane stream) overtakes while it is stalled."""
        for s in self.streams:
            if self.overtakes(s, consumer):
                return s
        pytest.fail(f"none of {N_STREAMS} fresh streams overlaps the given stream on this machine: a missing wait could not show")

    def roles(self, n, overlap):
        """n distinct streams such that roles (a, b) of every pair in `overlap` run concurrently."""
        for perm in itertools.permutations(range(N_STREAMS), n):
            if all(self.overlaps(perm[a], perm[b]) for a, b in overlap):
                return [self.streams[p] for p in perm]
        pytest.fail(f"none of {N_STREAMS} fresh streams gives {n} roles in which {overlap} overlap: every candidate pair serialised "
                    "(shared hardware queue), so a missing wait could not show on this machine")

    # ---- inputs
    def clip(self, seed, n_obj=3, frames=7):
        key = (seed, n_obj, frames)
        if key not in self._clips:
            cfg = self.syn.ClipConfig("stream-order", H, W, n_obj, 16, C, 8, 3)
            clip = self.syn.make_clip(cfg, seed, frames=frames)
            lab = np.stack([self.syn.one_hot(l, n_obj) for l in clip["lab"]])
            self._clips[key] = Clip(torch.from_numpy(clip["emb"]).to(self.dev), torch.from_numpy(lab).to(self.dev))
            torch.cuda.synchronize()
        return self._clips[key]

    def bias(self, n_obj=3):
        return (torch.arange(n_obj, dtype=torch.float32) * 0.07 - 0.2).to(self.dev)

    def init_rows(self, mc, label_pools, seed, n_frames=1):
        """Initial k-means rows [levels * O, kmax] int32 per frame that are in range for EVERY labelling in label_pools ([R, h, w, O] each): drawn
        from the per-object minimum of their row counts.  With several labellings every object must keep at least kmax rows in each, so that
        the sticky K -- a function of the labelling a chain actually reads -- is kmax whichever it reads."""
        levels, kmax = mc.cluster_levels, max(mc.cluster_levels)
        counts = np.stack([p.reshape(-1, p.shape[-1]).sum(0).cpu().numpy().astype(np.int64) for p in label_pools]).min(0)
        if len(label_pools) > 1:
            assert counts.min() >= kmax, f"an object has fewer than {kmax} rows in one labelling: {counts}"
        rows, _ = self.ops.kmeans_init_rows_draw(np.random.RandomState(seed), counts, levels, n_frames, kmax)
        out = [torch.from_numpy(rows[f]).to(self.dev) for f in range(n_frames)]
        torch.cuda.synchronize()
        return out

    def prep_into(self, dst, labels):
        """The label prep of `labels` written INTO the lists of `dst` (a LabelPrep of the same shape the test owns and has filled before)."""
        p = self.ops.label_prep(labels.reshape(-1, labels.shape[-1]))
        assert p.n == dst.n and p.n_obj == dst.n_obj
        for f in PREP_LISTS:
            getattr(dst, f).copy_(getattr(p, f))
        return dst


class Ctx:
    """One run of a case: how = "plain" (unsynchronised), "serial" (step() synchronises) or "stalled"."""

    def __init__(self, env, how, cycles=0):
        assert how in ("plain", "serial", "stalled")
        self.env, self.how, self.cycles = env, how, int(cycles)
        self.sent = torch.zeros(64, device=env.dev)
        self.n_stalls, self.events, self.snaps, self.flags, self.errors = 0, [], [], [], []
        self.t_enq, self.want = 0.0, None
        torch.cuda.synchronize()

    @property
    def stalled(self):
        return self.how == "stalled"

    def begin(self):
        """Everything enqueued so far (inputs, buffers prefilled with the other frame) is complete."""
        torch.cuda.synchronize()

    def step(self):
        if self.how == "serial":
            torch.cuda.synchronize()

    @contextmanager
    def timed(self):
        t0 = time.perf_counter()
        yield
        self.t_enq = max(self.t_enq, time.perf_counter() - t0)

    def stall(self, stream):
        """The bounded spin on `stream`, its sentinel's write and the event that says the spin is over."""
        if not self.stalled:
            return
        assert self.n_stalls < self.sent.numel()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(self.cycles)
            self.sent[self.n_stalls].fill_(1.0)
            ev = torch.cuda.Event()
            ev.record(stream)
        self.events.append(ev)
        self.n_stalls += 1

    def probe(self, stream):
        """The last stall's sentinel copied on `stream` with no wait at all."""
        if self.stalled:
            assert self.n_stalls > 0
            with torch.cuda.stream(stream):
                self.snaps.append(self.sent[self.n_stalls - 1].clone())

    def still_stalled(self):
        if self.stalled:
            assert self.n_stalls > 0
            self.flags.append(not self.events[-1].query())

    def finish(self):
        torch.cuda.synchronize()
        if not self.stalled:
            return
        assert self.flags and self.snaps and len(self.flags) >= self.n_stalls and len(self.snaps) >= self.n_stalls, \
            "a stalled run checks 'still stalled' and the overtaking probe for every stall"
        assert all(self.flags), f"the spin was over before the consumer's enqueue returned (stalls in order: {self.flags}): the consumer was not ahead"
        old = [float(s) == 0.0 for s in self.snaps]
        assert all(old), f"the consumer's stream did not run while the producer's stream span (probes in order: {old}): the streams serialised"
        assert not self.errors, self.errors


def snapshot(out):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def first_difference(got, want):
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    ne = got != want
    n = int(ne.sum())
    if n == 0 and torch.equal(got, want):
        return None
    where = ""
    if got.dim() == 4:                               # a proto-mask tensor [O, channels, h, w]
        where = f", channels {ne.any(dim=3).any(dim=2).any(dim=0).nonzero().flatten().tolist()}"
    elif got.dim() >= 2:
        where = f", first differing row {int(ne.reshape(ne.shape[0], -1).any(dim=1).nonzero()[0])}"
    return f"{n} of {got.numel()} elements differ{where} (NaN counts as different)"


def assert_same(got, want, what):
    torch.cuda.synchronize()
    assert set(got) == set(want)
    bad = {k: first_difference(got[k], want[k]) for k in sorted(want)}
    bad = {k: v for k, v in bad.items() if v is not None}
    assert not bad, f"{what}: {bad}"


def stalled_equals_serial(env, run, inp, other, stalled=True):
    """The method of the module docstring.  stalled=False: step 4 without a spin (a control with nothing to stall).  Returns the serial answer."""
    run(Ctx(env, "plain"), other, inp)
    torch.cuda.synchronize()
    want = snapshot(run(Ctx(env, "serial"), inp, other))
    want_other = snapshot(run(Ctx(env, "serial"), other, inp))
    assert any(first_difference(want[k], want_other[k]) is not None for k in want), "the other inputs give the same answer: stale data would go unnoticed"
    warm = Ctx(env, "plain")
    run(warm, other, inp)
    torch.cuda.synchronize()
    ctx = Ctx(env, "stalled", env.stall_cycles(warm.t_enq)) if stalled else Ctx(env, "plain")
    ctx.want = want
    got = run(ctx, inp, other)
    ctx.finish()
    assert_same(got, want, "stalled run != serial answer" if stalled else "pipelined run != serial answer")
    return want
