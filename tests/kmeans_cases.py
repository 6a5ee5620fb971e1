"""Cases, references and the sum-walk classifier for csrc/labels_kmeans.hip (TEST INFRASTRUCTURE ONLY; numpy / torch-CPU, no GPU).

The k-means contract is bits: labels, counts and code book equal scipy.cluster.vq.kmeans2(minit='matrix').  The update step of the fast
path rebuilds the sequential float32 sum of a cluster from integer folds per binade; everything delicate in it (round-half-even ties
resolved from a running parity, binade crossings, binades predicted from the previous Lloyd iteration, the literal fallback) lives in
the TAIL of a cluster, beyond its first HEAD = 20 * 512 members.  The cases below are the smallest that reach each of those paths; the
classifier says, from the oracle's labels alone, which ones a case reaches (tests/test_kmeans_host.py holds each case to its claim).

References:
  k-means          oracle.kmeans.kmeans2_matrix per segment (== scipy, tests/test_oracle_kmeans.py)
  ordered sum      np.add.accumulate(x[members], axis=0, dtype=float32)[-1] / float32(count)
  proxy set 1      ordered mean of pool[fg_rows[p]] over the segment-local p with labels[beg + p] == j (AEM:280, bug-compatible)
  label prep       torch on the CPU: labels > 0.9, labels < 0.1, labels.sum(1) > 0.9; lists by np.nonzero
  plan / replicate the few lines of numpy include/aoc_hip.h describes
  assignment       the oracle's own distance operands (oracle.kmeans.vq_parts) combined in numpy float32; lane_argmin restates the matrix-pipe
                   argmin from the slot layout, rep_plan the host's choice of kernel, replica groups and grid
"""
import functools

import numpy as np

CHUNK = 512                      # KS_CHUNK
HEAD = 20 * CHUNK                # KS_HEAD_CHUNKS * KS_CHUNK: members summed literally
KP_CROSS = 4                     # crossings a predicted chunk may record
KEPT_BIT = 0x80000000


# ------------------------------------------------------------------------------------------ references
def ordered_mean(x):
    """Sequential float32 sum of the rows of x, in row order, divided by float32(count): scipy's update_cluster_means."""
    x = np.ascontiguousarray(x, np.float32)
    return np.add.accumulate(x, axis=0, dtype=np.float32)[-1] / np.float32(x.shape[0])


def clamp_init(init, length):
    """km_init_kernel: a segment-local initial row outside [0, len) is clamped into it."""
    return np.clip(np.asarray(init, np.int64), 0, max(int(length) - 1, 0))


class KmCase:
    """One aoc_kmeans_segmented_ex call.  pool [P, C] float32; rows int32 packed row ids; offs int32 [S + 1]; seg_k int32 [S];
    init int32 [S, kmax] segment-local; `claims`: what the sum-walk classifier must find (host test).  n_rep > 1: the lists are already
    n_rep replicas of S / n_rep base segments (replicate_reference / replicate_levels_reference), for aoc_kmeans_segmented_rep."""

    def __init__(self, name, make, claims=()):
        self.name, self._make, self.claims = name, make, tuple(claims)

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def data(self):
        d = dict(self._make())
        d["pool"] = np.ascontiguousarray(d["pool"], np.float32)
        n = int(d["pool"].shape[0])
        d.setdefault("rows", np.arange(n, dtype=np.int32))
        d.setdefault("offs", np.array([0, len(d["rows"])], np.int32))
        d["rows"] = np.ascontiguousarray(d["rows"], np.int32)
        d["offs"] = np.ascontiguousarray(d["offs"], np.int32)
        d["seg_k"] = np.ascontiguousarray(d["seg_k"], np.int32)
        d["init"] = np.ascontiguousarray(d["init"], np.int32)
        d.setdefault("iters", 20)
        d["kmax"] = int(d["init"].shape[1])
        d["C"] = int(d["pool"].shape[1])
        d["n_rep"] = int(d.get("n_rep", 1))
        for a in ("pool", "rows", "offs", "seg_k", "init"):
            d[a].setflags(write=False)
        return d

    @functools.lru_cache(maxsize=None)
    def reference(self, trace=False):
        """Expected (centroids [S, kmax, C], labels [rows], counts [S, kmax], traces): the oracle per segment; slots j >= k are zero
        (km_init_kernel) and skipped segments have no labels (marked -1 here, not compared)."""
        from oracle import kmeans as okm
        d = self.data()
        S, kmax, C = len(d["seg_k"]), d["kmax"], d["C"]
        cen = np.zeros((S, kmax, C), np.float32)
        cnt = np.zeros((S, kmax), np.int32)
        lab = np.full(len(d["rows"]), -1, np.int32)
        traces = []
        for s in range(S):
            k, beg, end = int(d["seg_k"][s]), int(d["offs"][s]), int(d["offs"][s + 1])
            if k == 0:
                traces.append(None)
                continue
            x = d["pool"][d["rows"][beg:end]]
            out = okm.kmeans2_matrix(x, x[clamp_init(d["init"][s, :k], end - beg)], d["iters"], trace=trace)
            cen[s, :k], lab[beg:end], cnt[s, :k] = out[0], out[1], out[2]
            traces.append(out[3] if trace else None)
        return cen, lab, cnt, traces


def relu_gauss(rng, n, c, scale=0.3):
    return (np.maximum(rng.randn(n, c), 0.0) * scale).astype(np.float32)


TAIL_COLUMNS = ("dyadic", "late", "zero", "signed", "one_negative", "tiny_then_one", "e_minus_35", "huge", "control")


def tail_columns(n, seed=0, late=HEAD + 60, huge=1e17):
    """[n, 9] float32, one column per mechanism of the tail (TAIL_COLUMNS): dense exact ties (k / 4096); a running sum that is 0 at the
    start of the tail and then climbs through a dozen binades; identically zero; signed; one negative member inside the first tail
    chunk; x >> s (1e-20, then 1.0); exponents below -100 (1e-35); large values; a ReLU-Gaussian control.  `huge` is 1e17 for k-means:
    beyond 2^64 a squared row norm overflows float32, scipy's own distances are NaN and its labels undefined (it reads an
    uninitialised code), so there is no reference to equal.  The proxy sums have no distances and take 1e31 (exponent > 100)."""
    rng = np.random.RandomState(1000 + seed)
    x = np.zeros((n, len(TAIL_COLUMNS)), np.float32)
    x[:, 0] = rng.randint(0, 4096, n) / 4096.0
    x[late:, 1] = rng.randint(1, 4096, max(n - late, 0)) / 4096.0
    x[:, 3] = rng.randn(n)
    x[:, 4] = rng.randint(0, 4096, n) / 4096.0
    if n > HEAD + 300:
        x[HEAD + 300, 4] = -0.375
    x[:late, 5] = 1e-20
    x[late:, 5] = 1.0
    x[:, 6] = (np.abs(rng.randn(n)) + 0.5) * 1e-35
    x[:, 7] = (np.abs(rng.randn(n)) + 0.5) * huge
    x[:, 8] = np.maximum(rng.randn(n), 0.0) * 0.3
    return x


def tiled(cols, c):
    """cols tiled (or cut) to c channels: channel t = cols[:, t % width]."""
    return np.ascontiguousarray(cols[:, np.arange(c) % cols.shape[1]], np.float32)


def _tail_case(n, c, iters, k=1):
    def make():
        return dict(pool=tiled(tail_columns(n), c), seg_k=[k], init=[[7] * k], iters=iters)
    return make


ALL_TAIL_CLAIMS = ("tie_even", "tie_odd", "tie_and_crossing_in_chunk", "more_than_kp_cross", "tail_starts_at_zero", "negative_tail_member",
                   "x_over_u_2_24", "exponent_beyond_100")

# 1. tail arithmetic: one segment, K = 1, so membership is fixed and the sum is the segment in row order
TAIL_CASES = [KmCase(f"tail_n12000_it{it}", _tail_case(12000, 12, it), ALL_TAIL_CLAIMS) for it in (1, 2, 20)]
TAIL_CASES += [KmCase(f"tail_n{n}", _tail_case(n, 12, 3)) for n in (HEAD, HEAD + 1, HEAD + CHUNK, HEAD + CHUNK + 1)]


# 2. moving membership: two clusters whose counts cross HEAD in both directions, chunk binades that move between iterations
MOVING_SEED = 1


def moving_data(seed, n=20600, c=8):
    rng = np.random.RandomState(seed)
    t = rng.rand(n, 1)
    x = np.maximum(0.25 * rng.randn(n, c) + t, 0.0)
    x = (np.round(x * 1024.0) / 1024.0).astype(np.float32)
    init = rng.permutation(n)[:2].astype(np.int32)
    return x, init


def _moving():
    x, init = moving_data(MOVING_SEED)
    return dict(pool=x, seg_k=[2], init=init[None])


MOVING_CASE = KmCase("moving_membership", _moving, ("count_up_through_head", "count_down_through_head", "chunk_binade_moved"))

# 3. widths.  Fast path (C % 4 == 0, C <= 128): rank kernels <25> / <32>, one to five head groups of 28 and fold groups of 20 features,
# ragged last groups; C = 100 is the matrix-pipe assignment, kt = ceil(K / 16) = 1 .. 4; everything else is the generic path, NF = ceil(C / 64)
FAST_WIDTHS = (4, 28, 32, 60, 96, 104, 124, 128)
WIDTH_CASES = [KmCase(f"fast_C{c}", _tail_case(12000, c, 3), ("tie_even", "tie_odd")) for c in FAST_WIDTHS]


def _blobs(n, c, k, seed, with_tail=False):
    """Non-negative multiples of 1/1024 (exact ties in every sum) around k well-separated centres; with_tail: one blob of HEAD + 800 rows."""
    def make():
        rng = np.random.RandomState(seed)
        sizes = np.full(k, n // k)
        if with_tail:
            sizes[:] = (n - (HEAD + 800)) // max(k - 1, 1)
            sizes[k - 1] = HEAD + 800
        centre = rng.randint(0, 4, (k, c)).astype(np.float64)
        who = np.repeat(np.arange(k), sizes)
        rng.shuffle(who)
        x = np.maximum(centre[who] + 0.15 * rng.randn(len(who), c), 0.0)
        x = (np.round(x * 1024.0) / 1024.0).astype(np.float32)
        init = np.array([np.nonzero(who == j)[0][3] for j in range(k)], np.int32)
        return dict(pool=x, seg_k=[k], init=init[None])
    return make


MFMA_CASES = [KmCase("mfma_K1_tail", _tail_case(12000, 100, 3), ("tie_even", "tie_odd"))]
MFMA_CASES += [KmCase(f"mfma_K{k}", _blobs(3000 + 7 * k, 100, k, 40 + k)) for k in (16, 17, 33, 64)]
MFMA_CASES += [KmCase("mfma_K17_tail", _blobs(21000, 100, 17, 77, with_tail=True), ("tie_even", "tie_odd"))]


def _generic(c):
    def make():
        rng = np.random.RandomState(c)
        x = relu_gauss(rng, 700, c)
        x[:, 1] = 0.0
        x[:, 2] = np.float32(0.5) * rng.randint(0, 5, 700)
        return dict(pool=x, seg_k=[8], init=rng.permutation(700)[:8].astype(np.int32)[None])
    return make


GENERIC_CASES = [KmCase(f"generic_C{c}", _generic(c)) for c in (30, 70, 130, 200, 256)]


# 4. stitch grid: kmax * n_seg = 7 and 9 clusters, the tailed cluster in the last, partial block of 8 (1 is every K = 1 case above)
def _stitch7():
    d = _blobs(14000, 28, 7, 5, with_tail=True)()
    return d


def _stitch9():
    """Three segments x kmax 3: clusters 0 .. 8, the ninth (segment 2, j = 2) alone in the second block of 8 and tailed."""
    big = _blobs(12500, 28, 3, 6, with_tail=True)()
    rng = np.random.RandomState(66)
    small = (np.round(relu_gauss(rng, 41, 28) * 1024.0) / 1024.0).astype(np.float32)
    pool = np.concatenate([small, big["pool"]])
    n_big = len(big["pool"])
    offs = np.array([0, 40, 41, 41 + n_big], np.int32)
    init = np.array([[3, 17, 29], [0, 0, 0], list(big["init"][0])], np.int32)
    return dict(pool=pool, offs=offs, seg_k=[3, 1, 3], init=init)


STITCH_CASES = [KmCase("stitch_7_clusters", _stitch7, ("tie_even", "tie_odd")), KmCase("stitch_9_clusters", _stitch9, ("tie_even", "tie_odd"))]


# 5. assignment edges at C = 100: more segments than the LDS segment table holds (128), short segments, skipped ones, a 1-row segment
def _many_segments(n_seg):
    def make():
        rng = np.random.RandomState(n_seg)
        lens = rng.randint(1, 301, n_seg)
        lens[n_seg // 2] = 1
        lens[n_seg - 1] = 300
        k = np.minimum(16, lens)
        k[[5, n_seg // 2 + 1, n_seg - 2]] = 0                      # skipped segments in the middle (reference: centroid None)
        total = int(lens.sum())
        pool = relu_gauss(rng, total + 30, 100)
        rows = np.sort(rng.permutation(total + 30)[:total]).astype(np.int32)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        init = np.zeros((n_seg, 16), np.int32)
        for s in range(n_seg):
            init[s, :k[s]] = rng.permutation(lens[s])[:k[s]]
        return dict(pool=pool, rows=rows, offs=offs, seg_k=k, init=init)
    return make


DUP_SLOTS = (3, 19, 35, 51)


def _duplicates_k64():
    """K = 64, the same pool row (copied) as initial centroid 3, 19, 35 and 51: one per 16-cluster tile.  The distance tie goes to 3 in every
    iteration; 19, 35 and 51 stay empty and keep their centroid."""
    rng = np.random.RandomState(64)
    n = 2000
    x = relu_gauss(rng, n, 100)
    init = rng.permutation(n)[:64].astype(np.int32)
    row = (4.0 + 0.5 * rng.randint(0, 4, 100)).astype(np.float32)      # far from every other row, and so few bits that the mean of its
    for j in DUP_SLOTS:                                                # copies is the row itself: the four code words stay equal bit for bit
        x[init[j]] = row
    x[np.setdiff1d(np.arange(n), init)[:30]] = row
    return dict(pool=x, seg_k=[64], init=init[None])


def _init_out_of_range():
    rng = np.random.RandomState(8)
    x = relu_gauss(rng, 500, 100)
    init = rng.permutation(500)[:16].astype(np.int32)
    init[0], init[5], init[15] = -7, 500, 2 ** 31 - 1
    return dict(pool=x, seg_k=[16], init=init[None])


ASSIGN_CASES = [KmCase(f"segments_{s}", _many_segments(s)) for s in (128, 129, 180)]
ASSIGN_CASES += [KmCase("duplicates_K64", _duplicates_k64), KmCase("init_rows_out_of_range", _init_out_of_range)]



# 6. assignment ties.  Both matrix-pipe kernels keep cluster kt * 16 + g * 4 + r in register r of lane group g (tile kt): a lane scans
# its clusters with a strict <, then the four lane groups merge by two xor exchanges (16, then 32) with "lower distance, then lower index".
def slot_lane(slot):
    """(tile kt, lane group g, register r) of a cluster slot."""
    return slot >> 4, (slot >> 2) & 3, slot & 3


# K = 16: the same lane; xor-16 partners; xor-32 partners; two two-step merges.  K = 64: the lower index in the HIGHER lane group through a later
# tile, for every pair of lane groups -- (1, 0), (2, 0), (3, 0), (3, 1), (3, 0) again across tiles 1 | 2, and (2, 1), (3, 2) -- next to two pairs
# in index order across tiles 0 | 2 and 1 | 3
TIE_PAIRS = {16: ((1, 3), (2, 7), (2, 11), (6, 9), (7, 13)),
             64: ((5, 18), (9, 16), (13, 17), (14, 22), (6, 40), (23, 63), (31, 32), (9, 20), (13, 24))}
TIE_COPIES = 24


def _seg_offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _tie_pairs(k, pairs, iters, seed, n_rep=1):
    """Segments of 200 .. 400 rows; in each, TIE_COPIES rows hold one value that is far from every other row and has so few bits that the mean
    of its copies is the value itself (the _duplicates_k64 recipe).  Two of the copies are the initial code words of the slot pair
    pairs[(s + f) % len(pairs)] of segment s in replica f; no other slot starts on a copy.  `pairs` in the result: the pair per segment."""
    def make():
        rng = np.random.RandomState(seed)
        n_seg = 2 * len(pairs) if n_rep == 1 else len(pairs)
        lens = rng.randint(200, 401, n_seg)
        offs = _seg_offsets(lens)
        pool = relu_gauss(rng, int(offs[-1]), 100)
        init = np.zeros((n_rep * n_seg, k), np.int32)
        for s in range(n_seg):
            copies = np.sort(rng.permutation(lens[s])[:TIE_COPIES])
            pool[offs[s] + copies] = (4.0 + 0.5 * rng.randint(0, 4, 100)).astype(np.float32)
            others = np.setdiff1d(np.arange(lens[s]), copies)
            for f in range(n_rep):
                row = rng.permutation(others)[:k]
                a, b = pairs[(s + f) % len(pairs)]
                row[a], row[b] = rng.permutation(copies)[:2]           # which copy sits in the lower slot is left to chance: the tie is by value
                init[f * n_seg + s] = row
        planted = [pairs[(s + f) % len(pairs)] for f in range(n_rep) for s in range(n_seg)]
        rows, offs_out, seg_k = replicate_reference(np.arange(offs[-1], dtype=np.int32), offs, np.full(n_seg, k, np.int32), n_rep)
        return dict(pool=pool, rows=rows, offs=offs_out, seg_k=seg_k, init=init, iters=iters, n_rep=n_rep, pairs=planted)
    return make


TIE_PAIR_CASES = [KmCase(f"tie_pairs_K{k}_it{it}", _tie_pairs(k, TIE_PAIRS[k], it, 7000 + k)) for k in (16, 64) for it in (1, 3)]

# rows and initial code words on the lattice {0, 1, 2}^C: every product, sum and distance is a small integer, exact in float32 in any
# order, so equal distances between DISTINCT code words are frequent and are true ties.  One row; 255, 256, 257 (the 256-row block and both
# neighbours); 1 500.  K = 33 puts slot 32 alone in a third tile; the one-row segment starts from 33 equal code words.
LATTICE_LENS = (1, 255, 256, 257, 1500)
LATTICE_K = 33
LATTICE_WIDTHS = (96, 100, 128, 70)          # km_assign_rank_kernel<25>, the matrix pipe, km_assign_rank_kernel<32>, km_assign_generic_kernel


def _lattice(c):
    def make():
        rng = np.random.RandomState(3000 + c)
        offs = _seg_offsets(LATTICE_LENS)
        pool = rng.randint(0, 3, (int(offs[-1]), c)).astype(np.float32)
        init = np.stack([rng.permutation(n)[:LATTICE_K] if n >= LATTICE_K else np.arange(LATTICE_K) % n for n in LATTICE_LENS])
        return dict(pool=pool, offs=offs, seg_k=[LATTICE_K] * len(LATTICE_LENS), init=init, iters=1)
    return make


LATTICE_CASES = [KmCase(f"tie_lattice_C{c}", _lattice(c)) for c in LATTICE_WIDTHS]

# rows = one offset of about 3 per feature plus noise of 1e-3: |x|^2 and |c|^2 are near 9 C, their ulp (2^-14 .. 2^-13) is of the size of the
# differences between distances (2 C 1e-6), so the label of many rows is decided by where the three terms are rounded
NEAR_TIE_SHAPES = [(100, 16, 1), (100, 16, 2), (100, 40, 1), (100, 40, 2), (96, 16, 1), (96, 40, 2), (128, 16, 1), (128, 40, 2), (70, 16, 1), (70, 40, 2)]


def _near_tie(c, k, iters):
    def make():
        rng = np.random.RandomState(100 * c + k)
        n = 1500
        x = ((3.0 + 0.25 * rng.rand(c)) + 1e-3 * rng.randn(n, c)).astype(np.float32)
        return dict(pool=x, seg_k=[k], init=rng.permutation(n)[:k].astype(np.int32)[None], iters=iters)
    return make


NEAR_TIE_CASES = [KmCase(f"near_tie_offset_C{c}_K{k}_it{it}", _near_tie(c, k, it)) for c, k, it in NEAR_TIE_SHAPES]

KMEANS_CASES = (TAIL_CASES + [MOVING_CASE] + WIDTH_CASES + MFMA_CASES + GENERIC_CASES + STITCH_CASES + ASSIGN_CASES + TIE_PAIR_CASES + LATTICE_CASES
                + NEAR_TIE_CASES)


# 7. replicated lists at C = 100 (aoc_kmeans_segmented_rep with n_rep stated): replica f of base segment s is segment f * n_base + s, every
# replica lists the same rows and starts from initial rows of its own
def _rep_lists(rng, lens, n_rep, kmax, k=None, levels=None, iters=20, edit=None):
    """Base segments of `lens` rows (a sorted random subset of a slightly larger pool), replicated n_rep times with min(k, len) clusters each, or
    with the sticky per-replica levels; `edit(seg_k [n_rep, n_base])` may change cluster counts afterwards."""
    lens = np.asarray(lens, np.int64)
    offs = _seg_offsets(lens)
    total, n_base = int(offs[-1]), len(lens)
    pool = relu_gauss(rng, total + 30, 100)
    rows = np.sort(rng.permutation(total + 30)[:total]).astype(np.int32)
    if levels is None:
        rows_out, offs_out, seg_k = replicate_reference(rows, offs, np.minimum(k, lens), n_rep)
    else:
        rows_out, offs_out, seg_k = replicate_levels_reference(rows, offs, n_rep, levels)
    seg_k = seg_k.copy()
    if edit is not None:
        edit(seg_k.reshape(n_rep, n_base))
    init = np.zeros((n_rep * n_base, kmax), np.int32)
    for sr in range(n_rep * n_base):
        init[sr, :seg_k[sr]] = rng.permutation(lens[sr % n_base])[:seg_k[sr]]
    return dict(pool=pool, rows=rows_out, offs=offs_out, seg_k=seg_k, init=init, iters=iters, n_rep=n_rep)


def _rep_uniform(lens, n_rep, k, seed, iters=20):
    return lambda: _rep_lists(np.random.RandomState(seed), lens, n_rep, k, k=k, iters=iters)


def _rep_levels(lens, n_rep, levels, seed):
    return lambda: _rep_lists(np.random.RandomState(seed), lens, n_rep, max(levels), levels=levels)


REP_BASE40_DEAD = (5, 20, 38)                       # base segments no replica clusters
REP_BASE40_ONLY = {7: 0, 9: 1, 39: 2}               # base segment -> the one replica that clusters it


def _rep_base40():
    rng = np.random.RandomState(4040)
    lens = np.concatenate([[1, 255, 256, 257], rng.randint(40, 500, 36)])

    def edit(seg_k):
        seg_k[:, list(REP_BASE40_DEAD)] = 0
        for s, f in REP_BASE40_ONLY.items():
            seg_k[np.arange(seg_k.shape[0]) != f, s] = 0
    return _rep_lists(rng, lens, 3, 40, k=40, iters=5, edit=edit)


def _rep_over_grid_cap():
    """32 base segments (the most the replica kernel's LDS table holds), 22 short ones of one work item each among 10 of three or four: about
    50 items per group, and 22 replicas at K = 40 are 11 groups of two -- more items than the 512 workgroups the grid is capped at."""
    rng = np.random.RandomState(512)
    lens = rng.permutation(np.concatenate([rng.randint(1, 40, 22), rng.randint(520, 860, 10)]))
    return _rep_lists(rng, lens, 22, 40, k=40, iters=2)


REP_TIE_PAIRS = tuple(p for p in TIE_PAIRS[64] if p[1] < 40)
REP_CASES = [KmCase(f"rep_K40_n{n}", _rep_uniform((300, 257, 700, 41), n, 40, 4000 + n)) for n in (2, 3, 5)]
REP_CASES += [KmCase("rep_levels_40_8_48", _rep_levels((700, 257, 300), 3, (40, 8, 48), 4048)),
              KmCase("rep_K16_n13", _rep_uniform((300, 130, 600), 13, 16, 4013)),
              KmCase("rep_K24_n7", _rep_uniform((300, 257, 130), 7, 24, 4024)),            # not asked for: <25, 2>, groups of 3 + 3 + 1, held to the oracle
              KmCase("rep_base40", _rep_base40),
              KmCase("rep_level_zero", _rep_levels((500, 300, 5, 0, 400), 4, (16, 0, 8), 4000)),
              KmCase("rep_over_grid_cap", _rep_over_grid_cap),
              KmCase("rep_tie_pairs", _tie_pairs(40, REP_TIE_PAIRS, 3, 7040, n_rep=3))]


# ------------------------------------------------------------------------------------------ assignment rules and plans, restated
def distances(dot, xs, cs):
    """The float32 distance scipy compares, from the oracle's operands (oracle.kmeans.vq_parts): (-2 dot + |x|^2) + |c|^2, one rounding each."""
    return (np.float32(-2.0) * dot + xs[:, None]) + cs[None, :]


def lane_argmin(dist, in_lane="<", merge="lowest"):
    """The argmin of the matrix-pipe kernels restated from the slot layout (slot_lane): per lane group a scan over its clusters, tiles in
    order, with `in_lane` ("<" or "<="); then g0 | g1 and g2 | g3 exchange (xor 16), then the two winners (xor 32), and lane group 0's value
    is the label.  merge: "lowest" = (d2 < low || (d2 == low && a2 < arg)); "highest" = a2 > arg; "keep" = the d2 == low clause dropped."""
    n, k = dist.shape
    kt = (k + 15) // 16
    d = np.full((n, kt * 16), np.inf, np.float32)
    d[:, :k] = dist
    r = np.arange(n)
    cand = []
    for g in range(4):
        slots = np.array([t * 16 + g * 4 + q for t in range(kt) for q in range(4)])
        dg = d[:, slots]
        pos = np.argmin(dg, 1) if in_lane == "<" else dg.shape[1] - 1 - np.argmin(dg[:, ::-1], 1)
        low = dg[r, pos]
        arg = np.where(np.isinf(low) & (in_lane == "<"), 0, slots[pos])      # low = INFINITY, arg = 0 is where a lane starts
        cand.append((low, arg))

    def exchange(mine, other):
        take = other[0] < mine[0]
        if merge != "keep":
            take |= (other[0] == mine[0]) & ((other[1] < mine[1]) if merge == "lowest" else (other[1] > mine[1]))
        return np.where(take, other[0], mine[0]), np.where(take, other[1], mine[1])
    return exchange(exchange(cand[0], cand[1]), exchange(cand[2], cand[3]))[1].astype(np.int32)


KM_REP_LDS_BUDGET = 78 * 1024
KM_ASSIGN_GRID_CAP = 512
KM_REP_SEG_LDS = 32


def rep_plan(kmax, n_rep, n_base=1, base_rows=0):
    """What aoc_kmeans_segmented_rep launches for the assignment at C = 100: the kernel, its KT, and for the replica kernel the code books that
    fit one group (`fit`), the groups and the grid."""
    kt = (kmax + 15) // 16
    fixed = 4 * 16 * 116 * 4 + 4 * kmax * 4
    per = (kt * 16 * 116 + kt * 16) * 4 + 256
    fit = min(16, (KM_REP_LDS_BUDGET - fixed) // per)
    gcap = KM_ASSIGN_GRID_CAP * 3 // 2 if kt == 1 else KM_ASSIGN_GRID_CAP
    if n_rep <= 1 or fit < 2:
        return dict(kernel="km_assign_mfma_kernel", kt=kt, fit=fit, gcap=gcap)
    n_groups = (n_rep + fit - 1) // fit
    n_grp = (n_rep + n_groups - 1) // n_groups
    return dict(kernel="km_assign_mfma_rep_kernel", kt=kt, fit=fit, gcap=gcap, n_groups=n_groups, n_grp=n_grp,
                groups=[min(n_grp, n_rep - g * n_grp) for g in range(n_groups)], grid=min((base_rows // 256 + n_base) * n_groups, gcap))


def rep_case_plan(case):
    """rep_plan of a replicated case, called as the GPU test calls it (rows_capacity = the replicated rows, the pool no shorter than the base
    lists), plus `items`: the (group, base segment, block) work items in the order the persistent workgroups index them."""
    d = case.data()
    n_rep, n_base = d["n_rep"], len(d["seg_k"]) // d["n_rep"]
    assert len(d["pool"]) * n_base >= len(d["rows"]) // n_rep
    plan = rep_plan(d["kmax"], n_rep, n_base, len(d["rows"]) // n_rep)
    live = (d["seg_k"].reshape(n_rep, n_base) > 0).any(0)
    blocks = [(int(d["offs"][s + 1] - d["offs"][s]) + 255) // 256 if live[s] else 0 for s in range(n_base)]
    plan["items"] = [(g, s, b) for g in range(plan.get("n_groups", 0)) for s in range(n_base) for b in range(blocks[s])]
    return plan


def is_fast(case):
    """The widths aoc_kmeans_segmented_ex sums by the scan-sum pipeline when pool_rows is stated."""
    c = case.data()["C"]
    return c % 4 == 0 and c <= 128


# ------------------------------------------------------------------------------------------ sum-walk classifier
def _exponent(v):
    """floor(log2 |v|) per element (float64 in, exact); 0 -> a sentinel far below every float32 exponent."""
    m, e = np.frexp(np.abs(v))
    return np.where(v == 0, -10000, e - 1)


def classify(x, traces, k):
    """Walk the exact float32 running sum s of every (iteration, cluster, feature), members in row order, and report what the tail
    (member index >= HEAD) meets.  u = ulp of s's binade; a member x is a tie when |x/u - rint(x/u)| == 1/2, at the parity of s/u.
    x [n, d] float32; traces [iters, n] the oracle's labels of every assignment."""
    x64 = np.ascontiguousarray(x, np.float32).astype(np.float64)
    rep = dict(tie_even=0, tie_odd=0, crossings=0, tie_and_crossing_in_chunk=0, chunk_binade_moved=0, more_than_kp_cross=0,
               negative_tail_member=0, tail_starts_at_zero=0, x_over_u_2_24=0, exponent_beyond_100=0, count_up_through_head=0,
               count_down_through_head=0, tailed_clusters=0, counts=[])
    prev_start, prev_cnt = {}, None
    for it, lab in enumerate(traces):
        cnt = np.bincount(lab, minlength=k)
        rep["counts"].append(cnt.tolist())
        if prev_cnt is not None:
            rep["count_up_through_head"] += int(np.sum((prev_cnt <= HEAD) & (cnt > HEAD)))
            rep["count_down_through_head"] += int(np.sum((prev_cnt > HEAD) & (cnt <= HEAD)))
        prev_cnt = cnt
        for j in range(k):
            if cnt[j] <= HEAD:
                continue
            rep["tailed_clusters"] += 1
            xm = x64[lab == j]
            run = np.add.accumulate(xm.astype(np.float32), axis=0, dtype=np.float32).astype(np.float64)
            s, xt, after = run[HEAD - 1:-1], xm[HEAD:], run[HEAD:]          # s before each tail member, the member, s after it
            es, ea = _exponent(s), _exponent(after)
            live = s != 0
            u = np.ldexp(1.0, np.where(live, es - 23, 0))
            q = np.where(live, np.abs(xt) / u, 0.0)
            tie = live & (np.abs(q - np.rint(q)) == 0.5)
            odd = np.mod(np.abs(s) / u, 2.0) == 1.0
            cross = live & (after != 0) & (ea != es)
            rep["tie_even"] += int(np.sum(tie & ~odd))
            rep["tie_odd"] += int(np.sum(tie & odd))
            rep["crossings"] += int(cross.sum())
            rep["more_than_kp_cross"] += int(np.sum(cross.sum(0) > KP_CROSS))
            rep["negative_tail_member"] += int(np.sum(xt < 0))
            rep["tail_starts_at_zero"] += int(np.sum(s[0] == 0))
            rep["x_over_u_2_24"] += int(np.sum(q >= 2.0 ** 24))
            ex = _exponent(xt)
            rep["exponent_beyond_100"] += int(np.sum(live & (np.abs(es) > 100)) + np.sum((xt != 0) & (np.abs(ex) > 100)))
            n_ch = (len(xt) + CHUNK - 1) // CHUNK
            for c in range(n_ch):
                sl = slice(c * CHUNK, (c + 1) * CHUNK)
                rep["tie_and_crossing_in_chunk"] += int(np.sum(tie[sl].any(0) & cross[sl].any(0)))
                start = es[c * CHUNK]
                old = prev_start.get((j, c))
                if old is not None:
                    rep["chunk_binade_moved"] += int(np.sum(old != start))
                prev_start[(j, c)] = start
            for key in [key for key in prev_start if key[0] == j and key[1] >= n_ch]:
                del prev_start[key]
        for key in [key for key in prev_start if cnt[key[0]] <= HEAD]:
            del prev_start[key]
    return rep


def classify_case(case):
    """Classifier totals over the segments of a case (distinct columns only: a tiled pool repeats them)."""
    d = case.data()
    _, _, _, traces = case.reference(trace=True)
    total = None
    for s, tr in enumerate(traces):
        if tr is None:
            continue
        beg, end = d["offs"][s], d["offs"][s + 1]
        x = d["pool"][d["rows"][beg:end]]
        x = x[:, np.unique(x, axis=1, return_index=True)[1]] if x.shape[0] > HEAD else x[:, :1]
        rep = classify(x, tr, int(d["seg_k"][s]))
        if total is None:
            total = rep
        else:
            for key, v in rep.items():
                total[key] = total[key] + v if key != "counts" else total[key]
    return total


def sum_ties_away(x):
    """The sequential float32 sum with ties rounded AWAY from zero instead of to even (a wrong kernel the tie cases must tell apart).
    Needs s + x exact in float64 (true for the dyadic columns)."""
    s = np.zeros(x.shape[1], np.float64)
    for row in np.asarray(x, np.float64):
        t = s + row
        r = t.astype(np.float32).astype(np.float64)
        lo = np.where(r > t, np.nextafter(r.astype(np.float32), np.float32(-np.inf)).astype(np.float64), r)
        hi = np.where(r < t, np.nextafter(r.astype(np.float32), np.float32(np.inf)).astype(np.float64), r)
        tie = (r != t) & ((t - lo) == (hi - t))
        s = np.where(tie, np.where(t > 0, hi, lo), r)
    return s.astype(np.float32)


# ------------------------------------------------------------------------------------------ proxies (aoc_build_proxies)
def proxy_case(c, seed=0):
    """A two-object pool with hand-written labels: segment 0 (k = 3 of kmax = 4) has cluster 0 above HEAD members, cluster 1 empty;
    segment 1 has k = 2.  Objects interleave in the pool and a few rows are not kept, so fg_rows[p] != obj_rows[beg + p]: set 1 is
    the mean over the GLOBAL kept-row list at segment-LOCAL indices (AEM:280 as written).  The rows cluster 0 gathers are
    tail_columns in order, so its sum meets the same ties and crossings as the k-means tail case."""
    rng = np.random.RandomState(600 + seed)
    n0, n1, kmax = 12900, 900, 4
    n_pool = n0 + n1 + 25
    obj = np.full(n_pool, -1, np.int64)                                 # -1: row not kept
    kept = np.sort(rng.permutation(n_pool)[:n0 + n1])
    obj[kept] = rng.permutation(np.repeat([0, 1], [n0, n1]))
    fg_rows = kept.astype(np.int32)
    obj_rows = np.concatenate([np.nonzero(obj == 0)[0], np.nonzero(obj == 1)[0]]).astype(np.int32)
    offs = np.array([0, n0, n0 + n1], np.int32)
    labels = np.empty(n0 + n1, np.int32)
    labels[:n0] = np.where(rng.rand(n0) < 0.93, 0, 2)
    labels[n0:] = rng.randint(0, 2, n1)
    pool = relu_gauss(rng, n_pool, c)
    members = fg_rows[np.nonzero(labels[:n0] == 0)[0]]
    assert len(members) > HEAD + 100
    pool[members] = tiled(tail_columns(len(members), seed=seed, huge=1e31), c)
    centroids = relu_gauss(rng, 2 * kmax, c).reshape(2, kmax, c)
    return dict(pool=pool, fg_rows=fg_rows, obj_rows=obj_rows, offs=offs, seg_k=np.array([3, 2], np.int32), labels=labels,
                centroids=centroids, kmax=kmax, C=c)


def proxy_reference(d):
    """(proxies [S, 2, kmax, C], counts [S, kmax], sqnorm64 [S, 2, kmax], bound [S, 2, kmax]).  Set 0 = centroids; set 1 = ordered mean, 0 for an
    empty cluster; slots j >= k are 0.  The norm is +inf for j >= k and for an empty cluster of set 1; elsewhere float64 sum a^2,
    held under gamma_C * sum a^2 (C products and C - 1 additions in any order, each rounded once) plus C underflowed squares;
    a sum a^2 beyond float32's range is +inf in float32 whatever the order (the 1e31 column: one square already overflows)."""
    S, kmax, C = len(d["seg_k"]), d["kmax"], d["C"]
    prox = np.zeros((S, 2, kmax, C), np.float32)
    cnt = np.zeros((S, kmax), np.int64)
    for s in range(S):
        k, beg, end = int(d["seg_k"][s]), int(d["offs"][s]), int(d["offs"][s + 1])
        prox[s, 0, :k] = d["centroids"][s, :k]
        for j in range(k):
            p = np.nonzero(d["labels"][beg:end] == j)[0]
            cnt[s, j] = len(p)
            if len(p):
                prox[s, 1, j] = ordered_mean(d["pool"][d["fg_rows"][p]])
    sq = (prox.astype(np.float64) ** 2).sum(-1)
    eps = C * 2.0 ** -24
    bound = eps / (1.0 - eps) * sq + C * 2.0 ** -149
    assert not ((sq > 3.0e38) & (prox.astype(np.float64) ** 2 < 3.5e38).all(-1)).any(), "overflow must come from a single square"
    sq[sq > 3.0e38] = np.inf
    for s in range(S):
        k = int(d["seg_k"][s])
        sq[s, :, k:] = np.inf
        sq[s, 1, :k][cnt[s, :k] == 0] = np.inf
    return prox, cnt, sq, bound


# ------------------------------------------------------------------------------------------ label prep
F09, F01 = np.float32(0.9), np.float32(0.1)
THRESHOLDS = (F09, np.nextafter(F09, np.float32(1)), F01, np.nextafter(F01, np.float32(0)))
LABEL_KINDS = ("one_hot", "multi_hot", "kept_right_for_none", "right_not_kept", "zero", "soft", "at_0.9", "above_0.9", "at_0.1", "below_0.1")


def label_case(n, n_obj, nothing_kept=False):
    """labels [n, n_obj] float32 and the kind of every row.  The last object never has a row of its own when n_obj >= 3.  Soft rows are
    multiples of 2^-10 and a threshold row holds one non-zero entry, so every row sum is exact in any order."""
    rng = np.random.RandomState(n * 31 + n_obj)
    lab = np.zeros((n, n_obj), np.float32)
    live = n_obj - 1 if n_obj >= 3 else n_obj
    kinds = rng.randint(0, len(LABEL_KINDS), n)
    kinds[:min(n, len(LABEL_KINDS))] = rng.permutation(len(LABEL_KINDS))[:min(n, len(LABEL_KINDS))]
    if nothing_kept:
        kinds = np.where(rng.rand(n) < 0.5, LABEL_KINDS.index("right_not_kept"), LABEL_KINDS.index("zero"))
    o1 = rng.randint(0, live, n)
    o2 = (o1 + 1 + rng.randint(0, max(live - 1, 1), n)) % live
    r = np.arange(n)
    for i, kind in enumerate(LABEL_KINDS):
        m = kinds == i
        if kind == "one_hot" or (n_obj == 1 and kind in ("multi_hot", "kept_right_for_none")):
            lab[r[m], o1[m]] = 1.0
        elif kind == "multi_hot":
            lab[r[m], o1[m]] = 1.0
            lab[r[m], o2[m]] = 1.0
        elif kind == "kept_right_for_none":
            lab[r[m], o1[m]] = 0.5
            lab[r[m], o2[m]] += 0.5                                # o2 == o1 only when live == 1 ... then it is a one-hot row
        elif kind == "right_not_kept":
            lab[r[m], o1[m]] = 1.0
            if n_obj >= 2:
                lab[r[m], (o1[m] + 1) % n_obj] = -0.5
        elif kind == "soft":
            lab[m] = rng.randint(0, 300, (int(m.sum()), n_obj)) / 1024.0
            if n_obj >= 3:
                lab[m, n_obj - 1] = np.minimum(lab[m, n_obj - 1], 0.25)
        elif kind != "zero":
            lab[r[m], o1[m]] = THRESHOLDS[LABEL_KINDS.index(kind) - 6]
    return lab, kinds


def label_prep_reference(lab):
    """The reference's own expressions, evaluated by torch on the CPU (AEM:197, 252, 585), lists by np.nonzero."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(lab, np.float32))
    n, n_obj = lab.shape
    right = (t > 0.9).numpy()
    wrong = (t < 0.1).numpy()
    keep = (t.sum(1) > 0.9).numpy()
    w = (np.uint64(1) << np.arange(n_obj, dtype=np.uint64))
    right_bits = ((right.astype(np.uint64) * w).sum(1) + keep.astype(np.uint64) * np.uint64(KEPT_BIT)).astype(np.uint32)
    wrong_bits = (wrong.astype(np.uint64) * w).sum(1).astype(np.uint32)
    fg_rows = np.nonzero(keep)[0].astype(np.int32)
    lists = [np.nonzero(keep & right[:, o])[0].astype(np.int32) for o in range(n_obj)]
    counts = np.array([len(l) for l in lists] + [len(fg_rows)], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts[:n_obj])]).astype(np.int32)
    obj_rows = np.concatenate(lists) if lists else np.zeros(0, np.int32)
    return dict(right_bits=right_bits, wrong_bits=wrong_bits, fg_rows=fg_rows, obj_rows=obj_rows.astype(np.int32), counts=counts,
                obj_offsets=offsets)


LABEL_N = (1, 63, 64, 65, 255, 256, 257, 262144 + 257)
LABEL_OBJ = (1, 2, 17, 30)


# ------------------------------------------------------------------------------------------ plan and replicate
def plan_reference(counts, cluster_num):
    """AEM:268: k[o] = min(k[o - 1], counts[o]), k[-1] = cluster_num (sticky)."""
    return np.minimum.accumulate(np.concatenate([[cluster_num], counts]))[1:].astype(np.int32)


def replicate_reference(rows, offs, seg_k, n_rep):
    """Replica f's lists follow replica f - 1's: rows at f * total, offsets shifted by f * total, total = offs[-1]."""
    total = int(offs[-1])
    rows_out = np.tile(np.asarray(rows[:total], np.int32), n_rep)
    offs_out = np.concatenate([f * total + np.asarray(offs[:-1], np.int64) for f in range(n_rep)] + [[n_rep * total]]).astype(np.int32)
    return rows_out, offs_out, np.tile(np.asarray(seg_k, np.int32), n_rep)


def replicate_levels_reference(rows, offs, n_rep, levels):
    """Replica f clusters at levels[f % n_levels], made sticky from the segment sizes like plan_reference."""
    lens = np.diff(np.asarray(offs, np.int64))
    seg_k = np.concatenate([plan_reference(lens, levels[f % len(levels)]) for f in range(n_rep)])
    rows_out, offs_out, _ = replicate_reference(rows, offs, np.zeros(len(lens), np.int32), n_rep)
    return rows_out, offs_out, seg_k.astype(np.int32)
