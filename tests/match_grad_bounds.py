"""Float64 references, derived bounds, cases and inputs for the training-time global matching: aoc_dense_match_argmin (the ARG instantiation of
dense_match_partial_kernel / dense_match_finalize_kernel in csrc/correlation.hip) and the gradient kernels of csrc/match_grad.hip
(aoc_dense_match_grad, aoc_proxy_match_grad).  Shared by test_match_grad_host.py (no GPU) and test_gpu_match_grad.py.  Pure numpy; the
library is not imported here.  U, gamma and the per-pair distance bound are those of float64_bounds.py / global_match_bounds.py.

Forward.  dense_forward_ref is global_match_bounds.dense_ref's reference (min over the kept rows of D + PAD wrong, bound by
min_with_bound, then transform_ref) that also returns the minimiser: the POOL ROW of the first minimum in ascending row order (np.argmin),
-1 where the minimum is a padded distance (>= PAD / 2) or no row is kept, and the float64 gap to the runner-up.

Backward, read off match_grad.hip (every product, sum and difference rounds once: -ffp-contract=off):
  g     mg_gate: fl(fl(go * 0.5) * fl(1 - fl(T^ T^))), go * 0.5 exact.  With |T^ - T| <= e_T (the forward bound):
          e_tt = 2 |T| e_T + e_T^2, then + U (T^2 + e_tt);   w = 1 - T^2:  e_w = e_tt + U (|w| + e_tt);
          e_g  = |go / 2| e_w + e_go (|w| + e_w) / 2, then + U (|g| + that)        (e_go: the error of grad_out itself, 0 unless stated)
  term  fl(fl(2 g^) * fl(x - y)): 2 g^ exact; the difference is off by U |x - y|; the product by the two errors and one rounding:
          e_term = 2 e_g a (1 + U) + 2 |g| a U, then + U (2 |g| a + that),  a = |x - y|
  sums  a sum of terms each of which passes through at most k additions is off by sum e_term + gamma(k) sum (|term| + e_term), with k:
          grad_query   n_obj                     mg_pairs_kernel / pg_pairs_kernel: `acc +=` over the objects, ascending
          grad_pool    the row's pairs, if at most MG_LIST = 256 (mg_rows_kernel adds the ranked list in order); a hot row: the most pairs
                       it has in one of the MG_NSEG = 32 pair-id ranges (mg_hot_kernel) + 32 (mg_hot_final_kernel)
          grad_bias    min(m, 256) + ceil(m / 256)   mg_bias_partial_kernel, mg_bias_final_kernel
          proxies      min(m, 64) + ceil(m / 64) for S = sum g q (each term fl(g^ q): e_g |q|, one rounding) and for G = sum g
                       (pg_partial_kernel, pg_final_kernel); then fl(2 fl(fl(p G^) - S^)): the product, the difference, an exact doubling.
No measured number goes into a bound.  The gradients depend on arg discontinuously, so the tests demand arg == the float64 argmin and the
host test demands that no case (outside the planted duplicates) has a best / runner-up gap under 100 x the forward distance bound.

Inputs (grad_case_inputs).  Random embeddings at these widths put thousands of pairs within the forward bound of a tie, so the structure is
planted: the pixels come in groups (sizes 1, 2, 3, 5, 8, 13, 21, 34, 70, 100, repeating) around a base vector b (scale 1.2 / sqrt(C)) with a
jitter of length 0.03; for every (group, present object) one kept pool row b + delta, |delta|^2 drawn from [0.4, 1.4], right for that
object alone, wins the whole group, so lists of 1 .. 100 pairs from different pixels and objects arise; background rows (scale 2 / sqrt(C),
distances of 3 and more) fill the pool up to n_fg kept rows, one row in nine is not kept, and the rows are shuffled.  Distances of
0.4 .. 1.4 under biases N(0, 0.3^2) keep T well inside (0.05, 0.95)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from float64_bounds import U, gamma
from global_match_bounds import PAD, dense_nsplit, min_with_bound, pair_distances, proxy_ref, transform_ref

f32 = np.float32
MG_LIST, MG_NSEG, MG_CHUNK, MG_BIAS_PIX, PG_PIX = 256, 32, 64, 256, 64
GROUP_SIZES = (1, 2, 3, 5, 8, 13, 21, 34, 70, 100)
GAP_FACTOR = 100.0


# ------------------------------------------------------------------------------------------ forward with argmin
def labels_to_bits(labels_flat):
    """aoc_label_prep's definitions on [n, O] labels: kept rows (label sum > 0.9), wrong bits (label < 0.1)."""
    lab = np.asarray(labels_flat, np.float64)
    kept = np.nonzero(lab.sum(1) > 0.9)[0]
    wrong = lab < 0.1
    return kept, wrong


def dense_forward_ref(query, pool, labels_flat, bias):
    """-> dict(T, tol_T [O, m]; raw, tol_raw; arg [O, m] int64 (pool row, -1); gap [O, m] (float64 runner-up minus best among the object's
    candidates, +inf where there is one candidate or none); e_best [O, m]: the forward distance bound of the winning pair)."""
    m, n_obj = query.shape[0], labels_flat.shape[1]
    kept, wrong = labels_to_bits(labels_flat)
    if kept.size == 0:
        one = np.ones((n_obj, m))
        return dict(T=one, tol_T=np.zeros((n_obj, m)), raw=np.full((n_obj, m), np.inf), tol_raw=np.zeros((n_obj, m)),
                    arg=np.full((n_obj, m), -1, np.int64), gap=np.full((n_obj, m), np.inf), e_best=np.zeros((n_obj, m)))
    D, E = pair_distances(query, pool[kept])
    Ep = E + U * (np.abs(D + PAD) + E)
    raw, tol, gap, e_best = (np.empty((n_obj, m)) for _ in range(4))
    arg = np.empty((n_obj, m), np.int64)
    ar = np.arange(m)
    for o in range(n_obj):
        w = wrong[kept, o]
        A, EA = np.where(w[None, :], D + PAD, D), np.where(w[None, :], Ep, E)
        raw[o], tol[o] = min_with_bound(A, EA, np.inf)
        j = A.argmin(1)
        arg[o] = np.where(raw[o] < 0.5 * PAD, kept[j], -1)
        e_best[o] = EA[ar, j]
        if A.shape[1] > 1:
            part = np.partition(A, 1, axis=1)
            gap[o] = part[:, 1] - part[:, 0]
        else:
            gap[o] = np.inf
    T, tol_T = transform_ref(raw, tol, bias)
    return dict(T=T, tol_T=tol_T, raw=raw, tol_raw=tol, arg=arg, gap=gap, e_best=e_best)


def proxy_forward_ref(query, proxies, bias):
    """-> (T, tol_T) [O, m] of aoc_proxy_corr_min with single-proxy sets, norms computed in the kernel, transform = 1."""
    n_obj = proxies.shape[0]
    raw, tol = proxy_ref(query, proxies, None, np.arange(n_obj), np.ones(n_obj, np.int64))
    return transform_ref(raw, tol, bias)


# ------------------------------------------------------------------------------------------ gradients and their bounds
def gate_ref(go, T, tol_T, e_go=0.0):
    """g = go (1 - T^2) / 2 and its bound (module docstring).  Arrays of one shape."""
    go, T, tol_T = (np.asarray(a, np.float64) for a in (go, T, tol_T))
    e_go = np.broadcast_to(np.asarray(e_go, np.float64), go.shape)
    w = 1.0 - T * T
    g = 0.5 * go * w
    e_tt = 2.0 * np.abs(T) * tol_T + tol_T * tol_T
    e_tt = e_tt + U * (T * T + e_tt)
    e_w = e_tt + U * (np.abs(w) + e_tt)
    e_g = 0.5 * np.abs(go) * e_w + 0.5 * e_go * (np.abs(w) + e_w)
    return g, e_g + U * (np.abs(g) + e_g)


def _term_err(g, e_g, a):
    """The bound of fl(fl(2 g^) fl(x - y)) with a = |x - y| (broadcast)."""
    e = 2.0 * e_g * a * (1.0 + U) + 2.0 * np.abs(g) * a * U
    return e + U * (2.0 * np.abs(g) * a + e)


def _hot_k(pids, n_pairs):
    """The additions a term of a hot row passes through at most: its pair-id range's matches, then the MG_NSEG partial rows."""
    seg = -(-(-(-n_pairs // MG_NSEG)) // MG_CHUNK) * MG_CHUNK
    return int(np.bincount(np.asarray(pids) // seg, minlength=MG_NSEG).max()) + MG_NSEG


def dense_grad_ref(go, T, tol_T, arg, query, pool, e_go=0.0):
    """go, T, tol_T, arg [O, m]; query [m, C], pool [n, C] float32.  -> dict(grad_query, tol_query [m, C]; grad_pool, tol_pool [n, C];
    grad_bias, tol_bias [O]; g, e_g [O, m]; counts [n]: pairs per pool row)."""
    q, p = np.asarray(query, f32).astype(np.float64), np.asarray(pool, f32).astype(np.float64)
    n_obj, m = T.shape
    n, C = p.shape
    g, e_g = gate_ref(go, T, tol_T, e_go)
    gq, tq = np.zeros((m, C)), np.zeros((m, C))
    mag_q = np.zeros((m, C))
    gp, tp, mag_p = np.zeros((n, C)), np.zeros((n, C)), np.zeros((n, C))
    pairs_of = [[] for _ in range(n)]
    for i in range(m):                                   # ascending pixel, then object: the order of every list
        for o in range(n_obj):
            r = int(arg[o, i])
            if r < 0:
                continue
            diff = q[i] - p[r]
            term = 2.0 * g[o, i] * diff
            e = _term_err(g[o, i], e_g[o, i], np.abs(diff))
            gq[i] += term
            tq[i] += e
            mag_q[i] += np.abs(term) + e
            gp[r] -= term
            tp[r] += e
            mag_p[r] += np.abs(term) + e
            pairs_of[r].append(i * n_obj + o)
    tq = tq + gamma(n_obj) * mag_q
    counts = np.asarray([len(l) for l in pairs_of])
    k_row = np.asarray([len(l) if len(l) <= MG_LIST else _hot_k(l, m * n_obj) for l in pairs_of], np.float64)
    tp = tp + gamma(np.maximum(k_row, 1.0))[:, None] * mag_p
    k_b = min(m, MG_BIAS_PIX) + -(-m // MG_BIAS_PIX)
    gb = g.sum(1)
    tb = e_g.sum(1) + gamma(k_b) * (np.abs(g) + e_g).sum(1)
    return dict(grad_query=gq, tol_query=tq, grad_pool=gp, tol_pool=tp, grad_bias=gb, tol_bias=tb, g=g, e_g=e_g, counts=counts)


def proxy_grad_ref(go, T, tol_T, query, proxies, e_go=0.0):
    """-> dict(grad_query, tol_query [m, C]; grad_proxies, tol_proxies [O, C]; grad_bias, tol_bias [O])."""
    q, p = np.asarray(query, f32).astype(np.float64), np.asarray(proxies, f32).astype(np.float64)
    n_obj, m = T.shape
    g, e_g = gate_ref(go, T, tol_T, e_go)
    diff = q[None, :, :] - p[:, None, :]                                    # [O, m, C]
    term = 2.0 * g[:, :, None] * diff
    e = _term_err(g[:, :, None], e_g[:, :, None], np.abs(diff))
    gq = term.sum(0)
    tq = e.sum(0) + gamma(n_obj) * (np.abs(term) + e).sum(0)
    k = min(m, PG_PIX) + -(-m // PG_PIX)
    G = g.sum(1)
    e_G = e_g.sum(1) + gamma(k) * (np.abs(g) + e_g).sum(1)
    gq_term = g[:, :, None] * q[None, :, :]
    e_t = e_g[:, :, None] * np.abs(q)[None, :, :]
    e_t = e_t + U * (np.abs(gq_term) + e_t)
    S = gq_term.sum(1)
    e_S = e_t.sum(1) + gamma(k) * (np.abs(gq_term) + e_t).sum(1)
    pG = p * G[:, None]
    e_pG = np.abs(p) * e_G[:, None]
    e_pG = e_pG + U * (np.abs(pG) + e_pG)
    d = pG - S
    e_d = e_pG + e_S
    e_d = e_d + U * (np.abs(d) + e_d)
    return dict(grad_query=gq, tol_query=tq, grad_proxies=2.0 * d, tol_proxies=2.0 * e_d, grad_bias=G, tol_bias=e_G)


def ratio(got, want, tol):
    """-> the worst |got - want| / tol (0 where both vanish); asserts nothing."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def check(got, want, tol, what, report=None):
    """Prints the figures, then asserts |got - want| <= tol elementwise.  -> the worst error / bound."""
    r = ratio(got, want, tol)
    err = np.abs(np.asarray(got, np.float64) - want)
    print(f"{what}: worst error {err.max() if err.size else 0.0:.3e}, worst error / bound {r:.3f}, bound up to {np.max(tol) if np.size(tol) else 0.0:.3e}")
    if report is not None:
        report.append((what, r))
    assert r <= 1.0, f"{what}: {int((err > tol).sum())} elements outside the bound, worst error / bound {r:.3f}"
    return r


# ------------------------------------------------------------------------------------------ cases
GradCase = namedtuple("GradCase", "name C m n_obj n_fg absent layout kind")


def _gcase(name, C, m, n_obj, n_fg=None, absent=None, layout="planes", kind="groups"):
    return GradCase(name, C, m, n_obj, n_fg, absent, layout, kind)


# every C with every class of m and of objects at least once; layouts alternate.  n_fg None: the planted rows plus 40 background rows.
DENSE_GRAD_CASES = [
    _gcase("C4_m17_O3", 4, 17, 3),
    _gcase("C36_m99_O17", 36, 99, 17, layout="pixels"),
    _gcase("C100_m257_O3", 100, 257, 3),
    _gcase("C128_m1_O1", 128, 1, 1, layout="pixels"),
    _gcase("C100_m99_O30", 100, 99, 30, absent=7),
    _gcase("C36_m257_O1", 36, 257, 1, layout="pixels"),
    _gcase("C128_m17_O17", 128, 17, 17, absent=16),
    _gcase("C4_m1_O30", 4, 1, 30, layout="pixels"),
    _gcase("rows17001", 36, 17, 3, n_fg=17001),                       # several 128-row chunks per n-split, 64 n-splits
    _gcase("hot_row", 100, 257, 3, kind="hot"),                       # one kept row per object: every list has 257 pairs
    _gcase("hot_row_C36_O30", 36, 257, 30, kind="hot", layout="pixels"),
]
NO_ROWS = _gcase("no_rows", 36, 17, 3, n_fg=0)
TIES = _gcase("ties", 36, 17, 3, n_fg=2100, kind="ties")             # 132 tiles over 64 n-splits: three tiles per split
DENSE_BY_NAME = {c.name: c for c in DENSE_GRAD_CASES + [NO_ROWS, TIES]}

# C above what the forward kernels of the dense path take: the gradient entry alone, on the float32 rounding of the reference's T and
# its argmin (wide_case_ref).  Above C = 128 the gradient kernels stage 32 query rows per step: a list of 34 pairs, and a hot row.
WIDE_GRAD_CASES = [_gcase("C256_m99_O3", 256, 99, 3), _gcase("hot_C256_m257_O1", 256, 257, 1, kind="hot", layout="pixels")]
DENSE_BY_NAME.update({c.name: c for c in WIDE_GRAD_CASES})
PROXY_WIDE_CASES = [("p_C256_m99_O3", 256, 99, 3)]

PROXY_GRAD_CASES = [("p_C4_m1_O1", 4, 1, 1), ("p_C36_m99_O3", 36, 99, 3), ("p_C128_m257_O30", 128, 257, 30), ("p_C36_m257_O1", 36, 257, 1),
                    ("p_C4_m99_O30", 4, 99, 30), ("p_C128_m1_O3", 128, 1, 3)]


def _unit(rng, C):
    v = rng.standard_normal(C)
    return v / np.sqrt((v * v).sum())


def argmin_split_ranges(m, n_fg):
    """The [first, last + 1) positions of fg_rows per non-empty n-split of the ARG launches (one A tile per wave: dense_nsplit(m, 1))."""
    ns = dense_nsplit(m, 1)
    n_tiles = (n_fg + 15) // 16
    tps = (n_tiles + ns - 1) // ns
    return [(16 * s * tps, min(n_fg, 16 * min(n_tiles, (s + 1) * tps))) for s in range(ns) if s * tps < n_tiles]


def grad_case_inputs(case):
    """-> dict(query [m, C], pool [n, C] float32, labels [n, O] float32 (one-hot kept rows, zero rows not kept), bias [O] float32, grad_out
    [O, m] float32, dup (ties only): [(winner row, its later copies)])."""
    C, m, n_obj = case.C, case.m, case.n_obj
    rng = np.random.RandomState(zlib.crc32(("match_grad/" + case.name).encode()) & 0x7FFFFFFF)
    s = 1.2 / np.sqrt(C)
    present = [o for o in range(n_obj) if o != case.absent]
    bias = (0.3 * rng.standard_normal(n_obj)).astype(f32)
    grad_out = rng.standard_normal((n_obj, m)).astype(f32)
    if case.n_fg == 0:
        query = (s * rng.standard_normal((m, C))).astype(f32)
        pool = (s * rng.standard_normal((40, C))).astype(f32)
        return dict(query=query, pool=pool, labels=np.zeros((40, n_obj), f32), bias=bias, grad_out=grad_out)
    if case.kind == "hot":
        base = s * rng.standard_normal(C)
        query = (base[None, :] + 0.3 * s * rng.standard_normal((m, C))).astype(f32)
        rows = [(base + np.sqrt(rng.uniform(0.4, 1.4)) * _unit(rng, C), o) for o in present]
        extra = 9                                                            # rows that are not kept
    else:
        query = np.empty((m, C))
        rows, i, gi = [], 0, 0
        while i < m:
            size = min(GROUP_SIZES[gi % len(GROUP_SIZES)], m - i)
            base = s * rng.standard_normal(C)
            for k in range(size):
                query[i + k] = base + 0.03 * _unit(rng, C)
            for o in present:
                rows.append((base + np.sqrt(rng.uniform(0.4, 1.4)) * _unit(rng, C), o))
            i, gi = i + size, gi + 1
        query = query.astype(f32)
        n_fg = len(rows) + 40 if case.n_fg is None else case.n_fg
        assert n_fg >= len(rows)
        for _ in range(n_fg - len(rows)):
            rows.append(((2.0 / np.sqrt(C)) * rng.standard_normal(C), present[rng.randint(len(present))]))
        extra = max(4, len(rows) // 9)
    order = rng.permutation(len(rows) + extra)
    n = order.size
    pool = ((2.0 / np.sqrt(C)) * rng.standard_normal((n, C))).astype(f32)
    labels = np.zeros((n, n_obj), f32)
    for slot, (vec, o) in zip(order[:len(rows)], rows):
        pool[slot] = vec.astype(f32)
        labels[slot, o] = 1.0
    out = dict(query=query, pool=pool, labels=labels, bias=bias, grad_out=grad_out)
    if case.kind == "ties":
        # a winner at a position whose split holds a later tile: exact copies one position on (the same tile, the next lane: the cross-lane
        # index reduction decides), 16 positions on (the same lane of the next tile of the same n-split: the lane's strict `<` decides) and
        # five n-splits on (the finalize kernel decides); the copies carry the winner's label
        kept, _ = labels_to_bits(labels)
        ranges = argmin_split_ranges(m, kept.size)
        fwd = dense_forward_ref(query, pool, labels, bias)
        dup = []
        used = set()
        for o in range(n_obj):
            for i in range(m):
                r = int(fwd["arg"][o, i])
                pos = int(np.searchsorted(kept, r))
                sp = next(k for k, (b, e) in enumerate(ranges) if b <= pos < e)
                b, e = ranges[sp]
                if r in used or pos % 16 == 15 or pos + 16 >= e or sp + 5 >= len(ranges) or len(dup) >= 3:
                    continue
                later = [int(kept[pos + 1]), int(kept[pos + 16]), int(kept[ranges[sp + 5][0] + 3])]
                if any(x in used for x in later) or any((fwd["arg"] == x).any() for x in later):
                    continue
                for x in later:
                    pool[x], labels[x] = pool[r], labels[r]
                used.update([r] + later)
                dup.append((r, later))
        assert len(dup) == 3, "ties: no winner found whose n-split holds a later tile"
        out["dup"] = dup
    return out


def proxy_case_inputs(name, C, m, n_obj):
    rng = np.random.RandomState(zlib.crc32(("match_grad/" + name).encode()) & 0x7FFFFFFF)
    s = 0.7 / np.sqrt(C)                                  # |q - p|^2 about 2 C s^2 = 1: T around 0.46
    return dict(query=(s * rng.standard_normal((m, C))).astype(f32), proxies=(s * rng.standard_normal((n_obj, C))).astype(f32),
                bias=(0.3 * rng.standard_normal(n_obj)).astype(f32), grad_out=rng.standard_normal((n_obj, m)).astype(f32))


@functools.lru_cache(maxsize=None)
def dense_case_ref(name):
    """-> (inputs, forward reference, gradient reference) of a dense case, computed once.  Treat as read-only."""
    inp = grad_case_inputs(DENSE_BY_NAME[name])
    fwd = dense_forward_ref(inp["query"], inp["pool"], inp["labels"], inp["bias"])
    grad = dense_grad_ref(inp["grad_out"], fwd["T"], fwd["tol_T"], fwd["arg"], inp["query"], inp["pool"])
    return inp, fwd, grad


@functools.lru_cache(maxsize=None)
def wide_case_ref(name):
    """-> (inputs, forward reference, T32 [O, m] float32, gradient reference) of a WIDE case: the gradient kernels get T32, the float32
    rounding of the reference's T, so for them T is T32 exactly (no forward error) and the reference is taken at T32."""
    inp = grad_case_inputs(DENSE_BY_NAME[name])
    fwd = dense_forward_ref(inp["query"], inp["pool"], inp["labels"], inp["bias"])
    T32 = fwd["T"].astype(f32)
    grad = dense_grad_ref(inp["grad_out"], T32.astype(np.float64), np.zeros_like(fwd["T"]), fwd["arg"], inp["query"], inp["pool"])
    return inp, fwd, T32, grad


@functools.lru_cache(maxsize=None)
def proxy_case_ref(name):
    case = next(c for c in PROXY_GRAD_CASES + PROXY_WIDE_CASES if c[0] == name)
    inp = proxy_case_inputs(*case)
    T, tol_T = proxy_forward_ref(inp["query"], inp["proxies"], inp["bias"])
    return inp, (T, tol_T), proxy_grad_ref(inp["grad_out"], T, tol_T, inp["query"], inp["proxies"])


def check_case_conditions(name, fwd, planted_dup=False):
    """The conditions on the inputs (float64 only): outside the planted duplicates no (pixel, object) pair has a best / runner-up gap under
    GAP_FACTOR x the forward distance bound of its winner; at least half of the live pairs have T in (0.05, 0.95)."""
    live = fwd["arg"] >= 0
    if not live.any():
        return
    if not planted_dup:
        margin = fwd["gap"][live] / np.maximum(fwd["e_best"][live], 1e-300)
        assert margin.min() >= GAP_FACTOR, f"{name}: a best / runner-up gap is only {margin.min():.1f} x the forward bound"
    T = fwd["T"][live]
    assert ((T > 0.05) & (T < 0.95)).mean() >= 0.5, f"{name}: only {((T > 0.05) & (T < 0.95)).mean():.2f} of the live outputs are unsaturated"


def check_proxy_conditions(name, T):
    """The k = 1 proxy path has no argmin; what is left of the conditions: at least half of the outputs have T in (0.05, 0.95)."""
    live = (T > 0.05) & (T < 0.95)
    assert live.mean() >= 0.5, f"{name}: only {live.mean():.2f} of the outputs are unsaturated"


# ------------------------------------------------------------------------------------------ fixtures
FIXTURES_DENSE = ("match_grad_dense_C100_O3", "match_grad_dense_C36_O4", "match_grad_dense_C4_O2", "match_grad_dense_C128_O17",
                  "match_grad_atrous2", "match_grad_atrous2_objpix", "match_grad_absent")
FIXTURE_UNLABELLED = "match_grad_unlabelled"
FIXTURE_PROXY = "match_grad_proxy"


def twin_labels(labels, rate, obj_pix):
    """AEM:648-657 on a copy: with atrous_rate > 1 an object with more than obj_pix rate^2 labelled pixels keeps its label on the
    rate-strided grid only."""
    lab = np.asarray(labels, np.float64).copy()
    if rate > 1:
        h, w, _ = lab.shape
        on = (np.arange(h) % rate == 0)[:, None] & (np.arange(w) % rate == 0)[None, :]
        big = lab.sum((0, 1)) > obj_pix * rate * rate
        lab[:, :, big] = lab[:, :, big] * on[:, :, None]
    return lab


def fixture_ref(fx):
    """The numpy reference on a recorded dense fixture -> (fwd, grad) with grad_out = the recorded weight."""
    h, w, C = fx["in_query"].shape
    n_obj = fx["in_labels"].shape[2]
    lab = twin_labels(fx["in_labels"], int(fx["atrous_rate"]), int(fx["atrous_obj_pixel_num"])).reshape(-1, n_obj)
    q, p = fx["in_query"].reshape(-1, C).astype(f32), fx["in_ref"].reshape(-1, C).astype(f32)
    fwd = dense_forward_ref(q, p, lab, fx["in_bias"])
    go = fx["weight"].reshape(h * w, n_obj).T
    return fwd, dense_grad_ref(go, fwd["T"], fwd["tol_T"], fwd["arg"], q, p)


def fixture_proxy_ref(fx):
    h, w, C = fx["in_query"].shape
    n_obj = fx["in_ref"].shape[0]
    q, p = fx["in_query"].reshape(-1, C).astype(f32), fx["in_ref"].astype(f32)
    T, tol_T = proxy_forward_ref(q, p, fx["in_bias"])
    return (T, tol_T), proxy_grad_ref(fx["weight"].reshape(h * w, n_obj).T, T, tol_T, q, p)
