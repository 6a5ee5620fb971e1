"""Float64 references, derived bounds, cases and inputs for the training-time cluster matching (csrc/cluster_grad.hip):
aoc_proxy_set_match_argmin, aoc_proxy_set_match_grad and aoc_centroid_avg_grad, and their composition in aoc_amd.cluster_train.  Shared
by test_cluster_grad_host.py (no GPU) and test_gpu_cluster_grad.py.  Pure numpy; the library is not imported here.  U, gamma, the gate
g and the check / ratio helpers are those of float64_bounds.py / match_grad_bounds.py.

Forward (set_forward_ref).  The kernel repeats proxy_corr_min_kernel term by term: d = fl(fl(q2^ + p2^) - 2 acc^), every sum of C products
within gamma(C) x (the sum of the terms' magnitudes) whatever its order (local_match_bounds.pair_distances' derivation).  Here the proxies
may carry an error of their own, |p^ - p| <= e_p per channel (the fp32 means of aoc_build_proxies against the float64 means of the
reference: a sum of n rows and one division, e_p = gamma(n + 1) sum |x| / n).  With a = |q - p|:
    dD  = sum_c (2 a_c e_p_c + e_p_c^2)                       the distance moves by at most this
    the magnitudes the roundings act on are evaluated at |p| + e_p:  e_q2 = gamma(C) |q|^2, e_p2 = gamma(C) |p + e_p|^2 (or, for a norm
    that is supplied, |float64(supplied) - |p|^2| evaluated), e_dot = gamma(C) sum |q_c| (|p_c| + e_p_c),
    e_s = e_q2 + e_p2 + U (|q|^2 + |p + e_p|^2 + e_q2 + e_p2),  pre = e_s + 2 e_dot,  E = pre + U (|D| + dD + pre) + dD.
The minimum over a set and the transform are global_match_bounds.min_with_bound / transform_ref.  arg = the first minimum in ascending
slot order (np.argmin over the live slots), -1 for a set without a live slot; gap = float64 runner-up minus best.

Backward of the set minimum (set_grad_ref), read off cluster_grad.hip (every product, sum and difference rounds once: -ffp-contract=off).
g and e_g: match_grad_bounds.gate_ref (cg_gate is mg_gate's expression).
  grad_query   cg_query_grad_kernel: acc += fl(fl(2 g^) fl(q - p^*)) over the sets, ascending: a term's bound is match_grad_bounds'
               _term_err with a -> a + e_p plus 2 |g| e_p for the moved operand; a term passes through at most n_set additions.
  grad_proxies cg_partial_kernel adds fl(g^ q) of a chunk's pixels in order (a chunk holds per = ceil(m / n_chunk) pixels,
               n_chunk = min(128, ceil(m / 32))), cg_rows_kernel the chunks of every set that holds the row: a term of S = sum g q and of
               G = sum g passes through at most per + n_chunk n_sets(r) + n_sets(r) additions.  Then fl(2 fl(fl(p^ G^) - S^)).
  grad_bias    the slot sums (per + n_chunk additions) added over the slots of the sets that name the element: + sum of those set sizes.
The bound covers one launch (at most 64 sets); a call with more adds the launches' results, one more rounding each
(set_grad_ref_launches).

Backward of centroid_avg (centroid_grad_ref): a term is fl(x^ / n), n exact: e_x / n + U (|x| / n + e_x / n); a row adds at most n_seg.

No measured number goes into a bound.  The gradients depend on arg discontinuously, so the tests demand arg == the float64 argmin and the
host test demands that no case has a best / runner-up gap under GAP_FACTOR x the forward distance bound of its winner.
"""
import functools
import zlib

import numpy as np

from float64_bounds import U, gamma
from global_match_bounds import PAD, min_with_bound, transform_ref
from match_grad_bounds import GAP_FACTOR, check, gate_ref, ratio, twin_labels  # noqa: F401  (re-exported for the tests)

f32 = np.float32
CG_SETS, CG_MAX_CHUNKS, CG_CHUNK_MIN = 64, 128, 32
MAX_CLUSTERS = 64


def n_chunks(m):
    return int(min(CG_MAX_CHUNKS, max(1, -(-m // CG_CHUNK_MIN))))


def align256(x):
    return -(-int(x) // 256) * 256


def set_grad_workspace_bytes(m, C, n_slot):
    """The formula include/aoc_hip.h states for aoc_proxy_set_match_grad."""
    return align256(n_slot * n_chunks(m) * (C + 1) * 4 + 16) + align256(n_slot * 4 + 16)


def centroid_grad_workspace_bytes(n_seg, kmax):
    return align256(n_seg * kmax * 4 + 16)


# ------------------------------------------------------------------------------------------ forward with argmin
def pair_distances_ep(q, p, e_p=None, e_p2=None):
    """q [m, C], p [n, C] float64 (exact operands) -> (D, E) [m, n]: module docstring.  e_p [n, C] or None; e_p2 [n] replaces the derived
    norm error where given (a supplied norm)."""
    C = q.shape[1]
    g = gamma(max(C, 1))
    exact = e_p is None
    e_p = np.zeros_like(p) if exact else e_p
    pm = np.abs(p) + e_p
    q2, p2, p2m = (q * q).sum(1), (p * p).sum(1), (pm * pm).sum(1)
    D = (q2[:, None] + p2[None, :]) - 2.0 * (q @ p.T)
    dD = np.zeros_like(D)
    if not exact:
        for j in np.nonzero(e_p.any(1))[0]:
            dD[:, j] = (2.0 * np.abs(q - p[j]) * e_p[j] + e_p[j] * e_p[j]).sum(1)
    e_q2 = g * q2
    e_p2 = g * p2m if e_p2 is None else e_p2
    e_dot = g * (np.abs(q) @ pm.T)
    e_s = e_q2[:, None] + e_p2[None, :] + U * (q2[:, None] + p2m[None, :] + e_q2[:, None] + e_p2[None, :])
    pre = e_s + 2.0 * e_dot
    return D, pre + U * (np.abs(D) + dD + pre) + dD


def set_forward_ref(query, proxies, sqnorm, set_begin, set_size, set_bias, e_p=None, live=None):
    """query [m, C]; proxies [n_proxy, C] (float32, or float64 with e_p); sqnorm [n_proxy] float32 (+inf = ignore) or None; set_bias
    [n_set] or None.  live [n_proxy] bool instead of sqnorm: the kernel gets norms that are fp32 sums of the proxies' squares (the derived
    gamma(C) |p|^2) with +inf marks where live is False.
    -> dict(T, tol_T, raw, tol_raw [n_set, m]; arg [n_set, m] int64 (slot within the set, -1); gap, e_best [n_set, m]).  gap = float64
    runner-up minus best among the slots whose proxy differs from the winner's: bit-equal proxies (duplicated code-book entries) tie exactly,
    the lowest slot wins in the kernel and in np.argmin alike, and whichever wins the value and every gradient are the same."""
    q, p = np.asarray(query, np.float64), np.asarray(proxies, np.float64)
    n_proxy, m, n_set = p.shape[0], q.shape[0], len(set_size)
    e_p2 = None
    if live is None:
        live = np.ones(n_proxy, bool) if sqnorm is None else np.isfinite(sqnorm)
        if sqnorm is not None:
            e_p2 = np.where(live, np.abs(np.where(live, sqnorm, 0).astype(np.float64) - (p * p).sum(1)), 0.0)
    D, E = pair_distances_ep(q, p, e_p, e_p2)
    raw, tol, gap, e_best = (np.empty((n_set, m)) for _ in range(4))
    arg = np.empty((n_set, m), np.int64)
    ar = np.arange(m)
    for s, (b, n) in enumerate(zip(set_begin, set_size)):
        cols = np.arange(b, b + n)
        cols = cols[live[cols]]
        raw[s], tol[s] = min_with_bound(D[:, cols], E[:, cols], PAD)
        if cols.size == 0:
            arg[s], gap[s], e_best[s] = -1, np.inf, 0.0
            continue
        j = D[:, cols].argmin(1)
        arg[s], e_best[s], gap[s] = cols[j] - b, E[:, cols][ar, j], np.inf
        distinct = cols[np.sort(np.unique(p[cols], axis=0, return_index=True)[1])]      # the first of every group of bit-equal proxies
        if distinct.size > 1:
            part = np.partition(D[:, distinct], 1, axis=1)
            gap[s] = part[:, 1] - part[:, 0]
    T, tol_T = transform_ref(raw, tol, None if set_bias is None else np.asarray(set_bias, np.float64))
    return dict(T=T, tol_T=tol_T, raw=raw, tol_raw=tol, arg=arg, gap=gap, e_best=e_best)


# ------------------------------------------------------------------------------------------ gradients and their bounds
def _term_err(g, e_g, a, e_a):
    """The bound of fl(fl(2 g^) fl(x - y^)) with a = |x - y| and |y^ - y| <= e_a."""
    am = a + e_a
    e = 2.0 * e_g * am * (1.0 + U) + 2.0 * np.abs(g) * am * U + 2.0 * np.abs(g) * e_a
    return e + U * (2.0 * np.abs(g) * a + e)


def set_grad_ref(go, T, tol_T, arg, query, proxies, set_begin, set_size, set_bias_index, n_bias, e_p=None, e_go=0.0):
    """go, T, tol_T, arg [n_set, m]; query [m, C]; proxies [n_proxy, C].  -> dict(grad_query, tol_query [m, C]; grad_proxies, tol_proxies
    [n_proxy, C]; grad_bias, tol_bias [n_bias]; g, e_g [n_set, m]; chosen [n_proxy]: pairs per proxy row)."""
    q, p = np.asarray(query, np.float64), np.asarray(proxies, np.float64)
    n_set, m = T.shape
    n_proxy, C = p.shape
    assert n_set <= CG_SETS, "the bound covers one launch"
    e_p = np.zeros_like(p) if e_p is None else e_p
    g, e_g = gate_ref(go, T, tol_T, e_go)
    nch = n_chunks(m)
    per = -(-m // nch)
    gq, tq, mq = np.zeros((m, C)), np.zeros((m, C)), np.zeros((m, C))
    S, eS, mS = np.zeros((n_proxy, C)), np.zeros((n_proxy, C)), np.zeros((n_proxy, C))
    G, eG, mG = np.zeros(n_proxy), np.zeros(n_proxy), np.zeros(n_proxy)
    chosen = np.zeros(n_proxy, np.int64)
    sets_of = np.zeros(n_proxy, np.int64)
    gb, tb, mb, kb = np.zeros(n_bias), np.zeros(n_bias), np.zeros(n_bias), np.zeros(n_bias)
    for s in range(n_set):
        b, n = int(set_begin[s]), int(set_size[s])
        sets_of[b:b + n] += 1
        kb[set_bias_index[s]] += n
        live = (arg[s] >= 0) & (arg[s] < n)
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            continue
        r = b + arg[s, idx]
        gs, es = g[s, idx], e_g[s, idx]
        diff = q[idx] - p[r]
        term = 2.0 * gs[:, None] * diff
        e = _term_err(gs[:, None], es[:, None], np.abs(diff), e_p[r])
        gq[idx] += term
        tq[idx] += e
        mq[idx] += np.abs(term) + e
        t = gs[:, None] * q[idx]                                             # fl(g^ q): e_g |q| and one rounding
        et = es[:, None] * np.abs(q[idx])
        et = et + U * (np.abs(t) + et)
        np.add.at(S, r, t)
        np.add.at(eS, r, et)
        np.add.at(mS, r, np.abs(t) + et)
        np.add.at(G, r, gs)
        np.add.at(eG, r, es)
        np.add.at(mG, r, np.abs(gs) + es)
        np.add.at(chosen, r, 1)
        bi = int(set_bias_index[s])
        gb[bi] += gs.sum()
        tb[bi] += es.sum()
        mb[bi] += (np.abs(gs) + es).sum()
    tq = tq + gamma(max(n_set, 1)) * mq
    k_row = per + nch * np.maximum(sets_of, 1) + sets_of
    eS = eS + gamma(k_row)[:, None] * mS
    eG = eG + gamma(k_row) * mG
    pG = p * G[:, None]
    e_pG = np.abs(p) * eG[:, None] + e_p * (np.abs(G) + eG)[:, None]
    e_pG = e_pG + U * (np.abs(pG) + e_pG)
    d = pG - S
    e_d = e_pG + eS
    e_d = e_d + U * (np.abs(d) + e_d)
    tb = tb + gamma(per + nch + kb) * mb
    return dict(grad_query=gq, tol_query=tq, grad_proxies=2.0 * d, tol_proxies=2.0 * e_d, grad_bias=gb, tol_bias=tb, g=g, e_g=e_g, chosen=chosen)


def set_grad_ref_launches(go, T, tol_T, arg, query, proxies, set_begin, set_size, set_bias_index, n_bias):
    """set_grad_ref for a call with more than CG_SETS sets: the entry runs one launch per CG_SETS sets, in set order, and every launch after
    the first adds its result to what the output holds -- one more rounding per launch and element.  -> set_grad_ref's gradients and bounds."""
    out = None
    for s0 in range(0, T.shape[0], CG_SETS):
        sl = slice(s0, s0 + CG_SETS)
        r = set_grad_ref(go[sl], T[sl], tol_T[sl], arg[sl], query, proxies, set_begin[sl], set_size[sl], set_bias_index[sl], n_bias)
        if out is None:
            out = {k: r[k] for k in ("grad_query", "tol_query", "grad_proxies", "tol_proxies", "grad_bias", "tol_bias", "chosen")}
            continue
        for k in ("query", "proxies", "bias"):
            # grad_proxies and grad_bias: the launch's own value, then one addition.  grad_query: the kernel goes on adding the launch's
            # terms to what the row holds, so the earlier launches' sum passes through one more addition per set of this launch
            more = gamma(T[sl].shape[0]) * (np.abs(out["grad_" + k]) + out["tol_" + k]) if k == "query" else 0.0
            v, t = out["grad_" + k] + r["grad_" + k], out["tol_" + k] + r["tol_" + k] + more
            out["grad_" + k], out["tol_" + k] = v, t + U * (np.abs(v) + t)
        out["chosen"] = out["chosen"] + r["chosen"]
    return out


def centroid_grad_ref(grad_proxies, tol_proxies, fg_rows, n_fg, seg_offsets, seg_k, labels, pool_rows):
    """grad_proxies, tol_proxies [n_seg, 2, kmax, C] float64 (only [:, 1] is read); the rest as aoc_centroid_avg_grad takes them (host
    arrays).  -> (grad_pool, tol_pool [pool_rows, C], n_from [pool_rows]: how many segments gave the row a non-zero gradient)."""
    n_seg, _, kmax, C = grad_proxies.shape
    gp, tp, mp = np.zeros((pool_rows, C)), np.zeros((pool_rows, C)), np.zeros((pool_rows, C))
    n_from = np.zeros(pool_rows, np.int64)
    for s in range(n_seg):
        o0, o1 = int(seg_offsets[s]), int(seg_offsets[s + 1])
        lab = np.asarray(labels[o0:o1])
        cnt = np.bincount(lab[(lab >= 0) & (lab < kmax)], minlength=kmax)
        for pos in range(min(o1 - o0, int(n_fg))):
            j = int(lab[pos])
            if j < 0 or j >= kmax or j >= int(seg_k[s]) or cnt[j] < 1:
                continue
            x, ex = grad_proxies[s, 1, j] / cnt[j], tol_proxies[s, 1, j] / cnt[j]
            ex = ex + U * (np.abs(x) + ex)
            row = int(fg_rows[pos])
            gp[row] += x
            tp[row] += ex
            mp[row] += np.abs(x) + ex
            n_from[row] += bool(np.any(x != 0))
    return gp, tp + gamma(max(n_seg, 1)) * mp, n_from


# ------------------------------------------------------------------------------------------ the whole function on numpy arrays
def cluster_state(pool, labels_flat, levels, km_labels, km_centroids):
    """The cluster state of matching.cluster_proxies in float64 from given assignments: pool [n, C] float32, labels_flat [n, O], levels
    [L]; km_labels / km_centroids: per segment (level-major, then object) the labels [n_o] and the code book [K, C] float32, None for
    an object without a row.  Set 1 follows the reference's indexing (AEM:280): cluster j averages the rows fg[p] of the GLOBAL kept-row
    array over the segment-local p with label j.  -> dict(proxies, e_p [S, 2, kmax, C] float64; live [S, 2, kmax]; fg_rows, n_fg,
    seg_offsets [S + 1], seg_k [S], labels (packed), counts [O]) -- None when no row is kept."""
    lab = np.asarray(labels_flat, np.float64)
    p64 = np.asarray(pool, f32).astype(np.float64)
    n_obj, C = lab.shape[1], p64.shape[1]
    fg = np.nonzero(lab.sum(1) > 0.9)[0]
    if fg.size == 0:
        return None
    counts = [int((lab[fg, o] > 0.9).sum()) for o in range(n_obj)]
    kmax, S = max(levels), len(levels) * n_obj
    proxies, e_p = np.zeros((S, 2, kmax, C)), np.zeros((S, 2, kmax, C))
    live = np.zeros((S, 2, kmax), bool)
    seg_k, offs, packed = [], [0], []
    for li, k in enumerate(levels):
        for o in range(n_obj):
            s = li * n_obj + o
            k = min(k, counts[o])                                            # AEM:268: sticky within a call
            seg_k.append(k)
            if k == 0:
                offs.append(offs[-1])
                continue
            l, c = np.asarray(km_labels[s]), np.asarray(km_centroids[s], f32).astype(np.float64)
            assert l.size == counts[o] and c.shape == (k, C)
            proxies[s, 0, :k], live[s, 0, :k] = c, True
            for j in np.unique(l):
                rows = p64[fg[np.nonzero(l == j)[0]]]
                proxies[s, 1, j] = rows.sum(0) / rows.shape[0]
                e_p[s, 1, j] = gamma(rows.shape[0] + 1) * np.abs(rows).sum(0) / rows.shape[0]
                live[s, 1, j] = True
            packed.append(l.astype(np.int64))
            offs.append(offs[-1] + l.size)
    return dict(proxies=proxies, e_p=e_p, live=live, fg_rows=fg, n_fg=fg.size, seg_offsets=np.asarray(offs), seg_k=np.asarray(seg_k),
                labels=np.concatenate(packed) if packed else np.zeros(0, np.int64), counts=counts, kmax=kmax)


def plane_sets(levels, n_obj, kmax, m):
    """cluster_train._plane_sets restated: (level l, object o, set f) -> proxy rows, size, plane offset, object."""
    L = len(levels)
    begin, size, off, obj = [], [], [], []
    for l, k in enumerate(levels):
        for o in range(n_obj):
            for f in range(2):
                begin.append(((l * n_obj + o) * 2 + f) * kmax)
                size.append(min(k, kmax))
                off.append((o * 2 * L + 2 * l + f) * m)
                obj.append(o)
    return begin, size, off, obj


def cluster_match_ref(query, pool, labels_flat, bias, levels, km_labels, km_centroids, grad_planes=None, e_go=0.0):
    """The function of cluster_train on flat arrays: query [m, C], pool [n, C] float32, labels_flat [n, O], bias [O]; grad_planes
    [O * 2L, m] in plane order (o 2L + 2l + f) or None.  -> dict(planes, tol_planes [O * 2L, m], fwd, state, and with grad_planes:
    grad_query, tol_query, grad_pool, tol_pool, grad_bias, tol_bias, grad_proxies, n_from); planes only (ones) when nothing is labelled."""
    q = np.asarray(query, f32).astype(np.float64)
    m, C = q.shape
    n_obj, L = labels_flat.shape[1], len(levels)
    st = cluster_state(pool, labels_flat, levels, km_labels, km_centroids)
    if st is None:
        return dict(planes=None, state=None)
    kmax = st["kmax"]
    begin, size, off, obj = plane_sets(levels, n_obj, kmax, m)
    order = [o // m for o in off]                                            # set -> plane
    P, EP = st["proxies"].reshape(-1, C), st["e_p"].reshape(-1, C)
    fwd = set_forward_ref(q, P, None, begin, size, np.asarray(bias, np.float64)[obj], EP, live=st["live"].reshape(-1))
    planes, tol = np.empty((len(begin), m)), np.empty((len(begin), m))
    planes[order], tol[order] = fwd["T"], fwd["tol_T"]
    out = dict(planes=planes, tol_planes=tol, fwd=fwd, state=st, sets=(begin, size, off, obj), order=order)
    if grad_planes is not None:
        go = np.asarray(grad_planes, np.float64)[order]
        ego = np.broadcast_to(np.asarray(e_go, np.float64), (len(begin), m))[order] if np.ndim(e_go) else e_go
        gr = set_grad_ref(go, fwd["T"], fwd["tol_T"], fwd["arg"], q, P, begin, size, obj, n_obj, EP, ego)
        S = L * n_obj
        gpool, tpool, n_from = centroid_grad_ref(gr["grad_proxies"].reshape(S, 2, kmax, C), gr["tol_proxies"].reshape(S, 2, kmax, C), st["fg_rows"],
                                                 st["n_fg"], st["seg_offsets"], st["seg_k"], st["labels"], pool.shape[0])
        out.update(grad_query=gr["grad_query"], tol_query=gr["tol_query"], grad_pool=gpool, tol_pool=tpool, grad_bias=gr["grad_bias"],
                   tol_bias=gr["tol_bias"], grad_proxies=gr["grad_proxies"], chosen=gr["chosen"], n_from=n_from)
    return out


# ------------------------------------------------------------------------------------------ fixtures
FIXTURES = ("cluster_grad_C36_O3", "cluster_grad_C100_O4_bias", "cluster_grad_absent", "cluster_grad_atrous2", "cluster_grad_dup_empty")
FIXTURE_UNLABELLED = "cluster_grad_unlabelled"


def fixture_km(fx):
    """The km log of a fixture -> (labels, centroids, rows) per object (None for an object without a row): kmeans2 is called for the
    objects whose sticky K is not 0, in ascending order."""
    n_obj = fx["in_labels"].shape[2]
    lab = twin_labels(fx["in_labels"], int(fx["atrous_rate"]), int(fx["atrous_obj_pixel_num"])).reshape(-1, n_obj)
    kept = lab.sum(1) > 0.9
    labels, cents, rows = [], [], []
    i, k = 0, int(fx["cluster_num"])
    for o in range(n_obj):
        k = min(k, int((lab[kept, o] > 0.9).sum()))                          # AEM:268: sticky, so the objects after an absent one have no call either
        if k == 0:
            labels.append(None), cents.append(None), rows.append(None)
            continue
        labels.append(fx[f"km{i}_labels"]), cents.append(fx[f"km{i}_centroid"]), rows.append(fx[f"km{i}_rows"])
        i += 1
    assert i == int(fx["km_calls"])
    return labels, cents, rows


@functools.lru_cache(maxsize=None)
def _fixture_ref_cached(name):
    from conftest import load_golden
    return fixture_ref(load_golden(name))


def fixture_ref_by_name(name):
    """fixture_ref of a committed fixture, computed once.  Treat as read-only."""
    return _fixture_ref_cached(name)


def fixture_ref(fx):
    """The numpy reference on a recorded fixture (ori_size None) with grad_out = the recorded weight -> cluster_match_ref's dict plus
    out [1, h, w, O, 2], tol_out and grad_ref / tol_ref [h, w, C] (the pool is the whole map)."""
    h, w, C = fx["in_query"].shape
    n_obj = fx["in_labels"].shape[2]
    lab = twin_labels(fx["in_labels"], int(fx["atrous_rate"]), int(fx["atrous_obj_pixel_num"])).reshape(-1, n_obj)
    q, p = fx["in_query"].reshape(-1, C).astype(f32), fx["in_ref"].reshape(-1, C).astype(f32)
    if not (lab.sum(1) > 0.9).any():
        return dict(out=np.ones((1, h, w, n_obj, 2)), planes=None, state=None)
    km_labels, km_cents, _ = fixture_km(fx)
    go = fx["weight"].reshape(h * w, n_obj * 2).T                            # [1, h, w, O, 2] -> planes o * 2 + f
    ref = cluster_match_ref(q, p, lab, fx["in_bias"], [int(fx["cluster_num"])], km_labels, km_cents, go)
    ref["out"] = ref["planes"].T.reshape(1, h, w, n_obj, 2)
    ref["tol_out"] = ref["tol_planes"].T.reshape(1, h, w, n_obj, 2)
    ref["grad_ref"], ref["tol_ref"] = ref["grad_pool"].reshape(h, w, C), ref["tol_pool"].reshape(h, w, C)
    return ref


def check_fixture_conditions(name, fx, ref):
    """The conditions of a gradient fixture, on the recorded inputs alone (float64)."""
    fwd, st = ref["fwd"], ref["state"]
    live = fwd["arg"] >= 0
    margin = fwd["gap"][live] / np.maximum(fwd["e_best"][live], 1e-300)
    assert margin.min() >= GAP_FACTOR, f"{name}: a best / runner-up gap is only {margin.min():.1f} x the forward bound"
    T = ref["out"]
    assert ((T > 0.05) & (T < 0.95)).mean() >= 0.5, f"{name}: only {((T > 0.05) & (T < 0.95)).mean():.2f} of the outputs are unsaturated"
    begin, size, off, obj = ref["sets"]
    present = [o for o in range(len(st["counts"])) if st["seg_k"][o] > 0]
    for s in range(len(begin)):
        if s % 2 == 1 and obj[s] in present and st["seg_k"][obj[s]] > 1:
            assert np.unique(fwd["arg"][s]).size >= 2, f"{name}: one slot of object {obj[s]}'s set 1 wins everywhere"
    if len(present) >= 2:
        assert (ref["n_from"] >= 2).any(), f"{name}: no pool row receives gradient from two segments"


# ------------------------------------------------------------------------------------------ cases of the entry points
def _rng(name):
    return np.random.RandomState(zlib.crc32(("cluster_grad/" + name).encode()) & 0x7FFFFFFF)


ARGMIN_C = (4, 36, 100, 128, 132, 256)
ARGMIN_M = (1, 63, 64, 65, 257)
ARGMIN_SIZES = (1, 2, 16, 17, 33, 64)
TIE_SLOTS = ((1, 3), (2, 18), (31, 32))


def argmin_case_inputs(C, m, n_extra_sets=0, marks=True, ties=False):
    """Sets of every size of ARGMIN_SIZES, an empty set, an all-ignored set (size 5) and n_extra_sets more of size 3; proxies scattered
    around the query's cloud so that distances are 0.4 .. 3.  marks: one slot in five of the sets of size >= 16 carries a +inf norm.
    ties: sets of size 64 with two bit-equal proxies at TIE_SLOTS, the pair being the nearest of every pixel.
    -> dict(query, proxies, sqnorm (float32, the fp32 sum of squares, +inf marks), begin, size, bias [n_set] float32)."""
    rng = _rng(f"argmin/{C}/{m}/{n_extra_sets}/{int(marks)}/{int(ties)}")
    s = 0.7 / np.sqrt(C)
    query = (s * rng.standard_normal((m, C))).astype(f32)
    sizes = [64] * len(TIE_SLOTS) if ties else list(ARGMIN_SIZES) + [0, 5] + [3] * n_extra_sets
    begin, pos = [], 2                                                       # two rows outside every set in front
    for n in sizes:
        begin.append(pos)
        pos += n + 1                                                         # and one between the sets
    proxies = (s * rng.standard_normal((pos, C))).astype(f32)
    sq = (proxies.astype(f32) ** 2).sum(1, dtype=f32)
    if ties:
        proxies *= f32(4.0)                                                  # everything else far out
        for b, (lo, hi) in zip(begin, TIE_SLOTS):
            proxies[b + lo] = (0.1 * s * rng.standard_normal(C)).astype(f32)     # near the centre of the cloud: nearest of every pixel
            proxies[b + hi] = proxies[b + lo]
        sq = (proxies ** 2).sum(1, dtype=f32)
    elif marks:
        for b, n in zip(begin, sizes):
            if n >= 16:
                sq[b + rng.permutation(n)[:n // 5]] = np.inf
        sq[begin[len(ARGMIN_SIZES) + 1]:begin[len(ARGMIN_SIZES) + 1] + 5] = np.inf     # the all-ignored set
    bias = (0.3 * rng.standard_normal(len(sizes))).astype(f32)
    return dict(query=query, proxies=proxies, sqnorm=sq, begin=begin, size=sizes, bias=bias)


def redraw_near_ties(inp, fwd_of, rng, scale):
    """Draws the query pixels that sit within GAP_FACTOR x the forward bound of a tie again until none is left."""
    for _ in range(50):
        fwd = fwd_of(inp)
        near = ((fwd["gap"] < 1.2 * GAP_FACTOR * fwd["e_best"]) & (fwd["arg"] >= 0)).any(0)
        if not near.any():
            return fwd
        inp["query"][near] = (scale * rng.standard_normal((int(near.sum()), inp["query"].shape[1]))).astype(f32)
    raise AssertionError("near-ties remain after 50 redraws")


@functools.lru_cache(maxsize=None)
def argmin_case_ref(C, m, n_extra_sets=0, marks=True, use_norms=True):
    """-> (inputs, forward reference) of an argmin case, gap-checked (near-tie pixels drawn again).  Treat as read-only."""
    inp = argmin_case_inputs(C, m, n_extra_sets, marks)
    rng = _rng(f"argmin-redraw/{C}/{m}")
    sq = inp["sqnorm"] if use_norms else None
    fwd = redraw_near_ties(inp, lambda i: set_forward_ref(i["query"], i["proxies"], sq, i["begin"], i["size"], i["bias"]), rng, 0.7 / np.sqrt(C))
    return inp, fwd


GRAD_C = ARGMIN_C
GRAD_M = ARGMIN_M
GRAD_OBJECTS = (1, 3, 17, 30)


def grad_case_inputs(C, m, n_obj, kind="general"):
    """n_obj objects with two sets each (sizes 16 and 5; the second object's second set is all-ignored: an arg = -1 column), two proxy rows
    outside every set.  kind "hot": every set has size 3 and slot 1 sits in the middle of the query cloud (chosen by all m pixels), the
    other slots far away (chosen by nobody).  -> argmin_case_inputs' dict plus bias_index [n_set], n_bias, bias [n_bias], grad_out."""
    rng = _rng(f"grad/{C}/{m}/{n_obj}/{kind}")
    s = 0.7 / np.sqrt(C)
    query = (s * rng.standard_normal((m, C))).astype(f32)
    sizes = [3, 3] * n_obj if kind == "hot" else [16, 5] * n_obj
    begin, pos = [], 2
    for n in sizes:
        begin.append(pos)
        pos += n
    proxies = (s * rng.standard_normal((pos, C))).astype(f32)
    if kind == "hot":
        for b in begin:
            proxies[b] = (6.0 * s * rng.standard_normal(C)).astype(f32)
            proxies[b + 1] = (0.1 * s * rng.standard_normal(C)).astype(f32)
            proxies[b + 2] = (6.0 * s * rng.standard_normal(C)).astype(f32)
    sq = (proxies ** 2).sum(1, dtype=f32)
    if kind != "hot" and n_obj > 1:
        sq[begin[3]:begin[3] + sizes[3]] = np.inf
    bias_index = [s_ // 2 for s_ in range(len(sizes))]
    bias = (0.3 * rng.standard_normal(n_obj)).astype(f32)
    grad_out = rng.standard_normal((len(sizes), m)).astype(f32)
    return dict(query=query, proxies=proxies, sqnorm=sq, begin=begin, size=sizes, bias_index=bias_index, n_bias=n_obj, bias=bias, grad_out=grad_out)


@functools.lru_cache(maxsize=None)
def grad_case_ref(C, m, n_obj, kind="general"):
    """-> (inputs, forward reference, T32, gradient reference).  The gradient entry gets T32, the float32 rounding of the reference's T, and
    the reference's arg, so for it T is T32 exactly (no forward error) and the reference is taken at T32."""
    inp = grad_case_inputs(C, m, n_obj, kind)
    rng = _rng(f"grad-redraw/{C}/{m}/{n_obj}/{kind}")
    set_bias = inp["bias"][inp["bias_index"]]
    fwd = redraw_near_ties(inp, lambda i: set_forward_ref(i["query"], i["proxies"], i["sqnorm"], i["begin"], i["size"], set_bias), rng,
                           0.7 / np.sqrt(C))
    T32 = fwd["T"].astype(f32)
    ref_of = set_grad_ref if len(inp["size"]) <= CG_SETS else set_grad_ref_launches
    grad = ref_of(inp["grad_out"], T32.astype(np.float64), np.zeros_like(fwd["T"]), fwd["arg"], inp["query"], inp["proxies"], inp["begin"],
                  inp["size"], inp["bias_index"], inp["n_bias"])
    return inp, fwd, T32, grad


def pullback_case(levels=1):
    """Segments of 5, 40, 0 and 300 rows (per level) over 345 kept rows of a 400-row pool, kmax 8, seg_k = (5, 8, 0, 6): cluster 3 of the
    last segment is empty.  -> dict(grad_proxies [S, 2, 8, C] float32, fg_rows, n_fg, seg_offsets, seg_k, labels, pool_rows, C)."""
    rng = _rng(f"pullback/{levels}")
    C, kmax, pool_rows, n_fg = 36, 8, 400, 345
    lens, ks = [5, 40, 0, 300] * levels, [5, 8, 0, 6] * levels
    fg_rows = np.sort(rng.permutation(pool_rows)[:n_fg]).astype(np.int32)
    labels, offs = [], [0]
    for n, k in zip(lens, ks):
        l = rng.randint(0, max(k, 1), n)
        if k == 6:
            l[l == 3] = 4                                                    # an empty cluster
        labels.append(l)
        offs.append(offs[-1] + n)
    S = len(lens)
    gp = rng.standard_normal((S, 2, kmax, C)).astype(f32)
    return dict(grad_proxies=gp, fg_rows=fg_rows, n_fg=n_fg, seg_offsets=np.asarray(offs, np.int32), seg_k=np.asarray(ks, np.int32),
                labels=np.concatenate(labels).astype(np.int32), pool_rows=pool_rows, C=C, kmax=kmax)
