"""References and bounds for the training-time front end (csrc/frontend_grad.hip, aoc_amd.frontend_train), shared by
tests/test_frontend_grad_host.py and tests/test_gpu_frontend_grad.py.

Two kinds of reference:

* numpy RESTATEMENTS in float32 of the kernels' stated rules (aoc_fg2bg_grad, aoc_proto_aggregate, aoc_proto_aggregate_grad): the lowest
  (object, channel) among equal minima wins, sums run in ascending object order from the stated first term.  A fixed-order sum of at most O
  float32 terms is reproduced exactly, so the device result must equal them bit for bit.  ``highest`` / ``descending`` switch to the wrong
  rule, so the host test can show that the planted inputs tell the rules apart.
* float64 references with a bound derived from the kernels' float32 expressions (no measured number): a sum of n terms that went through at
  most n additions is within gamma(n) x the sum of the absolute terms; a product or a correctly rounded division adds one U.
  - fg2bg / aggregation gradient on tie-free inputs: the winner element holds a sum of at most O terms, every other element one term or an
    exact copy.
  - pooling gradient: Np and Nn are float32 sums of hw terms (thread t of 256 adds ceil(hw / 256) terms, then 8 tree levels); their error
    moves the quotients gpos / (Np + eps), gneg / (Nn + eps); each term is one product (the negative one also the rounding of 1 - l); the
    2 O terms are added one after the other.
"""
import zlib

import numpy as np

from float64_bounds import U, eps32, gamma
from match_grad_bounds import check, ratio  # noqa: F401  (re-exported for the tests)

f32, f64 = np.float32, np.float64

MAPS = ((1, 1), (5, 7), (13, 9), (31, 33))          # hw = 1, 35, 117, 1023: no multiple of a wave or of a vector of four
MAPS_VEC = ((4, 8), (16, 20))                        # hw = 32, 320: multiples of four -- the 16-byte instantiation of every kernel
OBJECTS = (1, 2, 3, 17, 30)
CHANNELS = (4, 36, 100, 128)
POOL_THREADS = 256


def rng(*key):
    return np.random.RandomState(zlib.crc32(repr(tuple(int(k) for k in key)).encode()))


# ------------------------------------------------------------------------------------------ winners
def _first_min(v, excluded, highest=False):
    """v [n, X], excluded [n, X] bool -> per x the first row (the last with ``highest``) that holds the minimum of the rows not excluded; a
    strict comparison from the first candidate on, so +inf columns resolve like any other.  -1 where every row is excluded."""
    n, X = v.shape
    best, bv = np.full(X, -1), np.zeros(X, v.dtype)
    for r in (range(n - 1, -1, -1) if highest else range(n)):
        take = ~excluded[r] & ((best < 0) | (v[r] < bv))
        best, bv = np.where(take, r, best), np.where(take, v[r], bv)
    return best


def two_lowest(vals, highest=False):
    """vals [n, X] -> (a1, a2): per x the position of the minimum and the position of the minimum among the rows other than a1, among equal
    values the lowest position (``highest``: the wrong rule).  a2 = -1 for n == 1."""
    n, X = vals.shape
    a1 = _first_min(vals, np.zeros((n, X), bool), highest)
    return a1, _first_min(vals, np.arange(n)[:, None] == a1[None, :], highest)


def fg2bg_winners(dis, highest=False):
    """dis [O, c, X] -> (o1, c1, o2, c2): the lowest entry and the lowest entry among the objects other than o1, ties to the lowest (o, c)
    in concatenation order (object-major, AEM:13-19)."""
    O, nc, X = dis.shape
    flat = dis.reshape(O * nc, X)
    a1 = _first_min(flat, np.zeros((O * nc, X), bool), highest)
    o1 = a1 // nc
    a2 = _first_min(flat, (np.arange(O * nc)[:, None] // nc) == o1[None, :], highest)
    return o1, a1 % nc, a2 // nc, a2 % nc


def _ordered_sum(terms, skip, first=None, descending=False):
    """float32 sum over the rows o of terms [O, X] with o != skip[x], in ascending (descending) o, starting from ``first`` (0.0f)."""
    O, X = terms.shape
    acc = np.zeros(X, f32) if first is None else first.astype(f32).copy()
    for o in (range(O - 1, -1, -1) if descending else range(O)):
        acc = np.where(skip != o, (acc + terms[o]).astype(f32), acc)
    return acc


def fg2bg_min_np(dis):
    """aoc_fg2bg_min's values: out[o, x] = min over o' != o and c of dis[o', c, x]."""
    O, nc, X = dis.shape
    per = dis.min(axis=1)
    return np.stack([np.delete(per, o, axis=0).min(axis=0) for o in range(O)])[:, None, :]


def fg2bg_grad_np(grad_out, dis, highest=False, descending=False):
    """aoc_fg2bg_grad restated: grad_out [O, X], dis [O, c, X] float32 -> grad_dis [O, c, X] float32."""
    O, nc, X = dis.shape
    o1, c1, o2, c2 = fg2bg_winners(dis, highest)
    x = np.arange(X)
    gd = np.zeros_like(dis, dtype=f32)
    gd[o2, c2, x] = grad_out[o1, x]
    gd[o1, c1, x] = _ordered_sum(grad_out.astype(f32), o1, None, descending)
    return gd


def fg2bg_grad_tol(grad_out, dis):
    """Bound on |kernel - float64| for tie-free dis: the first winner holds a sum of O - 1 terms started at 0.0f (O - 1 additions)."""
    O, nc, X = dis.shape
    o1, c1, _, _ = fg2bg_winners(dis)
    tol = np.zeros(dis.shape, f64)
    tol[o1, c1, np.arange(X)] = gamma(O - 1) * (np.abs(grad_out.astype(f64)).sum(0) - np.abs(grad_out.astype(f64))[o1, np.arange(X)])
    return tol


# ------------------------------------------------------------------------------------------ aggregation
def channel_layout(n_cluster, n_local, background=True):
    """-> dict of channel begins in the order of aocnet.py:355-358 and n_ch."""
    lay = dict(glob=0, cluster=1, proxy=1 + n_cluster, local=2 + n_cluster, lproxy=2 + n_cluster + n_local, mask=2 + n_cluster + 2 * n_local)
    n_ch = lay["mask"] + 1
    if background:
        lay.update(local_bg=n_ch, global_bg=n_ch + n_local)
        n_ch += n_local + 1
    lay["n_ch"] = n_ch
    return lay


def _others_min(col):
    """col [O, X] -> per object the min over the OTHER objects (one object: its own map, AEM:10-11)."""
    O = col.shape[0]
    if O == 1:
        return col.copy()
    return np.stack([np.delete(col, o, axis=0).min(axis=0) for o in range(O)])


def aggregate_np(glob, cluster, proxy, local, lproxy, prev, background=True):
    """aoc_proto_aggregate restated (values only: a min of float32 values is exact).  Sources [O, k, X], prev [O, X] -> feat [O, n_ch, X]."""
    O, _, X = glob.shape
    lay = channel_layout(cluster.shape[1], local.shape[1], background)
    feat = np.full((O, lay["n_ch"], X), np.nan, f32)
    for name, src in (("glob", glob), ("cluster", cluster), ("proxy", proxy), ("local", local), ("lproxy", lproxy)):
        feat[:, lay[name]:lay[name] + src.shape[1]] = src
    feat[:, lay["mask"]] = prev
    if background:
        for j in range(local.shape[1]):
            feat[:, lay["local_bg"] + j] = _others_min(local[:, j])
        feat[:, lay["global_bg"]] = _others_min(glob[:, 0])
    return feat


def aggregate_torch(src, prev, O, background):
    """aocnet.py:341-358 on plane tensors [O, k, X] under torch autograd (the oracle's foreground2background is AEM:9-23)."""
    import torch
    from oracle import matching as om
    glob, cluster, proxy, local, lproxy = src
    cat = [glob, cluster, proxy, local, lproxy, prev[:, None]]
    if background:
        lbg = om.foreground2background(local.permute(0, 2, 1).unsqueeze(1), O)                   # [O, 1, X, nl], aocnet.py:351-353
        cat += [lbg.squeeze(1).permute(0, 2, 1), om.foreground2background(glob, O)]
    return torch.cat(cat, 1)


def _column_grad(g_fg, g_bg, fg, highest, descending):
    """One foreground column [O, X] with its background column: grad_fg[o'] = g_fg[o'], then + g_bg[o] for winner(o) = o' in ascending o."""
    O, X = fg.shape
    if O == 1:
        return (g_fg + g_bg).astype(f32)
    o1, o2 = two_lowest(fg, highest)
    x = np.arange(X)
    out = g_fg.astype(f32).copy()
    out[o2, x] = (g_fg[o2, x] + g_bg[o1, x]).astype(f32)
    out[o1, x] = _ordered_sum(g_bg.astype(f32), o1, g_fg[o1, x], descending)
    return out


def aggregate_grad_np(grad_feat, feat, n_cluster, n_local, background=True, highest=False, descending=False):
    """aoc_proto_aggregate_grad restated -> (g_global, g_cluster, g_proxy, g_local, g_local_proxy) float32 [O, k, X]."""
    lay = channel_layout(n_cluster, n_local, background)
    take = lambda name, k: grad_feat[:, lay[name]:lay[name] + k].astype(f32).copy()
    g_glob, g_cluster, g_proxy, g_local, g_lproxy = take("glob", 1), take("cluster", n_cluster), take("proxy", 1), take("local", n_local), take("lproxy", n_local)
    if background:
        g_glob[:, 0] = _column_grad(grad_feat[:, lay["glob"]], grad_feat[:, lay["global_bg"]], feat[:, lay["glob"]], highest, descending)
        for j in range(n_local):
            g_local[:, j] = _column_grad(grad_feat[:, lay["local"] + j], grad_feat[:, lay["local_bg"] + j], feat[:, lay["local"] + j], highest, descending)
    return g_glob, g_cluster, g_proxy, g_local, g_lproxy


def aggregate_grad_tol(grad_feat, n_cluster, n_local, background=True):
    """Bound on |kernel - float64| for tie-free foreground columns: an element is a sum of at most O terms (its foreground gradient and the
    background gradients of the others): gamma(O - 1) x the absolute terms, wherever the winners are; copies are exact."""
    lay = channel_layout(n_cluster, n_local, background)
    a = np.abs(grad_feat.astype(f64))
    O = a.shape[0]
    zeros = lambda k: np.zeros((O, k, a.shape[2]), f64)
    t_glob, t_local = zeros(1), zeros(n_local)
    if background:
        g = gamma(max(O - 1, 1))
        t_glob[:, 0] = g * (a[:, lay["glob"]] + a[:, lay["global_bg"]].sum(0)[None])
        for j in range(n_local):
            t_local[:, j] = g * (a[:, lay["local"] + j] + a[:, lay["local_bg"] + j].sum(0)[None])
    return t_glob, zeros(n_cluster), zeros(1), t_local, zeros(n_local)


def aggregate_case(h, w, O, n_cluster, n_local, seed, ties=False):
    """Five sources in (-1, 1] like the matchers' T, a one-hot previous label, a cotangent.  ``ties``: saturated stretches (T == 1.0f, what an
    unlabelled object gives) and copied columns, so that equal minima occur for two, three and all objects."""
    rs = rng(h, w, O, n_cluster, n_local, seed)
    X = h * w
    mk = lambda k: np.tanh(rs.standard_normal((O, k, X))).astype(f32)
    src = [mk(1), mk(n_cluster), mk(1), mk(n_local), mk(n_local)]
    if ties:
        for s in (0, 3):
            a = src[s]
            a[:, :, ::5] = 1.0                                    # every object saturated
            if O >= 2:
                a[1, :, 1::5] = a[0, :, 1::5]                     # two equal, possibly the minimum
                a[:2, :, 2::5] = -0.75                            # two equal minima
            if O >= 3:
                a[:3, :, 3::5] = -0.5                             # a three-way tie
                a[O - 1, :, 4::5] = a[O - 2, :, 4::5]
    prev = np.eye(O, dtype=f32)[rs.randint(0, O, X)].T.copy()
    n_ch = channel_layout(n_cluster, n_local, True)["n_ch"]
    return src, prev, rs.standard_normal((O, n_ch, X)).astype(f32)


# ------------------------------------------------------------------------------------------ planted inputs for the tie and order rules
PLANTED_GRAD = np.array([1.5, 1.0, 0.25, 2.0 ** -24, 2.0 ** -24], f32)


def planted_fg2bg():
    """dis [5, 2, 6], grad_out [5, 6].  Columns: 0 an exact tie between two objects; 1 a tie between the winner and the runner-up (equal
    to it in another object AND in its own second channel); 2 a tie of three and more; 3 all +inf; 4 +inf but one; 5 tie-free.  grad_out
    makes the order of the sum visible: x + 0.25 + 2^-24 + 2^-24 stays x + 0.25 added upwards (each 2^-24 is half an ulp and rounds to
    even) and is x + 0.25 + 2^-23 added downwards; its first two entries differ, so swapping two tied winners shows too."""
    inf = np.inf
    dis = np.array([[[3, 0.5, 1, inf, inf, 4], [5, 0.5, 7, inf, inf, 6]],
                    [[3, 0.5, 1, inf, inf, 2], [9, 2.0, 8, inf, 0.25, 5]],
                    [[4, 3.0, 1, inf, inf, 3], [6, 4.0, 9, inf, inf, 7]],
                    [[8, 3.0, 2, inf, inf, 9], [7, 5.0, 1, inf, inf, 8]],
                    [[9, 9.0, 9, inf, inf, 9], [9, 9.0, 9, inf, inf, 9]]], f32)
    return dis, np.repeat(PLANTED_GRAD[:, None], 6, axis=1)


def planted_aggregate():
    """Sources for O = 5, one cluster pair, two radii, X = 6, with the same six kinds of column in the global map and in both local channels
    (T-like values; 1.0 stands for the saturated +inf distance).  The foreground cotangents of those columns are zero and the background
    ones PLANTED_GRAD, so every element shows the rule alone."""
    rs = np.random.RandomState(5)
    X, O = 6, 5
    col = np.array([[0.25, -0.5, 0.1, 1.0, 1.0, 0.4],
                    [0.25, -0.5, 0.1, 1.0, -0.25, 0.2],
                    [0.50, 0.3, 0.1, 1.0, 1.0, 0.3],
                    [0.75, 0.3, 0.6, 1.0, 1.0, 0.9],
                    [0.90, 0.9, 0.9, 1.0, 1.0, 0.95]], f32)
    glob = col[:, None, :].copy()
    local = np.stack([col, col[::-1]], axis=1).copy()               # the second radius in reversed object order: other winners
    mk = lambda k: np.tanh(rs.standard_normal((O, k, X))).astype(f32)
    src = [glob, mk(2), mk(1), local, mk(2)]
    prev = np.eye(O, dtype=f32)[rs.randint(0, O, X)].T.copy()
    lay = channel_layout(2, 2, True)
    grad_feat = rs.standard_normal((O, lay["n_ch"], X)).astype(f32)
    for ch in (lay["global_bg"], lay["local_bg"], lay["local_bg"] + 1):
        grad_feat[:, ch] = PLANTED_GRAD[:, None]
    for ch in (lay["glob"], lay["local"], lay["local"] + 1):
        grad_feat[:, ch] = 0.0
    return src, prev, grad_feat


# ------------------------------------------------------------------------------------------ pooling gradient
def pool_case(h, w, O, C, seed, soft=False, empty=None, full=None, with_neg=True):
    """labels [O, hw] (one-hot, or soft = a softmax), grad_pos / grad_neg [O, C].  ``empty``: an object with no pixel; ``full``: an object
    that owns every pixel (one-hot only)."""
    rs = rng(h, w, O, C, seed)
    X = h * w
    if soft:
        z = rs.standard_normal((O, X))
        lab = (np.exp(z) / np.exp(z).sum(0)).astype(f32)
    else:
        owner = rs.randint(0, O, X)
        if full is not None:
            owner[:] = full
        elif empty is not None and O > 1:
            owner[owner == empty] = (empty + 1) % O
        lab = np.eye(O, dtype=f32)[owner].T.copy()
    gpos = rs.standard_normal((O, C)).astype(f32)
    gneg = rs.standard_normal((O, C)).astype(f32) if with_neg else None
    return lab, gpos, gneg


HEAD_FIXTURES = ("frontend_grad_heads_C36_O4", "frontend_grad_heads_C100_O1")
FG2BG_FIXTURES = ("frontend_grad_fg2bg_O4_c1", "frontend_grad_fg2bg_O3_c6")


def pool_forward_tol(emb, lab, epsilon):
    """Bound on |aoc_masked_mean_pool - float64| for ONE-HOT labels (the counts are then exact integers): emb [C, X], lab [O, X] ->
    (tol_pos, tol_neg) [O, C].  A float32 sum of n terms, added in any order, is within gamma(n - 1) x the sum of the absolute terms;
    pos = S_pos / (Np + eps) adds the rounding of the denominator and of the division, neg = (S_all - S_pos) / (Nn + eps) the subtraction."""
    eps = eps32(epsilon)
    a, l = np.abs(emb.astype(f64)), lab.astype(f64)
    n = a.shape[1]
    pos_abs, all_abs = l @ a.T, a.sum(1)[None, :]
    Np, Nn = l.sum(1)[:, None], (1.0 - l).sum(1)[:, None]
    return gamma(n + 1) * pos_abs / (Np + eps), gamma(n + 2) * (all_abs + pos_abs) / (Nn + eps)


def pool_grad_ref(lab, gpos, gneg, epsilon):
    """-> (grad_emb [C, hw] float64, tol).  lab [O, hw]."""
    eps = eps32(epsilon)
    l = lab.astype(f64)
    lm = 1.0 - l
    O, X = l.shape
    n_add = -(-X // POOL_THREADS) + 8                              # additions a label went through on its way into Np / Nn
    Np, Nn = l.sum(1), lm.sum(1)
    dNp = gamma(n_add) * np.abs(l).sum(1)
    dNn = gamma(n_add + 1) * np.abs(lm).sum(1)                     # + the rounding of 1 - l

    def weights(g, N, dN):
        d = N + eps
        dd = dN + U * (np.abs(d) + dN)                             # fl(N^ + eps)
        assert (d - dd > 0).all()
        wt = g.astype(f64) / d[:, None]
        dw = np.abs(g.astype(f64)) * (dd / (d * (d - dd)))[:, None] + U * np.abs(g.astype(f64)) / (d - dd)[:, None]
        return wt, dw
    wp, dwp = weights(gpos, Np, dNp)
    want = wp.T @ l
    a_l, a_lm = np.abs(l), np.abs(lm)
    term_abs = np.abs(wp).T @ a_l
    term_err = dwp.T @ a_l + U * ((np.abs(wp) + dwp).T @ a_l)
    n_terms = O
    if gneg is not None:
        wn, dwn = weights(gneg, Nn, dNn)
        want = want + wn.T @ lm
        term_abs = term_abs + np.abs(wn).T @ a_lm
        term_err = term_err + (1 + U) * (dwn.T @ a_lm) + 2 * U * ((np.abs(wn) + dwn).T @ a_lm)
        n_terms = 2 * O
    return want, term_err + gamma(n_terms) * (term_abs + term_err)
