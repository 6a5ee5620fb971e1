"""Float64 references, bounds, slips, cases and inputs for the exact-fp32 global matching kernels of csrc/correlation.hip and their `.half()`
modes: proxy_corr_min_kernel (aoc_proxy_corr_min, aoc_proxy_corr_min_f16, aoc_proxy_corr_min_batched with AOC_CORR_FP32) and
gather_sqnorm_kernel + dense_match_partial_kernel + dense_match_finalize_kernel (aoc_dense_match_min, aoc_dense_match_min_f16).  Shared by
test_global_match_host.py (no GPU) and test_gpu_global_match.py.  Pure numpy; the library is not imported here.  U, gamma and the
(want, tol) / slip convention are those of float64_bounds.py; the per-pair distance and its bound (pair_distances), the bound of
aoc_proto_transform (local_transform_ref) and the float16 constants are those of local_match_bounds.py.

The references (float64, on the float32 inputs widened; in f16 mode on the inputs rounded to float16 first):
  proxy   want[s, i] = min over the live proxies p of set s of (|q_i|^2 + |p|^2) - 2 q_i.p; a proxy is live when its supplied norm is finite
          or no norms are supplied; PAD where a set has no live proxy.  The `.half()` entry pads with the same float32 5e4, not with 49984:
          proxy_corr_min_kernel's `if (v == INFINITY) v = AOC_PAD_DISTANCE` is not rounded, and the reference line it cites (AEM:312) builds
          the constant as a float32 tensor, `torch.ones(..) * WRONG_LABEL_PADDING_DISTANCE`, outside the float16 arithmetic.
  dense   want[i, o] = min over kept rows j of D[i, j] + PAD wrong[j, o]; +inf raw and 1.0 transformed when no row is kept
          (dense_match_finalize_kernel's `*n_fg_ptr == 0` branch).  f16 mode pads with aoc_h(AOC_PAD_DISTANCE) = 49984 (`padv`).

The bound of a distance is pair_distances' E with these readings of the kernels (every sum of C terms passes a term through at most C
roundings, so gamma(C) holds whatever the order):
  |q|^2   load_a_fragment: lane kq adds the squares of channels kq, kq + 4, .. one after the other (C / 4 roundings), then two shuffle adds;
          f16: `part += aoc_hr(a * a)` and `q2 = aoc_hr(part)`, pair_distances' norm_err;
  |p|^2   proxies, norms not supplied or f16 mode: the staged-image loop `v += aoc_hr(r * r)` over kq, t, one sequential sum, then
          aoc_hr(v); dense: gather_sqnorm_kernel's `s += aoc_hr(v * v)` over the channels in order, then aoc_hr(s).  Proxies with
          proxy_sqnorm supplied, fp32 mode: the kernel takes the caller's float32 value as it is, so the error of that term is
          |float64(supplied) - |p|^2|, evaluated, not bounded (pair_distances' e_p2 argument);
  q.p     C / 4 (padded with zero operands to TMAX) steps of v_mfma_f32_16x16x4_f32 on one accumulator, four products each.  THE ONE
          MODELLING ASSUMPTION, the one local_match_bounds.py already makes: the instruction's internal order and rounding are not
          documented; a term is taken to pass through at most as many roundings as there are terms (C), each to nearest.  A term really meets
          about C / 4 accumulator steps plus a tree of two inside the instruction, so the assumption leaves a wide margin;
  d       `(q2r[r] + t.p2) - 2.0f * acc[r]`: two roundings (2 acc is exact); f16: aoc_h(aoc_h(q2 + p2) - 2 aoc_h(acc)).
A padded dense candidate adds `d + padv[o]`: one float32 rounding of D + PAD, E_pad = E + U (|D + PAD| + E).  In f16 mode it is
`aoc_h(d + padv[o])`; that rounding is evaluated rather than bounded (a relative 2^-11 of 49984 would be 24): rounding is monotone, so
the result lies between the float16 roundings of the float32 sums at D + 49984 -+ E_pad, and the reference is the float16 rounding at
D + 49984 itself.  An unpadded candidate adds exactly 0.
The minimum (min_with_bound): the kernel's minimum m^ is some candidate's value, m^ = a^_j >= a_j - E_j, and m^ <= a^_j* <= a_j* + E_j* for
the true minimiser j*.  So only the candidates with a_j - E_j <= a_j* + E_j* can be the kernel's choice, and |m^ - m| is at most the
largest E among those.  (A padded row, whose E is 3e-3, does not loosen the bound of a pixel that has an unpadded row of the object.)
Transformed outputs go through local_transform_ref: both kernels call the same aoc_proto_transform as the window kernels.

No constant here is fitted to a kernel's output.  Every slip is the same reference with one deliberate mistake (SLIPS); proxy_slips(case) and
dense_slips(case) name those a case can show, and test_global_match_host.py proves that each leaves the bound there.

Inputs: features s randn with s = 0.5 / sqrt(C), so distances are O(1) and transformed outputs sit where the sigmoid is steep; biases of
mixed signs in [0.25, 1].  Structure is planted: for each place a kernel could lose or wrongly take a candidate, one query gets a near
copy of itself there, q + delta with |delta| = 5e-3 k exactly (1e-2 s randn has this length on average at k = 1; the exact
length keeps C = 4 from drawing a short one), k = 1 for candidates that must NOT count and k >= 2, all different, for those that must, so
that plants that share a query on a one-pixel map stay apart by far more than the bound.

The fp16-split proxy kernels of correlation_batched.hip (aoc_proxy_corr_min_batched with AOC_CORR_SPLIT, aoc_proxy_corr_min_records and its
cached form) have their own per-pair bound, split_pair_distances, and their own transform bound, cb_transform_ref; both docstrings derive
them.  The fp16-split dense entry of dense_split.hip (aoc_dense_match_min_split) uses the same per-pair bound and its own finalize
step, split_dense_ref."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from float64_bounds import U, _check_bound, gamma          # noqa: F401  (re-exported for the tests)
from local_match_bounds import PAD, PAD_H, SUBH, UH, check_bound, local_transform_ref, pair_distances       # noqa: F401

f32 = np.float32
PLANT_LEN = 5.0e-3          # |delta| of a planted near copy at k = 1

SLIPS = {
    "past_the_end": "a set also takes the next proxy",
    "inf_counts": "proxies with a +inf norm count",
    "last_tile_dropped": "the last, partial 16-row tile of a set of more than 16 proxies is lost",
    "absent_is_inf": "an absent set gives +inf and not PAD (raw outputs)",
    "other_bias": "set s is transformed with the bias of set s + 1",
    "tail_channels": "channels from 16 (C // 16) on are dropped",
    "unkept_counts": "pool rows that are not kept count",
    "wrong_excluded": "a wrong-labelled row is left out instead of padded",
    "wrong_unpadded": "a wrong-labelled row counts without its padding",
    "boundary_rows_dropped": "the planted positions of fg_rows are removed",
    "high_objects": "object o >= 16 reads bit o - 16",
    "pad_f16": "5e4 where the f16 mode has 49984",
    "two_products": "the split sum without ql.ph",
    "one_product": "the split sum with the hi-plane product only",
    "norm_one_piece": "only the first fp16 piece of -16 |p|^2",
}


# ------------------------------------------------------------------------------------------ restated host arithmetic of correlation.hip
def tile_row_stride(C):
    """aoc_tile_row_stride."""
    return 4 * ((C // 4 + 3) // 4 * 4) + 4


def proxy_tile_bytes(C):
    return 16 * tile_row_stride(C) * 4 + 16 * 4


def proxy_max_tiles(C):
    """aoc_corr_fp32_batched: 16-column proxy tiles per launch, `130 * 1024 / tile_bytes` capped at PC_MAX_TILES = 20."""
    return min(20, 130 * 1024 // proxy_tile_bytes(C))


def proxy_instantiation(C):
    """TMAX of the proxy_corr_min_kernel instantiation the entry dispatches."""
    return 25 if C == 100 else 32 if C <= 128 else 64


def proxy_launches(C, set_begin, set_size, set_off):
    """aoc_corr_fp32_batched's packing loop -> [(tiles, transposed output columns (0 = direct stores), dynamic LDS bytes)] per launch."""
    max_tiles, launches = proxy_max_tiles(C), []
    st = {"n": 0, "n_out": 0, "over": False}

    def add_out():
        if st["n_out"] >= 64:
            st["over"] = True
        else:
            st["n_out"] += 1

    def flush():
        if st["n"]:
            n_out = 0 if st["over"] else st["n_out"]
            launches.append((st["n"], n_out, st["n"] * proxy_tile_bytes(C) + 4 * 16 * (n_out + 1) * 4))
        st.update(n=0, n_out=0, over=False)

    set_begin, set_size, set_off = ([int(v) for v in a] for a in (set_begin, set_size, set_off))
    s, n_set = 0, len(set_size)
    while s < n_set:
        if set_size[s] == 1:
            run = 1
            step = set_off[s + 1] - set_off[s] if s + 1 < n_set else 0
            while (run < 16 and s + run < n_set and set_size[s + run] == 1 and set_begin[s + run] == set_begin[s] + run
                   and set_off[s + run] - set_off[s + run - 1] == step):
                run += 1
            if st["n"] + 1 > max_tiles:
                flush()
            for _ in range(run):
                add_out()
            st["n"] += 1
            s += run
        else:
            nt = 1 if set_size[s] == 0 else (set_size[s] + 15) // 16
            assert nt <= max_tiles
            if st["n"] + nt > max_tiles:
                flush()
            add_out()
            st["n"] += nt
            s += 1
    flush()
    return launches


def dense_na(n_obj):
    return 2 if n_obj <= 4 else 1


def dense_nsplit(m, na):
    """dense_nsplit of correlation.hip (release build: four rounds at most), in the same double arithmetic."""
    row_blocks = (m + 16 * 8 * na - 1) // (16 * 8 * na)
    best, best_eff = 1, 0.0
    for k in range(1, 5):
        ns = min(64, max(1, (256 * k) // row_blocks))
        blocks = row_blocks * ns
        rounds = (blocks + 255) // 256
        eff = blocks / (256.0 * rounds)
        if eff >= best_eff - 0.005:
            best_eff = max(eff, best_eff)
            best = ns
    return best


def dense_workspace_bytes(m, capacity, n_obj):
    """aoc_dense_match_workspace_bytes."""
    up = lambda v: (v + 255) // 256 * 256
    return up(capacity * 4 + 16) + up(dense_nsplit(m, dense_na(n_obj)) * m * n_obj * 4)


def dense_split_ranges(m, n_fg, n_obj):
    """dense_match_partial_kernel's [first, last + 1) positions of fg_rows per non-empty n-split (grid y)."""
    ns = dense_nsplit(m, dense_na(n_obj))
    n_tiles = (n_fg + 15) // 16
    tps = (n_tiles + ns - 1) // ns
    out = []
    for s in range(ns):
        beg, end = s * tps, min(n_tiles, (s + 1) * tps)
        if beg < end:
            out.append((16 * beg, min(n_fg, 16 * end)))
    return out


# ------------------------------------------------------------------------------------------ the minimum of bounded values
def min_with_bound(A, EA, empty):
    """-> (want, tol) [m]: the row minima of A [m, n] and their bound given |a^ - a| <= EA elementwise (see the module docstring);
    (empty, 0) where there is no column."""
    m = A.shape[0]
    if A.shape[1] == 0:
        return np.full(m, empty, np.float64), np.zeros(m)
    ar = np.arange(m)
    j = A.argmin(1)
    want = A[ar, j]
    reach = want + EA[ar, j]
    tol = np.where(A - EA <= reach[:, None], EA, 0.0).max(1)
    return want, tol


def transform_ref(want_raw, tol_raw, bias):
    """local_transform_ref on [n, m] arrays (n sets or objects, bias [n] or None)."""
    n, m = want_raw.shape
    with np.errstate(invalid="ignore"):          # a slipped reference may hold +inf
        want, tol = local_transform_ref(want_raw.reshape(n, 1, 1, m), tol_raw.reshape(n, 1, 1, m), bias)
    return want.reshape(n, m), tol.reshape(n, m)


# ------------------------------------------------------------------------------------------ proxy correlation
def proxy_ref(query, proxies, sqnorm, set_begin, set_size, f16=False, slip=None):
    """-> (want_raw, tol_raw) [n_set, m] float64.  query [m, C], proxies [n_proxy, C] float32, sqnorm [n_proxy] float32 (+inf = ignore) or None."""
    assert slip is None or slip in SLIPS, slip
    C, n_proxy = query.shape[1], proxies.shape[0]
    live = np.ones(n_proxy, bool) if sqnorm is None or slip == "inf_counts" else np.isfinite(sqnorm)
    e_p2 = None
    if sqnorm is not None and not f16:
        p = proxies.astype(np.float64)
        e_p2 = np.where(np.isfinite(sqnorm), np.abs(np.where(np.isfinite(sqnorm), sqnorm, 0).astype(np.float64) - (p * p).sum(1)), 0.0)
        if slip == "inf_counts":
            e_p2 = np.where(np.isfinite(sqnorm), e_p2, gamma(C) * (p * p).sum(1))
    D, E = pair_distances(query, proxies, f16, channels=16 * (C // 16) if slip == "tail_channels" else None, e_p2=e_p2)
    n_set, m = len(set_size), query.shape[0]
    want, tol = np.empty((n_set, m)), np.empty((n_set, m))
    for s, (b, n) in enumerate(zip(set_begin, set_size)):
        if slip == "last_tile_dropped" and n > 16 and n % 16:
            n = n // 16 * 16
        if slip == "past_the_end" and b + n < n_proxy:
            n = n + 1
        cols = np.arange(b, b + n)
        cols = cols[live[cols]]
        want[s], tol[s] = min_with_bound(D[:, cols], E[:, cols], np.inf if slip == "absent_is_inf" else PAD)
    return want, tol


ProxyCase = namedtuple("ProxyCase", "name C m kind norms layout bias f16 extra frames")


def _pcase(name, C, m, kind="general", norms="marked", layout="planes", bias=True, f16=False, extra=0, frames=0):
    return ProxyCase(name, C, m, kind, norms, layout, bias, f16, extra, frames)


# what rotates over the m of the grid: proxy_sqnorm supplied with +inf marks / NULL / supplied without marks, plane or pixel-major output,
# set_bias or NULL
_BY_M = {1: ("marked", "planes", True), 15: ("none", "pixels", True), 16: ("given", "planes", False), 17: ("marked", "pixels", True),
         65: ("marked", "planes", False), 150: ("marked", "pixels", True)}


def _proxy_cases():
    c = []
    for C in (4, 36, 100, 124, 128, 132, 256):
        for m, (norms, layout, bias) in _BY_M.items():
            c.append(_pcase(f"C{C}_m{m}", C, m, norms=norms, layout=layout, bias=bias))
    c.append(_pcase("two_launches_C100", 100, 33, extra=2))            # 18 tiles > max_tiles = 17
    c.append(_pcase("three_launches_C256", 256, 33, layout="pixels"))  # 16 tiles, max_tiles = 7
    for C in (100, 128, 256):                                          # one launch of exactly max_tiles: the largest LDS request of each instantiation
        c.append(_pcase(f"fill_C{C}", C, 33, kind="fill"))
    for C in (100, 36):
        c.append(_pcase(f"singles70_C{C}", C, 33, kind="singles70"))   # more than 64 output columns: direct stores
        c.append(_pcase(f"singles64_C{C}", C, 33, kind="singles64", layout="pixels"))
    for C in (100, 36, 132):
        c.append(_pcase(f"f16_C{C}", C, 65, f16=True, layout="pixels" if C == 36 else "planes"))
    c.append(_pcase("frames33_C100", 100, 17, frames=33))
    return c


def proxy_structure(case):
    """-> dict(set_begin, set_size, plane [n_set] (the output plane of each set), n_proxy, marks (proxies whose supplied norm is +inf), plants
    [(proxy, k)]: near copies of queries, k = 1 where the proxy must not count).  Groups are separated by a proxy that belongs to no set.
    general: sets of 0, 1, 2, 16, 17 and 33 proxies; five consecutive single-proxy sets with a constant output step; two pairs of single-proxy
    sets with a gap in set_begin between them; four consecutive single-proxy sets whose output planes go +1, +2, -1 (a changed step); a set
    of three proxies all marked; a marked single-proxy set; `extra` more sets of 16."""
    sb, ss, plane, marks, plants = [], [], [], [], []
    pos = [0]

    def multi(n, plant=(), mark=(), past=False):
        b = pos[0]
        sb.append(b), ss.append(n), plane.append(len(plane))
        plants.extend((b + i, 2) for i in plant)
        marks.extend(b + i for i in mark)
        if past:
            plants.append((b + n, 1))
        pos[0] = b + n + 1
        return b

    def singles(n, planes=None, plant=(), mark=()):
        b = pos[0]
        base = len(plane)
        for i in range(n):
            sb.append(b + i), ss.append(1), plane.append(base + (planes[i] if planes else i))
        plants.extend((b + i, 2) for i in plant)
        marks.extend(b + i for i in mark)
        pos[0] = b + n + 1

    if case.kind == "general":
        multi(0)
        multi(1)
        multi(2, plant=(0,), past=True)                      # the first proxy of a set; the proxy just past its end
        b = multi(16, plant=(15,), mark=(7,))                # the last proxy of a set; a marked proxy inside it ..
        plants.append((b + 7, 1))                            # .. that is a near copy and must not count
        multi(17, plant=(16,))                               # the only proxy of a second, partial tile
        multi(33, plant=(0, 16, 32))                         # first proxy, first of the second tile, last of the last partial tile
        singles(5, plant=(2,))
        singles(2), singles(2)                               # b, b + 1, gap, b + 3, b + 4
        singles(4, planes=(0, 1, 3, 2))
        b = multi(3, mark=(0, 1, 2))                         # an absent set ..
        plants.append((b + 1, 1))
        b = multi(1, mark=(0,))                              # .. and an absent single-proxy set
        plants.append((b, 1))
        for _ in range(case.extra):
            multi(16, plant=(3,))
    elif case.kind == "fill":
        multi(33, plant=(32,), past=True)
        multi(17, plant=(16,))
        b = multi(3, mark=(0, 1, 2))
        plants.append((b + 2, 1))
        for _ in range(proxy_max_tiles(case.C) - 6):
            multi(16, plant=(15,))
    else:
        n = int(case.kind[len("singles"):])
        pos[0] = 1
        singles(n, plant=(0, 15, 16, n - 1), mark=(n // 2 + 2,))     # one absent single-proxy set inside the run
        plants.append((1 + n // 2 + 2, 1))
    # every plant that must count gets its own k >= 2
    k, out = 2, []
    for p, kk in plants:
        out.append((p, 1) if kk == 1 else (p, k))
        k += kk != 1
    n_proxy = pos[0] + 1
    return dict(set_begin=np.asarray(sb, np.int32), set_size=np.asarray(ss, np.int32), plane=np.asarray(plane), n_proxy=n_proxy,
                marks=sorted(set(marks)), plants=out)


def _unit(rng, C):
    v = rng.standard_normal(C)
    return v / np.sqrt((v * v).sum())


def proxy_inputs(case, frame=0):
    """-> dict(query, proxies, sqnorm or None, bias or None, set_begin, set_size, set_off, stride, out_len, named (flat indices the call writes,
    [n_set, m])).  planes: set s at plane[s] (m + 3) + 2 + i; pixels: at i n_set + s, the pixel-major layout.  The buffer has out_len
    elements, more than the layout names."""
    st = proxy_structure(case)
    C, m = case.C, case.m
    rng = np.random.RandomState(zlib.crc32(f"{case.name}/{frame}".encode()) & 0x7FFFFFFF)
    s = 0.5 / np.sqrt(C)
    query = (s * rng.standard_normal((m, C))).astype(f32)
    proxies = (s * rng.standard_normal((st["n_proxy"], C))).astype(f32)
    for t, (p, k) in enumerate(st["plants"]):
        proxies[p] = (query[t % m].astype(np.float64) + PLANT_LEN * k * _unit(rng, C)).astype(f32)
    sqnorm = None
    if case.norms != "none":
        sqnorm = (proxies * proxies).sum(1, dtype=f32)       # some float32 value near |p|^2: its error is evaluated, whatever it is
        if case.norms == "marked":
            sqnorm[st["marks"]] = np.inf
    n_set = len(st["set_size"])
    bias = None
    if case.bias:
        bias = (rng.uniform(0.25, 1.0, n_set) * np.where(np.arange(n_set) % 2 == 0, 1.0, -1.0)).astype(f32)
    if case.layout == "planes" or case.frames:
        set_off, stride = st["plane"].astype(np.int64) * (m + 3) + 2, 1
        out_len = n_set * (m + 3) + 7
    else:
        set_off, stride = np.arange(n_set, dtype=np.int64), n_set
        out_len = n_set * m + 5
    named = set_off[:, None] + stride * np.arange(m)[None, :]
    assert np.unique(named).size == named.size and named.max() < out_len
    return dict(query=query, proxies=proxies, sqnorm=sqnorm, bias=bias, set_begin=st["set_begin"], set_size=st["set_size"], set_off=set_off,
                stride=stride, out_len=out_len, named=named)


def absent_sets(case):
    """Sets without a live proxy: empty ones, and with +inf marks those whose every proxy is marked."""
    st = proxy_structure(case)
    marks = set(st["marks"]) if case.norms == "marked" else set()
    return [s for s, (b, n) in enumerate(zip(st["set_begin"], st["set_size"])) if all(p in marks for p in range(b, b + n))]


def proxy_slips(case, transformed=False):
    st = proxy_structure(case)
    kinds = ["past_the_end"]
    if case.norms == "marked" and st["marks"]:
        kinds.append("inf_counts")
    if any(n > 16 and n % 16 for n in st["set_size"]):
        kinds.append("last_tile_dropped")
    if case.C % 16:
        kinds.append("tail_channels")
    if transformed:
        if case.bias:
            kinds.append("other_bias")
    elif absent_sets(case):
        kinds.append("absent_is_inf")
    return kinds


def _bundle(ref, transform, raw_kinds, t_kinds, bias, skip_t=()):
    """ref(slip=None) -> (want, tol); transform(want, tol, bias) -> (want, tol).  -> dict(raw=(want, tol, {slip: want}), transformed=...):
    the slipped references of raw_kinds, and of t_kinds transformed (other_bias: the true reference under the next set's bias)."""
    want, tol = ref()
    raw = {k: ref(slip=k)[0] for k in raw_kinds}
    want_t, tol_t = transform(want, tol, bias)
    t = {}
    for k in t_kinds:
        if k == "other_bias":
            t[k] = transform(want, tol, np.roll(bias, -1))[0]
        elif k not in skip_t:
            t[k] = transform(raw[k] if k in raw else ref(slip=k)[0], np.zeros_like(tol), bias)[0]
    for a in (want, tol, want_t, tol_t, *raw.values(), *t.values()):
        a.setflags(write=False)
    return dict(raw=(want, tol, raw), transformed=(want_t, tol_t, t))


@functools.lru_cache(maxsize=None)
def proxy_case_ref(name, frame=0):
    """The reference of a case, computed once: -> dict(raw=(want, tol, {slip: want}), transformed=(want, tol, {slip: want})).  Read-only."""
    case = PROXY_BY_NAME[name]
    inp = proxy_inputs(case, frame)
    ref = functools.partial(proxy_ref, inp["query"], inp["proxies"], inp["sqnorm"], inp["set_begin"], inp["set_size"], case.f16)
    return _bundle(ref, transform_ref, proxy_slips(case), proxy_slips(case, transformed=True), inp["bias"])


# ------------------------------------------------------------------------------------------ dense matching
def _round_h(x):
    """A float64 value through the kernel's float32 sum and aoc_h."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(f32).astype(np.float16).astype(np.float64)


def dense_ref(query, pool, fg_rows, wrong_bits, n_obj, f16=False, slip=None, planted=()):
    """-> (want_raw, tol_raw) [n_obj, m] float64.  fg_rows: the kept rows (positions 0 .. n_fg - 1 only); wrong_bits [pool rows]."""
    assert slip is None or slip in SLIPS, slip
    m, C = query.shape
    rows = np.asarray(fg_rows, np.int64)
    if slip == "boundary_rows_dropped":
        rows = np.delete(rows, list(planted))
    if slip == "unkept_counts":
        rows = np.arange(pool.shape[0])
    if rows.size == 0:
        return np.full((n_obj, m), np.inf), np.zeros((n_obj, m))
    D, E = pair_distances(query, pool[rows], f16, channels=16 * (C // 16) if slip == "tail_channels" else None)
    pad = PAD if (slip == "pad_f16" or not f16) else PAD_H
    Ep = E + U * (np.abs(D + pad) + E)
    if f16:
        Dp = _round_h(D + pad)
        Ep = np.maximum(_round_h(D + pad + Ep) - Dp, Dp - _round_h(D + pad - Ep))
    else:
        Dp = D + pad
    bits = np.asarray(wrong_bits).astype(np.int64)[rows] & 0xFFFFFFFF
    want, tol = np.empty((n_obj, m)), np.empty((n_obj, m))
    for o in range(n_obj):
        w = ((bits >> (o - 16 if slip == "high_objects" and o >= 16 else o)) & 1).astype(bool)
        if slip == "wrong_excluded":
            want[o], tol[o] = min_with_bound(D[:, ~w], E[:, ~w], np.inf)
        elif slip == "wrong_unpadded":
            want[o], tol[o] = min_with_bound(D, E, np.inf)
        else:
            want[o], tol[o] = min_with_bound(np.where(w[None, :], Dp, D), np.where(w[None, :], Ep, E), np.inf)
    return want, tol


DenseCase = namedtuple("DenseCase", "name C m n_fg n_obj f16 layout")


def _dense_cases():
    c = []

    def add(name, C, m, n_fg, n_obj, f16=False):
        c.append(DenseCase(name, C, m, n_fg, n_obj, f16, "planes" if len(c) % 2 == 0 else "pixels"))      # strides (1, m) / (n_obj, 1)

    for C in (100, 36):
        for n_obj in (1, 4, 5, 8, 9, 16, 17, 24, 25, 30):          # (NA, OMAX) = (2, 4), (1, 8), (1, 16); a second launch above 16 objects
            add(f"C{C}_O{n_obj}", C, 150, 400, n_obj)
    for C in (4, 64, 124, 128):
        add(f"C{C}_O7", C, 150, 400, 7)
    for n_fg in (1, 16, 17, 1000, 9001, 17001):                    # 64 n-splits: empty splits, 8 + 1 and 8 + 8 + 1 tiles per split
        add(f"rows{n_fg}", 100, 150, n_fg, 5)
    for m in (1, 15, 129, 257):                                    # NA = 2: a block of 256 pixels partly and just over filled
        add(f"m{m}_O3", 100, m, 400, 3)
    add("no_rows", 100, 33, 0, 5)
    for C in (100, 64):
        for n_obj in (3, 17):
            add(f"f16_C{C}_O{n_obj}", C, 150, 400, n_obj, f16=True)
    return c


def absent_object(n_obj):
    """The object no row is right for, where there are more than four: object 3."""
    return 3 if n_obj > 4 else None


def dense_plant_positions(case):
    """Positions of fg_rows that get a near copy of a query: 0, 15, 16, 127, 128, n_fg - 1; the first and last row of the first n-split's range
    and of the last non-empty one; the first row of the first split's second and third 128-row chunk."""
    n = case.n_fg
    pos = {0, 15, 16, 127, 128, n - 1}
    ranges = dense_split_ranges(case.m, n, case.n_obj)
    for beg, end in (ranges[0], ranges[-1]) if ranges else ():
        pos |= {beg, end - 1}
    if ranges:
        pos |= {ranges[0][0] + 128, ranges[0][0] + 256} & set(range(*ranges[0]))
    return sorted(p for p in pos if 0 <= p < n)


def dense_inputs(case, onehot=False):
    """-> dict(query, pool, fg_rows [pool rows] int32, n_fg, wrong [pool rows] uint32, counts [n_obj + 1] int32, bias, planted).  Built in numpy,
    never through label_prep.  The pool has n_fg kept rows and about an eighth as many that are not kept (pool row 0 among them, so
    fg_rows is a proper subset and not the identity).  A kept row is right for one object (wrong for every other; the absent object has
    none) or, one in twenty, soft: wrong only for the absent object, right for none.  A tenth of the rows carry every bit from n_obj up,
    bit 31 included.  (A pool of one kept row has that row soft.)  One row that is not kept is the nearest copy of the last query (k = 1), and the positions of fg_rows past n_fg all
    name it: a kernel that reads past n_fg meets it.  Planted kept rows (dense_plant_positions) are one-hot.
    onehot: no soft rows (what the split kernels need).  right_bits, obj_rows, obj_offsets and counts are what aoc_label_prep would give:
    bit o = right for o, bit 31 = kept; per object the kept rows right for it, ascending, packed at obj_offsets[o]."""
    C, m, n_fg, n_obj = case.C, case.m, case.n_fg, case.n_obj
    rng = np.random.RandomState(zlib.crc32(("dense/" + case.name + ("/onehot" if onehot else "")).encode()) & 0x7FFFFFFF)
    s = 0.5 / np.sqrt(C)
    n_pool = n_fg + max(4, n_fg // 8)
    query = (s * rng.standard_normal((m, C))).astype(f32)
    pool = (s * rng.standard_normal((n_pool, C))).astype(f32)
    unkept = np.sort(np.concatenate([[0], 1 + rng.choice(n_pool - 1, n_pool - n_fg - 1, replace=False)]))
    kept = np.setdiff1d(np.arange(n_pool), unkept)
    assert kept.size == n_fg
    absent = absent_object(n_obj)
    present = np.asarray([o for o in range(n_obj) if o != absent])
    owner = present[rng.randint(0, present.size, n_pool)]
    planted = np.asarray(dense_plant_positions(case), np.int64)
    for t, p in enumerate(planted):
        pool[kept[p]] = (query[t % m].astype(np.float64) + PLANT_LEN * (2 + t) * _unit(rng, C)).astype(f32)
        owner[kept[p]] = present[t % present.size]
    if case.name == "hi_margin":
        a, b = plant_hi_margin(query[HI_QUERY])
        for pos, row in zip(HI_POS, (a, b)):
            assert pos not in planted
            pool[kept[pos]], owner[kept[pos]] = row, present[0]
    trap = unkept[-1]
    pool[trap] = (query[m - 1].astype(np.float64) + PLANT_LEN * _unit(rng, C)).astype(f32)
    all_obj = (1 << n_obj) - 1
    wrong = all_obj & ~(1 << owner.astype(np.int64))
    soft = rng.random_sample(n_pool) < 0.05
    soft[kept[planted]] = False
    if case.name == "hi_margin":
        soft[kept[list(HI_POS)]] = False
    soft[unkept] = False
    if onehot:
        soft[:] = False
    elif n_fg == 1:
        soft[kept[0]] = True        # a single kept row: soft, so that not every object but one is padded
    wrong[soft] = 0 if absent is None else 1 << absent
    high = rng.random_sample(n_pool) < 0.1
    if n_fg:
        high[kept[0]] = True
    wrong[high] |= (0xFFFFFFFF << n_obj) & 0xFFFFFFFF
    fg_rows = np.full(n_pool, trap, np.int32)
    fg_rows[:n_fg] = kept
    is_kept = np.zeros(n_pool, bool)
    is_kept[kept] = True
    right = np.where(is_kept, (1 << 31) | np.where(soft, 0, 1 << owner.astype(np.int64)), 0)
    counts = np.zeros(n_obj + 1, np.int32)
    obj_rows = np.full(n_obj * n_pool, trap, np.int32)
    offsets = np.zeros(n_obj + 1, np.int32)
    for o in range(n_obj):
        rows_o = np.nonzero(is_kept & ~soft & (owner == o))[0]
        counts[o] = rows_o.size
        obj_rows[offsets[o]:offsets[o] + rows_o.size] = rows_o
        offsets[o + 1] = offsets[o] + rows_o.size
    counts[n_obj] = n_fg
    bias = (rng.uniform(0.25, 1.0, n_obj) * np.where(np.arange(n_obj) % 2 == 0, 1.0, -1.0)).astype(f32)
    return dict(query=query, pool=pool, fg_rows=fg_rows, n_fg=n_fg, wrong=wrong.astype(np.uint32), counts=counts, bias=bias,
                right=right.astype(np.uint32), obj_rows=obj_rows, obj_offsets=offsets, planted=[int(p) for p in planted])


def dense_layout(case):
    """-> (pixel stride, object stride, buffer length, named [n_obj, m]): the call writes at a view that starts at element 2."""
    m, n_obj = case.m, case.n_obj
    ps, os_ = (1, m) if case.layout == "planes" else (n_obj, 1)
    named = 2 + ps * np.arange(m)[None, :] + os_ * np.arange(n_obj)[:, None]
    return ps, os_, m * n_obj + 9, named


def dense_slips(case):
    if case.n_fg == 0:
        return []
    kinds = ["unkept_counts", "boundary_rows_dropped"]
    if case.n_obj >= 2:
        kinds.append("wrong_unpadded")
    if absent_object(case.n_obj) is not None:
        kinds.append("wrong_excluded")
        if case.f16:
            kinds.append("pad_f16")
    if case.n_obj > 16:
        kinds.append("high_objects")
    if case.C % 16:
        kinds.append("tail_channels")
    return kinds


@functools.lru_cache(maxsize=None)
def dense_case_ref(name):
    """-> dict(raw=(want, tol, {slip: want}), transformed=(want, tol, {slip: want})); the n_fg = 0 case has +inf raw and 1.0 transformed and
    no bound to check.  Read-only arrays."""
    case = DENSE_BY_NAME[name]
    inp = dense_inputs(case)
    args = (inp["query"], inp["pool"], inp["fg_rows"][:case.n_fg], inp["wrong"], case.n_obj, case.f16)
    want, tol = dense_ref(*args)
    slips = {k: dense_ref(*args, slip=k, planted=inp["planted"])[0] for k in dense_slips(case)}
    if case.n_fg == 0:
        return dict(raw=(want, tol, {}), transformed=(np.ones_like(want), tol, {}))
    want_t, tol_t = transform_ref(want, tol, inp["bias"])
    t_slips = {k: transform_ref(v, np.zeros_like(tol), inp["bias"])[0] for k, v in slips.items()
                if k not in ("pad_f16", "wrong_excluded")}             # 49984, 5e4 or +inf: 1.0 either way
    for a in (want, tol, want_t, tol_t, *slips.values(), *t_slips.values()):
        a.setflags(write=False)
    return dict(raw=(want, tol, slips), transformed=(want_t, tol_t, t_slips))


# ------------------------------------------------------------------------------------------ fp16-split proxy correlation
SPLIT_K = 337        # accumulated terms: 3 products x 7 k-steps x 16 slots, plus one for the stacked column-wise tile's `acc[r] + acc[r + 8]`


def split_planes(x):
    """cb_split_pair / split_rows_kernel: hi = float16(2^10 x), lo = float16(2^10 x - hi), as float64.  2^10 x and 2^10 x - hi are exact in
    float32, so numpy reproduces both pieces bit for bit."""
    v = np.asarray(x, f32) * f32(1024.0)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(f32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def norm_pieces(norm):
    """cb_stage_frame: the three float16 pieces n0, n1, n2 of a = -16 norm (float32, exact), as float64 [3, n]."""
    a = f32(-16.0) * np.asarray(norm, f32)
    n0 = a.astype(np.float16)
    r1 = a - n0.astype(f32)
    n1 = r1.astype(np.float16)
    n2 = (r1 - n1.astype(f32)).astype(np.float16)
    return np.stack([n0, n1, n2]).astype(np.float64)


def split_pair_distances(query, proxies, sqnorm, records=False, products=3, pieces=3, channels=None):
    """D[i, j] and E[i, j] of the fp16-split kernels of correlation_batched.hip (C = 100).  The split is evaluated, not bounded: with
    qh, ql, ph, pl the float16 pieces of 2^10 q, 2^10 p and n0, n1, n2 those of -16 |p|^2 (the float32 norm the kernel uses), the value the
    accumulator would hold in exact arithmetic is
        S = qh.ph + qh.pl + ql.ph + 2^15 (n0 + n1 + n2)          (cb_tile_compute's three chained products; the query side of the norm
                                                                   slots is CB_QCONST = 2^15)
    and its distance from T = 2^20 (q.p - |p|^2 / 2) is the representation error, |S - T|, in float64.  With proxy_sqnorm supplied the
    pieces are those of the caller's float32 value; with NULL the kernel's own norm is a chain of 100 fmaf (cb_stage_frame), whose value
    is not restated: the pieces are then taken from the float64 norm and the error gets gamma(100) |p|^2 for the chain and
    2^-25 + 2^-33 |a| for three roundings to float16 (half a subnormal spacing, and 33 bits kept).
    On top: the fp32 accumulation inside the matrix instructions, gamma(SPLIT_K) sum |terms| (the modelling assumption of the module
    docstring: at most as many roundings as terms); |q|^2: convert_raw's two fmaf chains of 25 per lane half, `sq + sq1` and cb_halfsum,
    gamma(27) |q|^2, or in the records path split_rows_kernel's sequential `s += e * e`, gamma(100) |q|^2; `q2 + CB_UNSCALE * raw`: the
    scaling by 2^-19 is exact, the sum rounds once.  products / pieces / channels: the slips two_products, one_product, norm_one_piece and
    tail_channels (everything, a supplied norm included, from the first `channels` channels only)."""
    q, p = np.asarray(query, f32), np.asarray(proxies, f32)
    if channels is not None:
        q, p = q[:, :channels], p[:, :channels]
        if sqnorm is not None:
            sqnorm = np.where(np.isfinite(sqnorm), (p * p).sum(1, dtype=f32), sqnorm).astype(f32)
    q64, p64 = q.astype(np.float64), p.astype(np.float64)
    q2, p2 = (q64 * q64).sum(1), (p64 * p64).sum(1)
    qh, ql = split_planes(q)
    ph, pl = split_planes(p)
    extra = np.zeros(p.shape[0])
    if sqnorm is not None:
        fin = np.isfinite(sqnorm)
        n = norm_pieces(np.where(fin, sqnorm, 0).astype(f32))
    else:
        n = norm_pieces(p2.astype(f32))
        extra = 2.0 ** 15 * (16.0 * (gamma(100) * p2 + np.abs(p2.astype(f32).astype(np.float64) - p2)) + 2.0 ** -25 + 2.0 ** -33 * 16.0 * p2)
    S = qh @ ph.T + 2.0 ** 15 * n[:pieces].sum(0)[None, :]
    A = np.abs(qh) @ np.abs(ph).T + 2.0 ** 15 * np.abs(n).sum(0)[None, :]
    if products >= 2:
        S = S + qh @ pl.T
    if products >= 3:
        S = S + ql @ ph.T
    A = A + np.abs(qh) @ np.abs(pl).T + np.abs(ql) @ np.abs(ph).T
    T = 2.0 ** 20 * (q64 @ p64.T - 0.5 * p2[None, :])
    D = q2[:, None] - 2.0 ** -19 * T
    e_q2 = gamma(100 if records else 27) * q2
    E = e_q2[:, None] + 2.0 ** -19 * (np.abs(S - T) + extra[None, :] + gamma(SPLIT_K) * A)
    E = E + U * (np.abs(D) + E)
    return D, E, q2[:, None] - 2.0 ** -19 * S


def _split_slipped(query, proxies, sqnorm, records, slip):
    """(D, E) of split_pair_distances; under one of the split slips D is the slipped sum's distance."""
    C = query.shape[1]
    kw = {"two_products": dict(products=2), "one_product": dict(products=1), "norm_one_piece": dict(pieces=1),
          "tail_channels": dict(channels=16 * (C // 16))}.get(slip, {})
    D, E, Ds = split_pair_distances(query, proxies, sqnorm, records, **kw)
    return (Ds if kw else D), E


def split_proxy_ref(query, proxies, sqnorm, set_begin, set_size, records=False, slip=None):
    """-> (want_raw, tol_raw) [n_set, m]: proxy_ref's reference under the split kernels' bound; the split slips return the minimum of the
    slipped sum's distances."""
    assert slip is None or slip in SLIPS, slip
    n_proxy = proxies.shape[0]
    live = np.ones(n_proxy, bool) if sqnorm is None or slip == "inf_counts" else np.isfinite(sqnorm)
    if slip == "inf_counts" and sqnorm is not None:
        sqnorm = np.where(np.isfinite(sqnorm), sqnorm, (proxies.astype(np.float64) ** 2).sum(1)).astype(f32)
    D, E = _split_slipped(query, proxies, sqnorm, records, slip)
    n_set, m = len(set_size), query.shape[0]
    want, tol = np.empty((n_set, m)), np.empty((n_set, m))
    for s, (b, n) in enumerate(zip(set_begin, set_size)):
        if slip == "past_the_end" and b + n < n_proxy:
            n = n + 1
        cols = np.arange(b, b + n)
        cols = cols[live[cols]]
        want[s], tol[s] = min_with_bound(D[:, cols], E[:, cols], np.inf if slip == "absent_is_inf" else PAD)
    return want, tol


def _g(t):
    return 2.0 / (1.0 + np.exp(-t)) - 1.0


def cb_transform_ref(want_raw, tol_raw, bias):
    """cb_transform of the raw reference [n_set, m]: 2 rcp(1 + exp2((d + b) * -log2(e))) - 1 with the hardware v_exp_f32 and v_rcp_f32, both
    documented to 1 ulp (a relative 2 U), not expf and a division.  t^ = fl(d^ + b): e_t = tol_raw + U (|t| + tol_raw).  The float32
    constant is within U of log2(e) and the product rounds once: in units of t that is 2 U (1 + U) |t| more.  exp is decreasing: the
    kernel's e lies in [exp(-(t + e_t)) (1 - 2 U), exp(-(t - e_t)) (1 + 2 U)] (plus 2^-126 for a flushed denormal); 1 + e rounds once, rcp
    is within 2 U, the doubling is exact and the subtraction rounds once.  Evaluated at both ends, not linearised."""
    want_raw, tol_raw = np.asarray(want_raw, np.float64), np.asarray(tol_raw, np.float64)
    b = np.zeros(want_raw.shape[0]) if bias is None else np.asarray(bias, f32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = want_raw + b[:, None]
        e_t = tol_raw + U * (np.abs(t) + tol_raw)
        e_t = e_t + 2.0 * U * (1.0 + U) * (np.abs(t) + e_t)
        want = _g(t)
        e_lo = np.exp(-(t + e_t)) * (1.0 - 2.0 * U)
        e_hi = np.exp(-(t - e_t)) * (1.0 + 2.0 * U) + 2.0 ** -126
        f_hi = 2.0 / ((1.0 + e_lo) * (1.0 - U)) * (1.0 + 2.0 * U) - 1.0
        f_lo = 2.0 / ((1.0 + e_hi) * (1.0 + U)) * (1.0 - 2.0 * U) - 1.0
        tol = np.maximum(f_hi - want, want - f_lo)
        tol = np.where(np.isfinite(tol), tol, 0.0)
        tol = tol + U * (np.abs(want) + tol)
    return want, tol


def _split_cases():
    c = []
    for m in (1, 31, 32, 33, 150):                       # the 8-, 16- and more-than-16-proxy row-group classes, a stacked column-wise tile
        c.append(_pcase(f"split_m{m}", 100, m, norms="none" if m == 31 else "marked", bias=m != 32))
    c.append(_pcase("split_passes", 100, 65, extra=8))   # more proxy tiles than one LDS image holds
    c.append(_pcase("split_singles17", 100, 65, kind="singles17"))      # the unstacked column-wise tile
    c.append(_pcase("split_singles33", 100, 65, kind="singles33"))      # a second launch for the 33rd
    c.append(_pcase("split_singles70", 100, 65, kind="singles70"))      # more than 64 sets
    c.append(_pcase("split_frames33", 100, 33, frames=33))
    return c


def split_slips(case, transformed=False):
    kinds = [k for k in proxy_slips(case, transformed) if k != "last_tile_dropped"]      # tiles of 32 rows here; tail_channels stays: 96 .. 99
    return kinds + ["two_products", "one_product", "norm_one_piece"]


@functools.lru_cache(maxsize=None)
def split_case_ref(name, records=False, frame=0):
    """As proxy_case_ref, for the split kernels (records: the |q|^2 of the records path)."""
    case = SPLIT_BY_NAME[name]
    inp = proxy_inputs(case, frame)
    ref = functools.partial(split_proxy_ref, inp["query"], inp["proxies"], inp["sqnorm"], inp["set_begin"], inp["set_size"], records)
    return _bundle(ref, cb_transform_ref, split_slips(case), split_slips(case, transformed=True), inp["bias"])


# ------------------------------------------------------------------------------------------ fp16-split dense matching
def seq_sqnorm32(x):
    """split_rows_kernel's `s += e * e` over the channels in order, float32: the norm whose three pieces ride in a record."""
    x = np.asarray(x, f32)
    s = np.zeros(x.shape[0], f32)
    for c in range(x.shape[1]):
        s = s + x[:, c] * x[:, c]
    return s


def split_dense_ref(query, pool, fg_rows, wrong_bits, n_obj, slip=None, planted=()):
    """-> (want_raw, tol_raw) [n_obj, m] for aoc_dense_match_min_split on one-hot labels: dense_ref's reference under the bound of
    dense_prune_kernel + dense_split_finalize_kernel.  A pair's value is the three-product sum of split_pair_distances (7 + 14 matrix
    instructions of 16 slots on one accumulator, 336 <= SPLIT_K terms; the pool norm and its pieces are split_rows_kernel's, restated
    exactly by seq_sqnorm32; |q|^2 is the same kernel's sequential sum).  Pruning only skips pairs that cannot hold the maximum, so the
    value is that of evaluating every pair.  The finalize step: own[o] = `qq + SP_UNSCALE * best` per object (the rounding already in E),
    v = fminf(own[o], others + AOC_PAD_DISTANCE) with others the minimum of the other objects' own: one more rounding of others + PAD."""
    assert slip is None or slip in SLIPS, slip
    m = query.shape[0]
    rows = np.asarray(fg_rows, np.int64)
    if slip == "boundary_rows_dropped":
        rows = np.delete(rows, list(planted))
    if slip == "unkept_counts":
        rows = np.arange(pool.shape[0])
    if rows.size == 0:
        return np.full((n_obj, m), np.inf), np.zeros((n_obj, m))
    D, E = _split_slipped(query, pool[rows], seq_sqnorm32(pool[rows]), True, slip)
    bits = np.asarray(wrong_bits).astype(np.int64)[rows]
    own, own_tol = np.empty((n_obj, m)), np.empty((n_obj, m))
    for o in range(n_obj):
        cols = np.nonzero((bits >> o) & 1 == 0)[0]
        own[o], own_tol[o] = min_with_bound(D[:, cols], E[:, cols], np.inf)
    want, tol = np.empty((n_obj, m)), np.empty((n_obj, m))
    for o in range(n_obj):
        rest = [o2 for o2 in range(n_obj) if o2 != o and np.isfinite(own[o2, 0])]
        if slip == "wrong_unpadded":
            a, e = own.T, own_tol.T
        elif rest:
            oth, oth_tol = min_with_bound(own[rest].T, own_tol[rest].T, np.inf)
            oth_tol = oth_tol + U * (np.abs(oth + PAD) + oth_tol)
            a, e = np.stack([own[o], oth + PAD], 1), np.stack([own_tol[o], oth_tol], 1)
        else:
            a, e = own[o][:, None], own_tol[o][:, None]
        fin = np.isfinite(a).any(0)
        want[o], tol[o] = min_with_bound(a[:, fin], e[:, fin], np.inf)
    return want, tol


# The dense cases of up to 16 objects at C = 100, 36 and 4, on one-hot labels.  One kept row under five objects would leave a fifth of the
# outputs real distances: that shape runs at three objects here.  hi_margin: see plant_hi_margin.
HI_MARGIN = DenseCase("hi_margin", 100, 150, 400, 5, False, "planes")
SPLIT_DENSE_CASES = [c._replace(name="rows1_O3", n_obj=3) if c.name == "rows1" else c
                     for c in _dense_cases() if not c.f16 and c.n_obj <= 16 and c.C in (100, 36, 4)] + [HI_MARGIN]
HI_QUERY, HI_POS = 100, (40, 300)        # the query of the hi_margin pair and the positions of fg_rows of its rows A and B


def plant_hi_margin(query):
    """-> rows A, B for `query` such that A is the true nearest row, by more than the split bound, while the hi-plane product alone ranks B
    first by a wide margin: only the cross products decide it (what dense_prune_kernel's rescoring is for).  Both sit at
    h = float16(2^10 (q + delta)), delta = -0.02 sign(q) per channel (|delta| = 0.2: far nearer than any random row); A = (h + 7/16 ulp(h)
    sign(q)) / 2^10 and B the same with -, so both have the hi plane h and lo planes +- 7/16 ulp sign(q).  Then qh.pl differs by
    sum |qh| 7/8 ulp, about 100 accumulator units or 2e-4 in distance, in B's favour for a kernel that drops it, and A is nearer than B by
    4 delta.eps, about 1e-4.  The host test checks both margins on the float64 values."""
    q = query.astype(np.float64)
    sg = np.where(q >= 0, 1.0, -1.0)
    h = (1024.0 * (q - 0.02 * sg)).astype(np.float16)
    ulp = np.abs(np.spacing(np.abs(h))).astype(np.float64)
    h = h.astype(np.float64)
    return ((h + 0.4375 * ulp * sg) / 1024.0).astype(f32), ((h - 0.4375 * ulp * sg) / 1024.0).astype(f32)


def split_dense_slips(case):
    if case.n_fg == 0:
        return []
    kinds = ["unkept_counts", "boundary_rows_dropped", "norm_one_piece"]
    if case.C % 16:
        kinds.append("tail_channels")
    if case.m > 1:      # a single query has only planted near copies for minima: q ~ p, and the cross products it drops stay inside the bound
        kinds += ["two_products", "one_product"]
    if case.n_obj >= 2:
        kinds.append("wrong_unpadded")
    return kinds


@functools.lru_cache(maxsize=None)
def split_dense_case_ref(name):
    case = {c.name: c for c in SPLIT_DENSE_CASES}[name]
    inp = dense_inputs(case, onehot=True)
    args = (inp["query"], inp["pool"], inp["fg_rows"][:case.n_fg], inp["wrong"], case.n_obj)
    want, tol = split_dense_ref(*args)
    if case.n_fg == 0:
        return dict(raw=(want, tol, {}), transformed=(np.ones_like(want), tol, {}))
    slips = {k: split_dense_ref(*args, slip=k, planted=inp["planted"])[0] for k in split_dense_slips(case)}
    want_t, tol_t = transform_ref(want, tol, inp["bias"])
    t_slips = {k: transform_ref(v, np.zeros_like(tol), inp["bias"])[0] for k, v in slips.items()}
    return dict(raw=(want, tol, slips), transformed=(want_t, tol_t, t_slips))


# Take-over: a value that breaks a precondition of the split arithmetic (|x| 2^10 <= 65000, |x|^2 <= 4000) makes the exact-fp32 kernel recompute
# the launch inside the same call.  Such a call is held to the fp32 bound (proxy_ref) and must be bit-equal to the fp32 entry.
TAKEOVER_CASES = [_pcase("takeover_query", 100, 33, layout="planes"), _pcase("takeover_proxy", 100, 33, layout="planes")]


def takeover_inputs(case):
    """proxy_inputs with one value out of range: 70 in the last query (no plant copies it), or 64 in proxy 5 of the set of 33."""
    inp = proxy_inputs(case)
    if case.name == "takeover_query":
        inp["query"][case.m - 1, 7] = 70.0
    else:
        st = proxy_structure(case)
        p = int(st["set_begin"][list(st["set_size"]).index(33)]) + 5
        inp["proxies"][p, 3] = 64.0
        inp["sqnorm"][p] = (inp["proxies"][p] * inp["proxies"][p]).sum(dtype=f32)
    return inp


@functools.lru_cache(maxsize=None)
def takeover_case_ref(name):
    case = TAKEOVER_BY_NAME[name]
    inp = takeover_inputs(case)
    ref = functools.partial(proxy_ref, inp["query"], inp["proxies"], inp["sqnorm"], inp["set_begin"], inp["set_size"])
    return _bundle(ref, transform_ref, proxy_slips(case), proxy_slips(case, transformed=True), inp["bias"])


TAKEOVER_BY_NAME = {c.name: c for c in TAKEOVER_CASES}

# The dense entry's take-overs: soft labels (a kept row that is not right for exactly one object sets split_plan_kernel's gate), one query
# value with |x| 2^10 > 65000 and |x|^2 > 4000, one such pool value.  Held to the fp32 bound (dense_ref), bit-equal to aoc_dense_match_min.
DENSE_TAKEOVER_CASES = [DenseCase("takeover_soft", 100, 150, 400, 5, False, "planes"), DenseCase("takeover_soft_O16", 36, 150, 400, 16, False, "pixels"),
                        DenseCase("takeover_query_value", 100, 150, 400, 5, False, "pixels"), DenseCase("takeover_pool_value", 100, 150, 400, 3, False, "planes")]
DENSE_TAKEOVER_BY_NAME = {c.name: c for c in DENSE_TAKEOVER_CASES}


def dense_takeover_inputs(case):
    """dense_inputs with soft rows, or one-hot with one value out of range: 70 in query 100 (no plant copies it) or 64 in the kept row at
    position 50 of fg_rows (not planted)."""
    inp = dense_inputs(case, onehot="soft" not in case.name)
    if case.name == "takeover_query_value":
        inp["query"][100, 7] = 70.0
    elif case.name == "takeover_pool_value":
        assert 50 not in inp["planted"]
        inp["pool"][inp["fg_rows"][50], 3] = 64.0
    else:
        rows = inp["fg_rows"][:case.n_fg]
        assert ((inp["right"][rows].astype(np.int64) & ((1 << case.n_obj) - 1)) == 0).any(), "no soft row"
    return inp


@functools.lru_cache(maxsize=None)
def dense_takeover_ref(name):
    case = DENSE_TAKEOVER_BY_NAME[name]
    inp = dense_takeover_inputs(case)
    args = (inp["query"], inp["pool"], inp["fg_rows"][:case.n_fg], inp["wrong"], case.n_obj)
    want, tol = dense_ref(*args)
    slips = {k: dense_ref(*args, slip=k, planted=inp["planted"])[0] for k in dense_slips(case)}
    want_t, tol_t = transform_ref(want, tol, inp["bias"])
    t_slips = {k: transform_ref(v, np.zeros_like(tol), inp["bias"])[0] for k, v in slips.items() if k not in ("pad_f16", "wrong_excluded")}
    return dict(raw=(want, tol, slips), transformed=(want_t, tol_t, t_slips))
PROXY_CASES = _proxy_cases()
SPLIT_CASES = _split_cases()
SPLIT_BY_NAME = {c.name: c for c in SPLIT_CASES}
PROXY_BY_NAME = {c.name: c for c in PROXY_CASES}
DENSE_CASES = _dense_cases()
DENSE_BY_NAME = {c.name: c for c in DENSE_CASES}


# ------------------------------------------------------------------------------------------ checks shared by both test files
def check_conditions(name, want_raw, want_t, expect_pad):
    """The conditions on the float64 reference alone (never on a kernel's output): with more than four outputs at least a quarter are real
    distances; a case with an absent set or object has a pad output; more than half of the transformed non-pad outputs are below 0.99."""
    is_pad = want_raw >= PAD_H
    if want_raw.size > 4:
        assert (~is_pad).mean() >= 0.25, f"{name}: only {(~is_pad).mean():.3f} of the raw outputs are distances"
    if expect_pad:
        assert is_pad.any(), f"{name}: no pad output"
    live = want_t[~is_pad]
    assert live.size and (live < 0.99).mean() > 0.5, f"{name}: transformed outputs saturate"


def check_layout(buf, named, what):
    """buf: the whole NaN-filled output buffer after the call.  Every element the layout names is written (not NaN), every other one is
    still NaN.  -> buf[named]."""
    buf = np.asarray(buf)
    mask = np.zeros(buf.size, bool)
    mask[named.ravel()] = True
    assert not np.isnan(buf[mask]).any(), f"{what}: {int(np.isnan(buf[mask]).sum())} named outputs were not written"
    assert np.isnan(buf[~mask]).all(), f"{what}: {int((~np.isnan(buf[~mask])).sum())} elements outside the layout were written"
    return buf[named]


def compare(got, ref, what, report=None):
    """got [n, m] against ref = (want, tol, slips): _check_bound once per slip; prints the figures first.  -> worst error / bound."""
    want, tol, slips = ref
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    ratio = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    print(f"{what}: worst error {np.nanmax(err):.3e}, worst error / bound {ratio:.3f}, bound up to {tol.max():.3e}")
    if report is not None:
        report.append(ratio)
    assert slips, f"{what}: no slip to check the bound with"
    for kind, slip in slips.items():
        check_bound(got, want, tol, slip, f"{what}, slip {kind}")
    return ratio
