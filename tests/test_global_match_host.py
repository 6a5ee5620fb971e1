"""The references and bounds of tests/global_match_bounds.py checked without a GPU.

1. The plain float64 references are the oracle's: oracle.matching.flattened_pairwise_distances with a min over each set, and
   nearest_neighbor_features_per_object.  On features on the grid 2^-8 both sides compute the same real numbers and agree to 1e-12.
2. numpy float32 restatements of the kernels' order of operations lie inside the bound at every case of the GPU test: load_a_fragment's
   four k-permuted streams (lane kq adds the squares of channels kq, kq + 4, ..) and its two shuffle adds; the staged-image norm of
   proxy_corr_min_kernel in kq-major order; gather_sqnorm_kernel's sequential norm; a k-ordered chain of rounded products for the matrix
   instruction (what its order really is, is not documented: the bound does not depend on it); `(q2 + p2) - 2 acc`, `d + padv` and the
   minimum; np.float16 round trips where the kernels have aoc_h / aoc_hr.
3. Every slip named by proxy_slips(case) / dense_slips(case) leaves the bound at every case, and the conditions on the reference hold there.
4. The restated dense_nsplit and max_tiles arithmetic against what can be called without a device, and the rejections of the two entries:
   return codes only, nothing is launched.
5. The same for the fp16-split entries: the float16 pieces of every operand and of the norms are numpy's own roundings; the restatements
   have convert_raw's two fmaf chains per lane half or split_rows_kernel's sequential sum for |q|^2 (fmaf restated as in
   test_decoder_bounds_host.py), cb_stage_frame's chain of 100 fmaf for a norm that is not supplied, and one k-ordered float32 chain of
   the exact float16 products for the matrix instructions; the take-over cases break a precondition and keep the fp32 bound."""
import ctypes

import numpy as np
import pytest
import torch

import global_match_bounds as gb
from global_match_bounds import DENSE_CASES, PROXY_CASES, PAD, PAD_H
from test_local_match_host import _dot_chain, _h, _lds_cand_sq_norm, _lds_query_sq_norm, emulate_transform

f32 = np.float32
OK, INVALID_ARG, WORKSPACE, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4


def _grid(a):
    return (np.round(a.astype(np.float64) * 256.0) / 256.0).astype(f32)


# ------------------------------------------------------------------------------------------ 1. the references are the oracle's
@pytest.mark.parametrize("name", ["C100_m17", "C36_m65", "C132_m16"])
def test_proxy_reference_is_the_oracle(name):
    from oracle import matching as om
    case = gb.PROXY_BY_NAME[name]
    inp = gb.proxy_inputs(case)
    q, p = _grid(inp["query"]), _grid(inp["proxies"])
    want, _ = gb.proxy_ref(q, p, None, inp["set_begin"], inp["set_size"])
    qt, pt = torch.from_numpy(q).double(), torch.from_numpy(p).double()
    d = om.flattened_pairwise_distances(pt, pt.pow(2).sum(1), qt, qt.pow(2).sum(1))          # [m, n_proxy]
    for s, (b, n) in enumerate(zip(inp["set_begin"], inp["set_size"])):
        got = d[:, b:b + n].min(1)[0].numpy() if n else np.full(case.m, PAD)                   # AEM:310-313 for an absent object
        assert np.abs(got - want[s]).max() <= 1e-12


@pytest.mark.parametrize("name", ["C100_O5", "C36_O17", "rows17", "m15_O3"])
def test_dense_reference_is_the_oracle(name):
    from oracle import matching as om
    case = gb.DENSE_BY_NAME[name]
    inp = gb.dense_inputs(case)
    q, pool = _grid(inp["query"]), _grid(inp["pool"])
    rows = inp["fg_rows"][:case.n_fg]
    want, _ = gb.dense_ref(q, pool, rows, inp["wrong"], case.n_obj)
    wrong = np.stack([(inp["wrong"][rows].astype(np.int64) >> o) & 1 for o in range(case.n_obj)], 1)
    labels = torch.from_numpy(1.0 - wrong.astype(np.float64))                                  # < 0.1 exactly where the bit is set
    got = om.nearest_neighbor_features_per_object(torch.from_numpy(pool[rows]).double(), torch.from_numpy(q).double(), labels)
    assert np.abs(got[:, :, 0].numpy().T - want).max() <= 1e-12


# ------------------------------------------------------------------------------------------ 2. float32 restatements of the kernels
def _seq_sq_norm(x, f16):
    """gather_sqnorm_kernel."""
    s = np.zeros(x.shape[0], f32)
    for t in range(x.shape[1]):
        s = s + (_h(x[:, t] * x[:, t]) if f16 else x[:, t] * x[:, t])
    return _h(s) if f16 else s


def _distances(q, p, q2, p2, f16):
    acc = _dot_chain(q, p, range(q.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        if f16:
            d = _h(_h(q2[:, None] + p2[None, :]) - f32(2) * _h(acc))
        else:
            d = (q2[:, None] + p2[None, :]) - f32(2) * acc
    assert d.dtype == f32
    return d


def emulate_proxy(case, inp):
    """proxy_corr_min_kernel's raw output [n_set, m], float32 step by step."""
    q, p, f16 = inp["query"], inp["proxies"], case.f16
    if f16:
        q, p = _h(q), _h(p)
    q2 = _lds_query_sq_norm(q, f16)
    sq = inp["sqnorm"]
    p2 = _lds_cand_sq_norm(p, f16) if sq is None or f16 else sq.copy()
    if sq is not None:
        p2 = np.where(np.isfinite(sq), p2, f32(np.inf)).astype(f32)
    d = _distances(q, p, q2, p2, f16)
    out = np.empty((len(inp["set_size"]), case.m), f32)
    for s, (b, n) in enumerate(zip(inp["set_begin"], inp["set_size"])):
        v = d[:, b:b + n].min(1) if n else np.full(case.m, np.inf, f32)
        out[s] = np.where(np.isinf(v), f32(PAD), v)
    return out


def emulate_dense(case, inp):
    """gather_sqnorm_kernel + dense_match_partial_kernel + dense_match_finalize_kernel, raw [n_obj, m]."""
    f16 = case.f16
    rows = inp["fg_rows"][:case.n_fg]
    q, p = inp["query"], inp["pool"][rows]
    if f16:
        q, p = _h(q), _h(p)
    d = _distances(q, p, _lds_query_sq_norm(q, f16), _seq_sq_norm(p, f16), f16)
    bits = inp["wrong"][rows].astype(np.int64)
    padv = f32(PAD_H if f16 else PAD)
    out = np.empty((case.n_obj, case.m), f32)
    for o in range(case.n_obj):
        w = ((bits >> o) & 1).astype(bool)
        dp = d + padv
        cand = np.where(w[None, :], _h(dp) if f16 else dp, d)
        out[o] = cand.min(1)
    return out


def _transform(raw, bias):
    n, m = raw.shape
    b = np.zeros(n, f32) if bias is None else bias
    return emulate_transform(raw.reshape(n, 1, 1, m), b).reshape(n, m)


@pytest.mark.parametrize("case", PROXY_CASES, ids=lambda c: c.name)
def test_proxy_bound_holds_the_emulation_and_sheds_the_slips(case):
    inp = gb.proxy_inputs(case)
    ref = gb.proxy_case_ref(case.name)
    want, tol, slips = ref["raw"]
    gb.check_conditions(case.name, want, ref["transformed"][0], bool(gb.absent_sets(case)))
    assert (tol[want == PAD] == 0).all()
    assert set(slips) == set(gb.proxy_slips(case)) and set(ref["transformed"][2]) == set(gb.proxy_slips(case, transformed=True))
    got = emulate_proxy(case, inp)
    gb.compare(got, ref["raw"], f"{case.name} raw")
    gb.compare(_transform(got, inp["bias"]), ref["transformed"], f"{case.name} transformed")


@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: c.name)
def test_dense_bound_holds_the_emulation_and_sheds_the_slips(case):
    inp = gb.dense_inputs(case)
    ref = gb.dense_case_ref(case.name)
    if case.n_fg == 0:
        assert np.isinf(ref["raw"][0]).all() and (ref["transformed"][0] == 1.0).all()
        return
    want, tol, slips = ref["raw"]
    gb.check_conditions(case.name, want, ref["transformed"][0], gb.absent_object(case.n_obj) is not None)
    assert set(slips) == set(gb.dense_slips(case))
    rows = inp["fg_rows"][:case.n_fg]
    assert case.n_fg < inp["pool"].shape[0] and not np.array_equal(rows, np.arange(case.n_fg))
    got = emulate_dense(case, inp)
    gb.compare(got, ref["raw"], f"{case.name} raw")
    gb.compare(_transform(got, inp["bias"]), ref["transformed"], f"{case.name} transformed")


def test_bounds_are_of_the_size_of_the_number_formats():
    """Distances of O(1): the fp32 bounds are a few hundred float32 roundings and the f16 ones a few float16 roundings, not a fitted 5e-6;
    and the lists hold what the GPU test says they hold."""
    want, tol, _ = gb.proxy_case_ref("C100_m150")["raw"]
    assert 0 < tol.max() < 2e-5 and 0.2 < np.median(want[want < PAD_H]) < 1.0
    want, tol, _ = gb.dense_case_ref("C100_O5")["raw"]
    assert 0 < tol[want < PAD_H].max() < 2e-5 and tol.max() < 2 * gb.U * PAD * 1.01
    want, tol, _ = gb.dense_case_ref("f16_C100_O17")["raw"]
    assert 0 < tol[want < PAD_H].max() < 4e-3 and set(np.unique(tol[want >= PAD_H])) <= {0.0, 32.0}
    assert {gb.proxy_instantiation(c.C) for c in PROXY_CASES} == {25, 32, 64}
    assert {(gb.dense_na(c.n_obj), c.n_obj > 16) for c in DENSE_CASES} == {(2, False), (1, False), (1, True)}
    assert {c.layout for c in DENSE_CASES if not c.f16} == {c.layout for c in DENSE_CASES if c.f16} == {"planes", "pixels"}


# ------------------------------------------------------------------------------------------ 4. host arithmetic and rejections
def test_launch_packing_of_the_structure_cases():
    """What the cases are there for, from the restated packing loop: launches, tiles, transposed output columns, dynamic LDS."""
    assert gb.proxy_max_tiles(100) == 17 and gb.proxy_max_tiles(256) == 7 and gb.proxy_max_tiles(128) == 15 and gb.proxy_max_tiles(4) == 20

    def plan(name):
        case = gb.PROXY_BY_NAME[name]
        inp = gb.proxy_inputs(case)
        return gb.proxy_launches(case.C, inp["set_begin"], inp["set_size"], inp["set_off"])

    assert [l[0] for l in plan("C100_m65")] == [16]
    assert [l[0] for l in plan("two_launches_C100")] == [17, 1]
    assert [l[0] for l in plan("three_launches_C256")] == [6, 7, 2]
    assert len(plan("C132_m17")) == 2
    for C in (100, 128, 256):
        (tiles, n_out, lds), = plan(f"fill_C{C}")
        assert tiles == gb.proxy_max_tiles(C) and n_out > 0 and 64 * 1024 < lds <= 160 * 1024
    assert [l[:2] for l in plan("singles70_C100")] == [(5, 0)] and [l[:2] for l in plan("singles64_C100")] == [(4, 64)]
    # the general call: a run of five, two runs of two split by the gap in set_begin, two runs of two split by the changed step
    case = gb.PROXY_BY_NAME["C100_m65"]
    st = gb.proxy_structure(case)
    assert sorted(st["set_size"].tolist())[:1] == [0] and {1, 2, 16, 17, 33} <= set(st["set_size"].tolist())


def _lib():
    import aoc_amd
    return aoc_amd._lib.lib()


@pytest.mark.parametrize("m,cap,n_obj", [(150, 500, 5), (150, 500, 3), (1, 4, 1), (257, 450, 3), (257, 450, 17), (4000, 9000, 4),
                                         (20000, 100, 5), (40000, 100, 2), (100000, 7, 30)])
def test_restated_nsplit_is_the_library_s(m, cap, n_obj):
    L = _lib()
    got = L.aoc_dense_match_workspace_bytes(ctypes.c_int64(m), ctypes.c_int64(cap), n_obj)
    assert got == gb.dense_workspace_bytes(m, cap, n_obj)


def test_rejections_without_a_gpu():
    """Return codes of calls that fail validation before any launch.  The oversized set comes second, after a valid one: the entry has to
    reject it before it enqueues anything for the first (without a device a launch attempt reports AOC_ERR_LAUNCH instead)."""
    L = _lib()
    vp = ctypes.c_void_p
    dummy = (ctypes.c_float * 64)()
    p = ctypes.cast(dummy, vp)
    arr = lambda t, v: (t * len(v))(*v)

    def proxy(m=16, C=100, n_proxy=200, begin=(0,), size=(4,)):
        sb, ss, so = arr(ctypes.c_int32, begin), arr(ctypes.c_int32, size), arr(ctypes.c_int64, [i * m for i in range(len(size))])
        return L.aoc_proxy_corr_min(p, ctypes.c_int64(m), C, p, None, n_proxy, len(size), sb, ss, so, None, p, ctypes.c_int64(1), 0, None)

    assert gb.proxy_max_tiles(256) * 16 == 112
    # eight valid sets of one tile each overflow a launch of seven tiles: a packing loop that rejects the 113-proxy set (8 tiles) only when
    # it reaches it has flushed by then
    assert proxy(C=256, begin=tuple(16 * i for i in range(8)) + (4,), size=(16,) * 8 + (113,)) == UNSUPPORTED
    assert proxy(C=100, begin=tuple(16 * i for i in range(18)) + (4,), size=(16,) * 18 + (17 * 16 + 1,), n_proxy=400) == UNSUPPORTED
    assert proxy(C=256, begin=(0, 4), size=(4, 113)) == UNSUPPORTED
    assert proxy(C=6) == UNSUPPORTED and proxy(C=260) == UNSUPPORTED
    assert proxy(m=0) == INVALID_ARG
    assert proxy(begin=(198,), size=(4,)) == INVALID_ARG                      # runs past n_proxy
    assert proxy(size=(-1,)) == INVALID_ARG

    i32 = (ctypes.c_int32 * 8)()
    ip = ctypes.cast(i32, vp)

    def dense(m=100, C=100, cap=50, n_obj=3, short=0):
        ws = int(L.aoc_dense_match_workspace_bytes(ctypes.c_int64(max(m, 1)), ctypes.c_int64(max(cap, 1)), min(n_obj, 30))) - short
        return L.aoc_dense_match_min(p, ctypes.c_int64(m), C, p, ip, ip, ctypes.c_int64(cap), ip, None, n_obj, p, ctypes.c_int64(1),
                                     ctypes.c_int64(m), 0, p, ctypes.c_size_t(ws), None)

    assert dense(C=132) == UNSUPPORTED and dense(C=6) == UNSUPPORTED and dense(n_obj=31) == UNSUPPORTED
    assert dense(m=0) == INVALID_ARG and dense(cap=0) == INVALID_ARG
    assert dense(short=1) == WORKSPACE
    ws = ctypes.c_size_t(1 << 30)
    assert L.aoc_dense_match_min_split(p, p, p, 1, ctypes.c_int64(100), 100, p, p, ip, ctypes.c_int64(50), ip, ip, ip, ip, ip, ip, None, 17,
                                       p, ctypes.c_int64(1), ctypes.c_int64(100), 0, p, ws, None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------ the fp16-split proxy kernels
def _fmaf(a, b, c):
    """fmaf as in test_decoder_bounds_host.py: the float32 rounding of the float64 sum of the exact product and the addend."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _half_channels(h):
    """The 50 channels of lane half h in the order of convert_raw's registers (load_half_row)."""
    return list(range(48 * h, 48 * h + 48)) + [96 + 2 * h, 97 + 2 * h]


def _split_q2(q, records):
    if records:             # split_rows_kernel: s += e * e in channel order
        s = np.zeros(q.shape[0], f32)
        for c in range(q.shape[1]):
            s = s + q[:, c] * q[:, c]
        return s
    parts = []
    for h in (0, 1):        # convert_raw: two fmaf chains over the even and the odd registers, sq + sq1; cb_halfsum adds the halves
        x = q[:, _half_channels(h)]
        sq, sq1 = np.zeros(q.shape[0], f32), np.zeros(q.shape[0], f32)
        for e in range(25):
            sq, sq1 = _fmaf(x[:, 2 * e], x[:, 2 * e], sq), _fmaf(x[:, 2 * e + 1], x[:, 2 * e + 1], sq1)
        parts.append(sq + sq1)
    return parts[0] + parts[1]


def emulate_split_dense(case, inp):
    """split_rows_kernel + the three-product accumulator of dense_prune_kernel + dense_split_finalize_kernel, raw [n_obj, m]: one k-ordered
    float32 chain of the exact float16 products, k-step by k-step (hi x hi, then the two cross products), the norm slots in the last one."""
    rows = inp["fg_rows"][:case.n_fg]
    q, p = inp["query"], inp["pool"][rows]
    qh, ql = (a.astype(f32) for a in gb.split_planes(q))
    ph, pl = (a.astype(f32) for a in gb.split_planes(p))
    pieces = gb.norm_pieces(gb.seq_sqnorm32(p)).astype(f32)
    acc = np.zeros((q.shape[0], p.shape[0]), f32)
    for s in range(7):
        ch = [c for c in range(16 * s, 16 * s + 16) if c < case.C]
        for a, b in ((qh, ph), (qh, pl), (ql, ph)):
            for c in ch:
                acc = acc + a[:, c][:, None] * b[:, c][None, :]
            if s == 6 and a is qh and b is ph:
                for k in range(3):
                    acc = acc + f32(32768.0) * pieces[k][None, :]
    d = gb.seq_sqnorm32(q)[:, None] + f32(-1.0 / 524288.0) * acc
    assert d.dtype == f32
    bits = inp["wrong"][rows].astype(np.int64)
    own = np.full((case.n_obj, case.m), np.inf, f32)
    for o in range(case.n_obj):
        cols = (bits >> o) & 1 == 0
        if cols.any():
            own[o] = d[:, cols].min(1)
    out = np.empty_like(own)
    for o in range(case.n_obj):
        others = np.delete(own, o, 0).min(0) if case.n_obj > 1 else np.full(case.m, np.inf, f32)
        out[o] = np.minimum(own[o], others + f32(PAD))
    return out


@pytest.mark.parametrize("case", gb.SPLIT_DENSE_CASES, ids=lambda c: c.name)
def test_split_dense_bound_holds_the_emulation_and_sheds_the_slips(case):
    inp = gb.dense_inputs(case, onehot=True)
    ref = gb.split_dense_case_ref(case.name)
    if case.n_fg == 0:
        assert np.isinf(ref["raw"][0]).all()
        return
    rows = inp["fg_rows"][:case.n_fg]
    # one-hot: every kept row is right for exactly one object and wrong for every other, as split_plan_kernel demands
    mask = (1 << case.n_obj) - 1
    r, w = inp["right"][rows].astype(np.int64), inp["wrong"][rows].astype(np.int64)
    assert ((r >> 31) & 1 == 1).all() and all(bin(v & mask).count("1") == 1 for v in r) and ((~w & mask) == (r & mask)).all()
    assert int(inp["counts"][:case.n_obj].sum()) == case.n_fg and inp["obj_offsets"][case.n_obj] == case.n_fg
    gb.check_conditions(case.name, ref["raw"][0], ref["transformed"][0], gb.absent_object(case.n_obj) is not None)
    assert set(ref["raw"][2]) == set(gb.split_dense_slips(case))
    got = emulate_split_dense(case, inp)
    gb.compare(got, ref["raw"], f"{case.name} raw")
    gb.compare(_transform(got, inp["bias"]), ref["transformed"], f"{case.name} transformed")


def test_hi_margin_case_is_decided_by_the_cross_products():
    """The planted pair of the hi_margin case, on the float64 values: row A is the nearest row of its object by more than twice the bound,
    the hi-plane product alone puts row B in front by more than that again, and the one_product slip leaves the bound at that very output."""
    case = gb.HI_MARGIN
    inp = gb.dense_inputs(case, onehot=True)
    rows = inp["fg_rows"][:case.n_fg]
    q = inp["query"][gb.HI_QUERY:gb.HI_QUERY + 1]
    norms = gb.seq_sqnorm32(inp["pool"][rows])
    D, E, _ = gb.split_pair_distances(q, inp["pool"][rows], norms, records=True)
    D1 = gb.split_pair_distances(q, inp["pool"][rows], norms, records=True, products=1)[2]
    mine = np.nonzero((inp["wrong"][rows].astype(np.int64) & 1) == 0)[0]
    a, b = gb.HI_POS
    assert a in mine and b in mine
    assert mine[D[0, mine].argmin()] == a and mine[D1[0, mine].argmin()] == b
    others = np.setdiff1d(mine, [a])
    assert D[0, others].min() - D[0, a] > 2 * E[0].max() and D1[0, a] - D1[0, b] > 4 * E[0].max()
    want, tol, slips = gb.split_dense_case_ref(case.name)["raw"]
    assert want[0, gb.HI_QUERY] == D[0, a] and abs(slips["one_product"][0, gb.HI_QUERY] - want[0, gb.HI_QUERY]) > tol[0, gb.HI_QUERY]


@pytest.mark.parametrize("case", gb.DENSE_TAKEOVER_CASES, ids=lambda c: c.name)
def test_dense_takeover_cases_set_the_gate_and_keep_the_fp32_bound(case):
    inp = gb.dense_takeover_inputs(case)
    if "value" in case.name:
        x = inp["query"] if "query" in case.name else inp["pool"][inp["fg_rows"][:case.n_fg]]
        assert np.abs(x).max() * 1024 > 65000 and (x.astype(np.float64) ** 2).sum(1).max() > 4000
    ref = gb.dense_takeover_ref(case.name)
    assert set(ref["raw"][2]) == set(gb.dense_slips(case))
    got = emulate_dense(case, inp)
    gb.compare(got, ref["raw"], f"{case.name} raw")
    gb.compare(_transform(got, inp["bias"]), ref["transformed"], f"{case.name} transformed")


def emulate_split_proxy(case, inp, records):
    """cb_stage_frame + cb_tile_compute, raw [n_set, m]: float32 accumulation of the exact float16 products as one k-ordered chain (k-step by
    k-step: hi x hi, lo x hi, hi x lo), the norm slots in the hi x hi product of the last k-step."""
    q, p, sq = inp["query"], inp["proxies"], inp["sqnorm"]
    qh, ql = (a.astype(f32) for a in gb.split_planes(q))
    ph, pl = (a.astype(f32) for a in gb.split_planes(p))
    if sq is None:          # the chain of 100 fmaf in channel order
        norm = np.zeros(p.shape[0], f32)
        for c in range(100):
            norm = _fmaf(p[:, c], p[:, c], norm)
    else:
        norm = np.where(np.isfinite(sq), sq, 0).astype(f32)
    pieces = gb.norm_pieces(norm).astype(f32)
    order = [c for pair in zip(_half_channels(0), _half_channels(1)) for c in pair]     # both halves' slots of a k-step side by side
    acc = np.zeros((q.shape[0], p.shape[0]), f32)
    for s in range(7):
        ch = order[16 * s:16 * s + 16]
        for a, b in ((qh, ph), (qh, pl), (ql, ph)):
            for c in ch:
                acc = acc + a[:, c][:, None] * b[:, c][None, :]
            if s == 6 and a is qh and b is ph:
                for k in range(3):
                    acc = acc + f32(32768.0) * pieces[k][None, :]
    assert acc.dtype == f32
    d = _split_q2(q, records)[:, None] + f32(-1.0 / 524288.0) * acc
    if sq is not None:
        d = np.where(np.isfinite(sq)[None, :], d, f32(np.inf)).astype(f32)
    out = np.empty((len(inp["set_size"]), case.m), f32)
    for i, (b, n) in enumerate(zip(inp["set_begin"], inp["set_size"])):
        v = d[:, b:b + n].min(1) if n else np.full(case.m, np.inf, f32)
        out[i] = np.where(np.isinf(v), f32(PAD), v)
    return out


def emulate_cb_transform(raw, bias):
    """cb_transform in float32 (numpy's exp2 and division for the two hardware instructions)."""
    b = np.zeros(raw.shape[0], f32) if bias is None else bias
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp2((raw + b[:, None]) * f32(-1.44269504088896341))
        out = f32(2) * (f32(1) / (f32(1) + e)) - f32(1)
    assert out.dtype == f32
    return out


@pytest.mark.parametrize("records", [False, True], ids=["batched", "records"])
@pytest.mark.parametrize("case", gb.SPLIT_CASES, ids=lambda c: c.name)
def test_split_proxy_bound_holds_the_emulation_and_sheds_the_slips(case, records):
    inp = gb.proxy_inputs(case)
    ref = gb.split_case_ref(case.name, records)
    want, tol, slips = ref["raw"]
    gb.check_conditions(case.name, want, ref["transformed"][0], bool(gb.absent_sets(case)))
    assert (tol[want == PAD] == 0).all() and {"two_products", "one_product", "norm_one_piece"} <= set(slips)
    got = emulate_split_proxy(case, inp, records)
    gb.compare(got, ref["raw"], f"{case.name} raw")
    gb.compare(emulate_cb_transform(got, inp["bias"]), ref["transformed"], f"{case.name} transformed")


@pytest.mark.parametrize("case", gb.TAKEOVER_CASES, ids=lambda c: c.name)
def test_takeover_cases_break_a_precondition_and_keep_the_fp32_bound(case):
    inp = gb.takeover_inputs(case)
    x = inp["query"] if case.name == "takeover_query" else inp["proxies"]
    assert np.abs(x).max() * 1024 > 65000 and (x.astype(np.float64) ** 2).sum(1).max() > 4000
    ref = gb.takeover_case_ref(case.name)
    got = emulate_proxy(case, inp)
    gb.compare(got, ref["raw"], f"{case.name} raw")
    gb.compare(_transform(got, inp["bias"]), ref["transformed"], f"{case.name} transformed")


def test_split_reference_is_the_fp32_reference():
    """The same float64 minimum under another bound: about 1e-5 on distances of O(1), gamma(337) on the same data."""
    case = gb.SPLIT_BY_NAME["split_m150"]
    inp = gb.proxy_inputs(case)
    want, tol, _ = gb.split_case_ref(case.name)["raw"]
    w32, t32 = gb.proxy_ref(inp["query"], inp["proxies"], inp["sqnorm"], inp["set_begin"], inp["set_size"])
    assert np.abs(want - w32).max() <= 1e-12 and t32.max() < tol.max() < 5e-5
