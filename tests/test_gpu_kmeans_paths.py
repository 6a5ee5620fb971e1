"""csrc/labels_kmeans.hip driven directly at the cases of tests/kmeans_cases.py: k-means (labels, counts and code book equal the oracle ==
scipy bit for bit), the proxy build (sums and means to bits, squared norms under the derived float64 bound), label prep, plan and
replicate (array_equal to torch-CPU / numpy references).  tests/test_kmeans_host.py proves without a GPU that the references are right
and that every case reaches the path it is named for: the tail of a cluster beyond its 10 240 literal members (ties at both parities,
binade crossings, more than four of them, a wrong binade prediction, the literal fallback), every width group of the fast path, the
matrix-pipe assignment at one to four tiles of 16 clusters, the generic path at one to four features per lane, the stitch's ragged last
block, more segments than the assignment's LDS table holds; exact distance ties decided by every step of the matrix-pipe argmin (inside a
lane, across the xor-16 and xor-32 exchanges, the lower index in the higher lane group), true ties on an integer lattice at every assignment
kernel, rows whose label hangs on where the distance is rounded; replicated lists in groups of 2 .. 5 code books, with more than 32 base
segments, replicas and groups that skip a segment, ragged block ends, and more work items than workgroups.

Every k-means and proxy case runs twice: once through aoc_amd.ops with a workspace of its own, once through ctypes in ONE workspace
shared by the whole file that a differently shaped case has just used (what the frame pipeline does), into output buffers with a
sentinel margin.  The fast-path cases run a third time through aoc_kmeans_segmented (pool_rows = 0: the generic kernels) and must give
the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import kmeans_cases as kc

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4
MARGIN = 64
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    return aoc_amd


def dev(a):
    a = np.array(a, order="C")              # a copy: the cases' arrays are read-only
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def ptr(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset)


class Guarded:
    """A 4-byte-element device buffer between two sentinel margins, itself pre-filled with the sentinel."""

    def __init__(self, numel, dtype):
        self.raw = torch.full((int(numel) + 2 * MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
        self.n, self.dtype = int(numel), dtype

    @property
    def p(self):
        return ptr(self.raw, MARGIN)

    def get(self):
        """Payload as numpy; the margins must come back untouched."""
        raw = self.raw.cpu().numpy()
        assert (raw[:MARGIN] == SENTINEL).all() and (raw[MARGIN + self.n:] == SENTINEL).all(), "write outside the output buffer"
        return raw[MARGIN:MARGIN + self.n].view(self.dtype).copy()


_shared = {}


def shared_workspace(nbytes):
    """The file's one workspace: grown when a case needs more, never cleared, so every call finds what the last one left."""
    ws = _shared.get("ws")
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes) + 4096, dtype=torch.uint8, device="cuda")
        ws.fill_(0xA5)
        _shared["ws"] = ws
    return ws


@pytest.fixture(scope="module")
def on_device():
    """Device copies of a case's inputs, uploaded once."""
    cache = {}

    def get(case):
        if case.name not in cache:
            d = case.data()
            cache[case.name] = {k: dev(d[k]) for k in ("pool", "rows", "offs", "seg_k", "init")}
        return cache[case.name]
    return get


def km_call(aoc, case, t, entry, ws):
    """One k-means chain through ctypes in workspace `ws` -> (centroids, labels, counts) from guarded buffers."""
    L, d = aoc._lib.lib(), case.data()
    S, kmax, C, cap = len(d["seg_k"]), d["kmax"], d["C"], len(d["rows"])
    cen, lab, cnt = Guarded(S * kmax * C, np.float32), Guarded(cap, np.int32), Guarded(S * kmax, np.int32)
    lists = (ptr(t["rows"]), ptr(t["offs"]), ptr(t["seg_k"]), ptr(t["init"]), S)
    tail = (kmax, d["iters"], cap, cen.p, lab.p, cnt.p, ptr(ws), ws.numel(), aoc.ops._stream())
    if entry == "rep":
        rc = L.aoc_kmeans_segmented_rep(ptr(t["pool"]), len(d["pool"]), C, *lists, d["n_rep"], *tail)
    elif entry == "ex":
        rc = L.aoc_kmeans_segmented_ex(ptr(t["pool"]), len(d["pool"]), C, *lists, *tail)
    else:
        rc = L.aoc_kmeans_segmented(ptr(t["pool"]), C, *lists, *tail)
    assert rc == OK
    torch.cuda.synchronize()
    return cen.get().reshape(S, kmax, C), lab.get(), cnt.get().reshape(S, kmax)


def km_check(case, got, what):
    d = case.data()
    want_cen, want_lab, want_cnt, _ = case.reference()
    cen, lab, cnt = got
    for s, k in enumerate(d["seg_k"]):
        beg, end = d["offs"][s], d["offs"][s + 1]
        if k > 0:
            assert np.array_equal(lab[beg:end], want_lab[beg:end]), f"{what}: segment {s}: labels differ from the oracle"
        assert np.array_equal(cnt[s], want_cnt[s]), f"{what}: segment {s}: counts {cnt[s]} != {want_cnt[s]}"
        bad = np.nonzero((cen[s].view(np.int32) != want_cen[s].view(np.int32)).any(0))[0]
        assert bad.size == 0, f"{what}: segment {s}: code book differs from the oracle in features {bad[:12]} (slots j >= k must be 0)"


def scramble(aoc, case, on_device):
    """Run a differently shaped chain in the shared workspace (and hold it to the oracle as well)."""
    other = kc.STITCH_CASES[1] if case is not kc.STITCH_CASES[1] else kc.TAIL_CASES[4]
    d = other.data()
    ws = shared_workspace(aoc._lib.lib().aoc_kmeans_workspace_bytes(len(d["rows"]), len(d["seg_k"]), d["kmax"], d["C"]))
    km_check(other, km_call(aoc, other, on_device(other), "ex", ws), "workspace scrambler")


@pytest.mark.parametrize("case", kc.KMEANS_CASES, ids=lambda c: c.name)
def test_kmeans_case_equals_the_oracle_bit_for_bit(aoc, on_device, case):
    d, t = case.data(), on_device(case)
    L = aoc._lib.lib()
    cen, lab, cnt = aoc.ops.kmeans_segmented(t["pool"], t["rows"], t["offs"], t["seg_k"], t["init"], d["kmax"], d["iters"])
    first = (cen.cpu().numpy(), lab.cpu().numpy(), cnt.cpu().numpy())
    km_check(case, first, "own workspace")
    scramble(aoc, case, on_device)
    ws = shared_workspace(L.aoc_kmeans_workspace_bytes(len(d["rows"]), len(d["seg_k"]), d["kmax"], d["C"]))
    second = km_call(aoc, case, t, "ex", ws)
    km_check(case, second, "workspace another case has just used")
    live = np.concatenate([np.arange(d["offs"][s], d["offs"][s + 1]) for s in range(len(d["seg_k"])) if d["seg_k"][s] > 0])
    assert np.array_equal(first[0].view(np.int32), second[0].view(np.int32)) and np.array_equal(first[1][live], second[1][live])
    if kc.is_fast(case):
        third = km_call(aoc, case, t, "generic", ws)
        km_check(case, third, "aoc_kmeans_segmented (pool_rows = 0)")
        assert np.array_equal(first[0].view(np.int32), third[0].view(np.int32)), "the fast and the generic path differ"


@pytest.mark.parametrize("case", kc.REP_CASES, ids=lambda c: c.name)
def test_replicated_kmeans_equals_the_oracle_and_the_single_replica_chain(aoc, on_device, case):
    """aoc_kmeans_segmented_rep with n_rep stated (km_assign_mfma_rep_kernel: <25, 3> in groups of two at K = 40 and 48, <25, 1> in groups of
    up to six at K = 16; tests/test_kmeans_host.py holds every case to the plan and the edge it is named for) in the shared workspace a
    differently shaped chain has just used, into guarded outputs, and the same lists with n_rep = 1 (km_assign_mfma_kernel).  Both are held
    to the oracle, every replica of every case (rep_over_grid_cap too: its 22 replicas cost the oracle 1.5 s), and to each other: labels of
    the live segments, all counts, code books as int32."""
    d, t = case.data(), on_device(case)
    assert d["n_rep"] > 1
    scramble(aoc, case, on_device)
    ws = shared_workspace(aoc._lib.lib().aoc_kmeans_workspace_bytes(len(d["rows"]), len(d["seg_k"]), d["kmax"], d["C"]))
    fused = km_call(aoc, case, t, "rep", ws)
    km_check(case, fused, f"n_rep = {d['n_rep']}")
    plain = km_call(aoc, case, t, "ex", ws)
    km_check(case, plain, "n_rep = 1")
    live = np.concatenate([np.arange(d["offs"][s], d["offs"][s + 1]) for s in range(len(d["seg_k"])) if d["seg_k"][s] > 0])
    assert np.array_equal(fused[1][live], plain[1][live]), "labels"
    assert np.array_equal(fused[2], plain[2]), "counts"
    assert np.array_equal(fused[0].view(np.int32), plain[0].view(np.int32)), "code books"


# ------------------------------------------------------------------------------------------ proxies
def _proxy_inputs(c):
    d = kc.proxy_case(c)
    return d, {k: dev(d[k]) for k in ("pool", "fg_rows", "offs", "seg_k", "labels", "centroids")}


def proxy_check(d, prox, sqn, what):
    want, cnt, sq, bound = kc.proxy_reference(d)
    S, kmax, C = len(d["seg_k"]), d["kmax"], d["C"]
    prox, sqn = prox.reshape(S, 2, kmax, C), sqn.reshape(S, 2, kmax).astype(np.float64)
    for s in range(S):
        for a in range(2):
            bad = np.nonzero(prox[s, a].view(np.int32) != want[s, a].view(np.int32))
            assert bad[0].size == 0, f"{what}: segment {s}, set {a}: clusters {np.unique(bad[0])} features {np.unique(bad[1])[:12]} differ"
    inf = np.isinf(sq)
    assert np.array_equal(np.isposinf(sqn), inf), f"{what}: +inf norms {np.argwhere(np.isposinf(sqn) != inf)}"
    err = np.abs(sqn[~inf] - sq[~inf])
    print(f"{what}: norm error / bound max {np.max(err / bound[~inf]):.3f}")
    assert (err <= bound[~inf]).all(), f"{what}: norm error {err.max()} beyond the bound"


def proxy_call(aoc, d, t, ws):
    L = aoc._lib.lib()
    S, kmax, C = len(d["seg_k"]), d["kmax"], d["C"]
    prox, sqn = Guarded(S * 2 * kmax * C, np.float32), Guarded(S * 2 * kmax, np.float32)
    rc = L.aoc_build_proxies(ptr(t["pool"]), len(d["pool"]), C, ptr(t["fg_rows"]), ptr(t["offs"]), ptr(t["seg_k"]), ptr(t["labels"]),
                             ptr(t["centroids"]), S, kmax, len(d["labels"]), prox.p, sqn.p, ptr(ws), ws.numel() if ws is not None else 0,
                             aoc.ops._stream())
    assert rc == OK
    torch.cuda.synchronize()
    return prox.get(), sqn.get()


@pytest.mark.parametrize("c", [36, 100, 128, 130])
def test_build_proxies_sums_to_bits_and_norms_under_the_bound(aoc, on_device, c):
    """C = 36 / 100 / 128: the scan-sum pipeline (MODE 1); C = 130: km_accumulate_kernel<3, 1>."""
    d, t = _proxy_inputs(c)
    prox, sqn = aoc.ops.build_proxies(t["pool"], t["fg_rows"], t["offs"], t["seg_k"], t["labels"], t["centroids"])
    proxy_check(d, prox.cpu().numpy(), sqn.cpu().numpy(), "own workspace")
    scramble(aoc, None, on_device)
    ws = shared_workspace(aoc._lib.lib().aoc_build_proxies_workspace_bytes(len(d["labels"]), len(d["seg_k"]), d["kmax"]))
    proxy_check(d, *proxy_call(aoc, d, t, ws), "workspace a k-means chain has just used")


def test_build_proxies_slow_path_equals_the_fast_one(aoc):
    """C = 100 without a workspace takes km_accumulate_kernel<2, 1>: the same bits as the reference, hence as the fast path."""
    d, t = _proxy_inputs(100)
    slow = proxy_call(aoc, d, t, None)
    proxy_check(d, *slow, "NULL workspace")
    fast, _ = aoc.ops.build_proxies(t["pool"], t["fg_rows"], t["offs"], t["seg_k"], t["labels"], t["centroids"])
    assert np.array_equal(fast.cpu().numpy().reshape(-1).view(np.int32), slow[0].view(np.int32))


# ------------------------------------------------------------------------------------------ label prep
def label_prep_call(aoc, lab):
    L = aoc._lib.lib()
    n, n_obj = lab.shape
    t = dev(lab)
    out = dict(right_bits=Guarded(n, np.uint32), wrong_bits=Guarded(n, np.uint32), fg_rows=Guarded(n, np.int32),
               obj_rows=Guarded(n * n_obj, np.int32), counts=Guarded(n_obj + 1, np.int32), obj_offsets=Guarded(n_obj + 1, np.int32))
    ws = shared_workspace(L.aoc_label_prep_workspace_bytes(n, n_obj))
    rc = L.aoc_label_prep(ptr(t), n, n_obj, *[out[k].p for k in ("right_bits", "wrong_bits", "fg_rows", "obj_rows", "counts", "obj_offsets")],
                          ptr(ws), ws.numel(), aoc.ops._stream())
    assert rc == OK
    torch.cuda.synchronize()
    return {k: v.get() for k, v in out.items()}, t


def label_prep_check(aoc, lab):
    want = kc.label_prep_reference(lab)
    got, t = label_prep_call(aoc, lab)
    for k in ("right_bits", "wrong_bits", "counts", "obj_offsets"):
        assert np.array_equal(got[k], want[k]), k
    n_fg, n_rows = int(want["counts"][-1]), int(want["obj_offsets"][-1])
    assert np.array_equal(got["fg_rows"][:n_fg], want["fg_rows"]) and (got["fg_rows"][n_fg:] == SENTINEL).all()
    assert np.array_equal(got["obj_rows"][:n_rows], want["obj_rows"]) and (got["obj_rows"][n_rows:] == SENTINEL).all()
    right, wrong = aoc.ops.label_bits(t, want_wrong=False)
    assert wrong is None and np.array_equal(right.cpu().numpy().view(np.uint32), want["right_bits"])
    right, wrong = aoc.ops.label_bits(t)
    assert np.array_equal(right.cpu().numpy().view(np.uint32), want["right_bits"]) and np.array_equal(wrong.cpu().numpy().view(np.uint32), want["wrong_bits"])


@pytest.mark.parametrize("n_obj", kc.LABEL_OBJ)
@pytest.mark.parametrize("n", kc.LABEL_N)
def test_label_prep_equals_torch(aoc, n, n_obj):
    label_prep_check(aoc, kc.label_case(n, n_obj)[0])


def test_label_prep_with_nothing_kept(aoc):
    label_prep_check(aoc, kc.label_case(300, 4, nothing_kept=True)[0])


def test_label_prep_rejections(aoc):
    L = aoc._lib.lib()
    lab = dev(np.zeros((64, 31), np.float32))
    o = [Guarded(64 * 31, np.int32) for _ in range(6)]
    ws = shared_workspace(L.aoc_label_prep_workspace_bytes(64, 30))
    call = lambda n, n_obj, nbytes: L.aoc_label_prep(ptr(lab), n, n_obj, *[g.p for g in o], ptr(ws), nbytes, aoc.ops._stream())
    assert call(64, 30, ws.numel()) == OK
    assert call(0, 30, ws.numel()) == INVALID_ARG and call(64, 0, ws.numel()) == INVALID_ARG
    assert call(64, 31, ws.numel()) == UNSUPPORTED
    assert call(64, 30, L.aoc_label_prep_workspace_bytes(64, 30) - 1) == WORKSPACE
    bits = lambda n, n_obj: L.aoc_label_bits(ptr(lab), n, n_obj, o[0].p, None, aoc.ops._stream())
    assert bits(64, 30) == OK and bits(0, 30) == INVALID_ARG and bits(64, 0) == INVALID_ARG and bits(64, 31) == UNSUPPORTED
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ plan and replicate
@pytest.mark.parametrize("cluster_num", [0, 1, 16, 64])
def test_kmeans_plan_is_the_sticky_min(aoc, cluster_num):
    for counts in ([40, 0, 7, 90, 3], [40, 9, 7, 90], [5], [70, 65, 64, 100]):
        counts = np.array(counts, np.int32)
        got = aoc.ops.kmeans_plan(dev(np.append(counts, counts.sum()).astype(np.int32)), len(counts), cluster_num)
        assert np.array_equal(got.cpu().numpy(), kc.plan_reference(counts, cluster_num))


REP_LISTS = {
    "three_segments": ([0, 3, 3, 10], 10),
    "capacity_below_n_seg_plus_1": ([0, 1, 1, 2, 2, 3], 3),
    "capacity_above_the_lists": ([0, 300, 300, 777], 900),
}


def _rep_inputs(name):
    offs, cap = REP_LISTS[name]
    offs = np.array(offs, np.int32)
    rows = (np.arange(cap, dtype=np.int32) * 7 + 100)
    return rows, offs, cap


def _rep_check(got, want, cap, n_rep):
    rows_out, offs_out, k_out = got
    total = len(want[0]) // n_rep
    assert np.array_equal(rows_out[:n_rep * total], want[0]) and (rows_out[n_rep * total:] == SENTINEL).all()
    assert np.array_equal(offs_out, want[1]) and np.array_equal(k_out, want[2])


@pytest.mark.parametrize("n_rep", [1, 3])
@pytest.mark.parametrize("name", list(REP_LISTS))
def test_kmeans_replicate(aoc, name, n_rep):
    rows, offs, cap = _rep_inputs(name)
    S = len(offs) - 1
    seg_k = np.minimum(np.arange(S, dtype=np.int32) + 1, np.diff(offs)).astype(np.int32)
    out = Guarded(n_rep * cap, np.int32), Guarded(n_rep * S + 1, np.int32), Guarded(n_rep * S, np.int32)
    t = dev(rows), dev(offs), dev(seg_k)
    rc = aoc._lib.lib().aoc_kmeans_replicate(ptr(t[0]), ptr(t[1]), ptr(t[2]), S, n_rep, cap, out[0].p, out[1].p, out[2].p, aoc.ops._stream())
    assert rc == OK
    torch.cuda.synchronize()
    _rep_check([o.get() for o in out], kc.replicate_reference(rows, offs, seg_k, n_rep), cap, n_rep)


def _levels_call(aoc, rows_t, offs_t, S, n_rep, levels, cap, out, n_levels=None, rows_out=None):
    lv = np.ascontiguousarray(np.asarray(levels, np.int32))
    return aoc._lib.lib().aoc_kmeans_replicate_levels(ptr(rows_t), ptr(offs_t), S, n_rep, lv.ctypes.data_as(ctypes.c_void_p),
                                                      len(lv) if n_levels is None else n_levels, cap, out[0].p if rows_out is None else rows_out,
                                                      out[1].p, out[2].p, aoc.ops._stream())


@pytest.mark.parametrize("levels,n_rep", [([8, 16, 32], 1), ([8, 16, 32], 3), ([8, 16, 32], 4), ([8, 16, 32], 7), ([64], 1), ([64], 3), ([2, 0, 5], 5)])
@pytest.mark.parametrize("name", list(REP_LISTS))
def test_kmeans_replicate_levels(aoc, name, levels, n_rep):
    rows, offs, cap = _rep_inputs(name)
    S = len(offs) - 1
    out = Guarded(n_rep * cap, np.int32), Guarded(n_rep * S + 1, np.int32), Guarded(n_rep * S, np.int32)
    rows_t, offs_t = dev(rows), dev(offs)
    assert _levels_call(aoc, rows_t, offs_t, S, n_rep, levels, cap, out) == OK
    torch.cuda.synchronize()
    _rep_check([o.get() for o in out], kc.replicate_levels_reference(rows, offs, n_rep, levels), cap, n_rep)


def test_kmeans_replicate_levels_in_place_and_rejections(aoc):
    rows, offs, cap = _rep_inputs("three_segments")
    S = len(offs) - 1
    rows_t, offs_t = dev(rows), dev(offs)
    out = Guarded(3 * cap, np.int32), Guarded(3 * S + 1, np.int32), Guarded(3 * S, np.int32)
    # n_rep = 1 with rows_out == rows: only the offsets and cluster counts are written
    assert _levels_call(aoc, rows_t, offs_t, S, 1, [2], cap, out, rows_out=ptr(rows_t)) == OK
    torch.cuda.synchronize()
    want = kc.replicate_levels_reference(rows, offs, 1, [2])
    assert np.array_equal(rows_t.cpu().numpy(), rows) and np.array_equal(out[1].get()[:S + 1], want[1]) and np.array_equal(out[2].get()[:S], want[2])
    assert (out[0].get() == SENTINEL).all()
    call = lambda **kw: _levels_call(aoc, kw.get("rows", rows_t), kw.get("offs", offs_t), kw.get("S", S), kw.get("n_rep", 3), kw.get("levels", [8, 16]),
                                     kw.get("cap", cap), out, n_levels=kw.get("n_levels"), rows_out=kw.get("rows_out"))
    assert call() == OK
    assert call(rows_out=ptr(rows_t)) == INVALID_ARG                       # in place needs n_rep == 1
    assert call(S=0) == INVALID_ARG and call(n_rep=0) == INVALID_ARG and call(cap=0) == INVALID_ARG and call(n_levels=0) == INVALID_ARG
    assert call(rows=None) == INVALID_ARG and call(offs=None) == INVALID_ARG
    assert call(levels=[8, -1]) == INVALID_ARG and call(levels=[8, 65]) == INVALID_ARG
    assert call(levels=[1] * 9) == UNSUPPORTED
    assert call(n_rep=2 ** 28, cap=8) == INVALID_ARG                      # n_rep * rows_capacity must stay below 2^31
    torch.cuda.synchronize()
