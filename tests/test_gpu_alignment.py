"""The pointer-alignment contract on the device (include/aoc_hip.h "Pointer alignment", tests/alignment_cases.py; the host half is
tests/test_alignment_host.py).

No test here launches a kernel with a class-16 pointer off the 16-byte grid.  Through aoc_amd.ops every variant is first run under the decoding
stub (nothing is launched) and held to the host rule; only then is it run for real: a class-16 input off the grid reaches the library as an
aligned copy, a class-4 tensor as the caller's own storage, read and written with 4-byte accesses -- so every output must equal the aligned
call's bit for bit and the NaN / sentinel margins around the caller's tensors must stand.  The library's own refusal is host code: with the
front-end's copy switched off a class-16 pointer 4 bytes off the grid must come back as AOC_ERR_INVALID_ARG with outputs and workspace
untouched, and the same call, aligned, in the same workspace must give the canonical bits.

Shapes: the contract scene of tests/ops_contract_cases.py (C = 100, 48 pool rows, 40 pixels; a 5 x 6 map at C = 4; the tiny frame) and the
smallest cases of the kernels' own bounds modules at the other widths and paths (C = 36 / 4 / 128 dense matching, the register and the
LDS-image local kernels on 3 x 8 to 13 x 21 maps, 300-row replicated segments, the 12 000-row K = 1 segment that reaches the sum tail and the
ordered mean; the gradient entries on the cases of match_grad_bounds (dense C = 4 / 36 / 128 / 100, proxy C = 36 / 128 / 4), local_grad_bounds
(3 x 5 to 31 x 33 maps, both forward kernels, an atrous rate) and cluster_grad_bounds (set argmin and gradient at C = 4 / 36 / 100 / 128, the
pull-back through the proxy means at one and two levels))."""
import ctypes

import numpy as np
import pytest
import torch

import alignment_cases as ac
import ops_contract_cases as occ

pytestmark = pytest.mark.gpu

NAN = float("nan")
FILL = {torch.float32: NAN, torch.int32: -77, torch.uint8: 201}
INVALID = "AOC_ERR_INVALID_ARG"


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()
    return aoc_amd


def moved(t, k):
    """-> (the off-grid view, its guard: (buffer, first element, elements, fill))."""
    v, buf, lo = ac.off_grid(t, k, FILL[t.dtype])
    return v, (buf, lo, t.numel(), FILL[t.dtype])


def intact(guard):
    return ac.margins_intact(*guard)


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def same(got, want):
    """Equal shapes, dtypes and BITS (stricter than torch.equal, and NaN / inf compare like any other pattern)."""
    return len(got) == len(want) and all(g.shape == w.shape and g.dtype == w.dtype and torch.equal(_bytes(g), _bytes(w)) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------ through ops: the contract scene
@pytest.mark.parametrize("name", ac.covering())
def test_ops_off_the_grid(aoc, name):
    ops = aoc.ops
    errors = occ.ERRORS + (aoc._lib.AocHipError,)
    case, canon_a, canon_rec, canon_stub = ac.canonical(name, "cuda")
    a0 = case.build(ops, "cuda")
    want = [t.clone() for t in case.collect(case.call(ops, a0), a0)]
    torch.cuda.synchronize()
    failed, ran = [], 0
    for label, names, k in ac.variants(case, canon_a):
        a, guards = dict(case.build(ops, "cuda")), {}
        for n in names:
            a[n], guards[n] = moved(a[n], k)
        err, rec, stub = ac.run(case, a)                                     # under the stub: nothing is launched
        bad = ac.check_variant(case, canon_a, canon_stub, canon_rec, a, names, err, rec, stub, "cuda")
        if bad:
            failed.append(f"({name}, {label}) NOT LAUNCHED: {'; '.join(bad)}")
            continue
        ran += 1
        if err is None:
            got = case.collect(case.call(ops, a), a)
            torch.cuda.synchronize()
            if not same(got, want):
                failed.append(f"({name}, {label}): an output differs from the aligned call's")
        else:
            snaps = {n: g[0].clone() for n, g in guards.items()}
            with pytest.raises(errors):
                case.call(ops, a)
            torch.cuda.synchronize()
            for n, snap in snaps.items():
                if not torch.equal(guards[n][0].view(torch.uint8), snap.view(torch.uint8)):
                    failed.append(f"({name}, {label}): the refused call wrote into {n}")
        for n, g in guards.items():
            if not intact(g):
                failed.append(f"({name}, {label}): the margins around {n} were written")
    assert ran, f"{name}: no variant was run"
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------ the library's own refusal
def class16_positions(name):
    """{tensor of the case: [(entry, parameter)] class-16 positions it reaches} -- those the library enforces unconditionally."""
    case, a, _, stub = ac.canonical(name)
    out = {}
    for n in ac.tensors(case, a):
        hits = [(e, p) for e, p, addr in stub.seen if addr == a[n].data_ptr() and ac.CLASS[e][p] == 16 and e not in ac.CONDITIONAL]
        if hits:
            out[n] = hits
    return out


REFUSED = [n for n in ac.covering() if class16_positions(n)]
WS16 = ["kmeans_segmented", "build_proxies", "dense_match_min_split", "cluster_chain"]       # class-16 workspaces that ops allocates through _ws


class Workspaces:
    """Stands in for ops._ws: sentinel-filled buffers that are remembered (by size) and handed out again; `shift` bytes off the grid on demand."""

    def __init__(self, shift=0):
        self.bufs, self.shift = {}, shift

    def __call__(self, nbytes, device):
        n = max(int(nbytes), 16)
        if n not in self.bufs:
            self.bufs[n] = torch.full((n + 16,), 201, dtype=torch.uint8, device=device)
            assert self.bufs[n].data_ptr() % 16 == 0
        return self.bufs[n][self.shift:self.shift + n]

    def untouched(self):
        return all(bool((b == 201).all()) for b in self.bufs.values())


def _whole(t):
    return t._base if t._base is not None else t


def _refused_call(aoc, monkeypatch, case, a, ws, copy_off=True):
    """The call must come back as AOC_ERR_INVALID_ARG with every caller-provided output and every workspace untouched."""
    ops = aoc.ops
    outs = {n: _whole(t) for n, t in a.items() if torch.is_tensor(t) and ac.role(case, n) == occ.OUT}
    snaps = {n: t.clone() for n, t in outs.items()}
    with monkeypatch.context() as mp:
        if copy_off:
            mp.setattr(ops, "_a16", lambda what, t, output=False: t)
        mp.setattr(ops, "_ws", ws)
        with pytest.raises(aoc._lib.AocHipError, match=INVALID):
            case.call(ops, a)
    torch.cuda.synchronize()
    bad = [f"the refused call wrote into {n}" for n, t in outs.items() if not torch.equal(t.view(torch.uint8), snaps[n].view(torch.uint8))]
    if not ws.untouched():
        bad.append("the refused call wrote into its workspace")
    return bad


def _aligned_in(aoc, monkeypatch, case, ws):
    ops = aoc.ops
    ws.shift = 0
    a = case.build(ops, "cuda")
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_ws", ws)
        got = [t.clone() for t in case.collect(case.call(ops, a), a)]
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", REFUSED)
def test_library_refuses_class16_off_the_grid(aoc, monkeypatch, name):
    """Each class-16 pointer of the call 4 bytes off, one at a time, with the front-end's copy switched off: the refusal is the library's."""
    ops, case = aoc.ops, occ.CASES[name]
    a0 = case.build(ops, "cuda")
    want = [t.clone() for t in case.collect(case.call(ops, a0), a0)]
    torch.cuda.synchronize()
    failed = []
    for n, hits in class16_positions(name).items():
        a = dict(case.build(ops, "cuda"))
        a[n], guard = moved(a[n], 4)
        ws = Workspaces()
        failed += [f"({name}, {n} -> {hits[0][0]}.{hits[0][1]}): {b}" for b in _refused_call(aoc, monkeypatch, case, a, ws)]
        if not intact(guard):
            failed.append(f"({name}, {n}): the margins were written")
        if not same(_aligned_in(aoc, monkeypatch, case, ws), want):
            failed.append(f"({name}, {n}): the aligned call in the same workspace differs from the canonical one")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("name", WS16)
def test_library_refuses_a_class16_workspace_off_the_grid(aoc, monkeypatch, name):
    ops, case = aoc.ops, occ.CASES[name]
    assert any(p == "workspace" and ac.CLASS[e][p] == 16 for e, p, _ in ac.canonical(name)[3].seen)
    a0 = case.build(ops, "cuda")
    want = [t.clone() for t in case.collect(case.call(ops, a0), a0)]
    torch.cuda.synchronize()
    ws = Workspaces(shift=4)
    bad = _refused_call(aoc, monkeypatch, case, case.build(ops, "cuda"), ws, copy_off=False)
    assert not bad, f"{name}: " + "; ".join(bad)
    assert same(_aligned_in(aoc, monkeypatch, case, ws), want), f"{name}: the aligned call in the same workspace differs from the canonical one"


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_kmeans_refuses_directly(aoc):
    """aoc_kmeans_segmented_rep through ctypes: pool, centroids (an output ops allocates itself) and workspace 4 bytes off, one at a time."""
    ops, L = aoc.ops, aoc._lib.lib()
    s = occ.scene(ops, "cuda")
    P = occ.POOL
    n_seg, kmax, C, cap = P["O"], P["kmax"], P["C"], s["obj_rows"].numel()
    want = [t.clone() for t in ops.kmeans_segmented(s["pool"], s["obj_rows"], s["seg_offsets"], s["seg_k"], s["init_rows"], kmax)]
    nbytes = int(L.aoc_kmeans_workspace_bytes(cap, n_seg, kmax, C))

    def call(pool, cen, ws):
        lab, cnt = occ.blank("cuda", (cap,), torch.int32), occ.blank("cuda", (n_seg, kmax), torch.int32)
        rc = L.aoc_kmeans_segmented_rep(_p(pool), s["n"], C, _p(s["obj_rows"]), _p(s["seg_offsets"]), _p(s["seg_k"]), _p(s["init_rows"]), n_seg, 1, kmax, 20, cap,
                                        _p(cen), _p(lab), _p(cnt), _p(ws), nbytes, ops._stream())
        torch.cuda.synchronize()
        return rc, lab, cnt

    ws_buf = torch.full((nbytes + 16,), 201, dtype=torch.uint8, device="cuda")
    for which in ("pool", "centroids", "workspace"):
        pool = moved(s["pool"], 4)[0] if which == "pool" else s["pool"]
        cen, cen_guard = moved(occ.blank("cuda", (n_seg, kmax, C)), 4) if which == "centroids" else (occ.blank("cuda", (n_seg, kmax, C)), None)
        ws = ws_buf[4:4 + nbytes] if which == "workspace" else ws_buf[:nbytes]
        rc, lab, cnt = call(pool, cen, ws)
        assert rc == -1, f"{which} 4 bytes off the grid: return code {rc}"
        assert bool((cen == occ.SENTINEL[torch.float32]).all()) and bool((lab == -77).all()) and bool((cnt == -77).all()), f"{which}: an output was written"
        assert bool((ws_buf == 201).all()), f"{which}: the workspace was written"
    cen = occ.blank("cuda", (n_seg, kmax, C))
    rc, lab, cnt = call(s["pool"], cen, ws_buf[:nbytes])
    assert rc == 0 and torch.equal(cen, want[0]) and torch.equal(cnt, want[2]) and torch.equal(lab[:s["total"]], want[1][:s["total"]])


def test_atrous_subsample_refusal_and_the_four_byte_path(aoc):
    """The oldest of the host-side checks: X % 4 == 0 moves 16 bytes per thread and refuses either pointer off the grid; every other X moves
    4 bytes at a time and accepts both anywhere, with the aligned call's bits."""
    ops, L = aoc.ops, aoc._lib.lib()
    h, w, rate = 5, 7, 2
    H, W = 3, 4
    for X in (4, 8):
        x = occ.fl(occ._rs(4), h, w, X).cuda()
        want = ops.atrous_subsample(x, rate)
        assert torch.equal(want.cpu(), x.cpu()[::rate, ::rate])
        for which in ("in", "out"):
            src = moved(x, 4)[0] if which == "in" else x
            dst, guard = moved(occ.blank("cuda", (H, W, X)), 4) if which == "out" else (occ.blank("cuda", (H, W, X)), None)
            rc = L.aoc_atrous_subsample(_p(src), h, w, X, rate, _p(dst), ops._stream())
            torch.cuda.synchronize()
            assert rc == -1, f"X = {X}, `{which}` 4 bytes off the grid: return code {rc}"
            assert bool((dst == occ.SENTINEL[torch.float32]).all()), f"X = {X}: the refused call wrote its output"
        assert torch.equal(ops.atrous_subsample(moved(x, 4)[0], rate), want), "ops copies the input"
    for X in (3, 5):
        x = occ.fl(occ._rs(5), h, w, X).cuda()
        want = ops.atrous_subsample(x, rate)
        for k in ac.OFFSETS:
            src, g_in = moved(x, k)
            dst, g_out = moved(occ.blank("cuda", (H, W, X)), k)
            rc = L.aoc_atrous_subsample(_p(src), h, w, X, rate, _p(dst), ops._stream())
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(dst, want) and intact(g_in) and intact(g_out), f"X = {X}, {k} bytes off"


def test_batched_correlation_refuses_where_it_used_to_fall_back(aoc, monkeypatch):
    """aoc_proxy_corr_min_batched with a misaligned query or proxy table used to switch the split path off and run the exact-fp32 kernel on the
    same pointers; it refuses now (precision 'split' and 'fp32' alike), and aoc_proxy_corr_min_records refuses query_rec and the table."""
    ops = aoc.ops
    for name, fields in (("proxy_corr_min_batched", ("query", "table")), ("proxy_corr_min_records", ("q_records", "table"))):
        case = occ.CASES[name]
        for n in fields:
            a = dict(case.build(ops, "cuda"))
            a[n] = moved(a[n], 4)[0]
            bad = _refused_call(aoc, monkeypatch, case, a, Workspaces())
            assert not bad, f"{name}, {n}: " + "; ".join(bad)
    a = dict(occ.CASES["proxy_corr_min_batched"].build(ops, "cuda"))
    a["table"] = moved(a["table"], 4)[0]
    snap = a["out"].clone()
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_a16", lambda what, t, output=False: t)
        with pytest.raises(aoc._lib.AocHipError, match=INVALID):
            ops.proxy_corr_min_batched([(a["query"], a["table"], a["proxy_sqnorm"], a["set_bias"], a["out"])], *occ.set_lists(), precision="fp32")
    torch.cuda.synchronize()
    assert torch.equal(a["out"], snap)
    # the records form reads `query` in the take-over only, with 4-byte loads: class 4, accepted anywhere, same bits
    case = occ.CASES["proxy_corr_min_records"]
    a0 = case.build(ops, "cuda")
    want = [t.clone() for t in case.collect(case.call(ops, a0), a0)]
    a = dict(case.build(ops, "cuda"))
    a["query"], guard = moved(a["query"], 4)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_a16", lambda what, t, output=False: t)
        got = case.collect(case.call(ops, a), a)
    torch.cuda.synchronize()
    assert same(got, want) and intact(guard)


# ------------------------------------------------------------------------------------------ through ops: the other widths and paths
def sweep(call, tensors, what, outputs=()):
    """call(**tensors) -> list of outputs.  Every tensor 4 / 8 / 12 bytes off the grid inside NaN / sentinel margins, one at a time, then all the
    inputs at once: the aligned call's bits, the margins untouched.  `outputs` names the caller-provided destinations among the tensors."""
    want = [t.clone() for t in call(**{k: v.clone() for k, v in tensors.items()})]
    torch.cuda.synchronize()
    assert want, f"{what}: no output is compared"
    failed = []
    inputs = [n for n in tensors if n not in outputs]
    plan = [([n], k) for n in tensors for k in ac.OFFSETS] + [(inputs, k) for k in ac.OFFSETS]
    for names, k in plan:
        a, guards = {n: v.clone() for n, v in tensors.items()}, {}
        for n in names:
            a[n], guards[n] = moved(a[n], k)
        got = call(**a)
        torch.cuda.synchronize()
        if not same(got, want):
            failed.append(f"{what}, {'+'.join(names)} {k} bytes off: an output differs from the aligned call's")
        failed += [f"{what}, {n} {k} bytes off: the margins were written" for n, g in guards.items() if not intact(g)]
    assert not failed, "\n".join(failed)


def _t(x):
    x = np.array(x)                         # a writable copy: the case data is read-only
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


@pytest.mark.parametrize("name", ["C36_O1", "C4_O7", "C128_O7", "m15_O3", "rows17"])
def test_dense_matching_at_its_other_widths(aoc, name):
    import global_match_bounds as gb
    ops = aoc.ops
    case = gb.DENSE_BY_NAME[name]
    d = gb.dense_inputs(case)
    m, O, n_pool = case.m, case.n_obj, d["pool"].shape[0]
    tensors = dict(query=_t(d["query"]), pool=_t(d["pool"]), fg_rows=_t(d["fg_rows"]), wrong_bits=_t(d["wrong"]), counts=_t(d["counts"]), bias=_t(d["bias"]),
                   out=occ.blank("cuda", (O, m)), arg=occ.blank("cuda", (O, m), torch.int32))

    def call(query, pool, fg_rows, wrong_bits, counts, bias, out, arg):
        prep = ops.LabelPrep()
        prep.n, prep.n_obj, prep.fg_rows, prep.wrong_bits, prep.counts = n_pool, O, fg_rows, wrong_bits, counts
        prep.right_bits = prep.obj_rows = prep.obj_offsets = None
        plain = torch.empty(O, m, device="cuda")
        ops.dense_match_min(query, pool, prep, bias, plain, 1, m)
        ops.dense_match_argmin(query, pool, prep, bias, out, arg, 1, m)
        return [out, arg, plain]
    sweep(call, tensors, f"dense {name}", outputs=("out", "arg"))


@pytest.mark.parametrize("name", ["pair_C100", "pair_C36", "reg_map_3x8_r1_3", "reg_rate3_r3_7_12", "lds_C4_map_3x17", "reg_f16_C100_rate2"])
def test_local_matching_in_both_kernels(aoc, name):
    import local_match_bounds as lb
    ops = aoc.ops
    case = lb.CASE_BY_NAME[name]
    d = lb.local_inputs(case)
    tensors = dict(query=_t(d["query"]), prev=_t(d["prev"]), bits=_t(d["bits"]), bias=_t(d["bias"]))
    if case.pair:
        tensors["prev_b"] = _t(d["prev_b"])

    def call(query, prev, bits, bias, prev_b=None):
        outs = [ops.local_window_match(query, prev, bits, case.radii, bias, case.n_obj, True, case.rate, case.f16)]
        if not case.f16:
            outs += list(ops.local_window_match_argmin(query, prev, bits, case.radii, bias, case.n_obj, True, case.rate))
        if prev_b is not None:
            outs.append(ops.local_window_match_pair(query, prev, prev_b, bits, case.radii, bias, case.n_obj))
        return outs
    sweep(call, tensors, f"local {name}")


@pytest.mark.parametrize("name", ["tail_n12000_it2", "mfma_K1_tail", "rep_K16_n13"])
def test_kmeans_and_proxy_build_on_their_paths(aoc, name):
    """The 12 000-row K = 1 segment reaches the sum tail's and the ordered mean's LDS-direct loads (C = 12: the rank kernel; C = 100: the matrix
    pipe); 13 replicas of 300 / 130 / 600-row segments take the replica-fused assignment."""
    import kmeans_cases as kc
    ops = aoc.ops
    case = {c.name: c for c in kc.KMEANS_CASES + kc.REP_CASES}[name]
    d = case.data()
    tensors = dict(pool=_t(d["pool"]), rows=_t(d["rows"]), offs=_t(d["offs"]), seg_k=_t(d["seg_k"]), init=_t(d["init"]))
    live = np.concatenate([np.arange(d["offs"][s], d["offs"][s + 1]) for s in range(len(d["seg_k"])) if d["seg_k"][s] > 0])
    live = torch.from_numpy(live).cuda()

    def call(pool, rows, offs, seg_k, init):
        cen, lab, cnt = ops.kmeans_segmented(pool, rows, offs, seg_k, init, d["kmax"], d["iters"], n_rep=d["n_rep"])
        prox, sqn = ops.build_proxies(pool, rows, offs, seg_k, lab, cen)
        return [cen, lab[live], cnt, prox, sqn]
    sweep(call, tensors, f"k-means {name}")


def test_frame_call_refuses_its_workspace_off_the_grid(aoc):
    """aoc_frame_enqueue's own workspace (ops.FrameCall allocates it) 4 bytes off: refused, nothing written, the state record untouched; the same
    bytes on the grid then give the canonical frame."""
    ops = aoc.ops
    case = occ.CASES["FrameCall"]
    a0 = case.build(ops, "cuda")
    want = [t.clone() for t in case.collect(case.call(ops, a0), a0)]
    cfg, mc = aoc.synthetic.CONFIGS["tiny"], aoc.hotpath.MatchingConfig()
    call = ops.FrameCall(cfg.h, cfg.w, cfg.c, cfg.n_obj, 2, mc.MODEL_MULTI_LOCAL_DISTANCE, mc.cluster_levels, mc.MODEL_MATCHING_BACKGROUND, mc.MODEL_EPSILON,
                         torch.device("cuda", 0))
    call.reset()
    n = call.ws.numel()
    buf = torch.full((n + 16,), 201, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    a = case.build(ops, "cuda")
    prep = occ.mk_prep(ops, a)
    prep.n = cfg.h * cfg.w
    args = [a[k] for k in ("ref_emb", "ref_labels", "prev_emb", "prev_labels", "cur_emb", "bias")] + [prep, a["table"], a["sqn"]]
    table = a["table"].clone()
    call.ws = buf[4:4 + n]
    with pytest.raises(aoc._lib.AocHipError, match=INVALID):
        call(*args, pool_key=1)
    torch.cuda.synchronize()
    assert bool((buf == 201).all()) and torch.equal(a["table"], table) and call.state.initialised == 0
    call.ws = buf[:n]
    got = list(call(*args, pool_key=1))
    torch.cuda.synchronize()
    assert same(got, want)


def test_cached_correlation_refuses_its_workspace_off_the_grid(aoc):
    """aoc_proxy_corr_min_records_cached keeps tile tables with 8-byte members in its workspace (ops.CorrTableCache allocates it): 4 bytes off
    is refused before the tables or the host key are written."""
    ops = aoc.ops
    case = occ.CASES["proxy_corr_min_records(cache)"]
    a0 = case.build(ops, "cuda")
    want = [t.clone() for t in case.collect(case.call(ops, a0), a0)]
    a = case.build(ops, "cuda")
    qs = occ.mk_split(ops, a["q_records"], a["q_sqnorm"], a["overflow"], occ.POOL["m"], True)
    cache = ops.CorrTableCache(a["query"].device)
    n = cache.ws.numel()
    buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")         # (the flag word of this workspace is zeroed once by its owner)
    assert buf.data_ptr() % 16 == 0
    frames = [(a["query"], qs, a["table"], a["proxy_sqnorm"], a["set_bias"], a["out"])]
    snap = a["out"].clone()
    cache.ws = buf[4:4 + n]
    with pytest.raises(aoc._lib.AocHipError, match=INVALID):
        ops.proxy_corr_min_records(frames, *occ.set_lists(), cache=cache)
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and torch.equal(a["out"], snap) and cache.key.value == 0
    cache.ws = buf[:n]
    ops.proxy_corr_min_records(frames, *occ.set_lists(), cache=cache)
    torch.cuda.synchronize()
    assert same([a["out"]], want) and cache.key.value != 0


# ------------------------------------------------------------------------------------------ the gradient entries at their own smallest cases
@pytest.mark.parametrize("name", ["C4_m17_O3", "C36_m99_O17", "C128_m17_O17", "C100_m99_O30"])
def test_dense_match_gradient_off_the_grid(aoc, name):
    """aoc_dense_match_grad (all pointers class 4) at the widths of tests/match_grad_bounds.py: every input and every caller-provided gradient
    4 / 8 / 12 bytes off, the aligned call's bits.  T and arg come from one aligned forward call."""
    import match_grad_bounds as mb
    ops = aoc.ops
    case = mb.DENSE_BY_NAME[name]
    d = mb.grad_case_inputs(case)
    m, O, C, n = case.m, case.n_obj, case.C, d["pool"].shape[0]
    query, pool = _t(d["query"]), _t(d["pool"])
    prep = ops.label_prep(_t(d["labels"]))
    T, arg = torch.empty(O, m, device="cuda"), torch.empty(O, m, dtype=torch.int32, device="cuda")
    ops.dense_match_argmin(query, pool, prep, _t(d["bias"]), T, arg, 1, m)
    tensors = dict(grad_out=_t(d["grad_out"]), T=T, arg=arg, query=query, pool=pool, grad_query=occ.blank("cuda", (m, C)),
                   grad_pool=occ.blank("cuda", (n, C)), grad_bias=occ.blank("cuda", (O,)))

    def call(grad_out, T, arg, query, pool, grad_query, grad_pool, grad_bias):
        ops.dense_match_backward(grad_out, T, arg, 1, m, query, pool, O, grad_query=grad_query, grad_pool=grad_pool, grad_bias=grad_bias)
        return [grad_query, grad_pool, grad_bias]
    sweep(call, tensors, f"dense gradient {name}", outputs=("grad_query", "grad_pool", "grad_bias"))


@pytest.mark.parametrize("name,C,m,O", [c for c in __import__("match_grad_bounds").PROXY_GRAD_CASES if c[2] > 1])
def test_proxy_match_gradient_off_the_grid(aoc, name, C, m, O):
    import match_grad_bounds as mb
    ops = aoc.ops
    d = mb.proxy_case_inputs(name, C, m, O)
    query, proxies = _t(d["query"]), _t(d["proxies"])
    T = torch.empty(O, m, device="cuda")
    ops.proxy_corr_min(query, proxies, None, list(range(O)), [1] * O, [o * m for o in range(O)], _t(d["bias"]), T, 1)
    tensors = dict(grad_out=_t(d["grad_out"]), T=T, query=query, proxies=proxies, grad_query=occ.blank("cuda", (m, C)),
                   grad_proxies=occ.blank("cuda", (O, C)), grad_bias=occ.blank("cuda", (O,)))

    def call(grad_out, T, query, proxies, grad_query, grad_proxies, grad_bias):
        ops.proxy_match_backward(grad_out, T, 1, m, query, proxies, grad_query=grad_query, grad_proxies=grad_proxies, grad_bias=grad_bias)
        return [grad_query, grad_proxies, grad_bias]
    sweep(call, tensors, f"proxy gradient {name}", outputs=("grad_query", "grad_proxies", "grad_bias"))


@pytest.mark.parametrize("name", ["C4_3x5_r1_O30", "C128_2x8_r8_O3", "C100_15x17_r3", "C36_15x17_r3", "C100_15x17_rate2", "memory_C100_31x33"])
def test_local_match_gradient_off_the_grid(aoc, name):
    """aoc_local_window_match_argmin (query and prev class 16: copied) and aoc_local_match_grad (all class 4) on the maps of
    tests/local_grad_bounds.py: the register path at C = 100 / 128, the other widths' kernel at C = 36 / 4, an atrous rate, the 31 x 33 map."""
    import local_grad_bounds as lgb
    ops = aoc.ops
    case = lgb.BY_NAME[name]
    d = lgb.case_inputs(case)
    H, W, C, O = case.H, case.W, case.C, case.n_obj
    query, prev, bits, bias = _t(d["query"]), _t(d["prev"]), _t(d["bits"]), _t(d["bias"])
    T, arg = ops.local_window_match_argmin(query, prev, bits, case.radii, bias, O, True, case.rate)
    fwd = dict(query=query, prev=prev, bits=bits, bias=bias)
    sweep(lambda query, prev, bits, bias: list(ops.local_window_match_argmin(query, prev, bits, case.radii, bias, O, True, case.rate)), fwd,
          f"local argmin {name}")
    tensors = dict(grad_out=_t(d["grad_out"]), T=T, arg=arg, query=query, prev=prev, grad_query=occ.blank("cuda", (H, W, C)),
                   grad_prev=occ.blank("cuda", (H, W, C)), grad_bias=occ.blank("cuda", (O,)))

    def call(grad_out, T, arg, query, prev, grad_query, grad_prev, grad_bias):
        ops.local_match_backward(grad_out, T, arg, query, prev, lgb.window(case), grad_query=grad_query, grad_prev=grad_prev, grad_bias=grad_bias)
        return [grad_query, grad_prev, grad_bias]
    sweep(call, tensors, f"local gradient {name}", outputs=("grad_query", "grad_prev", "grad_bias"))


@pytest.mark.parametrize("C,m", [(4, 63), (36, 65), (100, 64), (128, 63)])
def test_set_argmin_and_gradient_off_the_grid(aoc, C, m):
    """aoc_proxy_set_match_argmin and aoc_proxy_set_match_grad (all pointers class 4, the proxy table included: 4-byte loads) on the smallest
    multi-tile cases of tests/cluster_grad_bounds.py."""
    import cluster_grad_bounds as cgb
    ops = aoc.ops
    d = cgb.argmin_case_inputs(C, m)
    S = len(d["size"])
    offs = [s * m for s in range(S)]
    tensors = dict(query=_t(d["query"]), proxies=_t(d["proxies"]), sqnorm=_t(d["sqnorm"]), bias=_t(d["bias"]), out=occ.blank("cuda", (S, m)),
                   arg=occ.blank("cuda", (S, m), torch.int32))

    def fwd(query, proxies, sqnorm, bias, out, arg):
        ops.proxy_set_match_argmin(query, proxies, sqnorm, d["begin"], d["size"], offs, bias, out, arg, 1)
        return [out, arg]
    sweep(fwd, tensors, f"set argmin C{C} m{m}", outputs=("out", "arg"))
    g = cgb.grad_case_inputs(C, m, 3)
    S = len(g["size"])
    offs = [s * m for s in range(S)]
    query, proxies = _t(g["query"]), _t(g["proxies"])
    T, arg = torch.empty(S, m, device="cuda"), torch.empty(S, m, dtype=torch.int32, device="cuda")
    ops.proxy_set_match_argmin(query, proxies, _t(g["sqnorm"]), g["begin"], g["size"], offs, _t(g["bias"][g["bias_index"]]), T, arg, 1)
    tensors = dict(grad_out=_t(g["grad_out"]), T=T, arg=arg, query=query, proxies=proxies, grad_query=occ.blank("cuda", (m, C)),
                   grad_proxies=occ.blank("cuda", tuple(proxies.shape)), grad_bias=occ.blank("cuda", (g["n_bias"],)))

    def bwd(grad_out, T, arg, query, proxies, grad_query, grad_proxies, grad_bias):
        ops.proxy_set_match_backward(grad_out, T, arg, 1, query, proxies, g["begin"], g["size"], offs, g["bias_index"], g["n_bias"],
                                     grad_query=grad_query, grad_proxies=grad_proxies, grad_bias=grad_bias)
        return [grad_query, grad_proxies, grad_bias]
    sweep(bwd, tensors, f"set gradient C{C} m{m}", outputs=("grad_query", "grad_proxies", "grad_bias"))


@pytest.mark.parametrize("levels", [1, 2])
def test_centroid_avg_gradient_off_the_grid(aoc, levels):
    import cluster_grad_bounds as cgb
    ops = aoc.ops
    d = cgb.pullback_case(levels)
    tensors = dict(grad_proxies=_t(d["grad_proxies"]), fg_rows=_t(d["fg_rows"]), n_fg=torch.tensor([d["n_fg"]], dtype=torch.int32, device="cuda"),
                   seg_offsets=_t(d["seg_offsets"]), seg_k=_t(d["seg_k"]), labels=_t(d["labels"]), grad_pool=occ.blank("cuda", (d["pool_rows"], d["C"])))

    def call(grad_proxies, fg_rows, n_fg, seg_offsets, seg_k, labels, grad_pool):
        ops.centroid_avg_backward(grad_proxies, fg_rows, n_fg, seg_offsets, seg_k, labels, d["pool_rows"], grad_pool=grad_pool)
        return [grad_pool]
    sweep(call, tensors, f"centroid_avg gradient levels={levels}", outputs=("grad_pool",))
