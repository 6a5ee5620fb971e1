"""The exact-fp32 global matching kernels of csrc/correlation.hip and their `.half()` modes (ops.proxy_corr_min,
ops.proxy_corr_min_batched(precision="fp32"), ops.dense_match_min) and the fp16-split proxy kernels of csrc/correlation_batched.hip
(ops.proxy_corr_min_batched(precision="split"), ops.proxy_corr_min_records with and without a table cache) and the fp16-split dense
entry of csrc/dense_split.hip (ops.dense_match(precision="split")) called directly and compared with the plain float64 references of
tests/global_match_bounds.py under the bounds derived there from the kernels' own expressions: raw distances and transformed outputs at
every case.  Every output buffer is filled with NaN and is larger than what the call may write: afterwards every element the layout names
is written and every other one is still NaN.  Every comparison goes through _check_bound once per slip of proxy_slips(case) /
dense_slips(case): the same reference with one deliberate mistake must leave the bound.  The dense inputs are built in numpy (an
ops.LabelPrep filled by hand), never through label_prep.  test_global_match_host.py proves without a GPU that the references are the
oracle's, that float32 restatements of the kernels lie inside the bounds and that every slip leaves them, at every case of this file.

Which instantiation a case runs: proxy_corr_min_kernel<25, EXACT> at C = 100, <32> at every other C up to 128, <64> above;
dense_match_partial_kernel with (NA, OMAX) = (2, 4) up to 4 objects, (1, 8) up to 8, (1, 16) above, and a second launch with
obj_base = 16 above 16 objects."""
import numpy as np
import pytest
import torch

import global_match_bounds as gb
from global_match_bounds import DENSE_CASES, PAD, PROXY_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    return aoc_amd


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def nan_buffer(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------------------ proxy correlation
def _run_proxy(aoc, case, inp, transform):
    out = nan_buffer(inp["out_len"])
    aoc.ops.proxy_corr_min(dev(inp["query"]), dev(inp["proxies"]), dev(inp["sqnorm"]), inp["set_begin"], inp["set_size"], inp["set_off"],
                           dev(inp["bias"]) if transform else None, out, inp["stride"], transform=transform, float16=case.f16)
    return gb.check_layout(out.cpu().numpy(), inp["named"], f"{case.name} transform={transform}")


def _compare_proxy(case, ref, raw, tr, tag=""):
    gb.check_conditions(case.name, ref["raw"][0], ref["transformed"][0], bool(gb.absent_sets(case)))
    gb.compare(raw, ref["raw"], f"proxy{'_f16' if case.f16 else ''} {case.name}{tag} raw")
    gb.compare(tr, ref["transformed"], f"proxy{'_f16' if case.f16 else ''} {case.name}{tag} transformed")


@pytest.mark.parametrize("case", [c for c in PROXY_CASES if not c.frames], ids=lambda c: c.name)
def test_proxy_corr_min(aoc, case):
    """aoc_proxy_corr_min / aoc_proxy_corr_min_f16.  The fill_* cases are one launch of exactly max_tiles tiles, above 64 KB of dynamic LDS:
    the call returns AOC_OK (ops raises otherwise) and meets the bound."""
    inp = gb.proxy_inputs(case)
    ref = gb.proxy_case_ref(case.name)
    raw = _run_proxy(aoc, case, inp, False)
    tr = _run_proxy(aoc, case, inp, True)           # set_bias = NULL where the case has no bias
    _compare_proxy(case, ref, raw, tr)
    torch.cuda.synchronize()


def test_proxy_corr_min_33_frames(aoc):
    """n_frames = 33 through aoc_proxy_corr_min_batched(AOC_CORR_FP32): the second frame table holds one frame.  Three different frames
    take turns; every frame has its own output buffer."""
    case = gb.PROXY_BY_NAME["frames33_C100"]
    inps = [gb.proxy_inputs(case, f) for f in range(3)]
    refs = [gb.proxy_case_ref(case.name, f) for f in range(3)]
    got = {}
    for transform in (False, True):
        held = [tuple(dev(i[k]) for k in ("query", "proxies", "sqnorm", "bias")) for i in inps]
        outs = [nan_buffer(inps[0]["out_len"]) for _ in range(case.frames)]
        frames = [(*held[f % 3][:3], held[f % 3][3] if transform else None, outs[f]) for f in range(case.frames)]
        aoc.ops.proxy_corr_min_batched(frames, inps[0]["set_begin"], inps[0]["set_size"], inps[0]["set_off"], transform=transform, precision="fp32")
        got[transform] = [gb.check_layout(o.cpu().numpy(), inps[0]["named"], f"frame {f} transform={transform}") for f, o in enumerate(outs)]
    for f in (0, 1, 2, 31, 32):
        _compare_proxy(case, refs[f % 3], got[False][f], got[True][f], tag=f" frame {f}")
    for f in range(3, case.frames):       # the same inputs, the same bits
        assert np.array_equal(got[False][f], got[False][f % 3]) and np.array_equal(got[True][f], got[True][f % 3]), f"frame {f}"


def _absent_rows(case):
    absent = gb.absent_sets(case)
    st = gb.proxy_structure(case)
    assert any(st["set_size"][s] == 1 for s in absent) or case.kind == "fill", "the case has no absent single-proxy set"
    return absent


@pytest.mark.parametrize("name", ["singles70_C100", "singles70_C36", "singles64_C100", "C100_m65", "C256_m17", "f16_C36"])
def test_absent_single_proxy_set_is_the_pad_distance_raw(aoc, name):
    """include/aoc_hip.h: an empty or all-ignored set yields AOC_PAD_DISTANCE, a single-proxy set with a +inf norm included (the
    column-wise branch of proxy_corr_min_kernel, direct stores above 64 output columns and the transpose buffer below; the `.half()` entry
    pads with the same float32 5e4)."""
    case = gb.PROXY_BY_NAME[name]
    raw = _run_proxy(aoc, case, gb.proxy_inputs(case), False)
    absent = _absent_rows(case)
    assert (raw[absent] == np.float32(PAD)).all(), f"{name}: absent sets hold {np.unique(raw[absent])}"


def test_absent_sets_are_the_pad_distance_in_the_split_entries(aoc):
    """The same contract, raw, in aoc_proxy_corr_min_batched(AOC_CORR_SPLIT), aoc_proxy_corr_min_records and its cached form, on the
    structure of an fp32 case."""
    case = gb.PROXY_BY_NAME["C100_m65"]
    inp = gb.proxy_inputs(case)
    absent = _absent_rows(case)
    q, p, sq = dev(inp["query"]), dev(inp["proxies"]), dev(inp["sqnorm"])
    named = inp["named"]
    out = nan_buffer(inp["out_len"])
    aoc.ops.proxy_corr_min_batched([(q, p, sq, None, out)], inp["set_begin"], inp["set_size"], inp["set_off"], transform=False, precision="split")
    got = gb.check_layout(out.cpu().numpy(), named, "batched split")
    assert (got[absent] == np.float32(PAD)).all()
    qs = aoc.ops.split_rows(q, tiled=True)
    for cache in (None, aoc.ops.CorrTableCache(q.device)):
        out = nan_buffer(inp["out_len"])
        aoc.ops.proxy_corr_min_records([(q, qs, p, sq, None, out)], inp["set_begin"], inp["set_size"], inp["set_off"], transform=False, cache=cache)
        got = gb.check_layout(out.cpu().numpy(), named, "records")
        assert (got[absent] == np.float32(PAD)).all()


# ------------------------------------------------------------------------------------------ the fp16-split proxy kernels
def _run_split(aoc, entry, inps, n_frames, transform):
    """-> per frame the named outputs [n_set, m].  entry: batched (AOC_CORR_SPLIT), records, cached (records with a tables_key)."""
    held = [tuple(dev(i[k]) for k in ("query", "proxies", "sqnorm", "bias")) for i in inps]
    outs = [nan_buffer(inps[0]["out_len"]) for _ in range(n_frames)]
    sets = (inps[0]["set_begin"], inps[0]["set_size"], inps[0]["set_off"])
    pick = lambda f: held[f % len(held)]
    if entry == "batched":
        frames = [(*pick(f)[:3], pick(f)[3] if transform else None, outs[f]) for f in range(n_frames)]
        aoc.ops.proxy_corr_min_batched(frames, *sets, transform=transform, precision="split")
    else:
        recs = [aoc.ops.split_rows(h[0], tiled=True) for h in held]
        frames = [(pick(f)[0], recs[f % len(held)], *pick(f)[1:3], pick(f)[3] if transform else None, outs[f]) for f in range(n_frames)]
        cache = aoc.ops.CorrTableCache(held[0][0].device) if entry == "cached" else None
        aoc.ops.proxy_corr_min_records(frames, *sets, transform=transform, cache=cache)
        assert all(int(r.overflow.item()) == 0 for r in recs), "the split preconditions hold for these inputs"
    return [gb.check_layout(o.cpu().numpy(), inps[0]["named"], f"{entry} frame {f} transform={transform}") for f, o in enumerate(outs)]


@pytest.mark.parametrize("entry", ["batched", "records", "cached"])
@pytest.mark.parametrize("case", gb.SPLIT_CASES, ids=lambda c: c.name)
def test_split_proxy_corr(aoc, case, entry):
    """aoc_proxy_corr_min_batched(AOC_CORR_SPLIT), aoc_proxy_corr_min_records and aoc_proxy_corr_min_records_cached under the bound of the
    split arithmetic (split_pair_distances, cb_transform_ref)."""
    n_frames = case.frames or 1
    n_in = 3 if case.frames else 1
    inps = [gb.proxy_inputs(case, f) for f in range(n_in)]
    refs = [gb.split_case_ref(case.name, entry != "batched", f) for f in range(n_in)]
    raw = _run_split(aoc, entry, inps, n_frames, False)
    tr = _run_split(aoc, entry, inps, n_frames, True)
    torch.cuda.synchronize()
    absent = gb.absent_sets(case)
    for f in sorted({0, 1, 2, n_frames - 2, n_frames - 1} & set(range(n_frames))):
        ref = refs[f % n_in]
        gb.check_conditions(case.name, ref["raw"][0], ref["transformed"][0], bool(absent))
        assert (raw[f][absent] == np.float32(PAD)).all()
        gb.compare(raw[f], ref["raw"], f"split_proxy {entry} {case.name} frame {f} raw")
        gb.compare(tr[f], ref["transformed"], f"split_proxy {entry} {case.name} frame {f} transformed")
    for f in range(n_in, n_frames):       # the same inputs, the same bits
        assert np.array_equal(raw[f], raw[f % n_in]) and np.array_equal(tr[f], tr[f % n_in]), f"frame {f}"


@pytest.mark.parametrize("entry", ["batched", "records", "cached"])
@pytest.mark.parametrize("case", gb.TAKEOVER_CASES, ids=lambda c: c.name)
def test_split_proxy_takeover(aoc, case, entry):
    """|x| 2^10 > 65000 and |x|^2 > 4000 in one query / one proxy: the exact-fp32 kernel recomputes the launch inside the same call.  Held to
    the fp32 bound, not the split one, and bit-equal to the fp32 entry."""
    inp = gb.takeover_inputs(case)
    ref = gb.takeover_case_ref(case.name)
    for transform in (False, True):
        held = tuple(dev(inp[k]) for k in ("query", "proxies", "sqnorm", "bias"))
        out, out32 = nan_buffer(inp["out_len"]), nan_buffer(inp["out_len"])
        sets = (inp["set_begin"], inp["set_size"], inp["set_off"])
        bias = held[3] if transform else None
        if entry == "batched":
            aoc.ops.proxy_corr_min_batched([(*held[:3], bias, out)], *sets, transform=transform, precision="split")
        else:
            rec = aoc.ops.split_rows(held[0], tiled=True)
            cache = aoc.ops.CorrTableCache(held[0].device) if entry == "cached" else None
            aoc.ops.proxy_corr_min_records([(held[0], rec, *held[1:3], bias, out)], *sets, transform=transform, cache=cache)
        aoc.ops.proxy_corr_min(*held[:3], *sets, bias, out32, 1, transform=transform)
        got = gb.check_layout(out.cpu().numpy(), inp["named"], f"{entry} {case.name} transform={transform}")
        assert np.array_equal(got, gb.check_layout(out32.cpu().numpy(), inp["named"], "fp32 entry")), "the take-over is not bit-equal to the fp32 entry"
        gb.compare(got, ref["transformed" if transform else "raw"], f"takeover {entry} {case.name} {'transformed' if transform else 'raw'}")


# ------------------------------------------------------------------------------------------ dense matching
def _prep(aoc, case, inp):
    prep = aoc.ops.LabelPrep()
    prep.n, prep.n_obj = inp["pool"].shape[0], case.n_obj
    prep.wrong_bits, prep.fg_rows, prep.counts = dev(inp["wrong"]), dev(inp["fg_rows"]), dev(inp["counts"])
    prep.right_bits = prep.obj_rows = prep.obj_offsets = None
    return prep


@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: c.name)
def test_dense_match_min(aoc, case):
    """aoc_dense_match_min / aoc_dense_match_min_f16."""
    inp = gb.dense_inputs(case)
    ref = gb.dense_case_ref(case.name)
    n_pool = inp["pool"].shape[0]
    L = aoc._lib.lib()
    # the restated dense_nsplit, before the planted positions rely on it
    assert L.aoc_dense_match_workspace_bytes(case.m, n_pool, case.n_obj) == gb.dense_workspace_bytes(case.m, n_pool, case.n_obj)
    ps, os_, length, named = gb.dense_layout(case)
    prep = _prep(aoc, case, inp)
    q, pool, bias = dev(inp["query"]), dev(inp["pool"]), dev(inp["bias"])
    got = {}
    for transform in (False, True):
        buf = nan_buffer(length)
        aoc.ops.dense_match_min(q, pool, prep, bias if transform else None, buf[2:], ps, os_, transform=transform, float16=case.f16)
        got[transform] = gb.check_layout(buf.cpu().numpy(), named, f"{case.name} transform={transform}")
    torch.cuda.synchronize()
    if case.n_fg == 0:      # include/aoc_hip.h: n_fg == 0 yields 1.0 everywhere when transform != 0, +inf otherwise
        assert np.isposinf(got[False]).all() and (got[True] == 1.0).all()
        return
    gb.check_conditions(case.name, ref["raw"][0], ref["transformed"][0], gb.absent_object(case.n_obj) is not None)
    fam = "dense_f16" if case.f16 else "dense"
    gb.compare(got[False], ref["raw"], f"{fam} {case.name} raw")
    gb.compare(got[True], ref["transformed"], f"{fam} {case.name} transformed")


def _run_split_dense(aoc, case, inp, tiled, transform, fp32=False):
    """-> (named outputs [n_obj, m], overflow flag).  fp32: the same call through aoc_dense_match_min."""
    prep = _prep(aoc, case, inp)
    prep.right_bits, prep.obj_rows, prep.obj_offsets = dev(inp["right"]), dev(inp["obj_rows"]), dev(inp["obj_offsets"])
    ps, os_, length, named = gb.dense_layout(case)
    q, pool = dev(inp["query"]), dev(inp["pool"])
    bias = dev(inp["bias"]) if transform else None
    buf = nan_buffer(length)
    if fp32:
        aoc.ops.dense_match_min(q, pool, prep, bias, buf[2:], ps, os_, transform=transform)
        return gb.check_layout(buf.cpu().numpy(), named, f"{case.name} fp32 entry"), 0
    pool_split = aoc.ops.split_rows(pool)
    query_split = aoc.ops.split_rows(q, overflow=pool_split.overflow, tiled=tiled)
    aoc.ops.dense_match(q, pool, prep, bias, buf[2:], ps, os_, transform=transform, precision="split", query_split=query_split, pool_split=pool_split)
    torch.cuda.synchronize()
    return gb.check_layout(buf.cpu().numpy(), named, f"{case.name} transform={transform}"), int(pool_split.overflow.item())


@pytest.mark.parametrize("tiled", [False, True], ids=["rows", "tiled"])
@pytest.mark.parametrize("case", gb.SPLIT_DENSE_CASES, ids=lambda c: c.name)
def test_split_dense_match(aoc, case, tiled):
    """aoc_dense_match_min_split through ops.dense_match(precision="split") on one-hot labels, the query records row-major and tile-major,
    under the bound of the split arithmetic (split_dense_ref).  The planted rows also test that pruning never drops the minimum; the
    hi_margin case has a nearest row that the hi-plane product alone ranks second (plant_hi_margin).
    The test sees the records' overflow flag but not the plan's one-hot gate: a quiet take-over by the fp32 kernels would pass under this
    looser bound.  The host test asserts that these inputs are one-hot as split_plan_kernel demands; here the cases of 1 000 rows and
    more and hi_margin must also differ in some bit from the fp32 entry's output, which a take-over would reproduce exactly."""
    inp = gb.dense_inputs(case, onehot=True)
    ref = gb.split_dense_case_ref(case.name)
    got = {}
    for transform in (False, True):
        got[transform], overflow = _run_split_dense(aoc, case, inp, tiled, transform)
        assert overflow == 0, "the split preconditions hold for these inputs"
    if case.n_fg == 0:
        assert np.isposinf(got[False]).all() and (got[True] == 1.0).all()
        return
    gb.check_conditions(case.name, ref["raw"][0], ref["transformed"][0], gb.absent_object(case.n_obj) is not None)
    gb.compare(got[False], ref["raw"], f"split_dense {case.name} {'tiled' if tiled else 'rows'} raw")
    gb.compare(got[True], ref["transformed"], f"split_dense {case.name} {'tiled' if tiled else 'rows'} transformed")
    if case.n_fg >= 1000 or case.name == "hi_margin":
        assert not np.array_equal(got[False], _run_split_dense(aoc, case, inp, tiled, False, fp32=True)[0]), "the fp32 kernels took the call over"


@pytest.mark.parametrize("tiled", [False, True], ids=["rows", "tiled"])
@pytest.mark.parametrize("case", gb.DENSE_TAKEOVER_CASES, ids=lambda c: c.name)
def test_split_dense_takeover(aoc, case, tiled):
    """Soft labels, one query value and one pool value with |x| 2^10 > 65000 and |x|^2 > 4000: the exact-fp32 kernels run inside the same
    aoc_dense_match_min_split call.  Held to the fp32 bound (dense_ref), not the split one, and bit-equal to aoc_dense_match_min."""
    inp = gb.dense_takeover_inputs(case)
    ref = gb.dense_takeover_ref(case.name)
    for transform in (False, True):
        got, overflow = _run_split_dense(aoc, case, inp, tiled, transform)
        assert overflow == (1 if "value" in case.name else 0)
        want32, _ = _run_split_dense(aoc, case, inp, tiled, transform, fp32=True)
        assert np.array_equal(got, want32), "the take-over is not bit-equal to the fp32 entry"
        gb.compare(got, ref["transformed" if transform else "raw"], f"dense_takeover {case.name} {'tiled' if tiled else 'rows'} {'transformed' if transform else 'raw'}")
