"""CPU-side checks of the differentiable global matching: the numpy float64 reference of tests/match_grad_bounds.py against the gradients the
reference's own autograd recorded (tests/golden/match_grad_*.npz), the conditions every case list of tests/test_gpu_match_grad.py has to meet,
the argument checks of the new entry points (they return before any launch, so no GPU is needed) and matching_train's host-side errors."""
import ctypes

import numpy as np
import pytest
import torch

import aoc_amd
import match_grad_bounds as mgb
from conftest import load_golden

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4


def _close(got, want, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max())
    assert err <= 1e-12 * scale, f"{what}: numpy reference and recorded value differ by {err / scale:.2e} relative"


@pytest.mark.parametrize("name", mgb.FIXTURES_DENSE)
def test_numpy_reference_reproduces_the_recorded_gradients(name):
    fx = load_golden(name)
    h, w, _ = fx["in_query"].shape
    n_obj = fx["in_labels"].shape[2]
    fwd, grad = mgb.fixture_ref(fx)
    _close(fwd["T"].T.reshape(1, h, w, n_obj, 1), fx["out"], name + " out")
    _close(grad["grad_query"].reshape(fx["grad_query"].shape), fx["grad_query"], name + " grad_query")
    _close(grad["grad_pool"].reshape(fx["grad_ref"].shape), fx["grad_ref"], name + " grad_ref")
    _close(grad["grad_bias"], fx["grad_bias"], name + " grad_bias")
    assert np.abs(fx["grad_query"]).max() > 1e-2, "the fixture's gradients vanish: it tests nothing"


def test_numpy_reference_reproduces_the_recorded_proxy_gradients():
    fx = load_golden(mgb.FIXTURE_PROXY)
    h, w, _ = fx["in_query"].shape
    n_obj = fx["in_ref"].shape[0]
    (T, _), grad = mgb.fixture_proxy_ref(fx)
    _close(T.T.reshape(1, h, w, n_obj, 1), fx["out"], "proxy out")
    _close(grad["grad_query"].reshape(fx["grad_query"].shape), fx["grad_query"], "proxy grad_query")
    _close(grad["grad_proxies"], fx["grad_ref"], "proxy grad_ref")
    _close(grad["grad_bias"], fx["grad_bias"], "proxy grad_bias")


def test_unlabelled_fixture_is_the_constant_without_a_graph():
    fx = load_golden(mgb.FIXTURE_UNLABELLED)
    assert (fx["out"] == 1.0).all() and "grad_query" not in fx and fx["in_labels"].sum() == 0


@pytest.mark.parametrize("name", mgb.FIXTURES_DENSE)
def test_fixture_inputs_meet_the_conditions(name):
    fx = load_golden(name)
    fwd, grad = mgb.fixture_ref(fx)
    mgb.check_case_conditions(name, fwd)
    assert (fx["in_labels"].sum(2) == 0).any(), "every map has unlabelled pixels"
    if name == "match_grad_absent":
        assert (fwd["arg"] < 0).any() and (fwd["T"][fwd["arg"] < 0] == 1.0).all()
        assert (grad["g"][fwd["arg"] < 0] == 0.0).all()


@pytest.mark.parametrize("name", [c.name for c in mgb.DENSE_GRAD_CASES] + [mgb.TIES.name])
def test_generated_inputs_meet_the_conditions(name):
    case = mgb.DENSE_BY_NAME[name]
    inp, fwd, grad = mgb.dense_case_ref(name)
    mgb.check_case_conditions(name, fwd, planted_dup=case.kind == "ties")
    if case.absent is not None:
        assert (fwd["arg"][case.absent] == -1).all() and (fwd["T"][case.absent] == 1.0).all()
    if case.kind == "hot":
        assert grad["counts"].max() == case.m > mgb.MG_LIST, "no hot row"
    if case.kind == "groups" and case.m >= 257:               # the groups of 70 and 100 pixels
        assert ((grad["counts"] > mgb.MG_CHUNK) & (grad["counts"] <= mgb.MG_LIST)).any(), "no list of more than one chunk"
    if case.kind == "ties":
        kept, _ = mgb.labels_to_bits(inp["labels"])
        ranges = mgb.argmin_split_ranges(case.m, kept.size)
        split_of = lambda r: next(k for k, (b, e) in enumerate(ranges) if b <= np.searchsorted(kept, r) < e)
        pos_of = lambda r: int(np.searchsorted(kept, r))
        for r, (lane, same, other) in inp["dup"]:
            assert all((inp["pool"][x] == inp["pool"][r]).all() and (inp["labels"][x] == inp["labels"][r]).all() for x in (lane, same, other))
            assert r < lane < same < other and (fwd["arg"] == r).any() and not np.isin(fwd["arg"], [lane, same, other]).any()
            assert pos_of(lane) // 16 == pos_of(r) // 16 and pos_of(lane) % 16 != pos_of(r) % 16, "same tile, another lane"
            assert split_of(same) == split_of(r) and pos_of(same) // 16 != pos_of(r) // 16 and pos_of(same) % 16 == pos_of(r) % 16
            assert split_of(other) != split_of(r)
    if name == "rows17001":
        ranges = mgb.argmin_split_ranges(case.m, 17001)           # many n-splits of more than two 128-row chunks each
        assert len(ranges) >= 60 and all(e - b > 2 * 128 for b, e in ranges[:-1])


@pytest.mark.parametrize("name", [c.name for c in mgb.WIDE_GRAD_CASES])
def test_wide_inputs_meet_the_conditions(name):
    case = mgb.DENSE_BY_NAME[name]
    inp, fwd, T32, grad = mgb.wide_case_ref(name)
    mgb.check_case_conditions(name, fwd)
    assert case.C > 128 and (np.abs(T32 - fwd["T"]) <= mgb.U * np.abs(fwd["T"])).all()
    if case.kind == "hot":
        assert grad["counts"].max() > mgb.MG_LIST
    else:
        assert grad["counts"].max() > mgb.MG_CHUNK // 2, "no list longer than the 32 rows staged per step above C = 128"


@pytest.mark.parametrize("name", [c[0] for c in mgb.PROXY_GRAD_CASES + mgb.PROXY_WIDE_CASES] + [mgb.FIXTURE_PROXY])
def test_proxy_inputs_meet_the_conditions(name):
    T = mgb.fixture_proxy_ref(load_golden(name))[0][0] if name == mgb.FIXTURE_PROXY else mgb.proxy_case_ref(name)[1][0]
    mgb.check_proxy_conditions(name, T)


def test_case_lists_cover_what_they_must():
    cs = mgb.DENSE_GRAD_CASES
    assert {c.C for c in cs} == {4, 36, 100, 128} and {1, 17, 99, 257} <= {c.m for c in cs} and {1, 3, 17, 30} <= {c.n_obj for c in cs}
    assert {c.layout for c in cs} == {"planes", "pixels"}
    ps = mgb.PROXY_GRAD_CASES
    assert {c[1] for c in ps} == {4, 36, 128} and {c[2] for c in ps} == {1, 99, 257} and {c[3] for c in ps} == {1, 3, 30}


# ------------------------------------------------------------------------------------------ argument checks (no launch, no GPU)
_HOST = (ctypes.c_char * 4096)()
P = ctypes.c_void_p(ctypes.addressof(_HOST))        # a non-null pointer; the entry points return before anything reads it
BIG = 1 << 40


def _argmin(query=P, m=17, C=36, pool=P, fg_rows=P, n_fg=P, cap=40, wrong=P, bias=P, n_obj=3, out=P, arg=P, ws=P, ws_bytes=BIG):
    return aoc_amd._lib.lib().aoc_dense_match_argmin(query, m, C, pool, fg_rows, n_fg, cap, wrong, bias, n_obj, out, arg, 1, m, 1, ws, ws_bytes, None)


def _dense_grad(go=P, T=P, arg=P, query=P, m=17, C=36, pool=P, n=40, n_obj=3, gq=P, gp=P, gb=P, ws=P, ws_bytes=BIG):
    return aoc_amd._lib.lib().aoc_dense_match_grad(go, T, arg, 1, m, query, m, C, pool, n, n_obj, gq, gp, gb, ws, ws_bytes, None)


def _proxy_grad(go=P, T=P, query=P, m=17, C=36, proxies=P, n_obj=3, gq=P, gp=P, gb=P, ws=P, ws_bytes=BIG):
    return aoc_amd._lib.lib().aoc_proxy_match_grad(go, T, 1, m, query, m, C, proxies, n_obj, gq, gp, gb, ws, ws_bytes, None)


@pytest.mark.parametrize("fn, pointers", [(_argmin, ("query", "pool", "fg_rows", "n_fg", "wrong", "out", "arg", "ws")),
                                          (_dense_grad, ("go", "T", "arg", "query", "pool", "ws")),
                                          (_proxy_grad, ("go", "T", "query", "proxies", "ws"))])
def test_entry_points_reject_bad_arguments_before_any_launch(fn, pointers):
    for name in pointers:
        assert fn(**{name: None}) == INVALID, f"{fn.__name__}: NULL {name}"
    assert fn(m=0) == INVALID and fn(m=-5) == INVALID
    assert fn(n_obj=0) == INVALID and fn(n_obj=-1) == INVALID
    assert fn(C=0) == INVALID and fn(C=-4) == INVALID
    assert fn(n_obj=aoc_amd.ops.MAX_OBJECTS + 1) == UNSUPPORTED
    assert fn(C=260) == UNSUPPORTED
    assert fn(ws_bytes=16) == WORKSPACE
    if fn is _dense_grad:
        assert fn(n=0) == INVALID and fn(n=-3) == INVALID
    if fn is _argmin:
        assert fn(cap=0) == INVALID and fn(cap=-1) == INVALID and fn(C=38) == UNSUPPORTED


def test_workspace_queries():
    L = aoc_amd._lib.lib()
    assert L.aoc_dense_match_argmin_workspace_bytes(0, 40, 3) == 0 and L.aoc_dense_match_argmin_workspace_bytes(17, 40, 0) == 0
    assert L.aoc_dense_match_grad_workspace_bytes(17, 0, 36, 3) == 0 and L.aoc_dense_match_grad_workspace_bytes(17, 40, 36, 31) == 0
    assert L.aoc_proxy_match_grad_workspace_bytes(17, 300, 3) == 0 and L.aoc_proxy_match_grad_workspace_bytes(-1, 36, 3) == 0
    one = L.aoc_dense_match_grad_workspace_bytes(13689, 13689, 100, 4)
    four = L.aoc_dense_match_grad_workspace_bytes(13689, 4 * 13689, 100, 4)
    assert 0 < one < 16 << 20 and four - one < 3 * 13689 * 3 * 4 + 4096, "the backward's workspace grows with m O + n, never with m O n"
    assert 0 < L.aoc_dense_match_argmin_workspace_bytes(13689, 13689, 4) < 64 << 20


# ------------------------------------------------------------------------------------------ matching_train on the host
def _cpu_args(requires_grad=True):
    q = torch.randn(5, 6, 4, requires_grad=requires_grad)
    return torch.randn(5, 6, 4), q, torch.ones(5, 6, 2)


def test_matching_train_has_no_cpu_fallback():
    mt = aoc_amd.matching_train
    ref, q, lab = _cpu_args()
    with pytest.raises(aoc_amd._lib.AocHipError, match="no CPU fallback"):
        mt.global_matching(ref, q, lab, 1, 0., None, 1, False, 0)
    with pytest.raises(aoc_amd._lib.AocHipError, match="no CPU fallback"):
        mt.global_matching_proxy(torch.randn(2, 4), q, lab, 1, 0., None, 1, False, 0)
    with torch.no_grad():                       # nothing to differentiate: the mirror is called, and reports the missing GPU itself
        with pytest.raises(aoc_amd._lib.AocHipError, match="no CPU fallback"):
            mt.global_matching(ref, q, lab, 1, 0., None, 1, False, 0)


def test_matching_train_refuses_float16_under_autograd():
    mt = aoc_amd.matching_train
    ref, q, lab = _cpu_args()
    with pytest.raises(aoc_amd._lib.AocHipError, match="use_float16"):
        mt.global_matching(ref, q, lab)                         # the reference's default argument is use_float16=True
    with pytest.raises(aoc_amd._lib.AocHipError, match="use_float16"):
        mt.global_matching_proxy(torch.randn(2, 4), q, lab, 1, torch.zeros(2, 1, 1, 1, requires_grad=True), None, 1, True, 0)


def test_matching_train_names_what_is_not_yet_differentiable():
    mt = aoc_amd.matching_train
    ref, q, lab = _cpu_args()
    with pytest.raises(aoc_amd._lib.AocHipError, match="global_matching_cluster2 is not yet differentiable"):
        mt.global_matching_cluster2(ref, q, lab, 1, 0., None, 1, False, 0)
    with pytest.raises(aoc_amd._lib.AocHipError, match="local_matching is not yet differentiable"):
        mt.local_matching(ref, q, lab, 0., [2], None, 1, False)


def test_inference_guard_points_to_matching_train():
    ref, q, lab = _cpu_args()
    with pytest.raises(aoc_amd._lib.AocHipError, match="inference-only.*matching_train.global_matching"):
        aoc_amd.matching.global_matching(ref, q, lab, 1, 0., None, 1, False, 0)
