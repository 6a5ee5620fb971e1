"""What can be checked without a GPU about the training-time local matching: that the numpy reference of tests/local_grad_bounds.py IS
the reference's function (it reproduces the outputs and gradients the reference's own autograd recorded, tests/golden/local_grad_*.npz),
the conditions every case of tests/test_gpu_local_grad.py has to meet, that the deliberate slips leave the derived bounds (so the GPU
test can see them), the argument checks of the new entry points (they return before any launch) and local_train's host-side behaviour."""
import ctypes

import numpy as np
import pytest
import torch

import aoc_amd
import local_grad_bounds as lgb
from conftest import load_golden

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4


def _close(got, want, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(np.asarray(got).reshape(np.shape(want)) - want).max())
    assert err <= 1e-10 * scale, f"{what}: numpy reference and recorded value differ by {err / scale:.2e} relative"


@pytest.mark.parametrize("name", lgb.FIXTURES)
def test_numpy_reference_reproduces_the_recorded_gradients(name):
    fx = load_golden(name)
    ref = lgb.fixture_ref(fx)
    _close(ref["out"], fx["out"], name + " out")
    _close(ref["grad_query"], fx["grad_query"], name + " grad_query")
    _close(ref["grad_prev"], fx["grad_prev"], name + " grad_prev")
    _close(ref["grad_bias"], fx["grad_bias"], name + " grad_bias")
    assert np.abs(fx["grad_query"]).max() > 1e-2 and np.abs(fx["grad_prev"]).max() > 1e-2, "the fixture's gradients vanish: it tests nothing"


def test_unlabelled_fixture_is_the_constant_with_zero_gradients():
    fx = load_golden(lgb.FIXTURE_UNLABELLED)
    assert fx["in_labels"].sum() == 0 and (fx["out"] == 1.0).all()
    assert all((fx[k] == 0.0).all() for k in ("grad_query", "grad_prev", "grad_bias"))
    ref = lgb.fixture_ref(fx)
    assert (ref["out"] == 1.0).all() and (ref["fwd"]["arg"] == -1).all()
    assert all((ref[k] == 0.0).all() for k in ("grad_query", "grad_prev", "grad_bias"))


@pytest.mark.parametrize("name", lgb.FIXTURES)
def test_fixture_inputs_meet_the_conditions(name):
    fx = load_golden(name)
    ref = lgb.fixture_ref(fx)
    lgb.check_conditions(name, ref["fwd"])
    radii, ori, rate, down = lgb.fixture_args(fx)
    assert (fx["in_labels"].sum(2) == 0).any(), "every map has unlabelled pixels"
    for W in (ref["Wd"], ref["Wo"]):                    # the resizes' weights are float32 values: torch's float32 weights are these exactly
        assert W is None or (W.astype(np.float32) == W).all()
    if name == "local_grad_absent":
        arg, T = ref["fwd"]["arg"], ref["fwd"]["T"]
        assert (arg[1] == -1).all() and (T[1] == 1.0).all() and ref["grad_bias"][1] == 0.0 and fx["grad_bias"][1] == 0.0
    if name == "local_grad_atrous2":
        assert rate == 2 and radii[-1] - radii[-1] % rate == 4
    if name == "local_grad_down_orisize_C100":
        assert ori is not None and ori != fx["in_query"].shape[:2] and ref["Wo"] is not None and ref["Wd"] is not None
    if name == "local_grad_nodown_O3":
        assert not down and ref["Wd"] is None and ref["Wo"] is None


def test_no_fixture_comes_from_the_for_loop_path():
    """The recording script passes allow_parallel=True in its one call of the reference; the fixtures' query gradients are not None / zero."""
    import os
    src = open(os.path.join(os.path.dirname(__file__), "golden", "make_golden_local_grad.py")).read()
    assert src.count("aem.local_matching(") == 1 and "ori_size, atrous_rate, False, down, True)" in src


@pytest.mark.parametrize("name", [c.name for c in lgb.CASES] + [lgb.PLANTED.name, lgb.PLANTED_LDS.name, lgb.MEMORY.name])
def test_generated_inputs_meet_the_conditions(name):
    case = lgb.BY_NAME[name]
    inp, fwd, grad = lgb.case_ref(name)
    lgb.check_conditions(name, fwd, exempt=lgb.planted_exempt(case))
    assert (inp["bits"] >> 31).any() and (inp["bits"][0] >> min(case.n_obj, 30)) & 1, "label bits at or above n_obj"
    if case.kind == "planted":
        W = case.W
        px = lambda rc: rc[0] * W + rc[1]
        arg, T = fwd["arg"].reshape(case.n_obj, len(case.radii), -1), fwd["T"].reshape(case.n_obj, len(case.radii), -1)
        # object 1: one labelled pixel; every query within R chooses it, nobody chooses its neighbours for that object
        single = px(lgb.SINGLE)
        ys, xs = np.divmod(np.arange(case.H * case.W), W)
        within = np.maximum(np.abs(ys - lgb.SINGLE[0]), np.abs(xs - lgb.SINGLE[1])) <= lgb.window(case)
        assert (arg[1, 0][within] == single).all() and (arg[1, 0][~within] == -1).all() and set(np.unique(arg[1])) == {-1, single}
        # ... and small windows that are empty while the large one is not: -1 and T exactly 1 in the small channels only
        small_empty = (arg[1, 1] == -1) & (arg[1, 0] == single)
        assert small_empty.any() and (T[1, 1][small_empty] == 1.0).all() and (T[1, 0][small_empty] < 1.0).all()
        # object 2: two bit-equal pixels; the largest channel reports the lower index, the small ones the inner pixel
        lo, hi, qi = px(lgb.DUP_LO), px(lgb.DUP_HI), px(lgb.DUP_QUERY)
        assert inp["dup"] == [(lo, hi)] and (inp["prev"].reshape(-1, case.C)[lo] == inp["prev"].reshape(-1, case.C)[hi]).all()
        assert arg[2, 0, qi] == lo and arg[2, 1, qi] == hi and arg[2, 2, qi] == hi
        assert T[2, 0, qi] == T[2, 1, qi]
        # object 3: absent
        assert (arg[3] == -1).all() and (T[3] == 1.0).all() and grad["grad_bias"][3] == 0.0
        assert grad["counts"][single] > 100 and lgb.window(case) == 6


def test_case_list_covers_what_it_must():
    cs = lgb.CASES
    assert {(c.H, c.W) for c in cs} >= {(1, 1), (3, 5), (2, 8), (3, 9), (15, 17), (27, 29)}
    assert {c.C for c in cs} == {4, 36, 100, 128} and {c.n_obj for c in cs} >= {1, 3, 17, 30} and {len(c.radii) for c in cs} >= {1, 6, 8}
    assert {c.rate for c in cs} == {1, 2, 3}
    assert any(c.radii == lgb.REAL and (c.H, c.W) == (27, 29) and c.C == 100 for c in cs)
    for C in (4, 36, 100, 128):
        assert {1, 2}.issubset({c.rate if c.rate < 3 else 2 for c in cs if c.C == C}), "every kernel sees an atrous rate above 1"


SLIP_CASES = {"ties_highest": lgb.PLANTED.name, "largest_everywhere": "C100_15x17_r3", "ring_only": "C36_15x17_r3", "no_gate": "C100_27x29_real"}


@pytest.mark.parametrize("slip", sorted(SLIP_CASES))
def test_deliberately_wrong_references_leave_the_gradient_bound(slip):
    name = SLIP_CASES[slip]
    case = lgb.BY_NAME[name]
    inp, fwd, grad = lgb.case_ref(name)
    if slip == "no_gate":
        wrong = lgb.grad_ref(inp["grad_out"], fwd["T"], fwd["tol_T"], fwd["arg"], inp["query"], inp["prev"], no_gate=True)
    else:
        bad = lgb.forward_ref(inp["query"], inp["prev"], inp["bits"], case.radii, case.rate, case.n_obj, inp["bias"], slip=slip, dup=inp["dup"])
        assert (bad["arg"] != fwd["arg"]).any(), f"{slip}: the slipped argmin is the right one on {name}"
        wrong = lgb.grad_ref(inp["grad_out"], fwd["T"], fwd["tol_T"], bad["arg"], inp["query"], inp["prev"])
    # bit-equal pixels give the query the same gradient whichever of them wins: that slip shows in grad_prev alone; arg slips leave grad_bias
    keys = {"no_gate": ("query", "prev", "bias"), "ties_highest": ("prev",)}.get(slip, ("query", "prev"))
    for key in keys:
        r = lgb.ratio(wrong["grad_" + key], grad["grad_" + key], grad["tol_" + key])
        assert r > 10.0, f"{slip} stays within {r:.2f} x the bound of grad_{key} on {name}: the GPU test could not see it"


# ------------------------------------------------------------------------------------------ argument checks (no launch, no GPU)
_HOST = (ctypes.c_char * 4096)()
P = ctypes.c_void_p(ctypes.addressof(_HOST))        # a non-null pointer; the entry points return before anything reads it
BIG = 1 << 40


def _radii(values):
    return (ctypes.c_int32 * len(values))(*values)


def _argmin(query=P, prev=P, bits=P, H=5, W=6, C=36, radii=(1, 2, 3), n_obj=3, out=P, arg=P, rate=1):
    r = _radii(radii) if radii is not None else None
    return aoc_amd._lib.lib().aoc_local_window_match_argmin(query, prev, bits, H, W, C, r, len(radii or ()), P, n_obj, out, arg, 1, rate, None)


def _grad(go=P, T=P, arg=P, query=P, prev=P, H=5, W=6, C=36, n_radii=3, n_obj=3, window=3, ws=P, ws_bytes=BIG):
    return aoc_amd._lib.lib().aoc_local_match_grad(go, T, arg, query, prev, H, W, C, n_radii, n_obj, window, P, P, P, ws, ws_bytes, None)


def test_entry_points_reject_bad_arguments_before_any_launch():
    for name in ("query", "prev", "bits", "out", "arg"):
        assert _argmin(**{name: None}) == INVALID, f"argmin: NULL {name}"
    assert _argmin(H=0) == INVALID and _argmin(W=-1) == INVALID and _argmin(n_obj=0) == INVALID and _argmin(rate=0) == INVALID
    assert _argmin(radii=(2, 2)) == INVALID and _argmin(radii=(-1,)) == INVALID
    assert _argmin(C=38) == UNSUPPORTED and _argmin(C=132) == UNSUPPORTED and _argmin(n_obj=aoc_amd.ops.MAX_OBJECTS + 1) == UNSUPPORTED
    assert _argmin(radii=(32,)) == UNSUPPORTED and _argmin(radii=tuple(range(1, 10))) == UNSUPPORTED
    for name in ("go", "T", "arg", "query", "prev", "ws"):
        assert _grad(**{name: None}) == INVALID, f"grad: NULL {name}"
    assert _grad(H=0) == INVALID and _grad(C=0) == INVALID and _grad(n_obj=-1) == INVALID and _grad(n_radii=0) == INVALID and _grad(window=-1) == INVALID
    assert _grad(C=260) == UNSUPPORTED and _grad(n_obj=31) == UNSUPPORTED and _grad(n_radii=9) == UNSUPPORTED and _grad(window=32) == UNSUPPORTED
    assert _grad(ws_bytes=16) == WORKSPACE


def test_workspace_query():
    L = aoc_amd._lib.lib()
    assert L.aoc_local_match_grad_workspace_bytes(0, 5, 36, 3, 3) == 0 and L.aoc_local_match_grad_workspace_bytes(5, 5, 36, 9, 3) == 0
    assert L.aoc_local_match_grad_workspace_bytes(5, 5, 300, 3, 3) == 0
    crop = L.aoc_local_match_grad_workspace_bytes(59, 59, 100, 6, 4)
    assert 2 * 59 * 59 * 24 * 4 <= crop < 2 * 59 * 59 * 24 * 4 + 8192, "two [HW, O n_radii] buffers and the bias partials: nothing grows with the window"


# ------------------------------------------------------------------------------------------ local_train on the host
def _cpu_args(requires_grad=True):
    q = torch.randn(5, 6, 4, requires_grad=requires_grad)
    return torch.randn(5, 6, 4), q, torch.ones(5, 6, 2)


def test_local_train_returns_the_mirror_when_no_gradient_is_wanted(monkeypatch):
    calls = []
    sentinel = object()

    def fake(*args):
        calls.append(args)
        return sentinel

    monkeypatch.setattr(aoc_amd.matching, "local_matching", fake)
    prev, q, lab = _cpu_args(requires_grad=False)
    assert aoc_amd.local_train.local_matching(prev, q, lab, 0.5, [2, 4], (7, 8), 2, True, False, False) is sentinel
    assert calls[-1] == (prev, q, lab, 0.5, [2, 4], (7, 8), 2, True, False, False), "every argument is passed on, in the reference's order"
    prev, q, lab = _cpu_args(requires_grad=True)
    with torch.no_grad():
        assert aoc_amd.local_train.local_matching_proxy(prev, q, lab) is sentinel
    assert calls[-1][3:] == (0., [15], None, 1, True, True, True), "the reference's defaults (AEM:968-971)"
    assert aoc_amd.local_train.local_matching_proxy is aoc_amd.local_train.local_matching


def test_local_train_refuses_float16_and_the_cpu_under_autograd():
    prev, q, lab = _cpu_args()
    with pytest.raises(aoc_amd._lib.AocHipError, match="use_float16"):
        aoc_amd.local_train.local_matching(prev, q, lab)                        # the reference's default argument is use_float16=True
    with pytest.raises(aoc_amd._lib.AocHipError, match="use_float16"):
        aoc_amd.local_train.local_matching(prev, q.detach(), lab, torch.zeros(2, 1, 1, 1, requires_grad=True), [2], None, 1, True)
    with pytest.raises(aoc_amd._lib.AocHipError, match="no CPU fallback"):
        aoc_amd.local_train.local_matching(prev, q, lab, 0., [2], None, 1, False)


def test_the_pinned_stub_and_the_inference_guard_point_to_local_train():
    prev, q, lab = _cpu_args()
    with pytest.raises(aoc_amd._lib.AocHipError, match="local_matching is not yet differentiable.*aoc_amd.local_train.local_matching"):
        aoc_amd.matching_train.local_matching(prev, q, lab, 0., [2], None, 1, False)
    with pytest.raises(aoc_amd._lib.AocHipError, match="global_matching_cluster2 is not yet differentiable") as info:
        aoc_amd.matching_train.global_matching_cluster2(prev, q, lab, 1, 0., None, 1, False, 0)
    assert "local_train" not in str(info.value)
    with pytest.raises(aoc_amd._lib.AocHipError, match="inference-only.*aoc_amd.local_train.local_matching is the differentiable form"):
        aoc_amd.matching.local_matching(prev, q, lab, 0., [2], None, 1, False)
