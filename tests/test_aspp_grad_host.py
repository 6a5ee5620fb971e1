"""What can be checked without a GPU about the differentiable ASPP (aoc_amd.aspp_train, csrc/aspp_grad.hip): the float64 references of
tests/aspp_grad_bounds.py against torch's float64 autograd of the reference's lines (aspp.py:19 four times and :46; :21-23 four times and
:61-65); that every slipped reference leaves its bound; that no element of a GPU case is undecided; the twin's surface (``_TRAINABLE`` hints,
``__all__``, the strict ``state_dict`` round trip, the wrappers absent from ``ops``' public names); that without a wanted gradient the twin goes
through the mirror's calls; the five wrappers against the address / lifetime / dtype contract of aoc_amd.ops with the library stubbed; the
argument checks of the new entry points; the references against the gradients recorded from the reference's own ASPP."""
import ast
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import aoc_amd
import aspp_grad_bounds as agb
import ops_contract_cases as occ
from aoc_amd import _lib, aspp, aspp_train as at, gates_train, ops
from conftest import GOLDEN

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4
f32, f64 = np.float32, np.float64
REL = 1e-12


def _close(got, want, what, rel=REL, scale=0.0):
    """scale: the size of the terms that cancel in `want`, where the result is what they leave behind"""
    got, want = agb.t64(got), agb.t64(want)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} against {tuple(want.shape)}"
    assert (got - want).abs().max() <= rel * max(float(want.abs().max()), scale, 1e-30), f"{what}: off by {float((got - want).abs().max()):.3e}"


def _leaf(a):
    return torch.from_numpy(np.asarray(a, f64)).requires_grad_(True)


# ------------------------------------------------------------------------------------------ the references against float64 autograd
@pytest.mark.parametrize("N,C,S,hw,with_mean", ((1, 3, 1, 5, False), (2, 5, 4, 7, True), (3, 8, 2, 12, True)))
def test_front_references_against_autograd(N, C, S, hw, with_mean):
    rs = agb.rng(N, C, S, hw, 11)
    n = rs.standard_normal
    x, gs, gm = n((N, C, hw)), [n((N, C, hw)) for _ in range(S)], n((N, C))
    al, ga, be = rs.uniform(0.5, 1.5, (S, C)), n((S, C)), 0.5 * n((S, C))
    lx, lal, lga, lbe = _leaf(x), _leaf(al), _leaf(ga), _leaf(be)
    vs, mean = agb.front_forward64(lx, lal, lga, lbe, 1e-5)
    loss = sum((v * torch.from_numpy(g)).sum() for v, g in zip(vs, gs))
    if with_mean:
        loss = loss + (mean * torch.from_numpy(gm)).sum()
    loss.backward()
    got = agb.front_chain(x, gs, gm if with_mean else None, al, ga, be, 1e-5)
    _close(got["grad_x"], lx.grad, "grad_x")
    _close(got["grad_alpha"], lal.grad, "grad_alpha")
    _close(got["grad_gamma"], lga.grad, "grad_gamma")
    _close(got["grad_beta"], lbe.grad, "grad_beta")


@pytest.mark.parametrize("N,C,groups,n_src,C_tail,hw", ((1, 4, 2, 1, 0, 5), (2, 4, 2, 4, 3, 7), (3, 8, 2, 2, 5, 12), (2, 6, 6, 3, 2, 9)))
def test_back_reference_against_autograd(N, C, groups, n_src, C_tail, hw):
    rs = agb.rng(N, C, groups, n_src, C_tail, hw, 12)
    n = rs.standard_normal
    C_total = n_src * C + C_tail
    us, w, b = [n((N, C, hw)) for _ in range(n_src)], 1 + 0.5 * n((n_src, C)), 0.5 * n((n_src, C))
    tail = n((N, C_tail)) if C_tail else None
    al, ga, be, g = rs.uniform(0.5, 1.5, C_total), n(C_total), 0.5 * n(C_total), n((N, C_total, hw))
    lus, lw, lb = [_leaf(u) for u in us], _leaf(w), _leaf(b)
    lt = _leaf(tail) if C_tail else None
    lal, lga, lbe = _leaf(al), _leaf(ga), _leaf(be)
    out = agb.back_forward64(lus, groups, list(lw), list(lb), 1e-5, lt, lal, lga, lbe, 1e-5)
    (out * torch.from_numpy(g)).sum().backward()
    sv = agb.back_saved64(us, groups, w, b, 1e-5, tail, al, ga, be, 1e-5)
    _close(sv["out"], out.detach(), "the saved forward")
    got, _ = agb.cat_grad_ref(g, us, sv["stats"], groups, w, b, tail, sv["plane_sumsq"], sv["gate"], al, ga, 1e-5)
    for k in range(n_src):
        _close(got["grad_u"][k][0], lus[k].grad, f"grad_u[{k}]")
    _close(got["grad_gamma"][0], lw.grad, "grad_gamma")
    _close(got["grad_beta"][0], lb.grad, "grad_beta")
    if C_tail:
        _close(got["grad_tail"][0], lt.grad, "grad_tail")
    _close(got["grad_gct_alpha"][0], lal.grad, "grad_gct_alpha")
    _close(got["grad_gct_gamma"][0], lga.grad, "grad_gct_gamma")
    _close(got["grad_gct_beta"][0], lbe.grad, "grad_gct_beta")


# ------------------------------------------------------------------------------------------ the slipped twins leave the bounds
def _leaves(want_tol, slipped, what):
    want, tol = want_tol
    assert ((agb.t64(slipped) - want).abs() > tol).any(), f"{what}: the slipped reference stays inside the bound (bound too loose)"


@pytest.mark.parametrize("hw", (35, 1025))
def test_front_slips_leave_the_bounds(hw):
    N, C, S = 2, 5, 4
    s = agb.front_case(N, C, S, hw)
    flat = lambda t: t.reshape(N * C, hw)
    x, gs = flat(s["x"]), [flat(g) for g in s["gs"]]
    dots = agb.plane_dot_multi_ref(x, gs)
    for kind in ("drop_last", "other_set"):
        _leaves(dots, agb.plane_dot_multi_ref(x, gs, kind)[0], f"plane_dot_multi {kind}")
    sq = (agb.t64(s["x"]) ** 2).sum(2).numpy().astype(f32)
    gates = np.stack([agb.gct_gate64(agb.t64(sq), s["alpha"][k], s["gamma"][k], s["beta"][k], 1e-5, False).numpy() for k in range(S)]).astype(f32)
    dg = dots[0].reshape(S, N, C).numpy().astype(f32)
    ref = agb.gct_gate_multi_grad_ref(dg, gates, sq, s["alpha"], s["gamma"], 1e-5)
    for kind in ("other_gate", "no_dM", "drop_last"):
        bad = agb.gct_gate_multi_grad_ref(dg, gates, sq, s["alpha"], s["gamma"], 1e-5, slip=kind)
        for name in (("dsum_total", "dsum") if kind != "drop_last" else ("grad_alpha", "grad_beta")):
            _leaves(ref[name], bad[name][0], f"gct_gate_multi_grad {kind} {name}")
    dst = ref["dsum_total"][0].reshape(-1).numpy().astype(f32)
    want = agb.front_apply_ref(gs, gates.reshape(S, -1), x, dst, s["dmean"].reshape(-1))
    for kind in agb.FRONT_SLIPS:
        _leaves(want, agb.front_apply_ref(gs, gates.reshape(S, -1), x, dst, s["dmean"].reshape(-1), kind)[0], f"front apply {kind}")


@pytest.mark.parametrize("key", [k for k in agb.BACK_CASES if k[0] * k[1] * k[3] * k[5] <= 2 * 8 * 4 * 1025 and k[5] > 1])
def test_back_slips_leave_the_bounds_and_no_element_is_undecided(key):
    s = agb.back_case(*key)
    args = agb.back_ref_args(s, agb.back_saved32(s))
    ref, und = agb.cat_grad_ref(**args)
    assert sum(int(u.sum()) for u in und) == 0, f"{key}: undecided ReLU elements; take another seed"
    n_src, C_tail = key[3], key[4]
    for kind in agb.BACK_SLIPS:
        if kind == "tail_no_hw" and not C_tail:
            continue
        bad, _ = agb.cat_grad_ref(**args, slip=kind)
        if kind == "tail_no_hw":
            _leaves(ref["grad_tail"], bad["grad_tail"][0], f"{key} {kind} grad_tail")
            continue
        _leaves(ref["grad_u"][n_src - 1], bad["grad_u"][n_src - 1][0], f"{key} {kind} grad_u")
        _leaves(ref["grad_beta"], bad["grad_beta"][0], f"{key} {kind} grad_beta")
        _leaves(ref["grad_gamma"], bad["grad_gamma"][0], f"{key} {kind} grad_gamma")


def test_planted_cases_are_exact_in_the_reference():
    """gamma = beta = 0 on a channel: z == 0, the mask is off and grad_u keeps only the group means; a tail entry <= 0: grad_tail exactly 0;
    GCT gamma = beta = 0 on a channel: its gate is exactly 1."""
    key = (2, 8, 2, 4, 4, 35)
    s = agb.back_case(*key)
    saved = agb.back_saved32(s)
    ref, _ = agb.cat_grad_ref(**agb.back_ref_args(s, saved))
    assert float(ref["grad_tail"][0][0, 0]) == 0.0 and float(ref["grad_tail"][0][-1, 1]) == 0.0 and float(ref["grad_tail"][1][0, 0]) == 0.0
    assert (saved["gate"][:, 2] == 1.0).all()
    assert float(agb.t64(saved["cat"])[:, 1].abs().max()) == 0.0                       # channel 1 of source 0: relu(0)
    assert float(ref["grad_gamma"][0][0, 1]) == 0.0 and float(ref["grad_beta"][0][0, 1]) == 0.0


def test_large_case_has_no_undecided_element():
    key = (3, 128, 32, 4, 128, 31 * 33)
    s = agb.back_case(*key)
    _, und = agb.cat_grad_ref(**agb.back_ref_args(s, agb.back_saved32(s)))
    assert sum(int(u.sum()) for u in und) == 0, f"{key}: undecided ReLU elements; take another seed"


# ------------------------------------------------------------------------------------------ the twin's surface
def test_state_dict_round_trip_and_signatures():
    twin, mirror = at.ASPP(), aspp.ASPP()
    a, b = twin.state_dict(), mirror.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    missing, unexpected = twin.load_state_dict(b, strict=True)
    assert not missing and not unexpected and all(torch.equal(twin.state_dict()[k], b[k]) for k in b)
    mirror.load_state_dict(twin.state_dict(), strict=True)
    assert inspect.signature(at.ASPP.__init__) == inspect.signature(aspp.ASPP.__init__)
    assert inspect.signature(at.ASPP.forward) == inspect.signature(aspp.ASPP.forward)
    assert inspect.signature(at._ASPPModule.__init__) == inspect.signature(aspp._ASPPModule.__init__)
    assert isinstance(twin.GCT, gates_train.GCT) and isinstance(twin.aspp3.GCT, gates_train.GCT)
    assert [(m.kernel_size, m.padding, m.dilation) for m in twin.modules() if isinstance(m, torch.nn.Conv2d)] == \
        [(m.kernel_size, m.padding, m.dilation) for m in mirror.modules() if isinstance(m, torch.nn.Conv2d)]
    assert "aspp_train" in aoc_amd.__all__ and aoc_amd.aspp_train is at


def test_mirrors_point_to_the_twin():
    assert ops._TRAINABLE["ASPP"] == "aspp_train.ASPP" and ops._TRAINABLE["_ASPPModule"] == "aspp_train._ASPPModule"
    x = torch.randn(1, 512, 2, 3, requires_grad=True)
    with pytest.raises(_lib.AocHipError, match="inference-only.*aspp_train.ASPP is the differentiable form"):
        aspp.ASPP()(x)
    with pytest.raises(_lib.AocHipError, match="inference-only.*aspp_train._ASPPModule is the differentiable form"):
        aspp._ASPPModule(512, 128, 1, 0, 1)(x)
    assert "aspp_train" in inspect.getdoc(ops.inference_only)
    with pytest.raises(_lib.AocHipError, match="no CPU fallback"):
        at.ASPP()(x)


@pytest.mark.parametrize("fused", (True, False))
def test_no_gradient_path_goes_through_the_mirrors_ops(monkeypatch, fused):
    """Library stubbed: under no_grad (and with nothing that wants a gradient) the twin makes exactly the mirror's ops calls, in its order."""
    def run(net):
        seen = []
        N, h, w = 2, 2, 3
        shapes = {"plane_sum_sumsq": lambda *a, **k: (None, torch.ones(N, 512), torch.ones(N, 512)), "gct_gate_multi": lambda *a, **k: torch.ones(4, N, 512),
                  "channel_scale_multi": lambda x, g, **k: [x.clone() for _ in range(4)], "linear": lambda m, w_, b_: torch.ones(N, 128),
                  "groupnorm_cat_relu": lambda *a, **k: (torch.ones(N, 640, h, w), torch.ones(N, 640)), "gct_gate": lambda s, *a: torch.ones_like(s),
                  "channel_scale": lambda x, g, out=None: x, "groupnorm_relu": lambda x, *a, **k: x, "plane_mean": lambda x: torch.ones(N, 512),
                  "plane_reduce": lambda x, m: torch.ones(x.shape[0], x.shape[1])}
        with monkeypatch.context() as mp:
            for name, fn in shapes.items():
                mp.setattr(ops, name, lambda *a, _n=name, _f=fn, **k: seen.append(_n) or _f(*a, **k))
            with torch.no_grad():
                net(torch.randn(N, 512, h, w).requires_grad_(True), fused=fused)
            for p in net.parameters():
                p.requires_grad_(False)
            net(torch.randn(N, 512, h, w), fused=fused)                     # autograd on, nothing wants a gradient: the same path
        return seen
    torch.manual_seed(3)
    twin, mirror = at.ASPP(), aspp.ASPP()
    for p in mirror.parameters():
        p.requires_grad_(False)
    got = run(twin)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "inference_only", lambda *a, **k: None)
        want = run(mirror)
    assert got == want and len(got) > 10


def test_wrappers_take_addresses_only_through_the_helpers():
    src = inspect.getsource(at)
    assert "data_ptr" not in src and "import ctypes" not in src
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ("_p", "_addr"):
            assert not any(isinstance(sub, ast.Call) for arg in node.args for sub in ast.walk(arg)), f"line {node.lineno}: a call expression inside _p(...)"
    public = {n for n, v in vars(ops).items() if callable(v) and not n.startswith("_") and getattr(v, "__module__", None) == ops.__name__}
    new = {"plane_dot_multi", "gct_gate_multi_backward", "channel_scale_multi_backward_apply", "groupnorm_cat_relu_forward", "groupnorm_cat_relu_backward"}
    assert not new & public and all(callable(getattr(at, n)) for n in new)


def test_wrappers_reject_mismatched_shapes_without_a_device():
    x = torch.zeros(2, 5, 3, 4)
    with pytest.raises(ValueError):
        at.plane_dot_multi(x, [])
    with pytest.raises(ValueError):
        at.plane_dot_multi(x, [x] * 9)
    with pytest.raises(ValueError):
        at.plane_dot_multi(x, [x, torch.zeros(2, 5, 4, 3)])
    with pytest.raises(ValueError):
        at.gct_gate_multi_backward(torch.zeros(4, 2, 5), torch.zeros(4, 2, 5), torch.zeros(2, 6), *([torch.zeros(4, 5)] * 3), 1e-5)
    with pytest.raises(ValueError):
        at.gct_gate_multi_backward(torch.zeros(4, 2, 5), torch.zeros(4, 2, 5), torch.zeros(2, 5), torch.zeros(3, 5), torch.zeros(4, 5), torch.zeros(4, 5), 1e-5)
    with pytest.raises(ValueError):
        at.channel_scale_multi_backward_apply([x, x], torch.zeros(3, 2, 5), x, torch.zeros(2, 5))
    with pytest.raises(ValueError):
        at.channel_scale_multi_backward_apply([x], torch.zeros(1, 2, 5), x, torch.zeros(2, 5), grad_x=torch.zeros(2, 5, 4, 3))
    us = [torch.zeros(2, 8, 3, 4)] * 2
    ok = dict(stats=torch.zeros(2, 8, 2), groups=4, gamma=None, beta=None, tail=torch.zeros(2, 3), plane_sumsq=torch.zeros(2, 19), gate=torch.zeros(2, 19),
              gct_alpha=torch.zeros(19), gct_gamma=torch.zeros(19), gct_eps=1e-5)
    with pytest.raises(ValueError):
        at.groupnorm_cat_relu_backward(torch.zeros(2, 18, 3, 4), us, **ok)
    with pytest.raises(ValueError):
        at.groupnorm_cat_relu_backward(torch.zeros(2, 19, 3, 4), us, **dict(ok, groups=3))
    with pytest.raises(ValueError):
        at.groupnorm_cat_relu_backward(torch.zeros(2, 19, 3, 4), us, **dict(ok, stats=torch.zeros(2, 7, 2)))
    with pytest.raises(ValueError):
        at.groupnorm_cat_relu_backward(torch.zeros(2, 19, 3, 4), us, **ok, out={"grad_tail": torch.zeros(2, 4)})
    with pytest.raises(_lib.AocHipError):                                              # well-formed, but on the CPU: no fallback
        at.groupnorm_cat_relu_backward(torch.zeros(2, 19, 3, 4), us, **ok)
    with pytest.raises(_lib.AocHipError):
        at.plane_dot_multi(x, [x, x])


# ------------------------------------------------------------------------------------------ the C entry points before any launch
def _ptrs(*bufs):
    return (ctypes.c_void_p * len(bufs))(*[ctypes.cast(b, ctypes.c_void_p).value if b is not None else None for b in bufs])


def test_entries_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    bufs = [(ctypes.c_float * 4096)() for _ in range(24)]
    p = lambda i: ctypes.cast(bufs[i], ctypes.c_void_p)

    def pd(x=p(0), gs=_ptrs(bufs[1], bufs[2]), n_set=2, planes=3, hw=7, dots=p(3)):
        return L.aoc_plane_dot_multi(x, gs, n_set, planes, hw, dots, None)
    assert pd(x=None) == INVALID and pd(gs=None) == INVALID and pd(dots=None) == INVALID and pd(gs=_ptrs(bufs[1], None)) == INVALID
    assert pd(n_set=0) == INVALID and pd(n_set=9, gs=_ptrs(*bufs[4:13])) == INVALID and pd(planes=0) == INVALID and pd(hw=0) == INVALID
    assert pd(planes=2 ** 31) == UNSUPPORTED and pd(dots=p(0)) == INVALID and pd(dots=p(2)) == INVALID

    need = L.aoc_gct_gate_multi_grad_workspace_bytes(4, 2, 5)
    assert need >= 4 * 2 * 5 * 4 and L.aoc_gct_gate_multi_grad_workspace_bytes(0, 2, 5) == 0

    def gg(dg=p(0), gate=p(1), s=p(2), al=p(3), ga=p(4), n_set=4, N=2, C=5, tot=p(5), ds=p(6), gal=p(7), gga=p(8), gbe=p(9), ws=p(10), nbytes=need):
        return L.aoc_gct_gate_multi_grad(dg, gate, s, al, ga, None, n_set, N, C, 1e-5, 0, tot, ds, gal, gga, gbe, ws, nbytes, None)
    assert gg(dg=None) == INVALID and gg(gate=None) == INVALID and gg(s=None) == INVALID and gg(al=None) == INVALID and gg(ga=None) == INVALID
    assert gg(n_set=0) == INVALID and gg(n_set=9) == INVALID and gg(N=0) == INVALID and gg(C=0) == INVALID and gg(N=31) == UNSUPPORTED
    assert gg(ds=None, nbytes=need - 1) == WORKSPACE and gg(ds=None, ws=None) == WORKSPACE
    assert gg(tot=p(6)) == INVALID and gg(gal=p(3)) == INVALID and gg(gbe=p(8)) == INVALID       # outputs on one another, on an input
    assert gg(tot=None, ds=None, gal=None, gga=None, gbe=None, ws=None, nbytes=0) == OK

    def ap(gs=_ptrs(bufs[0], bufs[1]), gates=p(2), x=p(3), tot=p(4), dm=p(5), n_set=2, planes=3, hw=7, gx=p(6)):
        return L.aoc_channel_scale_multi_grad_apply(gs, gates, x, tot, dm, n_set, planes, hw, gx, None)
    assert ap(gs=None) == INVALID and ap(gates=None) == INVALID and ap(x=None) == INVALID and ap(tot=None) == INVALID and ap(gx=None) == INVALID
    assert ap(gs=_ptrs(bufs[0], None)) == INVALID and ap(n_set=0) == INVALID and ap(n_set=9) == INVALID and ap(planes=0) == INVALID and ap(hw=0) == INVALID
    assert ap(planes=2 ** 31) == UNSUPPORTED and ap(gx=p(3)) == INVALID and ap(gx=p(1)) == INVALID and ap(gx=p(5)) == INVALID

    need = L.aoc_groupnorm_cat_relu_grad_workspace_bytes(2, 2, 8, 3, 4)
    assert need >= (6 * 2 * 19 + 2 * 2 * 4 * 2) * 4
    assert L.aoc_groupnorm_cat_relu_grad_workspace_bytes(0, 2, 8, 3, 4) == 0 and L.aoc_groupnorm_cat_relu_grad_workspace_bytes(9, 2, 8, 3, 4) == 0
    assert L.aoc_groupnorm_cat_relu_grad_workspace_bytes(2, 2, 8, 3, 3) == 0 and L.aoc_groupnorm_cat_relu_grad_workspace_bytes(2, 2, 8, -1, 4) == 0

    def cg(g=p(0), us=_ptrs(bufs[1], bufs[2]), n_src=2, N=2, C=8, hw=3, groups=4, st=p(3), tail=p(6), C_tail=3, sq=p(7), gate=p(8), al=p(9), ga=p(10),
           gus=_ptrs(bufs[11], bufs[12]), ggam=p(13), gbet=p(14), gt=p(15), gal=p(16), gga=p(17), gbe=p(18), ws=p(19), nbytes=need):
        return L.aoc_groupnorm_cat_relu_grad(g, us, n_src, N, C, hw, groups, st, p(4), p(5), tail, C_tail, sq, gate, al, ga, 1e-5, gus, ggam, gbet, gt, gal,
                                             gga, gbe, ws, nbytes, None)
    assert cg(g=None) == INVALID and cg(us=None) == INVALID and cg(st=None) == INVALID and cg(sq=None) == INVALID and cg(gate=None) == INVALID
    assert cg(al=None) == INVALID and cg(ga=None) == INVALID and cg(us=_ptrs(bufs[1], None)) == INVALID
    assert cg(n_src=0) == INVALID and cg(n_src=9) == INVALID and cg(N=0) == INVALID and cg(C=0) == INVALID and cg(hw=0) == INVALID and cg(groups=0) == INVALID
    assert cg(groups=3) == INVALID and cg(C_tail=-1) == INVALID and cg(tail=None) == INVALID and cg(C_tail=0, tail=None) == INVALID   # grad_tail without a tail
    assert cg(N=31) == UNSUPPORTED
    assert cg(nbytes=need - 1) == WORKSPACE and cg(ws=None) == WORKSPACE
    assert cg(gus=_ptrs(bufs[11], bufs[11])) == INVALID and cg(gus=_ptrs(bufs[1], bufs[12])) == INVALID and cg(gus=_ptrs(bufs[0], bufs[12])) == INVALID
    assert cg(ggam=p(14)) == INVALID and cg(gt=p(6)) == INVALID and cg(gal=p(9)) == INVALID and cg(ws=p(0)) == INVALID and cg(ws=p(13)) == INVALID
    assert cg(gus=None, ggam=None, gbet=None, gt=None, gal=None, gga=None, gbe=None, ws=None, nbytes=0) == OK


# ------------------------------------------------------------------------------------------ the gradients recorded from the reference's own ASPP
@pytest.mark.parametrize("name", agb.ASPP_FIXTURES)
def test_references_equal_the_recorded_gradients(name, golden):
    """The float64 gradients recorded from the reference's own ASPP under autograd (tests/golden/make_golden_aspp_grad.py) against the chain
    of this module's references: both fused stages by plane_dot_multi_ref / gct_gate_multi_grad_ref / front_apply_ref and cat_grad_ref, the
    convolutions between them by torch's float64 autograd."""
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 250000
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        assert z["in_x"].dtype == np.float16 and z["in_weight"].dtype == np.float16 and all(z[k].dtype == np.float16 for k in z.files if k.startswith("p_"))
        assert all(z[k].dtype == np.float64 for k in z.files if k.startswith("grad_"))
    fx = golden(name)
    N, h, w = agb.FIXTURE_SHAPES[name]
    assert fx["in_x"].shape == (N, 512, h, w)
    net = agb.load_fixture_parameters(at.ASPP(), fx)
    got, out = agb.aspp_chain64(fx["in_x"], fx["in_weight"], net.state_dict())
    _close(float((out * agb.t64(fx["in_weight"])).sum()), float(fx["loss"]), "the loss", rel=1e-12, scale=float((out.abs() * agb.t64(fx["in_weight"]).abs()).sum()))
    keys = [k[5:] for k in fx if k.startswith("grad_")]
    assert "x" in keys and "global_avg_pool.1.weight" in keys and "aspp1.atrous_conv.weight" in keys and "GCT.gamma" in keys and "aspp4.bn.bias" in keys
    assert len(keys) == 1 + 2 + 5 * 3 + 5 * 2
    for k in keys:
        rec = agb.t64(fx["grad_" + k])
        mine = agb.recorded_view(k, got[k]).reshape(rec.shape)
        _close(mine, rec, f"{name}: grad {k}")


# ------------------------------------------------------------------------------------------ the tensor contract, library stubbed
ERRORS = occ.ERRORS + (_lib.AocHipError,)


def _t(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(f32))


def _cases():
    N, C, S, G, H, W, Ct = 2, 4, 2, 2, 3, 5, 3
    Fi, OUT = occ.F, occ.OUT

    def mk(builder):
        return lambda ops_, device: {k: v.to(device) for k, v in builder(np.random.RandomState(7)).items()}
    z = torch.zeros
    gate_out = dict(dsum_total=(N, C), dsum=(S, N, C), grad_alpha=(S, C), grad_gamma=(S, C), grad_beta=(S, C))
    cat_out = dict(grad_gamma=(S, C), grad_beta=(S, C), grad_tail=(N, Ct), grad_gct_alpha=(S * C + Ct,), grad_gct_gamma=(S * C + Ct,), grad_gct_beta=(S * C + Ct,))
    return [
        occ.Case("plane_dot_multi", [], mk(lambda rs: dict(x=_t(rs, N, C, H, W), g0=_t(rs, N, C, H, W), g1=_t(rs, N, C, H, W), dots=z(S, N, C))),
                 {"x": Fi, "g0": Fi, "g1": Fi, "dots": OUT}, lambda ops_, a: at.plane_dot_multi(a["x"], [a["g0"], a["g1"]], a["dots"]), None),
        occ.Case("gct_gate_multi_backward", [], mk(lambda rs: dict(dgate=_t(rs, S, N, C), gate=_t(rs, S, N, C), sums=_t(rs, N, C), alpha=_t(rs, S, C), gamma=_t(rs, S, C),
                                                                   beta=_t(rs, S, C), **{k: z(*s) for k, s in gate_out.items()})),
                 dict({k: Fi for k in ("dgate", "gate", "sums", "alpha", "gamma", "beta")}, **{k: OUT for k in gate_out}),
                 lambda ops_, a: at.gct_gate_multi_backward(a["dgate"], a["gate"], a["sums"], a["alpha"], a["gamma"], a["beta"], 1e-5, False,
                                                            out={k: a[k] for k in gate_out}), None),
        occ.Case("channel_scale_multi_backward_apply", [], mk(lambda rs: dict(g0=_t(rs, N, C, H, W), g1=_t(rs, N, C, H, W), gates=_t(rs, S, N, C), x=_t(rs, N, C, H, W),
                                                                              dsum_total=_t(rs, N, C), dmean=_t(rs, N, C), grad_x=z(N, C, H, W))),
                 {"g0": Fi, "g1": Fi, "gates": Fi, "x": Fi, "dsum_total": Fi, "dmean": Fi, "grad_x": OUT},
                 lambda ops_, a: at.channel_scale_multi_backward_apply([a["g0"], a["g1"]], a["gates"], a["x"], a["dsum_total"], a["dmean"], a["grad_x"]), None),
        occ.Case("groupnorm_cat_relu_forward", [], mk(lambda rs: dict(x0=_t(rs, N, C, H, W), x1=_t(rs, N, C, H, W), gamma=_t(rs, S, C), beta=_t(rs, S, C), tail=_t(rs, N, Ct))),
                 {k: Fi for k in ("x0", "x1", "gamma", "beta", "tail")},
                 lambda ops_, a: at.groupnorm_cat_relu_forward([a["x0"], a["x1"]], G, a["gamma"], a["beta"], 1e-5, a["tail"]), None),
        occ.Case("groupnorm_cat_relu_backward", [], mk(lambda rs: dict(grad_out=_t(rs, N, S * C + Ct, H, W), u0=_t(rs, N, C, H, W), u1=_t(rs, N, C, H, W), stats=_t(rs, S, N * G, 2),
                                                                       gamma=_t(rs, S, C), beta=_t(rs, S, C), tail=_t(rs, N, Ct), sumsq=_t(rs, N, S * C + Ct),
                                                                       gate=_t(rs, N, S * C + Ct), gct_alpha=_t(rs, S * C + Ct), gct_gamma=_t(rs, S * C + Ct),
                                                                       gu0=z(N, C, H, W), gu1=z(N, C, H, W), **{k: z(*s) for k, s in cat_out.items()})),
                 dict({k: Fi for k in ("grad_out", "u0", "u1", "stats", "gamma", "beta", "tail", "sumsq", "gate", "gct_alpha", "gct_gamma")},
                      **{k: OUT for k in ("gu0", "gu1") + tuple(cat_out)}),
                 lambda ops_, a: at.groupnorm_cat_relu_backward(a["grad_out"], [a["u0"], a["u1"]], a["stats"], G, a["gamma"], a["beta"], a["tail"], a["sumsq"], a["gate"],
                                                                a["gct_alpha"], a["gct_gamma"], 1e-5, out=dict({k: a[k] for k in cat_out}, grad_u=[a["gu0"], a["gu1"]])), None),
    ]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.name)
def test_wrappers_keep_the_tensor_contract(monkeypatch, case):
    with monkeypatch.context() as mp:
        rec = occ.install(mp, ops)
        err, _ = occ.run_recorded(ops, case, case.build(ops, "cpu"), ERRORS)
    assert err is None and rec.calls and rec.records, f"{case.name}: the canonical call raised {err!r} or never reached the library"
    canon = rec.records
    assert all(r.shape is None or (r.contiguous and r.alive) for r in canon), f"{case.name}: the canonical call hands over a dead or strided tensor"
    ran = 0
    for label, transforms, role in occ.variants_of(case, narrow=True):
        a = occ.apply_variant(case.build(ops, "cpu"), transforms)
        if label.endswith(":strided") and all(a[n].is_contiguous() for n in transforms):
            continue
        with monkeypatch.context() as mp:
            rec = occ.install(mp, ops)
            err, _ = occ.run_recorded(ops, case, a, ERRORS)
        bad = occ.check_rule(canon, rec, err, role, "cpu")
        assert not bad, f"({case.name}, {label}): {'; '.join(bad)}"
        ran += 1
    assert ran
