"""What can be checked without a GPU about the differentiable calibration gates (aoc_amd.gates_train, csrc/gate_grad.hip): the float64
references of tests/gates_grad_bounds.py against torch's float64 autograd of the reference's lines (oracle.calibration) and against the
gradients recorded from the reference's own modules (tests/golden/gates_grad_*.npz); that every slipped reference leaves its bound; that
the random conditioning cases keep their undecided pixels under the cap; the twins' parameter names; the wrappers against the address /
lifetime / dtype contract of aoc_amd.ops with the library stubbed; the no-gradient path; the argument checks of the new entry points."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import aoc_amd
import gates_grad_bounds as ggb
import ops_contract_cases as occ
from aoc_amd import _lib, gates_train as gt, ops
from conftest import load_golden
from oracle import calibration as ocal

OK, INVALID, UNSUPPORTED = 0, -1, -4
f32, f64 = np.float32, np.float64
ERRORS = occ.ERRORS + (_lib.AocHipError,)
REL = 1e-12                                   # the tolerance test_frontend_grad_host.py uses for its recorded fixtures


def _close(got, want, what):
    got, want = ggb.t64(got), ggb.t64(want)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} against {tuple(want.shape)}"
    assert (got - want).abs().max() <= REL * max(float(want.abs().max()), 1e-30), f"{what}: off by {float((got - want).abs().max()):.3e}"


def _leaf(a):
    return torch.from_numpy(np.asarray(a, f64)).requires_grad_(True)


# ------------------------------------------------------------------------------------------ the references against float64 autograd
@pytest.mark.parametrize("O,c,D,h,w", ((1, 1, 1, 1, 1), (2, 5, 7, 3, 3), (3, 16, 40, 5, 7)))
def test_ia_gate_references_against_autograd(O, c, D, h, w):
    rs = ggb.rng(O, c, D, 1)
    x, head, W, b, gy = (rs.standard_normal(s) for s in ((O, c, h, w), (O, D), (c, D), (c,), (O, c, h, w)))
    lx, lh, lw, lb = _leaf(x), _leaf(head), _leaf(W / np.sqrt(D)), _leaf(b)
    out = ocal.ia_gate(lx, lh, lw, lb)                                             # ATT:12-17
    (out * torch.from_numpy(gy)).sum().backward()
    got = ggb.ia_gate_chain(x, head, W / np.sqrt(D), b, gy)
    for name, want in (("out", out.detach()), ("grad_x", lx.grad), ("grad_head", lh.grad), ("grad_weight", lw.grad), ("grad_bias", lb.grad)):
        _close(got[name], want, f"IA_gate {name}")


@pytest.mark.parametrize("mode,after_relu", (("l2", False), ("l1", False), ("l1", True)))
@pytest.mark.parametrize("N,C,hw", ((1, 1, 1), (3, 5, 35), (2, 300, 4)))
def test_gct_references_against_autograd(mode, after_relu, N, C, hw):
    rs = ggb.rng(N, C, hw, 2)
    x = rs.standard_normal((N, C, hw, 1))
    if after_relu:
        x = np.abs(x)
    al, ga, be, gy = rs.uniform(0.5, 1.5, (1, C, 1, 1)), rs.standard_normal((1, C, 1, 1)), rs.standard_normal((1, C, 1, 1)), rs.standard_normal(x.shape)
    lx, la, lg, lb = _leaf(x), _leaf(al), _leaf(ga), _leaf(be)
    out = ocal.gct_forward(lx, la, lg, lb, ggb.eps32(1e-5), mode, after_relu)      # gct.py:17-36, with the float epsilon the kernels take
    (out * torch.from_numpy(gy)).sum().backward()
    got = ggb.gct_chain(x, al, ga, be, 1e-5, mode, after_relu, gy)
    for name, want in (("out", out.detach()), ("grad_x", lx.grad), ("grad_alpha", la.grad.reshape(-1)), ("grad_gamma", lg.grad.reshape(-1)),
                       ("grad_beta", lb.grad.reshape(-1))):
        # one channel: e norm does not depend on alpha, and grad_alpha is what two terms of the size of grad_gamma gamma / alpha leave behind
        cancel = 8 * 2.0 ** -53 * float((lg.grad * lg.detach() / la.detach()).abs().max()) if name == "grad_alpha" else 0.0
        assert (ggb.t64(got[name]) - want).abs().max() <= REL * float(want.abs().max()) + cancel, f"GCT {mode} {name}"


def _block_params64(p):
    return {"CL_1.phi_w": _leaf(p["phi_w"]), "CL_1.phi_b": _leaf(p["phi_b"]), "CL_1.mlp_w": _leaf(p["w1"]), "CL_1.mlp_b": _leaf(p["b1"]),
            "CL_2.mlp_w": _leaf(p["w2"]), "CL_2.mlp_b": _leaf(p["b2"]), "CL_3.mlp_w": _leaf(p["w3"]), "CL_3.mlp_b": _leaf(p["b3"]),
            "mlp_w": _leaf(p["wm"]), "mlp_b": _leaf(p["bm"])}


@pytest.mark.parametrize("case", ggb.COND_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conditioning_block_references_against_autograd(case):
    s = ggb.cond_case(*case)
    beta = (s["k_rank"] + 0.5) / (s["x"].shape[2] * s["x"].shape[3])               # int(beta h w) = k_rank, free of float products that land on k
    lx, lh, lp = _leaf(s["x"]), _leaf(s["head"]), _block_params64(s["p"])
    out = ocal.conditioning_block(lx, lh, lp, beta)                                # CLB:66-86 restated
    (out * torch.from_numpy(s["grad_y"].astype(f64))).sum().backward()
    got = ggb.cond_block_chain(s["x"], s["head"], s["p"], s["k_rank"], s["grad_y"])
    assert lp["CL_1.phi_w"].grad is None and lp["CL_1.phi_b"].grad is None, "autograd reaches phi through the comparison"
    for name, want in (("out", out.detach()), ("grad_x", lx.grad), ("grad_head", lh.grad), ("grad_w1", lp["CL_1.mlp_w"].grad),
                       ("grad_b1", lp["CL_1.mlp_b"].grad), ("grad_w2", lp["CL_2.mlp_w"].grad), ("grad_b2", lp["CL_2.mlp_b"].grad),
                       ("grad_w3", lp["CL_3.mlp_w"].grad), ("grad_b3", lp["CL_3.mlp_b"].grad), ("grad_wm", lp["mlp_w"].grad), ("grad_bm", lp["mlp_b"].grad)):
        _close(got[name], want, f"conditioning_block {case} {name}")
    k = s["k_rank"]
    if s["kind"] == "constant":
        assert not got["mask"].any(), "constant planes: every score ties and the strict > keeps nothing"
    else:
        assert (got["mask"].sum(1) == k - 1).all(), "strict >: the pixels above the k-th largest score"
    if s["kind"] == "tie":
        tied = torch.from_numpy(s["tied"])
        sc = got["scores"].gather(1, tied)
        assert (sc[:, 0] == sc[:, 1]).all() and (sc[:, 0] == got["thr"]).all() and not got["mask"].gather(1, tied).any(), "the strict > keeps a tied pixel"
    if case[0] == 1:
        assert float(ggb.cond_codes_grad_ref(np.ones((1, 2 * case[1] + case[2])), *(np.ones(t) for t in ((1, case[1]), (1, case[1]), (1, case[2]))),
                                            s["p"]["w1"], s["p"]["w2"], s["p"]["w3"])["dpx"][0].abs().max()) == 0.0, "N = 1: dpx = dd - dd"


def test_conditioning_layer_reference_against_autograd():
    s = ggb.cond_case(3, 24, 5, 9, 11, 0.3, 11)
    gy = ggb.rng(12).standard_normal((3, 24))
    lx, lw, lb = _leaf(s["x"]), _leaf(s["p"]["w1"]), _leaf(s["p"]["b1"])
    out = ocal.conditioning_layer(lx, torch.from_numpy(s["p"]["phi_w"].astype(f64)), torch.from_numpy(s["p"]["phi_b"].astype(f64)), lw, lb,
                                  (s["k_rank"] + 0.5) / 99)
    (out * torch.from_numpy(gy)).sum().backward()
    got = ggb.cond_layer_chain(s["x"], s["p"], s["k_rank"], gy)
    for name, want in (("out", out.detach()), ("grad_x", lx.grad), ("grad_w1", lw.grad), ("grad_b1", lb.grad)):
        _close(got[name], want, f"conditioning_layer {name}")


# ------------------------------------------------------------------------------------------ the references ARE the reference's modules
@pytest.mark.parametrize("name", ggb.IA_FIXTURES)
def test_ia_gate_reference_reproduces_the_recorded_gradients(name):
    fx = load_golden(name)
    got = ggb.ia_gate_chain(fx["in_x"], fx["in_head"], fx["w_IA__weight"], fx["w_IA__bias"], fx["in_weight"])
    for key, rec in (("out", "out"), ("grad_x", "grad_x"), ("grad_head", "grad_head"), ("grad_weight", "grad_w_IA__weight"), ("grad_bias", "grad_w_IA__bias")):
        _close(got[key], fx[rec], f"{name} {key}")
        assert np.abs(fx[rec]).max() > 1e-3


@pytest.mark.parametrize("name", ggb.GCT_FIXTURES)
def test_gct_reference_reproduces_the_recorded_gradients(name):
    fx = load_golden(name)
    got = ggb.gct_chain(fx["in_x"], fx["w_alpha"], fx["w_gamma"], fx["w_beta"], float(fx["epsilon"]), str(fx["mode"]), bool(fx["after_relu"]), fx["in_weight"])
    for key, rec in (("out", "out"), ("grad_x", "grad_x"), ("grad_alpha", "grad_w_alpha"), ("grad_gamma", "grad_w_gamma"), ("grad_beta", "grad_w_beta")):
        _close(got[key], ggb.t64(fx[rec]).reshape(got[key].shape), f"{name} {key}")
        assert np.abs(fx[rec]).max() > 1e-3
    assert {str(fx["mode"]) for fx in map(load_golden, ggb.GCT_FIXTURES)} == {"l1", "l2"}


@pytest.mark.parametrize("name", ggb.BLOCK_FIXTURES)
def test_block_reference_reproduces_the_recorded_gradients(name):
    fx = load_golden(name)
    N, C, h, w = fx["in_x"].shape
    k = int(float(fx["beta"]) * w * h)
    w_ = lambda n: fx["w_" + n]
    p = dict(phi_w=w_("CL_1__phi_layer__weight").reshape(-1), phi_b=w_("CL_1__phi_layer__bias"), w1=w_("CL_1__mlp_layer__weight"), b1=w_("CL_1__mlp_layer__bias"),
             w2=w_("CL_2__mlp_layer__weight"), b2=w_("CL_2__mlp_layer__bias"), w3=w_("CL_3__mlp_layer__weight"), b3=w_("CL_3__mlp_layer__bias"),
             wm=w_("mlp_layer__weight"), bm=w_("mlp_layer__bias"))
    got = ggb.cond_block_chain(fx["in_x"], fx["in_head"], p, k, fx["in_weight"])
    pairs = [("out", "out"), ("grad_x", "grad_x"), ("grad_head", "grad_head"), ("grad_wm", "grad_w_mlp_layer__weight"), ("grad_bm", "grad_w_mlp_layer__bias")]
    pairs += [(f"grad_{t}{i}", f"grad_w_CL_{i}__mlp_layer__{n}") for i in (1, 2, 3) for t, n in (("w", "weight"), ("b", "bias"))]
    for key, rec in pairs:
        _close(got[key], fx[rec], f"{name} {key}")
    none = set(fx["none_grads"].tolist())
    assert {f"CL_{i}.phi_layer.{n}" for i in (1, 2, 3) for n in ("weight", "bias")} == none, "the reference's autograd gives phi_layer a gradient"
    if N == 1:
        assert np.abs(fx["grad_w_CL_2__mlp_layer__weight"]).max() == 0.0, "one sample: x_delta is zero and so is CL_2's weight gradient"
    # the float32 forward draws the same mask: the generator's separation, checked again on what was stored
    s, _, _, _, tol = ggb.cond_scores_ref(ggb.t64(fx["in_x"]).reshape(N, C, -1), ggb.t64(p["phi_w"]), ggb.t64(p["phi_b"]).reshape(()), k)
    top = torch.sort(s, dim=1, descending=True).values
    assert ((top[:, k - 1] - top[:, k]) >= 100 * tol.max()).all() and ((top[:, k - 2] - top[:, k - 1]) >= 100 * tol.max()).all()


def test_fixtures_are_small():
    import os
    from conftest import GOLDEN
    for name in ggb.IA_FIXTURES + ggb.GCT_FIXTURES + ggb.BLOCK_FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 100_000, name
    assert {load_golden(n)["in_x"].shape[0] for n in ggb.BLOCK_FIXTURES} == {1, 3}


# ------------------------------------------------------------------------------------------ every slip leaves its bound
def _leaves(want_tol, slipped, what):
    (want, tol), (bad, _) = want_tol, slipped
    assert (tol >= 0).all() and torch.isfinite(tol).all(), what
    assert (tol <= 1e-4 * max(float(want.abs().max()), 1e-30)).all() or float(want.abs().max()) == 0.0, f"{what}: not a float32 rounding bound"
    assert ((bad - want).abs() > tol).any(), f"{what}: the slipped reference stays inside the bound (bound too loose)"


def test_slips_leave_the_bounds():
    rs = ggb.rng(31)
    r = lambda *s: rs.standard_normal(s).astype(f32)
    gy, x, gain = r(6, 35), r(6, 35), (1 + np.tanh(r(6))).astype(f32)
    ref = ggb.channel_scale_grad_ref(gy, x, gain)
    _leaves(ref[0], ggb.channel_scale_grad_slip("prev_gain", gy, x, gain)[0], "channel_scale_grad grad_x")
    _leaves(ref[1], ggb.channel_scale_grad_slip("drop_last", gy, x, gain)[1], "channel_scale_grad dgain")

    dgain, g2, head, W = r(3, 5), (1 + np.tanh(r(3, 5))).astype(f32), r(3, 7), r(5, 7)
    ref = ggb.film_gain_grad_ref(dgain, g2, head, W)
    for kind in ("one_minus_t", "drop_last"):
        for k, name in enumerate(("grad_head", "grad_weight", "grad_bias")):
            _leaves(ref[k], ggb.film_gain_grad_ref(dgain, g2, head, W, kind)[k], f"film_gain_grad {name} {kind}")

    for l1 in (False, True):
        dgate, gate, s = r(3, 5), (1 + np.tanh(r(3, 5))).astype(f32), np.abs(r(3, 5)) * 30
        al, ga = rs.uniform(0.5, 1.5, 5).astype(f32), r(5)
        ref = ggb.gct_gate_grad_ref(dgate, gate, s, al, ga, 1e-5, l1)
        _leaves(ref[0], ggb.gct_gate_grad_ref(dgate, gate, s, al, ga, 1e-5, l1, "no_dM")[0], f"gct_gate_grad dsum no_dM l1={l1}")
        _leaves(ref[1], ggb.gct_gate_grad_ref(dgate, gate, s, al, ga, 1e-5, l1, "no_dM")[1], f"gct_gate_grad grad_alpha no_dM l1={l1}")
        for k, name in enumerate(("dsum", "grad_alpha", "grad_gamma", "grad_beta")):
            _leaves(ref[k], ggb.gct_gate_grad_ref(dgate, gate, s, al, ga, 1e-5, l1, "one_minus_t")[k], f"gct_gate_grad {name} one_minus_t l1={l1}")
            if k:
                _leaves(ref[k], ggb.gct_gate_grad_ref(dgate, gate, s, al, ga, 1e-5, l1, "drop_last")[k], f"gct_gate_grad {name} drop_last l1={l1}")
    for mode in (0, 1, 2):
        _leaves(ggb.gct_scale_grad_ref(gy, x, gain, r(6), mode), ggb.gct_scale_grad_ref(gy, x, gain, r(6) * 0 + 1, mode, True), f"gct_scale_grad mode {mode}")

    N, C, D = 3, 4, 6
    args = (r(N, 2 * C + D), r(N, C), r(N, C), r(N, D), r(C, C), r(C, C), r(D, D))
    ref = ggb.cond_codes_grad_ref(*args)
    minus, last = ggb.cond_codes_grad_ref(*args, "no_minus"), ggb.cond_codes_grad_ref(*args, "drop_last")
    _leaves(ref["dpx"], minus["dpx"], "cond_codes_grad dpx no_minus")
    _leaves(ref["grad_w2"], minus["grad_w2"], "cond_codes_grad grad_w2 no_minus")
    for name in ggb.CODE_OUTS:
        _leaves(ref[name], last[name], f"cond_codes_grad {name} drop_last")

    s = ggb.cond_case(3, 4, 6, 9, 11, 0.3, 13)
    sc, thr, _, _, _ = ggb.cond_forward64(torch.from_numpy(s["x"]).reshape(3, 4, -1), s["p"]["phi_w"], s["p"]["phi_b"], s["k_rank"])
    sc, thr = sc.float(), sc.float().topk(s["k_rank"], 1).values[:, -1]
    a = (s["grad_y"].reshape(3, 4, -1), gain[:3, None].repeat(4, 1), sc, thr, r(3, 4), r(3, 4))
    _leaves(ggb.cond_scale_grad_ref(*a), ggb.cond_scale_grad_ref(*a, slip=True), "cond_scale_grad >=")
    _leaves(ggb.cond_scale_grad_ref(None, None, *a[2:5], None), ggb.cond_scale_grad_ref(None, None, *a[2:5], None, slip=True), "cond_scale_grad layer >=")


def test_bounds_hold_for_a_float32_evaluation_in_another_order():
    """Sums of at most five terms: whatever order torch's float32 CPU kernels take is no deeper than the kernels' serial loops, so they must
    sit inside the same bounds (a bound that a correct float32 evaluation leaves is too tight)."""
    rs = ggb.rng(41)
    r = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(f32))
    gy, x, gain = r(6, 1023), r(6, 1023), 1 + torch.tanh(r(6))
    (gx, tx), _ = ggb.channel_scale_grad_ref(gy, x, gain)
    assert ggb.check(gy * gain[:, None], gx, tx, "grad_x") <= 1.0
    dgain, g2, head, W = r(3, 5), 1 + torch.tanh(r(3, 5)), r(3, 7), r(5, 7)
    da = dgain * (1 - (g2 - 1) * (g2 - 1))
    ref = ggb.film_gain_grad_ref(dgain, g2, head, W)
    for got, (want, tol) in zip((da @ W, da.t() @ head, da.sum(0)), ref):
        assert ggb.check(got, want, tol, "film_gain_grad") <= 1.0


# ------------------------------------------------------------------------------------------ the undecided pixels of the random cases
@pytest.mark.parametrize("case", [c for c in ggb.COND_CASES if c[-1] == "random"], ids=lambda c: "-".join(map(str, c)))
def test_random_cases_keep_their_undecided_pixels_under_the_cap(case):
    s = ggb.cond_case(*case)
    scores, thr, mask, near = ggb.mask_undecided(s["x"].reshape(case[0], case[1], -1), s["p"], s["k_rank"])
    assert float(near.double().mean(1).max()) <= ggb.MASK_CAP, f"{case}: {int(near.sum())} pixels within the score bound of the threshold: another seed"
    assert (mask.sum(1) == s["k_rank"] - 1).all()


# ------------------------------------------------------------------------------------------ the twins' surface
def test_state_dict_keys_equal_the_mirrors():
    from aoc_amd import attention, conditioning_layer as cl, gct
    pairs = ((gt.IA_gate(7, 5), attention.IA_gate(7, 5)), (gt.GCT(6), gct.GCT(6)), (gt.GCT(6, mode="l1", after_relu=True), gct.GCT(6, mode="l1", after_relu=True)),
             (gt.conditioning_layer(8, 0.5), cl.conditioning_layer(8, 0.5)), (gt.conditioning_block(8, 12, 0.3), cl.conditioning_block(8, 12, 0.3)),
             (gt.conditioning_block(8, attention_dim=20), cl.conditioning_block(8, attention_dim=20)))
    for twin, mirror in pairs:
        a, b = twin.state_dict(), mirror.state_dict()
        assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a), type(twin).__name__
        twin.load_state_dict(b)
        assert all(torch.equal(twin.state_dict()[k], b[k]) for k in b)
        assert inspect.signature(type(twin).__init__) == inspect.signature(type(mirror).__init__)
    g = gt.GCT(4)
    assert bool((g.alpha == 1).all()) and not bool(g.gamma.any()) and not bool(g.beta.any())
    assert "phi_layer" in gt.conditioning_layer.__doc__ and "None" in gt.conditioning_layer.__doc__
    assert "gates_train" in aoc_amd.__all__


def test_mirrors_point_to_the_twins():
    from aoc_amd import attention, conditioning_layer as cl, gct
    x, head = torch.randn(2, 4, 3, 3, requires_grad=True), torch.randn(2, 6)
    for what, call in (("IA_gate", lambda: attention.IA_gate(6, 4)(x, head)), ("GCT", lambda: gct.GCT(4)(x)),
                       ("conditioning_layer", lambda: cl.conditioning_layer(4)(x)), ("conditioning_block", lambda: cl.conditioning_block(4, 6)(x, head))):
        with pytest.raises(_lib.AocHipError, match=f"inference-only.*gates_train.{what} is the differentiable form"):
            call()


def test_no_gradient_path_goes_through_the_mirrors_ops(monkeypatch):
    seen = []
    for name in ("film_scale", "plane_reduce", "gct_gate", "channel_scale", "cond_gate_pool", "cond_codes", "linear"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: seen.append(_n) or (torch.zeros(2, 4), torch.zeros(2, 4)) if _n == "cond_gate_pool" and k.get("want_plane_mean")
                            else (seen.append(_n) or torch.zeros(2, 4)))
    x, head = torch.randn(2, 4, 3, 3), torch.randn(2, 6)
    frozen = lambda m: m.requires_grad_(False)                      # nothing wants a gradient: inputs without one, parameters frozen
    frozen(gt.IA_gate(6, 4))(x, head)
    frozen(gt.GCT(4))(x)
    frozen(gt.GCT(4, mode="l1"))(x)
    frozen(gt.conditioning_layer(4))(x)
    frozen(gt.conditioning_layer(4))(torch.randn(2, 4))
    frozen(gt.conditioning_block(4, 6))(x, head)
    with torch.no_grad():                                           # autograd off: the same, whatever requires_grad says
        gt.IA_gate(6, 4)(x.clone().requires_grad_(True), head)
    assert seen == ["film_scale", "plane_reduce", "gct_gate", "channel_scale", "plane_reduce", "gct_gate", "channel_scale", "cond_gate_pool", "linear",
                    "linear", "cond_gate_pool", "cond_codes", "film_scale", "film_scale"]


def test_guards():
    x, head = torch.randn(2, 4, 3, 3, requires_grad=True), torch.randn(2, 6)
    for call in (lambda: gt.IA_gate(6, 4)(x, head), lambda: gt.GCT(4)(x), lambda: gt.conditioning_layer(4)(x), lambda: gt.conditioning_block(4, 6)(x, head)):
        with pytest.raises(_lib.AocHipError, match="no CPU fallback"):
            call()
    with pytest.raises(IndexError, match="beta_rank"):
        gt.conditioning_layer(4)(torch.randn(2, 4, 1, 2, requires_grad=True))
    with pytest.raises(IndexError, match="beta_rank"):
        gt.conditioning_block(4, 6)(torch.randn(2, 4, 1, 2, requires_grad=True), head)
    with pytest.raises(ValueError, match="Unknown mode"):
        gt.GCT(4, mode="l3")(x)


# ------------------------------------------------------------------------------------------ the tensor contract, library stubbed
def _t(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(f32))


def _cases():
    N, C, D, H, W = 3, 4, 6, 3, 5
    F, OUT = occ.F, occ.OUT

    def mk(builder):
        return lambda ops_, device: {k: v.to(device) for k, v in builder(np.random.RandomState(7)).items()}
    z = torch.zeros
    code_out = dict(dgap=(N, C), dpx=(N, C), grad_head=(N, D), grad_w1=(C, C), grad_b1=(C,), grad_w2=(C, C), grad_b2=(C,), grad_w3=(D, D), grad_b3=(D,))
    return [
        occ.Case("channel_scale_backward", [], mk(lambda rs: dict(grad_y=_t(rs, N, C, H, W), x=_t(rs, N, C, H, W), gain=_t(rs, N, C), grad_x=z(N, C, H, W),
                                                                  dgain=z(N, C))),
                 {"grad_y": F, "x": F, "gain": F, "grad_x": OUT, "dgain": OUT},
                 lambda ops_, a: gt.channel_scale_backward(a["grad_y"], a["x"], a["gain"], a["grad_x"], a["dgain"]), None),
        occ.Case("film_gain_backward", [], mk(lambda rs: dict(dgain=_t(rs, N, C), gain=_t(rs, N, C), head=_t(rs, N, D), weight=_t(rs, C, D), grad_head=z(N, D),
                                                              grad_weight=z(C, D), grad_bias=z(C))),
                 {"dgain": F, "gain": F, "head": F, "weight": F, "grad_head": OUT, "grad_weight": OUT, "grad_bias": OUT},
                 lambda ops_, a: gt.film_gain_backward(a["dgain"], a["gain"], a["head"], a["weight"], a["grad_head"], a["grad_weight"], a["grad_bias"]), None),
        occ.Case("gct_gate_backward", [], mk(lambda rs: dict(dgate=_t(rs, N, C), gate=_t(rs, N, C), sums=_t(rs, N, C), alpha=_t(rs, 1, C, 1, 1),
                                                             gamma=_t(rs, 1, C, 1, 1), beta=_t(rs, 1, C, 1, 1), dsum=z(N, C), grad_alpha=z(C), grad_gamma=z(C),
                                                             grad_beta=z(C))),
                 {"dgate": F, "gate": F, "sums": F, "alpha": F, "gamma": F, "beta": F, "dsum": OUT, "grad_alpha": OUT, "grad_gamma": OUT, "grad_beta": OUT},
                 lambda ops_, a: gt.gct_gate_backward(a["dgate"], a["gate"], a["sums"], a["alpha"], a["gamma"], a["beta"], 1e-5, False, a["dsum"], a["grad_alpha"],
                                                      a["grad_gamma"], a["grad_beta"]), None),
        occ.Case("gct_scale_backward", [], mk(lambda rs: dict(grad_y=_t(rs, N, C, H, W), x=_t(rs, N, C, H, W), gate=_t(rs, N, C), dsum=_t(rs, N, C),
                                                              grad_x=z(N, C, H, W))),
                 {"grad_y": F, "x": F, "gate": F, "dsum": F, "grad_x": OUT},
                 lambda ops_, a: gt.gct_scale_backward(a["grad_y"], a["x"], a["gate"], a["dsum"], 1, a["grad_x"]), None),
        occ.Case("cond_codes_backward", [], mk(lambda rs: dict(dcode=_t(rs, N, 2 * C + D), gap=_t(rs, N, C), px=_t(rs, N, C), head=_t(rs, N, D), w1=_t(rs, C, C),
                                                               w2=_t(rs, C, C), w3=_t(rs, D, D), **{k: z(*s) for k, s in code_out.items()})),
                 dict({k: F for k in ("dcode", "gap", "px", "head", "w1", "w2", "w3")}, **{k: OUT for k in code_out}),
                 lambda ops_, a: gt.cond_codes_backward(a["dcode"], a["gap"], a["px"], a["head"], a["w1"], a["w2"], a["w3"], out={k: a[k] for k in code_out}), None),
        occ.Case("cond_scale_backward", [], mk(lambda rs: dict(grad_y=_t(rs, N, C, H, W), gain=_t(rs, N, C), scores=_t(rs, N, H * W), thr=_t(rs, N),
                                                               dgap=_t(rs, N, C), dpx=_t(rs, N, C), grad_x=z(N, C, H, W))),
                 {"grad_y": F, "gain": F, "scores": F, "thr": F, "dgap": F, "dpx": F, "grad_x": OUT},
                 lambda ops_, a: gt.cond_scale_backward(a["grad_y"], a["gain"], a["scores"], a["thr"], a["dgap"], a["dpx"], grad_x=a["grad_x"]), None),
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


def test_wrappers_take_addresses_only_through_the_helpers():
    src = inspect.getsource(gt)
    assert "data_ptr" not in src and "import ctypes" not in src
    import ast
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ("_p", "_addr"):
            assert not any(isinstance(sub, ast.Call) for arg in node.args for sub in ast.walk(arg)), f"line {node.lineno}: a call expression inside _p(...)"
    public = {n for n, v in vars(ops).items() if callable(v) and not n.startswith("_") and getattr(v, "__module__", None) == ops.__name__}
    assert not {"channel_scale_backward", "film_gain_backward", "gct_gate_backward", "gct_scale_backward", "cond_codes_backward", "cond_scale_backward"} & public


# ------------------------------------------------------------------------------------------ the C entry points before any launch
def test_entries_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(256)                         # never dereferenced: every call here returns before a launch

    def cs(gy=p, x=p, gain=p, planes=6, hw=35, gx=p, dg=p):
        return L.aoc_channel_scale_grad(gy, x, gain, planes, hw, gx, dg, None)
    assert cs(gy=None) == INVALID and cs(planes=0) == INVALID and cs(hw=0) == INVALID and cs(gain=None) == INVALID and cs(x=None) == INVALID
    assert cs(gx=None, dg=None) == OK and cs(planes=1 << 31) == UNSUPPORTED

    def fg(dg=p, g=p, head=p, w=p, O=3, D=7, c=5, gh=p, gw=p, gb=p):
        return L.aoc_film_gain_grad(dg, g, head, w, O, D, c, gh, gw, gb, None)
    assert fg(dg=None) == INVALID and fg(g=None) == INVALID and fg(O=0) == INVALID and fg(D=0) == INVALID and fg(c=0) == INVALID
    assert fg(w=None) == INVALID and fg(head=None) == INVALID and fg(O=31) == UNSUPPORTED and fg(c=65533) == UNSUPPORTED and fg(gh=None, gw=None, gb=None) == OK

    def gg(dg=p, g=p, s=p, al=p, ga=p, N=3, C=5, ds=p):
        return L.aoc_gct_gate_grad(dg, g, s, al, ga, None, N, C, 1e-5, 0, ds, p, p, p, None)
    assert gg(dg=None) == INVALID and gg(g=None) == INVALID and gg(s=None) == INVALID and gg(al=None) == INVALID and gg(ga=None) == INVALID
    assert gg(N=0) == INVALID and gg(C=0) == INVALID and gg(N=31) == UNSUPPORTED

    def gs(gy=p, x=p, g=p, ds=p, mode=1, planes=6, hw=35, gx=p):
        return L.aoc_gct_scale_grad(gy, x, g, ds, mode, planes, hw, gx, None)
    for k in ("gy", "x", "g", "ds", "gx"):
        assert gs(**{k: None}) == INVALID, k
    assert gs(mode=3) == INVALID and gs(mode=-1) == INVALID and gs(planes=0) == INVALID and gs(hw=0) == INVALID and gs(planes=1 << 31) == UNSUPPORTED

    def cc(dc=p, gap=p, px=p, head=p, w1=p, w2=p, w3=p, N=3, C=4, D=6):
        return L.aoc_cond_codes_grad(dc, gap, px, head, w1, w2, w3, N, C, D, p, p, p, p, p, p, p, p, p, None)
    for k in ("dc", "gap", "px", "head", "w1", "w2", "w3"):
        assert cc(**{k: None}) == INVALID, k
    assert cc(N=0) == INVALID and cc(C=-1) == INVALID and cc(C=0, D=0) == INVALID and cc(N=31) == UNSUPPORTED and cc(C=32765) == UNSUPPORTED
    assert L.aoc_cond_codes_grad(p, None, None, None, None, None, None, 3, 4, 6, None, None, None, None, None, None, None, None, None, None) == OK

    def sc(gy=p, gain=p, s=p, thr=p, N=3, C=4, hw=35, gx=p):
        return L.aoc_cond_scale_grad(gy, gain, s, thr, p, p, N, C, hw, gx, None)
    assert sc(s=None) == INVALID and sc(thr=None) == INVALID and sc(gx=None) == INVALID and sc(gain=None) == INVALID
    assert sc(N=0) == INVALID and sc(C=0) == INVALID and sc(hw=0) == INVALID and sc(N=31) == UNSUPPORTED and sc(N=30, C=1 << 27) == UNSUPPORTED
