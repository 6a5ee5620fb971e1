"""What can be checked without a GPU about the differentiable decoder forms (aoc_amd.decoder_train, csrc/norm_grad.hip): the float64
references of tests/decoder_grad_bounds.py against torch's float64 autograd of ``gain * relu(F.group_norm(x, G, gamma, beta, eps) + residual)``
and of the gated concatenation, and against the gradients recorded from the reference's own Bottleneck + IA_gate
(tests/golden/decoder_grad_*.npz); that every slipped reference leaves its bound; that no element of a GPU case is undecided; the twins'
surface; the two wrappers against the address / lifetime / dtype contract of aoc_amd.ops with the library stubbed; the argument checks of the
new entry points."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import aoc_amd
import decoder_grad_bounds as dgb
import ops_contract_cases as occ
from aoc_amd import _lib, decoder_memory, decoder_train as dt, gates_train, gct, ops
from conftest import GOLDEN, load_golden

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4
f32, f64 = np.float32, np.float64
ERRORS = occ.ERRORS + (_lib.AocHipError,)
REL = 1e-12


def _close(got, want, what, rel=REL, scale=0.0):
    """scale: the size of the terms that cancel in `want`, where the result is what they leave behind"""
    got, want = dgb.t64(got), dgb.t64(want)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} against {tuple(want.shape)}"
    assert (got - want).abs().max() <= rel * max(float(want.abs().max()), scale, 1e-30), f"{what}: off by {float((got - want).abs().max()):.3e}"


def _leaf(a):
    return torch.from_numpy(np.asarray(a, f64)).requires_grad_(True) if a is not None else None


# ------------------------------------------------------------------------------------------ the references against float64 autograd
@pytest.mark.parametrize("variant", dgb.GN_VARIANTS + ((True, True, False, True), (False, True, True, False)))
@pytest.mark.parametrize("N,C,groups,hw", ((2, 4, 4, 1), (2, 6, 3, 5), (3, 8, 2, 35), (2, 8, 1, 12)))      # 2, 4, 4, 1: one element per group
def test_groupnorm_reference_against_autograd(N, C, groups, hw, variant):
    res, relu, gain, affine = variant
    rs = dgb.rng(N, C, groups, hw, 3)
    n = rs.standard_normal
    x, r, gy, w, b, g = n((N, C, hw)), n((N, C, hw)), n((N, C, hw)), 1 + 0.5 * n(C), n(C), 1 + np.tanh(n((N, C)))
    lx, lr, lw, lb, lg = _leaf(x), _leaf(r if res else None), _leaf(w if affine else None), _leaf(b if affine else None), _leaf(g if gain else None)
    out = dgb.forward64(lx, lr, groups, lw, lb, 1e-5, relu, lg)
    (out * torch.from_numpy(gy)).sum().backward()
    got, _ = dgb.groupnorm_relu_grad_ref(gy, x, r if res else None, groups, w if affine else None, b if affine else None, 1e-5, relu, g if gain else None)
    # grad_x is what rstd gamma dz and the two group means leave of one another (exactly nothing for a group of one element)
    rstd = 1.0 / np.sqrt(x.reshape(N, groups, -1).var(2) + 1e-5)
    _close(got["grad_x"][0], lx.grad, "grad_x", scale=float(rstd.max() * np.abs(w if affine else 1.0).max() * got["grad_residual"][0].abs().max()))
    if res:
        _close(got["grad_residual"][0], lr.grad, "grad_residual")
    if affine:
        # xhat is what x and the mean leave of one another, times rstd
        _close(got["grad_gamma"][0], lw.grad, "grad_gamma", scale=float(rstd.max() * np.abs(x).max() * got["grad_residual"][0].abs().sum((0, 2)).max()))
        _close(got["grad_beta"][0], lb.grad, "grad_beta")
    if gain:
        _close(got["dgain"][0], lg.grad, "dgain")


@pytest.mark.parametrize("O,Cx,Cm,hw", ((1, 1, 0, 1), (2, 3, 5, 7), (3, 4, 4, 9)))
def test_cat_film_scale_reference_against_autograd(O, Cx, Cm, hw):
    rs = dgb.rng(O, Cx, Cm, hw, 4)
    n = rs.standard_normal
    D = 6
    x, mem, gy, head, W, b = n((O, Cx, hw)), (n((O, Cm, hw)) if Cm else None), n((O, Cx + Cm, hw)), n((O, D)), n((Cx + Cm, D)) / np.sqrt(D), n(Cx + Cm)
    lx, lm, lh, lw, lb = _leaf(x), _leaf(mem), _leaf(head), _leaf(W), _leaf(b)
    gain = 1.0 + torch.tanh(torch.nn.functional.linear(lh, lw, lb))
    out = torch.cat([lx, lm], 1) * gain[:, :, None] if Cm else lx * gain[:, :, None]                   # decoding_module.py:193-194, ATT:12-17
    (out * torch.from_numpy(gy)).sum().backward()
    got = dgb.cat_film_scale_grad_ref(gy, x, mem, gain.detach())
    _close(got["grad_x"][0], lx.grad, "grad_x")
    if Cm:
        _close(got["grad_mem"][0], lm.grad, "grad_mem")
    (gh, _), (gw, _), (gb, _) = dgb.film_gain_grad_ref(got["dgain"][0], gain.detach(), head, W)         # dgain through the existing gate backward
    _close(gh, lh.grad, "grad_head")
    _close(gw, lw.grad, "grad_weight")
    _close(gb, lb.grad, "grad_bias")


# ------------------------------------------------------------------------------------------ the references against the recorded gradients
@pytest.mark.parametrize("name", dgb.BOTTLENECK_FIXTURES)
def test_reference_reproduces_the_recorded_gradients(name):
    """The reference's own Bottleneck + IA_gate (gct.py:38-91, ATT:7-17) in float64, recorded by tests/golden/make_golden_decoder_grad.py, against
    the same chain with every normalisation differentiated by groupnorm_relu_grad_ref."""
    z = load_golden(name)
    inplanes, outplanes = (int(v) for v in z["planes"])
    D = z["in_head"].shape[1]
    blk, gate = dt.Bottleneck(inplanes, outplanes).double(), torch.nn.Linear(D, outplanes).double()
    holder = torch.nn.Module()
    holder.IA = gate
    dgb.set_conv_weights(blk, int(z["seed"]))
    named = dict([("blk." + k, p) for k, p in blk.named_parameters()] + [("gate.IA." + k, p) for k, p in gate.named_parameters()])
    stored = {k[2:].replace("__", "."): v for k, v in z.items() if k.startswith("w_")}
    assert set(stored) == {k for k in named if "conv" not in k and not k.startswith("blk.downsample.0")}
    for k, v in stored.items():
        dgb._fill(named[k], v.astype(f64))
    x, head = _leaf(z["in_x"]), _leaf(z["in_head"])
    out = dgb.bottleneck_chain64(blk, holder, x, head)
    loss = (out * torch.from_numpy(z["in_weight"].astype(f64))).sum()
    loss.backward()
    rel = 1e-9                                  # nn.GroupNorm's eps is the double 1e-5, the kernels' (and the references') the float 1e-5: 4e-13 of var + eps
    assert abs(loss.item() - float(z["loss"])) <= rel * abs(float(z["loss"]))
    _close(x.grad, z["grad_x"], "grad_x", rel)
    _close(head.grad, z["grad_head"], "grad_head", rel)
    for k in stored:
        _close(named[k].grad, z["grad_w_" + k.replace(".", "__")], k, rel)


def test_fixtures_are_small():
    for name in dgb.BOTTLENECK_FIXTURES:
        size = os.path.getsize(os.path.join(GOLDEN, name + ".npz"))
        assert size < 250_000, f"{name}: {size} bytes"
        z = load_golden(name)
        assert not any("conv" in k for k in z) and "out" not in z, "gradients of x, the head and the small parameters only"


# ------------------------------------------------------------------------------------------ the bounds
SMALL = ((2, 64, 32, 35), (3, 8, 2, 257), (2, 8, 1, 8209), (30, 32, 32, 9))


@pytest.mark.parametrize("N,C,groups,hw", SMALL)
def test_groupnorm_slips_leave_the_bounds(N, C, groups, hw):
    s = dgb.gn_case(N, C, groups, hw)
    seen = set()
    for variant in dgb.GN_VARIANTS:
        args = dgb.gn_args(s, variant, groups)
        ref, _ = dgb.groupnorm_relu_grad_ref(**args)
        for slip in dgb.gn_slips(variant, C, groups):
            bad, _ = dgb.groupnorm_relu_grad_ref(slip=slip, **args)
            left = [k for k in dgb.GN_OUTS if bool(((bad[k][0] - ref[k][0]).abs() > ref[k][1]).any())]
            assert left, f"{variant} {slip}: the slipped reference stays inside every bound"
            if slip in ("s2_no_gamma", "mean_hw"):
                assert "grad_x" in left
            seen.add(slip)
    assert seen == set(dgb.GN_SLIPS) or C == groups


def test_cat_slips_leave_the_bounds():
    for case in dgb.CAT_CASES[1:]:
        s = dgb.cat_case(*case)
        ref = dgb.cat_film_scale_grad_ref(s["grad_y"], s["x"], s["mem"], s["gain"])
        bad = dgb.cat_film_scale_grad_ref(s["grad_y"], s["x"], s["mem"], s["gain"], "next_gain")
        assert bool(((bad["grad_x"][0] - ref["grad_x"][0]).abs() > ref["grad_x"][1]).any())
        bad = dgb.cat_film_scale_grad_ref(s["grad_y"], s["x"], s["mem"], s["gain"], "drop_last")
        assert bool(((bad["dgain"][0] - ref["dgain"][0]).abs() > ref["dgain"][1]).any())


def test_bounds_hold_for_a_float32_evaluation_in_another_order():
    """numpy's float32 evaluation of the same mathematics (pairwise sums, its own statistics) stays inside the bounds"""
    N, C, groups, hw = 3, 8, 2, 257
    s = dgb.gn_case(N, C, groups, hw)
    ref, und = dgb.groupnorm_relu_grad_ref(**dgb.gn_args(s, (True, True, True, True), groups))
    assert int(und.sum()) == 0
    x, r, gy, w, b, g = (s[k].astype(f32) for k in ("x", "residual", "grad_y", "weight", "bias", "gain"))
    gc = C // groups
    xg = x.reshape(N, groups, -1)
    mean = np.repeat(xg.mean(2, dtype=f64).astype(f32), gc, 1)[:, :, None]
    rstd = np.repeat((1.0 / np.sqrt(xg.var(2, dtype=f64) + dgb.eps32(1e-5))).astype(f32), gc, 1)[:, :, None]
    a = rstd * w[None, :, None]
    z = x * a + (b[None, :, None] - mean * a) + r
    dz = np.where(z > 0, g[:, :, None] * gy, f32(0))
    xhat = (x - mean) * rstd
    A, B = dz.sum(2), (dz * xhat).sum(2)
    M = f32(gc * hw)
    c1 = np.repeat((w[None] * A).reshape(N, groups, gc).sum(2) / M, gc, 1)[:, :, None]
    c2 = np.repeat((w[None] * B).reshape(N, groups, gc).sum(2) / M, gc, 1)[:, :, None]
    got = {"grad_x": rstd * ((w[None, :, None] * dz - c1) - xhat * c2), "grad_residual": dz, "grad_gamma": B.sum(0), "grad_beta": A.sum(0),
           "dgain": (gy * np.maximum(z, 0)).sum(2)}
    for k in dgb.GN_OUTS:
        assert got[k].dtype == f32
        assert dgb.check(got[k], *ref[k], k) <= 1.0, k


@pytest.mark.parametrize("case", tuple(dgb.GN_CASES))
def test_gpu_cases_have_no_undecided_element(case):
    N, C, groups, hw = case
    s = dgb.gn_case(N, C, groups, hw)
    for variant in dgb.GN_VARIANTS:
        _, und = dgb.groupnorm_relu_grad_ref(**dgb.gn_args(s, variant, groups))
        assert int(und.sum()) == 0, f"{case} {variant}: {int(und.sum())} elements within the float32 bound of z = 0"
        assert int(und.sum()) <= dgb.MASK_CAP * und.numel()


def test_an_undecided_element_widens_its_bound():
    s = dgb.gn_case(2, 64, 32, 35)
    args = dgb.gn_args(s, (True, True, False, True), 32)
    ref, _ = dgb.groupnorm_relu_grad_ref(**args)
    z = dgb.forward64(dgb.t64(s["x"]), None, 32, dgb.t64(s["weight"]), dgb.t64(s["bias"]), 1e-5, False)
    args["residual"] = s["residual"].copy()
    args["residual"][1, 5, 7] = f32(-float(z[1, 5, 7]))                      # z + residual within a rounding of 0
    ref2, und = dgb.groupnorm_relu_grad_ref(**args)
    assert bool(und[1, 5, 7]) and int(und.sum()) == 1
    assert ref2["grad_residual"][1][1, 5, 7] >= abs(float(s["grad_y"][1, 5, 7])) and ref2["grad_beta"][1][5] > ref["grad_beta"][1][5]


# ------------------------------------------------------------------------------------------ the twins' surface
def test_state_dict_keys_equal_the_mirrors():
    for args in ((64, 128), (128, 128), (64, 128, 2, 3)):
        twin, mirror = dt.Bottleneck(*args), gct.Bottleneck(*args)
        a, b = twin.state_dict(), mirror.state_dict()
        assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
        twin.load_state_dict(b)
        assert all(torch.equal(twin.state_dict()[k], b[k]) for k in b)
        assert inspect.signature(dt.Bottleneck.__init__) == inspect.signature(gct.Bottleneck.__init__)
        assert inspect.signature(dt.Bottleneck.forward) == inspect.signature(gct.Bottleneck.forward)
        assert isinstance(twin.GCT1, gates_train.GCT) and (twin.downsample is None) == (mirror.downsample is None)
    for f in ("Modulator_1", "Modulator_2", "modulate"):
        assert inspect.signature(getattr(dt, f)) == inspect.signature(getattr(decoder_memory, f))
    assert "decoder_train" in aoc_amd.__all__


def test_mirrors_point_to_the_twins():
    x = torch.randn(2, 128, 3, 3, requires_grad=True)
    with pytest.raises(_lib.AocHipError, match="inference-only.*decoder_train.Bottleneck is the differentiable form"):
        gct.Bottleneck(128, 128)(x)
    dec = torch.nn.Module()
    for i in (1, 2, 3):
        setattr(dec, f"M1_Reweight_Layer_{i}", aoc_amd.attention.IA_gate(6, 256 if i == 1 else 128))
        setattr(dec, f"M2_Reweight_Layer_{i}", aoc_amd.attention.IA_gate(6, 256 if i == 1 else 128))
        setattr(dec, f"M1_Bottleneck_{i}", gct.Bottleneck(256 if i == 1 else 128, 128))
        setattr(dec, f"M2_Bottleneck_{i}", gct.Bottleneck(256 if i == 1 else 128, 128))
    head = torch.randn(2, 6)
    for k in (1, 2):
        with pytest.raises(_lib.AocHipError, match=f"inference-only.*decoder_train.Modulator_{k} is the differentiable form"):
            getattr(decoder_memory, f"Modulator_{k}")(dec, x, x.detach(), head)


def test_no_gradient_path_goes_through_the_mirrors_ops(monkeypatch):
    seen = []
    for name in ("groupnorm_relu", "groupnorm_relu_scale", "cat_film_scale", "film_scale"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: seen.append(_n) or torch.zeros(2, 4))
    x, head, w, b, gm = torch.randn(2, 4, 3, 3), torch.randn(2, 6), torch.randn(4, 6), torch.randn(4), torch.ones(4)
    dt.groupnorm_relu(x, 2, gm, gm)
    dt.groupnorm_relu(x, 2, gm, gm, gate=(head, w, b))
    dt.cat_film_scale(x[:, :2], x[:, 2:], head, w, b)
    dt.film_scale(x, head, w, b)
    with torch.no_grad():                                           # autograd off: the same, whatever requires_grad says
        dt.groupnorm_relu(x.clone().requires_grad_(True), 2, gm, gm)
    assert seen == ["groupnorm_relu", "groupnorm_relu_scale", "cat_film_scale", "film_scale", "groupnorm_relu"]


def test_guards():
    x = torch.randn(2, 4, 3, 3, requires_grad=True)
    head, w, b, gm = torch.randn(2, 6), torch.randn(4, 6), torch.randn(4), torch.ones(4)
    for call in (lambda: dt.groupnorm_relu(x, 2, gm, gm), lambda: dt.groupnorm_relu(x, 2, gm, gm, gate=(head, w, b)),
                 lambda: dt.cat_film_scale(x[:, :2], x[:, 2:].detach(), head, w, b), lambda: dt.film_scale(x, head, w, b)):
        with pytest.raises(_lib.AocHipError, match="no CPU fallback"):
            call()


# ------------------------------------------------------------------------------------------ the tensor contract, library stubbed
def _t(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(f32))


def _cases():
    N, C, G, H, W, Cm = 3, 4, 2, 3, 5, 2
    F, OUT = occ.F, occ.OUT

    def mk(builder):
        return lambda ops_, device: {k: v.to(device) for k, v in builder(np.random.RandomState(7)).items()}
    z = torch.zeros
    gn_out = dict(grad_x=(N, C, H, W), grad_residual=(N, C, H, W), grad_gamma=(C,), grad_beta=(C,), dgain=(N, C))
    return [
        occ.Case("groupnorm_relu_backward", [], mk(lambda rs: dict(grad_y=_t(rs, N, C, H, W), x=_t(rs, N, C, H, W), stats=_t(rs, N * G, 2), gamma=_t(rs, C),
                                                                   beta=_t(rs, C), residual=_t(rs, N, C, H, W), gain=_t(rs, N, C),
                                                                   **{k: z(*s) for k, s in gn_out.items()})),
                 dict({k: F for k in ("grad_y", "x", "stats", "gamma", "beta", "residual", "gain")}, **{k: OUT for k in gn_out}),
                 lambda ops_, a: dt.groupnorm_relu_backward(a["grad_y"], a["x"], a["stats"], G, a["gamma"], a["beta"], a["residual"], True, a["gain"],
                                                            out={k: a[k] for k in gn_out}), None),
        occ.Case("groupnorm_relu_forward", [], mk(lambda rs: dict(x=_t(rs, N, C, H, W), gamma=_t(rs, C), beta=_t(rs, C), residual=_t(rs, N, C, H, W),
                                                                  head=_t(rs, N, 6), weight=_t(rs, C, 6), bias=_t(rs, C))),
                 {k: F for k in ("x", "gamma", "beta", "residual", "head", "weight", "bias")},
                 lambda ops_, a: dt.groupnorm_relu_forward(a["x"], G, a["gamma"], a["beta"], 1e-5, a["residual"], True, (a["head"], a["weight"], a["bias"])), None),
        occ.Case("cat_film_scale_backward", [], mk(lambda rs: dict(grad_y=_t(rs, N, C + Cm, H, W), x=_t(rs, N, C, H, W), mem=_t(rs, N, Cm, H, W),
                                                                   gain=_t(rs, N, C + Cm), grad_x=z(N, C, H, W), grad_mem=z(N, Cm, H, W), dgain=z(N, C + Cm))),
                 {"grad_y": F, "x": F, "mem": F, "gain": F, "grad_x": OUT, "grad_mem": OUT, "dgain": OUT},
                 lambda ops_, a: dt.cat_film_scale_backward(a["grad_y"], a["x"], a["mem"], a["gain"], a["grad_x"], a["grad_mem"], a["dgain"]), None),
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
    src = inspect.getsource(dt)
    assert "data_ptr" not in src and "import ctypes" not in src
    import ast
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ("_p", "_addr"):
            assert not any(isinstance(sub, ast.Call) for arg in node.args for sub in ast.walk(arg)), f"line {node.lineno}: a call expression inside _p(...)"
    public = {n for n, v in vars(ops).items() if callable(v) and not n.startswith("_") and getattr(v, "__module__", None) == ops.__name__}
    assert not {"groupnorm_relu_backward", "groupnorm_relu_forward", "cat_film_scale_backward"} & public


# ------------------------------------------------------------------------------------------ the C entry points before any launch
def test_entries_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(256)                         # never dereferenced: every call here returns before a launch

    def gn(gy=p, x=p, st=p, N=2, C=64, hw=35, groups=32, gx=p, gr=p, gg=p, gb=p, dg=p, ws=p, nbytes=1 << 20):
        return L.aoc_groupnorm_relu_grad(gy, x, p, st, p, p, p, N, C, hw, groups, 1, gx, gr, gg, gb, dg, ws, nbytes, None)
    assert gn(gy=None) == INVALID and gn(x=None) == INVALID and gn(st=None) == INVALID and gn(N=0) == INVALID and gn(C=0) == INVALID
    assert gn(hw=0) == INVALID and gn(groups=0) == INVALID and gn(groups=5) == INVALID and gn(N=31) == UNSUPPORTED
    need = L.aoc_groupnorm_relu_grad_workspace_bytes(2, 64, 32)
    assert need >= (2 * 2 * 64 + 2 * 2 * 32) * 4 and gn(nbytes=need - 1) == WORKSPACE and gn(ws=None) == WORKSPACE
    assert gn(gx=None, gr=None, gg=None, gb=None, dg=None, ws=None, nbytes=0) == OK
    assert L.aoc_groupnorm_relu_grad_workspace_bytes(2, 64, 5) == 0 and L.aoc_groupnorm_relu_grad_workspace_bytes(0, 64, 32) == 0

    def cf(gy=p, x=p, mem=p, gain=p, O=3, Cx=4, Cm=2, hw=35, gx=p, gm=p, dg=p):
        return L.aoc_cat_film_scale_grad(gy, x, mem, gain, O, Cx, Cm, hw, gx, gm, dg, None)
    assert cf(gy=None) == INVALID and cf(O=0) == INVALID and cf(Cx=0) == INVALID and cf(Cm=-1) == INVALID and cf(hw=0) == INVALID
    assert cf(gain=None) == INVALID and cf(x=None) == INVALID and cf(mem=None) == INVALID and cf(Cm=0, mem=None) == INVALID      # grad_mem without a memory
    assert cf(O=31) == UNSUPPORTED and cf(gx=None, gm=None, dg=None) == OK
