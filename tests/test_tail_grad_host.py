"""What can be checked without a GPU about the differentiable decoder tail (aoc_amd.tail_train, csrc/tail_grad.hip): the float64 references of
tests/tail_grad_bounds.py against the adjoint identity, against torch's float64 autograd of the reference's lines written in plain torch and
against gradients recorded from the reference's own decoder_final, IA_logit and augment_background_logit; that every slipped twin leaves its
bound; that the random GPU cases have a decided background minimum at every pixel; the planted ties; the twins' surface, the wrappers' tensor
contract with the library stubbed, and every rejection code of the new entry points (no device is needed for a rejection)."""
import ast
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import aoc_amd
import ops_contract_cases as occ
import tail_grad_bounds as tgb
from aoc_amd import _lib, decoder_tail, gates_train, ops, tail_train as tt

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERRORS = occ.ERRORS + (_lib.AocHipError,)
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4
ALL_GEOMETRIES = tgb.STAGE_GEOMETRIES + (tgb.MAP_GEOMETRY,)


def close(got, want, what, rel=1e-12):
    got, want = tgb.t64(got), tgb.t64(want)
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= rel * scale, f"{what}: {err:.3e} against a largest value of {scale:.3e}"


# ------------------------------------------------------------------------------------------ 1 the adjoint identity
@pytest.mark.parametrize("geo", ALL_GEOMETRIES, ids=str)
def test_adjoint_dot_identity(geo):
    N, Ce, Cr, h, w, H, W = geo
    rs = tgb.rng(*geo, 1)
    x, g = torch.from_numpy(rs.standard_normal((2, h, w))), torch.from_numpy(rs.standard_normal((2, H, W)))
    lhs = float((tgb.upsample64(x, H, W) * g).sum())
    rhs = float((x * tgb.adjoint_ref(g, h, w)[0]).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), float((tgb.upsample64(x, H, W).abs() * g.abs()).sum())), (lhs, rhs)
    if (h, w) == (H, W):
        assert torch.equal(tgb.adjoint_ref(g, h, w)[0], g), "the identity geometry: t is grad_out"


# ------------------------------------------------------------------------------------------ 2 the references against float64 autograd
def _ia_gate(x, head, weight, bias):                                      # ATT:12-17
    return x * (1.0 + torch.tanh(F.linear(head, weight, bias)))[:, :, None, None]


def _delta(x):                                                            # decoding_module.py:172-174
    px1 = F.avg_pool2d(x, kernel_size=(x.size()[-2], x.size()[-1]), padding=0)
    return (torch.sum(px1, dim=0, keepdim=True) - px1).squeeze(-1).squeeze(-1)


def torch_shortcut_stage(x, low, head, weight, bias):                     # :163, :170-176
    up = F.interpolate(x, size=low.size()[2:], mode='bicubic', align_corners=True)
    cat = torch.cat([up, low], dim=1)
    return _ia_gate(cat, torch.cat([head, _delta(cat)], dim=1), weight, bias)


def torch_delta_gate(x, head, weight, bias):                              # :181-185
    return _ia_gate(x, torch.cat([head, _delta(x)], dim=1), weight, bias)


def torch_predict(x, head, fg_w, fg_b, bg_w, bg_b):                       # :144-160, 213-225
    n, c, h, w = x.size()

    def ia_logit(wt, b):
        out = F.linear(head, wt, b)
        return F.conv2d(x.reshape(1, n * c, h, w), weight=out[:, :c].reshape(n, c, 1, 1), bias=out[:, -1].reshape(-1), groups=n).view(n, 1, h, w)
    return torch_merge(ia_logit(fg_w, fg_b), ia_logit(bg_w, bg_b))


def torch_merge(fg, bg):
    pred = fg
    if fg.size(0) > 1:
        aug, _ = torch.min(bg[1:], dim=0, keepdim=True)
        pred = pred + torch.cat([aug, torch.zeros_like(aug).expand(fg.size(0) - 1, -1, -1, -1)], dim=0)
    return pred.permute(1, 0, 2, 3)


def _leaves(*arrays):
    return [torch.from_numpy(np.asarray(a, f64)).requires_grad_(True) for a in arrays]


@pytest.mark.parametrize("geo", tuple(g for g in ALL_GEOMETRIES if g[2] > 0), ids=str)
def test_shortcut_stage_reference_is_autograd(geo):
    s = tgb.stage_case(*geo)
    leaves = _leaves(s["x"], s["low"], s["head"], s["weight"], s["bias"])
    torch_shortcut_stage(*leaves).backward(torch.from_numpy(s["grad_out"].astype(f64)))
    ref = tgb.shortcut_stage_backward64(s["x"], s["low"], s["head"], s["weight"], s["bias"], s["grad_out"])
    for leaf, name in zip(leaves, ("grad_x", "grad_low", "grad_head", "grad_weight", "grad_bias")):
        close(ref[name], leaf.grad, f"{geo} {name}")


@pytest.mark.parametrize("N,hw", ((1, 35), (3, 35), (30, 9)))
def test_delta_gate_reference_is_autograd(N, hw):
    rs = tgb.rng(N, hw, 2)
    C, D = 6, 5
    x, head, weight, bias, gy = (rs.standard_normal(s_) for s_ in ((N, C, hw, 1), (N, D), (C, D + C), (C,), (N, C, hw, 1)))
    leaves = _leaves(x, head, weight, bias)
    torch_delta_gate(*leaves).backward(torch.from_numpy(gy))
    ref = tgb.delta_gate_backward64(x, head, weight, bias, gy)
    for leaf, name in zip(leaves, ("grad_x", "grad_head", "grad_weight", "grad_bias")):
        close(ref[name], leaf.grad, f"{N},{hw} {name}")


@pytest.mark.parametrize("N", (1, 2, 4))
def test_logit_head_reference_is_autograd(N):
    rs = tgb.rng(N, 3)
    C, D, h, w = 8, 5, 5, 7
    x, head, fg_w, fg_b, bg_w, bg_b, g = (rs.standard_normal(s_) for s_ in ((N, C, h, w), (N, D), (C + 1, D), (C + 1,), (C + 1, D), (C + 1,), (1, N, h, w)))
    leaves = _leaves(x, head, fg_w, fg_b, bg_w, bg_b)
    torch_predict(*leaves).backward(torch.from_numpy(g))
    ref = tgb.logit_head_backward64(x, head, fg_w, fg_b, bg_w, bg_b, g)
    names = ("grad_x", "grad_head", "grad_fg_weight", "grad_fg_bias", "grad_bg_weight", "grad_bg_bias")
    for leaf, name in zip(leaves, names):
        want = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)                    # one object: the bg head is never used
        close(ref[name], want, f"N={N} {name}")
    fg, bg = _leaves(rs.standard_normal((N, 1, h, w)), rs.standard_normal((N, 1, h, w)))
    torch_merge(fg, bg).backward(torch.from_numpy(g))
    pred, sel = tgb.background_merge_ref(fg.detach().reshape(N, -1), bg.detach().reshape(N, -1))
    gf, gb = tgb.background_merge_grad_ref(g.reshape(N, -1), sel)
    close(gf, fg.grad.reshape(N, -1), "merge grad_fg")
    close(gb, (bg.grad if bg.grad is not None else torch.zeros_like(bg)).reshape(N, -1), "merge grad_bg")
    close(pred, torch_merge(fg, bg).detach().reshape(N, -1), "merge pred")


# ------------------------------------------------------------------------------------------ 3 gradients recorded from the reference
class _Ref(torch.autograd.Function):
    """float64: a forward in plain torch, the backward from tail_grad_bounds' formulas (values only)"""

    @staticmethod
    def forward(ctx, kind, *args):
        ctx.kind = kind
        ctx.save_for_backward(*args)
        with torch.no_grad():
            return {"stage": torch_shortcut_stage, "delta": torch_delta_gate, "head": torch_predict}[kind](*args)

    @staticmethod
    def backward(ctx, g):
        a = ctx.saved_tensors
        if ctx.kind == "stage":
            r = tgb.shortcut_stage_backward64(*a, g)
            return (None,) + tuple(r[k] for k in ("grad_x", "grad_low", "grad_head", "grad_weight", "grad_bias"))
        if ctx.kind == "delta":
            r = tgb.delta_gate_backward64(*a, g)
            return (None,) + tuple(r[k] for k in ("grad_x", "grad_head", "grad_weight", "grad_bias"))
        r = tgb.logit_head_backward64(*a, g)
        return (None,) + tuple(r[k] for k in ("grad_x", "grad_head", "grad_fg_weight", "grad_fg_bias", "grad_bg_weight", "grad_bg_bias"))


class _Gct64(nn.Module):
    """gct.py:7-36, l2 mode, in plain torch"""

    def __init__(self, C, epsilon=1e-5):
        super().__init__()
        self.alpha, self.gamma, self.beta = (nn.Parameter(t(1, C, 1, 1)) for t in (torch.ones, torch.zeros, torch.zeros))
        self.epsilon = epsilon

    def forward(self, x):
        emb = (x.pow(2).sum((2, 3), keepdim=True) + self.epsilon).pow(0.5) * self.alpha
        norm = self.gamma / (emb.pow(2).mean(dim=1, keepdim=True) + self.epsilon).pow(0.5)
        return x * (1.0 + torch.tanh(emb * norm + self.beta))


class _Gate64(nn.Module):
    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.IA = nn.Linear(in_dim, out_dim)


def reference_chain(fx):
    """the recorded chain with the three tail forms replaced by this suite's float64 references -> (leaves, decoder)"""
    torch.set_default_dtype(torch.float64)
    try:
        dec = tgb.build_decoder(nn.Module(), _Gct64, _Gate64, int(fx["seed"]), **tgb.FIXTURE_DIMS)
    finally:
        torch.set_default_dtype(torch.float32)
    tgb.load_small(dec, fx)
    x, low, head = _leaves(fx["in_x"], fx["in_low_level_feat"], fx["in_IA_head"])
    gn = lambda bn, v: torch.relu(bn(v))
    l = gn(dec.bn_sc, dec.conv_sc(dec.GCT_sc(low)))
    v = _Ref.apply("stage", x, l, head, dec.IA10.IA.weight, dec.IA10.IA.bias)
    v = gn(dec.bn1, dec.conv1(v))
    v = _Ref.apply("delta", v, head, dec.IA11.IA.weight, dec.IA11.IA.bias)
    v = gn(dec.bn2, dec.conv2(v))
    pred = _Ref.apply("head", v, head, dec.IA_final_fg.weight, dec.IA_final_fg.bias, dec.IA_final_bg.weight, dec.IA_final_bg.bias)
    loss = (pred * torch.from_numpy(fx["in_weight"].astype(f64))).sum()
    loss.backward()
    return loss, (x, low, head), dec


@pytest.mark.parametrize("name", tgb.FIXTURES)
def test_references_reproduce_the_recorded_gradients(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 250_000
    assert not any("conv" in k for k in fx.files), "a fixture holds no convolution weight or gradient"
    loss, (x, low, head), dec = reference_chain(fx)
    # 1e-10, not the 1e-12 of the autograd comparisons above: those compare two float64 evaluations of ONE stage, this one two float64
    # evaluations of the whole chain (three convolutions of up to 648 terms, three GroupNorms with rstd up to eps^-1/2, a tanh behind each gate)
    # whose summation orders differ between the reference's autograd and this suite's formulas: a relative 2^-53 per operation, amplified by
    # the chain's conditioning, leaves about 1e-13 to 1e-12 of the largest entry; 1e-10 keeps two decades of room and is eight decades below
    # a float32 evaluation.  The float16 rounding of the stored parameters adds nothing: both sides read the same rounded values.
    assert abs(loss.item() - float(fx["loss"])) <= 1e-10 * max(1.0, abs(float(fx["loss"])))
    for leaf, key in ((x, "grad_x"), (low, "grad_low_level_feat"), (head, "grad_IA_head")):
        close(leaf.grad, fx[key], f"{name} {key}", rel=1e-10)
    for pname, p in tgb.small_parameters(dec):
        key = "grad_w_" + pname.replace(".", "__")
        if key in fx.files:
            close(p.grad, fx[key], f"{name} {key}", rel=1e-10)
        else:
            assert pname.startswith("IA_final_bg") and float(p.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 4 every slip leaves its bound
def leaves_bound(slipped, want_tol, what):
    want, tol = want_tol
    assert bool(((tgb.t64(slipped) - want).abs() > tol).any()), f"{what}: the slip stays inside the bound"
    assert float(tol.max()) < 1e-3 * max(float(want.abs().max()), 1e-30) or float(want.abs().max()) == 0.0, f"{what}: the bound is not a rounding bound"


def test_stage_slips_leave_the_bound():
    geo = (2, 3, 2, 5, 7, 9, 14)
    s = tgb.stage_case(*geo)
    Ce = geo[1]
    (t, et), (dg, edg) = tgb.stage_dots_ref(s["grad_out"], s["x"], s["low"])
    for kind in tgb.ADJOINT_SLIPS:
        (ts, _), (dgs, _) = tgb.stage_dots_ref(s["grad_out"], s["x"], s["low"], kind)
        leaves_bound(ts, (t, et), "t, " + kind)
        leaves_bound(dgs[:, :Ce], (dg[:, :Ce], edg[:, :Ce]), "dgain, " + kind)
    t32 = t.float().numpy()
    gx, gl = tgb.stage_apply_ref(s["grad_out"], t32, s["gain"], s["dpx"], Ce)
    for kind in ("no_feedback", "coarse_hw"):
        sx, sl = tgb.stage_apply_ref(s["grad_out"], t32, s["gain"], s["dpx"], Ce, kind)
        leaves_bound(sx[0], gx, "grad_x, " + kind)
        leaves_bound(sl[0], gl, "grad_low, " + kind)
    dd = tgb.rng(5).standard_normal((3, 7)).astype(f32)
    leaves_bound(tgb.delta_pullback_ref(dd, "no_sum")[0], tgb.delta_pullback_ref(dd), "dpx without the sum over the objects")
    gy, gain, dpx = s["grad_out"].reshape(2, 5, -1), s["gain"], s["dpx"]
    leaves_bound(tgb.delta_apply_ref(gy, gain, dpx, "no_feedback")[0], tgb.delta_apply_ref(gy, gain, dpx), "delta gate apply without the shift")


def test_head_slips_leave_the_bound():
    s = tgb.head_case(4, 128, 257)
    bg = tgb.bg_logits64(s["x"], s["wb_bg"])
    ref = tgb.logit_head_grad_ref(s["g"], tgb.select(bg), s["x"], s["wb_fg"], s["wb_bg"])
    for kind in ("bg_to_all_objects", "bg0_in_min"):
        bad = tgb.logit_head_grad_ref(s["g"], tgb.select(bg, kind), s["x"], s["wb_fg"], s["wb_bg"])
        leaves_bound(bad[0][0], ref[0], "grad_x, " + kind)
        leaves_bound(bad[2][0], ref[2], "grad_wb_bg, " + kind)
    p = tgb.planted_ties()
    bgp = tgb.bg_logits64(p["x"], p["wb_bg"])
    refp = tgb.logit_head_grad_ref(p["g"], tgb.select(bgp), p["x"], p["wb_fg"], p["wb_bg"])
    badp = tgb.logit_head_grad_ref(p["g"], tgb.select(bgp, "highest"), p["x"], p["wb_fg"], p["wb_bg"])
    assert bool(((badp[0][0] - refp[0][0]).abs() > refp[0][1]).any()) and bool(((badp[2][0] - refp[2][0]).abs() > refp[2][1]).any()), "highest index wins"


# ------------------------------------------------------------------------------------------ 5 the random cases have decided minima
@pytest.mark.parametrize("N,C,hw", tgb.HEAD_CASES)
def test_random_head_cases_are_decided(N, C, hw):
    s = tgb.head_case(N, C, hw)
    und = tgb.undecided_pixels(s["x"], s["wb_fg"], s["wb_bg"])
    assert int(und.sum()) == 0, f"{int(und.sum())} of {hw} pixels within twice the forward bound of a tie: choose another seed in HEAD_SEEDS"


# ------------------------------------------------------------------------------------------ 6 the planted ties
def test_planted_ties_tell_the_three_rules_apart():
    p = tgb.planted_ties()
    assert all(np.array_equal(v, np.round(v)) and np.abs(v).max() < 64 for v in p.values()), "small integers: every product and sum is exact in float32"
    bg = tgb.bg_logits64(p["x"], p["wb_bg"])
    sels = {r: tgb.select(bg, r) for r in tgb.RULES}
    assert tgb.arg_of(sels["lowest"]).tolist() == [1, 1, 2, 1, 2, 1] and tgb.arg_of(sels["highest"]).tolist() == [2, 3, 3, 3, 2, 1]
    assert sels["all"].sum(0).tolist() == [2, 3, 2, 2, 1, 1], "two-way, three-way, a tie with object N - 1, another two-way tie, and two pixels without one"
    grads = {r: tgb.logit_head_grad_ref(p["g"], sels[r], p["x"], p["wb_fg"], p["wb_bg"]) for r in tgb.RULES}
    for a, b in (("lowest", "highest"), ("lowest", "all"), ("highest", "all")):
        for k, what in ((0, "grad_x"), (2, "grad_wb_bg")):
            assert not torch.equal(grads[a][k][0], grads[b][k][0]), f"{a} and {b} give the same {what}"
        assert torch.equal(grads[a][1][0], grads[b][1][0]), "the fg rows do not depend on the tie"
    m = {r: tgb.background_merge_grad_ref(p["g"], sels[r])[1] for r in tgb.RULES}
    assert not torch.equal(m["lowest"], m["highest"]) and not torch.equal(m["lowest"], m["all"]) and float(m["lowest"][0].abs().max()) == 0.0
    # NaN never wins; a column of NaN and +inf selects nobody
    bad = bg.clone()
    bad[2] = float("nan")
    assert tgb.arg_of(tgb.select(bad)).tolist() == [1, 1, 3, 1, 1, 1]
    bad[1], bad[3] = float("nan"), float("inf")
    assert tgb.arg_of(tgb.select(bad)).tolist() == [0] * 6


# ------------------------------------------------------------------------------------------ 7 surface and contract
def test_twins_have_the_mirrors_signatures_and_are_named_by_them():
    for f in ("decoder_final", "predict", "augment_background_logit"):
        assert inspect.signature(getattr(tt, f)) == inspect.signature(getattr(decoder_tail, f))
        assert ops._TRAINABLE[f] == "tail_train." + f
    assert "tail_train" in aoc_amd.__all__ and "tail_train" in ops.inference_only.__doc__
    x = torch.randn(2, 4, 3, 3, requires_grad=True)
    head = torch.randn(2, 5)
    dec = nn.Module()
    dec.IA10, dec.IA11 = aoc_amd.attention.IA_gate(5 + 6, 6), aoc_amd.attention.IA_gate(5 + 2, 2)
    dec.IA_final_fg, dec.IA_final_bg = nn.Linear(5, 5), nn.Linear(5, 5)
    with pytest.raises(_lib.AocHipError, match="inference-only.*tail_train.decoder_final is the differentiable form"):
        decoder_tail.decoder_final(dec, x, x, head)
    with pytest.raises(_lib.AocHipError, match="inference-only.*tail_train.predict is the differentiable form"):
        decoder_tail.predict(dec, x, head)
    with pytest.raises(_lib.AocHipError, match="inference-only.*tail_train.augment_background_logit is the differentiable form"):
        decoder_tail.augment_background_logit(x[:, :1], x[:, :1])


def _carrier(gct_cls):
    return tgb.build_decoder(nn.Module(), gct_cls, gates_train.IA_gate, 5, Ce=64, Cr=8, D=6, Cl=8)


def test_decoder_final_refuses_the_inference_gct_and_needs_a_device():
    dec = _carrier(aoc_amd.gct.GCT)
    x, low, head = torch.randn(2, 64, 3, 4, requires_grad=True), torch.randn(2, 8, 5, 7), torch.randn(2, 6)
    with pytest.raises(_lib.AocHipError, match="gates_train.GCT"):
        tt.decoder_final(dec, x, low, head)
    for call in (lambda: tt.shortcut_stage(x, torch.randn(2, 8, 5, 7), head, torch.randn(72, 78), torch.randn(72)),
                 lambda: tt.delta_gate(x, head, torch.randn(64, 70), torch.randn(64)), lambda: tt.predict(_carrier(gates_train.GCT), x[:, :32], head),
                 lambda: tt.augment_background_logit(x[:, :1], x[:, 1:2].detach())):
        with pytest.raises(_lib.AocHipError, match="no CPU fallback"):
            call()


def test_no_gradient_path_goes_through_the_mirrors_ops(monkeypatch):
    seen = []
    for name in ("shortcut_stage", "plane_mean", "head_delta", "film_scale", "linear", "logit_head", "background_merge"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: seen.append(_n) or torch.zeros(2, 4))
    x, head = torch.randn(2, 4, 3, 3), torch.randn(2, 5)
    tt.shortcut_stage(x, x, head, torch.randn(8, 13), torch.randn(8))
    tt.delta_gate(x, head, torch.randn(4, 9), torch.randn(4))
    dec = nn.Module()
    dec.IA_final_fg, dec.IA_final_bg = nn.Linear(5, 5).requires_grad_(False), nn.Linear(5, 5).requires_grad_(False)
    tt.predict(dec, x, head)
    tt.augment_background_logit(x[:, :1], x[:, :1])
    with torch.no_grad():                                           # autograd off: the same, whatever requires_grad says
        tt.delta_gate(x.clone().requires_grad_(True), head, torch.randn(4, 9), torch.randn(4))
    assert seen == ["shortcut_stage", "plane_mean", "head_delta", "film_scale", "linear", "linear", "logit_head", "background_merge", "plane_mean",
                    "head_delta", "film_scale"]


def _t(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(f32))


def _cases():
    N, Ce, Cr, h, w, H, W, C = 3, 4, 2, 3, 4, 5, 6, 4
    F_, I_, OUT = occ.F, occ.I, occ.OUT
    z = torch.zeros

    def mk(builder):
        return lambda ops_, device: {k: v.to(device) for k, v in builder(np.random.RandomState(7)).items()}
    arg = lambda: torch.ones(H * W, dtype=torch.int32)
    return [
        occ.Case("shortcut_stage_backward_dots", [], mk(lambda rs: dict(grad_out=_t(rs, N, Ce + Cr, H, W), x=_t(rs, N, Ce, h, w), low=_t(rs, N, Cr, H, W),
                                                                        t=z(N, Ce, h, w), dgain=z(N, Ce + Cr))),
                 {"grad_out": F_, "x": F_, "low": F_, "t": OUT, "dgain": OUT},
                 lambda ops_, a: tt.shortcut_stage_backward_dots(a["grad_out"], a["x"], a["low"], a["t"], a["dgain"]), None),
        occ.Case("shortcut_stage_backward_apply", [], mk(lambda rs: dict(grad_out=_t(rs, N, Ce + Cr, H, W), t=z(N, Ce, h, w), gain=_t(rs, N, Ce + Cr),
                                                                         dpx=_t(rs, N, Ce + Cr), grad_low=z(N, Cr, H, W))),
                 {"grad_out": F_, "gain": F_, "dpx": F_, "t": OUT, "grad_low": OUT},
                 lambda ops_, a: tt.shortcut_stage_backward_apply(a["grad_out"], a["t"], a["gain"], a["dpx"], a["grad_low"]), None),
        occ.Case("delta_gate_backward_apply", [], mk(lambda rs: dict(grad_y=_t(rs, N, C, H, W), gain=_t(rs, N, C), dpx=_t(rs, N, C), grad_x=z(N, C, H, W))),
                 {"grad_y": F_, "gain": F_, "dpx": F_, "grad_x": OUT},
                 lambda ops_, a: tt.delta_gate_backward_apply(a["grad_y"], a["gain"], a["dpx"], a["grad_x"]), None),
        occ.Case("logit_head_forward", [], mk(lambda rs: dict(x=_t(rs, N, C, H, W), wb_fg=_t(rs, N, C + 1), wb_bg=_t(rs, N, C + 1), pred=z(1, N, H, W),
                                                              arg=z(H * W, dtype=torch.int32))),
                 {"x": F_, "wb_fg": F_, "wb_bg": F_, "pred": OUT, "arg": OUT},
                 lambda ops_, a: tt.logit_head_forward(a["x"], a["wb_fg"], a["wb_bg"], a["pred"], a["arg"]), None),
        occ.Case("logit_head_backward", [], mk(lambda rs: dict(grad_pred=_t(rs, 1, N, H, W), arg=arg(), x=_t(rs, N, C, H, W), wb_fg=_t(rs, N, C + 1),
                                                               wb_bg=_t(rs, N, C + 1), grad_x=z(N, C, H, W), grad_wb_fg=z(N, C + 1), grad_wb_bg=z(N, C + 1))),
                 {"grad_pred": F_, "arg": I_, "x": F_, "wb_fg": F_, "wb_bg": F_, "grad_x": OUT, "grad_wb_fg": OUT, "grad_wb_bg": OUT},
                 lambda ops_, a: tt.logit_head_backward(a["grad_pred"], a["arg"], a["x"], a["wb_fg"], a["wb_bg"],
                                                        out={k: a[k] for k in ("grad_x", "grad_wb_fg", "grad_wb_bg")}), None),
        occ.Case("background_merge_forward", [], mk(lambda rs: dict(fg=_t(rs, N, 1, H, W), bg=_t(rs, N, 1, H, W), pred=z(1, N, H, W),
                                                                    arg=z(H * W, dtype=torch.int32))),
                 {"fg": F_, "bg": F_, "pred": OUT, "arg": OUT}, lambda ops_, a: tt.background_merge_forward(a["fg"], a["bg"], a["pred"], a["arg"]), None),
        occ.Case("background_merge_backward", [], mk(lambda rs: dict(grad_pred=_t(rs, 1, N, H, W), arg=arg(), grad_fg=z(N, 1, H, W), grad_bg=z(N, 1, H, W))),
                 {"grad_pred": F_, "arg": I_, "grad_fg": OUT, "grad_bg": OUT},
                 lambda ops_, a: tt.background_merge_backward(a["grad_pred"], a["arg"], a["grad_fg"], a["grad_bg"]), None),
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
    src = inspect.getsource(tt)
    assert "data_ptr" not in src and "import ctypes" not in src
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ("_p", "_addr"):
            assert not any(isinstance(sub, ast.Call) for arg in node.args for sub in ast.walk(arg)), f"line {node.lineno}: a call expression inside _p(...)"
    public = {n for n, v in vars(ops).items() if callable(v) and not n.startswith("_") and getattr(v, "__module__", None) == ops.__name__}
    assert not {n for n in vars(tt) if n.endswith(("_backward", "_forward", "_backward_dots", "_backward_apply"))} & public


def test_entries_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(256)                         # never dereferenced: every call here returns before a launch
    need = L.aoc_shortcut_stage_grad_workspace_bytes(2, 3, 5, 7, 9, 14)
    assert need >= (2 * 3 * 5 * 7 + 2 * 3) * 4 and L.aoc_shortcut_stage_grad_workspace_bytes(31, 3, 5, 7, 9, 14) == 0
    assert L.aoc_shortcut_stage_grad_workspace_bytes(2, 0, 5, 7, 9, 14) == 0 and L.aoc_shortcut_stage_grad_workspace_bytes(2, 3, 0, 7, 9, 14) == 0

    def dots(go=p, x=p, low=p, N=2, Ce=3, Cr=2, h=5, H=9, t=p, dg=p, ws=p, nbytes=need):
        return L.aoc_shortcut_stage_grad_dots(go, x, low, N, Ce, Cr, h, 7, H, 14, t, dg, ws, nbytes, None)
    assert dots(go=None) == INVALID and dots(N=0) == INVALID and dots(Ce=0) == INVALID and dots(Cr=-1) == INVALID and dots(h=0) == INVALID and dots(H=0) == INVALID
    assert dots(x=None) == INVALID and dots(low=None) == INVALID and dots(N=31) == UNSUPPORTED and dots(H=1 << 20) == UNSUPPORTED
    assert dots(nbytes=need - 1) == WORKSPACE and dots(ws=None) == WORKSPACE and dots(t=None, ws=None) == WORKSPACE
    assert dots(t=None, dg=None, ws=None, nbytes=0) == OK

    def apply(go=p, gain=p, dpx=p, N=2, Ce=3, Cr=2, h=5, H=9, gx=p, gl=p):
        return L.aoc_shortcut_stage_grad_apply(go, gain, dpx, N, Ce, Cr, h, 7, H, 14, gx, gl, None)
    assert apply(N=0) == INVALID and apply(Ce=0) == INVALID and apply(Cr=-1) == INVALID and apply(h=0) == INVALID and apply(go=None) == INVALID
    assert apply(Cr=0) == INVALID and apply(N=31) == UNSUPPORTED and apply(H=1 << 20) == UNSUPPORTED and apply(gx=None, gl=None) == OK

    def dg(gy=p, gain=p, N=3, C=4, hw=35, gx=p):
        return L.aoc_delta_gate_grad_apply(gy, gain, p, N, C, hw, gx, None)
    assert dg(gy=None) == INVALID and dg(gain=None) == INVALID and dg(gx=None) == INVALID and dg(N=0) == INVALID and dg(C=0) == INVALID and dg(hw=0) == INVALID
    assert dg(N=31) == UNSUPPORTED

    def fwd(x=p, wf=p, wb=p, stride=9, N=2, C=8, hw=16, pred=p, arg=p):
        return L.aoc_logit_head_argmin(x, wf, wb, stride, N, C, hw, pred, arg, None)
    assert fwd(x=None) == INVALID and fwd(wf=None) == INVALID and fwd(wb=None) == INVALID and fwd(pred=None) == INVALID and fwd(arg=None) == INVALID
    assert fwd(stride=8) == INVALID and fwd(N=0) == INVALID and fwd(C=0) == INVALID and fwd(hw=0) == INVALID and fwd(N=31) == UNSUPPORTED

    def bwd(g=p, arg=p, x=p, wf=p, wb=p, stride=9, N=2, C=8, hw=16, gx=p, gf=p, gb=p):
        return L.aoc_logit_head_grad(g, arg, x, wf, wb, stride, N, C, hw, gx, gf, gb, None)
    assert bwd(g=None) == INVALID and bwd(arg=None) == INVALID and bwd(wf=None) == INVALID and bwd(wb=None) == INVALID and bwd(x=None) == INVALID
    assert bwd(stride=8) == INVALID and bwd(N=0) == INVALID and bwd(C=0) == INVALID and bwd(hw=0) == INVALID and bwd(N=31) == UNSUPPORTED
    assert bwd(gx=None, gf=None, gb=None) == OK

    assert L.aoc_background_merge_argmin(None, p, 2, 16, p, p, None) == INVALID and L.aoc_background_merge_argmin(p, None, 2, 16, p, p, None) == INVALID
    assert L.aoc_background_merge_argmin(p, p, 2, 16, p, None, None) == INVALID and L.aoc_background_merge_argmin(p, p, 2, 0, p, p, None) == INVALID
    assert L.aoc_background_merge_argmin(p, p, 31, 16, p, p, None) == UNSUPPORTED
    assert L.aoc_background_merge_grad(None, p, 2, 16, p, p, None) == INVALID and L.aoc_background_merge_grad(p, None, 2, 16, p, p, None) == INVALID
    assert L.aoc_background_merge_grad(p, p, 0, 16, p, p, None) == INVALID and L.aoc_background_merge_grad(p, p, 31, 16, p, p, None) == UNSUPPORTED
    assert L.aoc_background_merge_grad(p, p, 2, 16, None, None, None) == OK
