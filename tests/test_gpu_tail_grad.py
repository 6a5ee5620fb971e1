"""The differentiable decoder tail on the device: the entry points of csrc/tail_grad.hip through their wrappers, and the twins of
aoc_amd.tail_train through ``backward()``, against the float64 references and derived bounds of tests/tail_grad_bounds.py.  Every entry is driven
into NaN-margined outputs, aligned and one float off the 16-byte grid, twice (the same bits) and with each optional output alone (the same
bits).  The module tests record what every wrapper received and returned during the backward (the tape of tests/test_gpu_gates_grad.py and
tests/test_gpu_decoder_grad.py, extended by this module's wrappers), hold each call to its float64 reference AT THOSE TENSORS and read the
wiring off the tape, so no tolerance is added for the chain; the convolutions are torch's.  Each test prints its largest error / bound."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import aoc_amd
import decoder_grad_bounds as dgb
import gates_grad_bounds as ggb
import tail_grad_bounds as tgb
import test_gpu_decoder_grad as tgd
import test_gpu_gates_grad as tgg
import test_tail_grad_host as tth
from aoc_amd import _lib, decoder_tail, gates_train as gt, ops, tail_train as tt
from test_gpu_gates_grad import DEV, dev, margins, shifted, untouched, _np

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORST = {}
RHO, UNDECIDED = [], []                 # per held output of a module test: its largest bound over its largest value; undecided ReLU elements per call


def held(entry, got, want_tol, what):
    want, tol = want_tol
    _note_rho(want, tol)
    r = ggb.check(_np(got), want, tol, what)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, f"{what}: error / bound {r:.3f}"
    return r


def _note_rho(want, tol):
    want, tol = ggb.t64(want), ggb.t64(tol)
    if want.numel() and float(want.abs().max()) > 0.0:            # an output that is exactly 0 (one object: the inter-object code and its pull-back) has no relative bound
        RHO.append(float(tol.max()) / float(want.abs().max()))


class SummedBounds:
    """while open, every `held` of test_gpu_gates_grad and of test_gpu_decoder_grad notes, as this module's own does, the output's relative
    bound (its largest tolerance over its largest reference value) in RHO"""

    def __enter__(self):
        self.saved = [(m, m.held) for m in (tgg, tgd)]
        for m, f in self.saved:
            m.held = lambda entry, got, want_tol, what, _f=f: (_note_rho(*want_tol), _f(entry, got, want_tol, what))[1]
        return self

    def __exit__(self, *exc):
        for m, f in self.saved:
            m.held = f


def worst(prefix):
    return ", ".join(f"{k[len(prefix):]} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith(prefix))


# ------------------------------------------------------------------------------------------ 1 the shortcut stage's two passes
STAGE_RUNS = tuple((g, m) for g in tgb.STAGE_GEOMETRIES + (tgb.MAP_GEOMETRY,) for m in ("gain", "no_gain", "Cr0") if not (m == "Cr0" and g[2] == 0))


@pytest.mark.parametrize("geo,mode", STAGE_RUNS, ids=str)
def test_shortcut_stage_grad(geo, mode):
    N, Ce, Cr, h, w, H, W = geo
    s = tgb.stage_case(*geo)
    if mode == "Cr0":
        Cr, s["low"], s["grad_out"] = 0, None, np.ascontiguousarray(s["grad_out"][:, :Ce])
        s["gain"], s["dpx"] = np.ascontiguousarray(s["gain"][:, :Ce]), np.ascontiguousarray(s["dpx"][:, :Ce])
    Ct = Ce + Cr
    ref_t, ref_dg = tgb.stage_dots_ref(s["grad_out"], s["x"], s["low"])
    for off in ((0, 1) if geo != tgb.MAP_GEOMETRY else (1,)):
        go, x = shifted(s["grad_out"], off), shifted(s["x"], off)
        low = shifted(s["low"], off) if Cr else None
        runs = []
        for _ in range(2):
            bt, ot = margins((N, Ce, h, w), off)
            bg, og = margins((N, Ct))
            rt, rg = tt.shortcut_stage_backward_dots(go, x, low, ot, og)
            assert rt is ot and rg is og and untouched(bt, (N, Ce, h, w), off) and untouched(bg, (N, Ct)), "written outside the outputs"
            runs.append((ot.clone(), og.clone()))
        what = f"shortcut_stage_grad {geo} {mode} off={off}"
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what + ": two runs differ"
        t, dgain = runs[0]
        held("stage t", t, ref_t, what + " t")
        held("stage dgain", dgain, ref_dg, what + " dgain")
        only_t, none = tt.shortcut_stage_backward_dots(go, x, low, want_gain=False)          # each output alone: the same bits
        none2, only_g = tt.shortcut_stage_backward_dots(go, x, low, want_t=False)
        assert none is None and none2 is None and torch.equal(only_t, t) and torch.equal(only_g, dgain), what + ": an output alone differs"
        if (h, w) == (H, W):
            assert torch.equal(t, go[:, :Ce]), "the identity geometry: t is grad_out bit for bit"
        gain, dpx = (dev(s["gain"]), dev(s["dpx"])) if mode != "no_gain" else (None, None)
        ref_x, ref_l = tgb.stage_apply_ref(s["grad_out"], _np(t), s["gain"] if gain is not None else None, s["dpx"] if dpx is not None else None, Ce)
        applied = []
        for _ in range(2):
            bx, ox = margins((N, Ce, h, w), off)
            ox.copy_(t)
            bl, ol = margins((N, Cr, H, W), off) if Cr else (None, None)
            rx, rl = tt.shortcut_stage_backward_apply(go, ox, gain, dpx, ol)
            assert rx is ox and rl is ol and untouched(bx, (N, Ce, h, w), off) and (not Cr or untouched(bl, (N, Cr, H, W), off)), "written outside the outputs"
            applied.append((ox.clone(), ol.clone() if Cr else None))
        assert torch.equal(applied[0][0], applied[1][0]) and (not Cr or torch.equal(applied[0][1], applied[1][1])), what + ": two apply runs differ"
        held("stage grad_x", applied[0][0], ref_x, what + " grad_x")
        if Cr:
            held("stage grad_low", applied[0][1], ref_l, what + " grad_low")
            gx_only, nl = tt.shortcut_stage_backward_apply(go, t.clone(), gain, dpx, want_low=False)
            nx, gl_only = tt.shortcut_stage_backward_apply(go, None, gain, dpx, channels=Ce)
            assert nl is None and nx is None and torch.equal(gx_only, applied[0][0]) and torch.equal(gl_only, applied[0][1]), what + ": an output alone differs"
        if mode == "no_gain":
            assert torch.equal(applied[0][0], t) and (not Cr or torch.equal(applied[0][1], go[:, Ce:])), "no gain, no feedback: a plain resize adjoint"
    dead_rows, dead_cols = ((tgb.dtb.bicubic_matrix(a, b)[3].sum(0) == 0).to(DEV) for a, b in ((h, H), (w, W)))
    if int(dead_rows.sum()):
        assert float(t[:, :, dead_rows].abs().max()) == 0.0, "source rows no tap reaches are written as 0"
    if int(dead_cols.sum()):
        assert float(t[:, :, :, dead_cols].abs().max()) == 0.0, "source columns no tap reaches are written as 0"
    assert geo != (2, 2, 1, 3, 4, 1, 1) or int(dead_cols.sum()) == 1, "one output pixel: its clamped taps end at column 2 of 4"
    print(f"shortcut_stage_grad {geo} {mode}: worst error / bound so far: {worst('stage ')}")


@pytest.mark.parametrize("N,hw", tgb.DELTA_CASES)
def test_delta_gate_apply(N, hw):
    C = 3
    rs = tgb.rng(N, hw, 4)
    gy, gain, dpx = rs.standard_normal((N, C, hw)).astype(f32), (1 + np.tanh(rs.standard_normal((N, C)))).astype(f32), rs.standard_normal((N, C)).astype(f32)
    ref = tgb.delta_apply_ref(gy, gain, dpx)
    for src_off, dst_off in ((0, 0), (1, 3)):                                  # the gradient plane at another misalignment than its source
        g_d = shifted(gy, src_off)
        runs = []
        for _ in range(2):
            b, o = margins(gy.shape, dst_off)
            r = tt.delta_gate_backward_apply(g_d, dev(gain), dev(dpx), o)
            assert r is o and untouched(b, gy.shape, dst_off), "written outside the output"
            runs.append(o.clone())
        assert torch.equal(runs[0], runs[1]), "two runs differ"
        held("delta apply", runs[0], ref, f"delta_gate_apply {N},{hw} offs {src_off},{dst_off}")
    plain = tt.delta_gate_backward_apply(dev(gy), dev(gain))
    held("delta apply", plain, tgb.delta_apply_ref(gy, gain, None), "without a shift")
    print(f"delta_gate_apply {N},{hw}: worst error / bound {WORST['delta apply']:.3f}")


# ------------------------------------------------------------------------------------------ 2 the logit head
def _head_device(s, off):
    N, C, hw = s["x"].shape
    return shifted(s["x"].reshape(N, C, 1, hw), off), dev(s["wb_fg"]), dev(s["wb_bg"]), shifted(s["g"].reshape(1, N, 1, hw), off)


def _check_head(s, what):
    N, C, hw = s["x"].shape
    sel = tgb.select(tgb.bg_logits64(s["x"], s["wb_bg"]))
    want_pred, tol_pred = tgb.dtb.logit_head_ref(tgb.t64(s["x"]), tgb.t64(s["wb_fg"]), tgb.t64(s["wb_bg"]))
    ref = tgb.logit_head_grad_ref(s["g"], sel, s["x"], s["wb_fg"], s["wb_bg"])
    for off in (0, 1):
        x, wf, wb, g = _head_device(s, off)
        pred, arg = tt.logit_head_forward(x, wf, wb)
        assert torch.equal(pred, ops.logit_head(x, wf, wb)), what + ": pred is not ops.logit_head's"
        held("head pred", pred.reshape(N, hw), (want_pred, tol_pred), what + " pred")
        if N > 1:
            assert arg.dtype == torch.int32 and torch.equal(arg.cpu(), tgb.arg_of(sel)), what + ": arg is not the float64 argmin (lowest index of a tie)"
        else:
            assert arg is None
        shapes = {"grad_x": (N, C, 1, hw), "grad_wb_fg": (N, C + 1), "grad_wb_bg": (N, C + 1)}
        runs = []
        for _ in range(2):
            bufs = {k: margins(shape, off if k == "grad_x" else 0) for k, shape in shapes.items()}
            got = tt.logit_head_backward(g, arg, x, wf, wb, out={k: v for k, (_, v) in bufs.items()})
            assert all(r is bufs[k][1] for r, k in zip(got, shapes)) and all(untouched(bufs[k][0], shapes[k], off if k == "grad_x" else 0) for k in shapes)
            runs.append([r.clone() for r in got])
        for k, (name, a, b) in enumerate(zip(shapes, *runs)):
            assert torch.equal(a, b), f"{what} {name}: two runs differ"
            held("head " + name, a.reshape(ref[k][0].shape), ref[k], f"{what} off={off} {name}")
            alone = tt.logit_head_backward(g, arg, x, wf, wb, want=tuple(j == k for j in range(3)))
            assert all((r is None) == (j != k) for j, r in enumerate(alone)) and torch.equal(alone[k], a), f"{what}: {name} alone differs"
        assert float(runs[0][2][0].abs().max()) == 0.0, "row 0 of grad_wb_bg is 0"
    return runs[0]


@pytest.mark.parametrize("N,C,hw", tgb.HEAD_CASES)
def test_logit_head(N, C, hw):
    _check_head(tgb.head_case(N, C, hw), f"logit_head {N},{C},{hw}")
    print(f"logit_head {N},{C},{hw}: worst error / bound so far: {worst('head ')}")


def test_logit_head_planted_ties_and_nan():
    p = tgb.planted_ties()
    gx, gf, gb = _check_head(p, "planted ties")
    bg = tgb.bg_logits64(p["x"], p["wb_bg"])
    ref = tgb.logit_head_grad_ref(p["g"], tgb.select(bg), p["x"], p["wb_fg"], p["wb_bg"])
    assert torch.equal(gx.reshape(4, 2, 6).cpu().double(), ref[0][0]) and torch.equal(gb.cpu().double(), ref[2][0]), "small integers: exact"
    for rule in ("highest", "all"):
        bad = tgb.logit_head_grad_ref(p["g"], tgb.select(bg, rule), p["x"], p["wb_fg"], p["wb_bg"])
        assert not torch.equal(gx.reshape(4, 2, 6).cpu().double(), bad[0][0]) and not torch.equal(gb.cpu().double(), bad[2][0]), rule
    q = {k: v.copy() for k, v in p.items()}
    q["x"][2, 0, :] = np.nan                                                  # object 2's bg logits are NaN at every pixel: it never wins
    x, wf, wb, g = _head_device(q, 0)
    pred, arg = tt.logit_head_forward(x, wf, wb)
    assert arg.tolist() == [1, 1, 3, 1, 1, 1] and torch.equal(pred.nan_to_num(7.0), ops.logit_head(x, wf, wb).nan_to_num(7.0))
    gx2, _, gb2 = tt.logit_head_backward(g, arg, x, wf, wb)
    assert float(gb2[2].abs().max()) == 0.0 and bool(torch.isfinite(gx2[[0, 1, 3]]).all()), "the NaN object gets no bg gradient"


@pytest.mark.parametrize("hw", tgb.MERGE_HW)
@pytest.mark.parametrize("N", (1, 2, 3, 4, 30))
def test_background_merge(N, hw):
    rs = tgb.rng(N, hw, 6)
    fg, bg, g = (rs.standard_normal((N, 1, 1, hw)).astype(f32) for _ in range(3))
    if N > 2 and hw > 1:
        bg[2, 0, 0, 0] = bg[1, 0, 0, 0]                                       # a planted tie unless another object is lower still
    want_pred, sel = tgb.background_merge_ref(fg.reshape(N, hw), bg.reshape(N, hw))
    pred, arg = tt.background_merge_forward(dev(fg), dev(bg))
    assert torch.equal(pred, ops.background_merge(dev(fg), dev(bg))) and (arg is None if N == 1 else torch.equal(arg.cpu(), tgb.arg_of(sel)))
    want_f, want_b = tgb.background_merge_grad_ref(g.reshape(N, hw), sel)
    runs = []
    for _ in range(2):
        (bf, of), (bb, ob) = margins((N, 1, 1, hw)), margins((N, 1, 1, hw), 1)
        rf, rb = tt.background_merge_backward(dev(g.reshape(1, N, 1, hw)), arg, of, ob)
        assert rf is of and rb is ob and untouched(bf, (N, 1, 1, hw)) and untouched(bb, (N, 1, 1, hw), 1)
        runs.append((of.clone(), ob.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0].reshape(N, hw).cpu().double(), want_f) and torch.equal(runs[0][1].reshape(N, hw).cpu().double(), want_b)
    only_f, none = tt.background_merge_backward(dev(g.reshape(1, N, 1, hw)), arg, want=(True, False))
    assert none is None and torch.equal(only_f, runs[0][0])


# ------------------------------------------------------------------------------------------ 3 the twins: every wrapper call on tape
class Tape(tgd.Tape):
    """tgd.Tape (the wrappers of gates_train and decoder_train) plus this module's; the apply pass overwrites t, so the tape keeps a copy"""
    TAIL = ("shortcut_stage_backward_dots", "shortcut_stage_backward_apply", "delta_gate_backward_apply", "logit_head_backward", "background_merge_backward")

    def __enter__(self):
        super().__enter__()
        self._tail = {n: getattr(tt, n) for n in self.TAIL}
        for n, f in self._tail.items():
            setattr(tt, n, lambda *a, _n=n, _f=f, **k: self._tail_note(_n, _f, a, k))
        return self

    def _tail_note(self, name, f, a, k):
        seen = tuple(v.clone() if (name == "shortcut_stage_backward_apply" and i == 1 and v is not None) else v for i, v in enumerate(a))
        res = f(*a, **k)
        kept = (res[0].clone() if res[0] is not None else None, res[1]) if name == "shortcut_stage_backward_dots" else res
        self.calls.append((name, seen, k, kept))
        return res

    def __exit__(self, *exc):
        for n, f in self._tail.items():
            setattr(tt, n, f)
        super().__exit__(*exc)


def hold_call(name, a, k, res):
    if name == "shortcut_stage_backward_dots":
        ref_t, ref_g = tgb.stage_dots_ref(_np(a[0]), _np(a[1]), _np(a[2]))
        if res[0] is not None:
            held("module stage t", res[0], ref_t, "t")
        held("module stage dgain", res[1], ref_g, "dgain")
    elif name == "shortcut_stage_backward_apply":
        Ce = a[1].shape[1] if a[1] is not None else k["channels"]
        tin = _np(a[1]) if a[1] is not None else np.zeros((a[0].shape[0], Ce, 1, 1), f32)
        ref_x, ref_l = tgb.stage_apply_ref(_np(a[0]), tin, _np(a[2]), _np(a[3]), Ce)
        if res[0] is not None:
            held("module stage grad_x", res[0], ref_x, "grad_x")
        if res[1] is not None:
            held("module stage grad_low", res[1], ref_l, "grad_low")
    elif name == "delta_gate_backward_apply":
        N, C = a[0].shape[:2]
        held("module delta apply", res.reshape(N, C, -1), tgb.delta_apply_ref(_np(a[0]).reshape(N, C, -1), _np(a[1]), _np(a[2])), "grad_x")
    elif name == "logit_head_backward":
        g, arg, x, wf, wb = a[:5]
        N, C = x.shape[:2]
        x3 = _np(x).reshape(N, C, -1)
        sel = torch.zeros(N, x3.shape[2], dtype=torch.float64)
        if arg is not None:
            und = tgb.undecided_pixels(x3, _np(wf), _np(wb))
            want = tgb.arg_of(tgb.select(tgb.bg_logits64(x3, _np(wb))))
            assert bool((arg.cpu()[~und] == want[~und]).all()), "arg differs from the float64 argmin at a decided pixel"
            sel[arg.cpu().long(), torch.arange(x3.shape[2])] = 1.0
            sel[0] = 0.0
        ref = tgb.logit_head_grad_ref(_np(g).reshape(N, -1), sel, x3, _np(wf), _np(wb) if wb is not None else None)
        for r, rf, n in zip(res, ref, ("grad_x", "grad_wb_fg", "grad_wb_bg")):
            if r is not None:
                held("module head " + n, r.reshape(rf[0].shape), rf, n)
    elif name == "background_merge_backward":
        g, arg = a[:2]
        N = g.shape[1]
        sel = torch.zeros(N, g.numel() // N, dtype=torch.float64)
        if arg is not None:
            sel[arg.cpu().long(), torch.arange(sel.shape[1])] = 1.0
            sel[0] = 0.0
        for r, want in zip(res, tgb.background_merge_grad_ref(_np(g).reshape(N, -1), sel)):
            if r is not None:
                assert torch.equal(r.reshape(N, -1).cpu().double(), want), "the merge's gradients are copies: exact"
    else:
        if name == "groupnorm_relu_backward":                                   # the elements within the float32 bound of z = 0, counted
            gy, x, _, groups, gamma, beta, residual, relu, gain = a[:9]
            UNDECIDED.append(int(dgb.groupnorm_relu_grad_ref(tgd._p3(gy), tgd._p3(x), tgd._p3(residual), groups, _np(gamma), _np(beta), 1e-5, relu,
                                                             _np(gain))[1].sum()))
        tgd.hold_call(name, a, k, res)


class Decoder(nn.Module):
    """carries the twins as methods, the way INTEGRATION.md binds them onto the reference's class"""
    decoder_final = tt.decoder_final
    predict = tt.predict


class MirrorDecoder(nn.Module):
    decoder_final = decoder_tail.decoder_final
    predict = decoder_tail.predict


def _decoder(fx, twin=True):
    dec = tgb.build_decoder(Decoder() if twin else MirrorDecoder(), gt.GCT if twin else aoc_amd.gct.GCT, gt.IA_gate if twin else aoc_amd.attention.IA_gate,
                            int(fx["seed"]), **tgb.FIXTURE_DIMS)
    tgb.load_small(dec, fx)
    return dec.to(DEV)


def _forward(dec, x, low, head):
    return dec.predict(dec.decoder_final(x, low, head), head)


def reference_float32(fx):
    """the reference's lines in plain PyTorch, float32, on the device, with the fixture's parameters -> its gradients by the fixture's keys"""
    dec = tgb.build_decoder(nn.Module(), tth._Gct64, tth._Gate64, int(fx["seed"]), **tgb.FIXTURE_DIMS)
    tgb.load_small(dec, fx)
    dec = dec.to(DEV)
    x, low, head = (dev(fx[k].astype(f32)).requires_grad_(True) for k in ("in_x", "in_low_level_feat", "in_IA_head"))
    gn = lambda bn, v: torch.relu(bn(v))
    with torch.enable_grad():
        v = tth.torch_shortcut_stage(x, gn(dec.bn_sc, dec.conv_sc(dec.GCT_sc(low))), head, dec.IA10.IA.weight, dec.IA10.IA.bias)
        v = tth.torch_delta_gate(gn(dec.bn1, dec.conv1(v)), head, dec.IA11.IA.weight, dec.IA11.IA.bias)
        pred = tth.torch_predict(gn(dec.bn2, dec.conv2(v)), head, dec.IA_final_fg.weight, dec.IA_final_fg.bias, dec.IA_final_bg.weight, dec.IA_final_bg.bias)
        pred.backward(dev(fx["in_weight"].astype(f32)))
    return _by_key((x, low, head), dec)


def _by_key(leaves, dec):
    out = dict(zip(("grad_x", "grad_low_level_feat", "grad_IA_head"), (l.grad for l in leaves)))
    out.update({"grad_w_" + n.replace(".", "__"): p.grad for n, p in tgb.small_parameters(dec)})
    return out


def against_the_recorded_gradients(name, fx, got, rho):
    """End to end: the device gradients of x, low_level_feat, IA_head and the small parameters against the gradients recorded from the
    reference's own float64 run.  The bound per tensor is a sum of two figures, neither taken from the code under test:
      * the reference's own error: what the reference's lines in plain float32 PyTorch, run on the same device with the same parameters, are off
        the recorded float64 gradients by (largest entry).  It measures what ANY float32 evaluation of this chain owes to the chain's
        conditioning: the convolutions' own float32 sums and the float32 activations every backward stage reads;
      * the kernels' own bounds, summed: every output held on the tape above has a derived relative bound rho_c (its largest tolerance over
        its largest reference value); a local error of that relative size is carried to the end at the gain the chain applies to the
        gradient itself, so it moves a final tensor by at most about rho_c times that tensor's largest entry: (sum_c rho_c) max |recorded|.
        This is a first-order statement at unit relative gain, not an operator-norm bound; a wiring mistake (a wrong cotangent, a missing
        contribution to IA_head) moves a tensor by its own size, five orders of magnitude beyond it.
    A ReLU decision within the float32 bound of z = 0 would move a gradient by its |grad_y| in either arm: the tape counts such elements and
    the fixtures' seeds leave none."""
    ref32 = reference_float32(fx)
    assert sum(UNDECIDED) == 0, f"{sum(UNDECIDED)} elements within the float32 bound of a ReLU's z = 0: the comparison is not decided"
    worst_ratio = 0.0
    for key in sorted(k for k in fx.files if k.startswith("grad_")):
        rec = torch.from_numpy(fx[key]).double()
        scale = float(rec.abs().max())
        e_hip = float((got[key].detach().cpu().double().reshape(rec.shape) - rec).abs().max())
        e_ref = float((ref32[key].detach().cpu().double().reshape(rec.shape) - rec).abs().max())
        tol = e_ref + rho * scale
        worst_ratio = max(worst_ratio, e_hip / max(tol, 1e-300))
        print(f"  {name} {key}: |hip - recorded| {e_hip:.3e}, reference's own float32 error {e_ref:.3e}, summed bounds {rho * scale:.3e}, largest entry {scale:.3e}")
        assert e_hip <= tol, f"{name} {key}: {e_hip:.3e} against {tol:.3e}"
    return worst_ratio


GN, GCT = ["groupnorm_relu_backward"], ["channel_scale_backward", "gct_gate_backward", "gct_scale_backward"]
CHAIN = (["logit_head_backward"] + GN + ["channel_scale_backward", "film_gain_backward", "delta_gate_backward_apply"] + GN
         + ["shortcut_stage_backward_dots", "film_gain_backward", "shortcut_stage_backward_apply"] + GN + GCT)


@pytest.mark.parametrize("name", tgb.FIXTURES[:2])
def test_decoder_final_and_predict_backward(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    dec = _decoder(fx)
    x, low, head, gy = (dev(fx[k].astype(f32)) for k in ("in_x", "in_low_level_feat", "in_IA_head", "in_weight"))
    N, D = head.shape
    tgd.mirror_bits(dec, lambda: _decoder(fx, twin=False), lambda m: _forward(m, x, low, head))      # without a graph: the mirror's bits
    records, hooks = tgd.record_convs(dec)
    params = dict(dec.named_parameters())
    for p in params.values():
        p.grad = None
    leaves = [t.clone().requires_grad_(True) for t in (x, low, head)]
    with Tape() as tape, torch.enable_grad():
        y = _forward(dec, *leaves)
        y.backward(gy)
    for hk in hooks:
        hk.remove()
    del RHO[:], UNDECIDED[:]
    with SummedBounds():
        for c in tape.calls:
            hold_call(*c)
    with torch.no_grad():
        ym = _forward(tgd.replayed(_decoder(fx, twin=False), dec, records), x, low, head)
    assert y.shape == ym.shape and torch.equal(y.detach(), ym), "the forward with a graph is not the mirror's"
    assert tape.names() == CHAIN, tape.names()
    c = tape.calls
    seen = {n: out for n, (_, out) in records.items()}
    same = lambda u, v: u is v or (u.data_ptr() == v.data_ptr() and u.numel() == v.numel())
    # the head receives the cotangent; bn2 its grad_x and conv2's output
    assert torch.equal(c[0][1][0], gy) and same(c[1][1][0], c[0][3][0]) and torch.equal(c[1][1][1], seen["conv2"])
    # IA11: the dots' dgain into the small backward, its pull-back and gain into the apply pass, whose result is bn1's cotangent
    assert c[3][1][0] is c[2][3][1] and same(c[4][1][0], c[2][1][0]) and c[4][1][1] is c[3][1][1] and same(c[5][1][0], c[4][3]) and torch.equal(c[5][1][1], seen["conv1"])
    held("module dpx", c[4][1][2], tgb.delta_pullback_ref(_np(c[3][3][0])[:, D:]), "IA11's delta pull-back")
    # IA10: pass A on the stage's own inputs, its dgain into the small backward, pass B on the same cotangent, on pass A's t, in place
    assert torch.equal(c[6][1][1], x) and c[7][1][0] is c[6][3][1] and c[8][1][0] is c[6][1][0] and torch.equal(c[8][1][1], c[6][3][0]) and c[8][1][2] is c[7][1][1]
    held("module dpx", c[8][1][3], tgb.delta_pullback_ref(_np(c[7][3][0])[:, D:]), "IA10's delta pull-back")
    assert torch.equal(leaves[0].grad, c[8][3][0]) and same(c[9][1][0], c[8][3][1]) and torch.equal(c[9][1][1], seen["conv_sc"]), "bn_sc receives pass B's grad_low"
    assert torch.equal(leaves[1].grad, c[12][3]), "low_level_feat's gradient is the GCT's apply pass"
    pg = {n: p.grad for n, p in params.items()}
    assert torch.equal(pg["IA10.IA.weight"], c[7][3][1]) and torch.equal(pg["IA11.IA.bias"], c[3][3][2]) and torch.equal(pg["bn2.weight"], c[1][3][2])
    assert all(g is not None and bool(torch.isfinite(g).all()) for n, g in pg.items() if not (N == 1 and n.startswith("IA_final_bg")))
    assert all(l.grad is not None and bool(torch.isfinite(l.grad).all()) for l in leaves)
    # the wrappers' fg / bg rows through the torch products of the two linear layers
    gf, gb = c[0][3][1], c[0][3][2]
    lin = tgb.head_linear_grad_ref(_np(gf), _np(head), _np(dec.IA_final_fg.weight))
    held("module linear", pg["IA_final_fg.weight"], lin[1], "IA_final_fg.weight")
    held("module linear", pg["IA_final_fg.bias"], lin[2], "IA_final_fg.bias")
    if N > 1:
        lin_bg = tgb.head_linear_grad_ref(_np(gb), _np(head), _np(dec.IA_final_bg.weight))
        held("module linear", pg["IA_final_bg.weight"], lin_bg[1], "IA_final_bg.weight")
        held("module linear", pg["IA_final_bg.bias"], lin_bg[2], "IA_final_bg.bias")
    rho = sum(RHO)                                                             # every output held above: the kernels', the pull-backs', the linear layers'
    ratio = against_the_recorded_gradients(name, fx, _by_key(leaves, dec), rho)
    print(f"decoder_final + predict {name}: worst error / bound so far: {worst('module ')}; end to end {ratio:.3f} of the bound, sum of rho {rho:.2e}")


def test_augment_background_logit_backward():
    N, h, w = 4, 5, 7
    rs = tgb.rng(N, h, w, 8)
    fg, bg, gy = (dev(rs.standard_normal(s_).astype(f32)) for s_ in ((N, 1, h, w), (N, 1, h, w), (1, N, h, w)))
    bg[2, 0, 0, :3] = bg[1, 0, 0, :3]                                         # three planted ties of objects 1 and 2
    lf, lb = fg.clone().requires_grad_(True), bg.clone().requires_grad_(True)
    with Tape() as tape, torch.enable_grad():
        y = tt.augment_background_logit(lf, lb)
        y.backward(gy)
    assert torch.equal(y.detach(), ops.background_merge(fg, bg)) and tape.names() == ["background_merge_backward"]
    hold_call(*tape.calls[0])
    want_f, want_b = tgb.background_merge_grad_ref(_np(gy).reshape(N, -1), tgb.select(tgb.t64(_np(bg)).reshape(N, -1)))
    assert torch.equal(lf.grad.reshape(N, -1).cpu().double(), want_f) and torch.equal(lb.grad.reshape(N, -1).cpu().double(), want_b)
    with torch.enable_grad():                                                 # a frozen bg: its gradient is not asked for
        with Tape() as tape:
            tt.augment_background_logit(lf, bg).backward(gy)
    assert tape.calls[0][3][1] is None


def test_frozen_parameters_ask_for_nothing_unwanted():
    fx = np.load(os.path.join(GOLDEN, tgb.FIXTURES[0] + ".npz"))
    dec = _decoder(fx).requires_grad_(False)
    x, low, head, gy = (dev(fx[k].astype(f32)) for k in ("in_x", "in_low_level_feat", "in_IA_head", "in_weight"))
    lx = x.clone().requires_grad_(True)
    with Tape() as tape, torch.enable_grad():
        _forward(dec, lx, low, head).backward(gy)
    by = {}
    for n, a, k, res in tape.calls:
        by.setdefault(n, []).append((a, k, res))
    assert lx.grad is not None and all(p.grad is None for p in dec.parameters())
    assert by["logit_head_backward"][0][2][1] is None and by["logit_head_backward"][0][2][2] is None, "frozen IA_final layers: no row gradients"
    assert all(res[1] is None and res[2] is None for _, _, res in by["film_gain_backward"]), "frozen gates: only grad_head_ext"
    assert by["shortcut_stage_backward_apply"][0][2][1] is None, "low_level_feat and the shortcut branch want no gradient"
    assert all(res[2] is None and res[3] is None for _, _, res in by["groupnorm_relu_backward"])
    assert "gct_gate_backward" not in by


def test_double_backward_raises():
    x = torch.randn(2, 4, 3, 3, device=DEV, requires_grad=True)
    head, w, b = torch.randn(2, 5, device=DEV), torch.randn(4, 9, device=DEV), torch.randn(4, device=DEV)
    with torch.enable_grad():
        for y in (tt.delta_gate(x, head, w, b), tt.logit_head(x, torch.randn(2, 5, device=DEV), torch.randn(2, 5, device=DEV)),
                  tt.shortcut_stage(x, torch.randn(2, 2, 5, 6, device=DEV), head, torch.randn(6, 11, device=DEV), None)):
            g, = torch.autograd.grad((y * y).sum(), x, create_graph=True)
            with pytest.raises(RuntimeError, match="once_differentiable"):
                g.sum().backward()


def test_tail_peak_memory():
    fx = np.load(os.path.join(GOLDEN, tgb.FIXTURES[0] + ".npz"))
    dec = _decoder(fx)
    N, Ce, Cr, Cl, D, Ch = 3, 64, 8, 16, 12, 32
    h, w, H, W = 9, 6, 17, 11
    rs = tgb.rng(N, 9)
    x, low, head, gy = (dev(rs.standard_normal(s).astype(f32)) for s in ((N, Ce, h, w), (N, Cl, H, W), (N, D), (1, N, H, W)))
    x.requires_grad_(True), low.requires_grad_(True), head.requires_grad_(True)

    def run():
        with torch.enable_grad():
            y = _forward(dec, x, low, head)
            y.backward(gy)
        return y.detach()
    run()                                                                      # warm-up: library, MIOpen and allocator
    for t in (x, low, head, *dec.parameters()):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    fine, coarse = N * H * W * 4, N * h * w * 4
    output = fine
    # saved: GCT_sc's input and conv_sc's (its output); bn_sc's input; the stage's x and low; conv1's input (the stage's output); bn1's input; IA11's x;
    # conv2's input; bn2's input; the head's x; arg; the small [N, C] tensors
    saved = (Cl + Cl + Cr + Cr + (Ce + Cr) + 5 * Ch) * fine + Ce * coarse + H * W * 4 + 16 * N * (Ce + Cr + D) * 4
    grads = Ce * coarse + Cl * fine + N * D * 4 + sum(p.numel() for p in dec.parameters()) * 4
    L = _lib.lib()
    work = (L.aoc_shortcut_stage_grad_workspace_bytes(N, Ce, h, w, H, W) + L.aoc_shortcut_stage_workspace_bytes(N, Ce, Cr, D)
            + sum(L.aoc_groupnorm_relu_workspace_bytes(N, g) + L.aoc_groupnorm_relu_grad_workspace_bytes(N, c, g) for c, g in ((Cr, 2), (Ch, 32), (Ch, 32))))
    budget = output + saved + grads + work
    print(f"decoder_final + predict {N},{Ce},{H}x{W}: peak {peak} bytes above the inputs, output + saved + gradients + workspaces {budget}")
    assert peak <= 2 * budget, f"peak {peak} bytes, twice the accounted tensors is {2 * budget}"
    del y
