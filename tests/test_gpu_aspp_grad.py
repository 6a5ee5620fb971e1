"""The differentiable ASPP on the device: the entry points of csrc/aspp_grad.hip through their wrappers, and the twin aoc_amd.aspp_train.ASPP
through ``backward()``, against the float64 references and derived bounds of tests/aspp_grad_bounds.py.  The module tests record what every
wrapper received and returned during the backward (the tape of tests/test_gpu_gates_grad.py / test_gpu_decoder_grad.py, extended by this
module's wrappers), hold each call to its float64 reference AT THOSE TENSORS and read the wiring off the tape; the convolutions are torch's
and their results are shared between the twin and the mirror.  Each test prints its largest error / bound per output before it asserts.
On the parent commit this module fails at its import of aoc_amd.aspp_train, and aspp.ASPP raises under autograd."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aoc_amd
import aspp_bounds as ab
import aspp_grad_bounds as agb
import gates_grad_bounds as ggb
import test_gpu_decoder_grad as tgd
import test_gpu_gates_grad as tgg
from aoc_amd import _lib, aspp, aspp_train as at, gates_train as gt, ops
from float64_bounds import _check_bound
from test_gpu_gates_grad import DEV, dev, margins, shifted, untouched, _np

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
WORST, RHO = {}, []


def _note_rho(want, tol):
    want, tol = agb.t64(want), agb.t64(tol)
    if want.numel():
        RHO.append(float(tol.max()) / max(float(want.abs().max()), 1e-300))


def held(entry, got, want_tol, what):
    want, tol = want_tol
    r = ggb.check(_np(got) if torch.is_tensor(got) else got, want, tol, what)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    _note_rho(want, tol)
    assert r <= 1.0, f"{what}: error / bound {r:.3f}"
    return r


def worst(prefix):
    return ", ".join(f"{k[len(prefix):]} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith(prefix))


def _planes(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.reshape(a.shape[0] * a.shape[1], -1)


def _p3(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.reshape(a.shape[0], a.shape[1], -1)


# ------------------------------------------------------------------------------------------ front 1: aoc_plane_dot_multi
# (N, C, n_set, hw): the issue's cases 1 - 3 over the sizes at which the thread / float4 / wave cuts change, the module's own shape
FRONT = [(1, 8, 1, hw) for hw in agb.HWS] + [(2, 8, 4, hw) for hw in agb.HWS] + [(30, 32, 2, 35), (3, 512, 4, 31 * 33), (2, 8, 8, 257)]      # the last: a full pointer list


@pytest.mark.parametrize("N,C,S,hw", FRONT)
def test_plane_dot_multi(N, C, S, hw):
    s = agb.front_case(N, C, S, hw)
    ref = agb.plane_dot_multi_ref(_planes(s["x"]), [_planes(g) for g in s["gs"]])
    slip = agb.plane_dot_multi_ref(_planes(s["x"]), [_planes(g) for g in s["gs"]], "drop_last")[0]
    for off in (0, 1):                                                         # 1: x a float off the 16-byte grid, set k at (off + k) % 4
        x_d = shifted(s["x"], off)
        g_d = [shifted(g, (off + k * off) % 4) for k, g in enumerate(s["gs"])]
        runs = []
        for _ in range(2):
            buf, out = margins((S, N, C))
            got = at.plane_dot_multi(x_d, g_d, out)
            assert got is out and untouched(buf, (S, N, C)), "written outside dots"
            runs.append(out.clone())
        assert torch.equal(runs[0], runs[1]), "two runs differ"
        what = f"plane_dot_multi {N},{C},{S},{hw} off={off}"
        if hw > 1:
            _check_bound(_np(runs[0]).reshape(S, N * C), ref[0], ref[1], slip, what)
        held("front dots", runs[0].reshape(S, N * C), ref, what)
        for k in range(S):                                                     # set k carries the bits of the single-set entry on (g_k, x)
            _, one = gt.channel_scale_backward(g_d[k], x_d, None, want_x=False)
            assert torch.equal(one, runs[0][k]), f"{what}: set {k} is not aoc_channel_scale_grad's"
    print(f"plane_dot_multi {N},{C},{S},{hw}: worst error / bound so far: {worst('front ')}")


# ------------------------------------------------------------------------------------------ front 2: aoc_gct_gate_multi_grad
@pytest.mark.parametrize("l1", (False, True))
@pytest.mark.parametrize("N,C,S", ((1, 8, 1), (2, 8, 4), (30, 32, 2), (3, 512, 4), (2, 300, 8)))
def test_gct_gate_multi_backward(N, C, S, l1):
    rs = agb.rng(N, C, S, int(l1), 21)
    n = lambda *sh: rs.standard_normal(sh).astype(f32)
    dgate, gate = n(S, N, C), (1 + np.tanh(n(S, N, C))).astype(f32)
    sums = (n(N, C) * 20).astype(f32) if l1 else (np.abs(n(N, C)) * 30).astype(f32)
    al, ga, be = rs.uniform(0.5, 1.5, (S, C)).astype(f32), n(S, C), (0.5 * n(S, C)).astype(f32)
    if S > 1:                                                                  # a set whose gamma and beta are 0: its gate is 1 and its dsum exactly 0
        ga[1], be[1], gate[1] = 0.0, 0.0, 1.0
    ref = agb.gct_gate_multi_grad_ref(dgate, gate, sums, al, ga, 1e-5, l1)
    bad = agb.gct_gate_multi_grad_ref(dgate, gate, sums, al, ga, 1e-5, l1, slip="other_gate")
    names = ("dsum_total", "dsum", "grad_alpha", "grad_gamma", "grad_beta")
    shapes = dict(zip(names, ((N, C), (S, N, C), (S, C), (S, C), (S, C))))
    args = (dev(dgate), dev(gate), dev(sums), dev(al), [dev(g).view(1, C, 1, 1) for g in ga], dev(be), 1e-5, l1)
    runs = []
    for _ in range(2):
        bufs = {k: margins(sh) for k, sh in shapes.items()}
        got = at.gct_gate_multi_backward(*args, out={k: v for k, (_, v) in bufs.items()})
        assert all(g is bufs[k][1] for g, k in zip(got, names)) and all(untouched(bufs[k][0], sh) for k, sh in shapes.items()), "written outside the outputs"
        runs.append([g.clone() for g in got])
    what = f"gct_gate_multi_grad N={N} C={C} S={S} l1={l1}"
    for i, name in enumerate(names):
        assert torch.equal(runs[0][i], runs[1][i]), "two runs differ"
        assert np.isfinite(_np(runs[0][i])).all(), name
        held("front gate " + name, runs[0][i], ref[name], f"{what} {name}")
    if S > 1 and C > 1:
        _check_bound(_np(runs[0][1]), ref["dsum"][0], ref["dsum"][1], bad["dsum"][0], what + " dsum against another set's gate")
        assert float(runs[0][1][1].abs().max()) == 0.0, "gamma = 0: dsum comes from du * gamma and is exactly 0"
    for k in range(S):                                                         # set k carries the bits of the single-set entry with row k
        one = gt.gct_gate_backward(args[0][k], args[1][k], args[2], args[3][k], args[4][k], args[5][k], 1e-5, l1)
        assert all(torch.equal(o, runs[0][i + 1][k]) for i, o in enumerate(one)), f"{what}: set {k} is not aoc_gct_gate_grad's"
    for i in range(5):                                                         # each optional output alone: the same bits
        only = at.gct_gate_multi_backward(*args, want=tuple(j == i for j in range(5)))
        assert all((o is None) == (j != i) for j, o in enumerate(only)) and torch.equal(only[i], runs[0][i]), f"{what}: {names[i]} alone differs"
    print(f"{what}: worst error / bound so far: {worst('front gate ')}")


# ------------------------------------------------------------------------------------------ front 3: aoc_channel_scale_multi_grad_apply
@pytest.mark.parametrize("N,C,S,hw", FRONT)
def test_channel_scale_multi_backward_apply(N, C, S, hw):
    s = agb.front_case(N, C, S, hw)
    rs = agb.rng(N, C, S, hw, 22)
    gates = (1 + np.tanh(rs.standard_normal((S, N, C)))).astype(f32)
    dst = rs.standard_normal((N, C)).astype(f32)
    flat = [_planes(g) for g in s["gs"]]
    x2 = _planes(s["x"])
    for dmean in (s["dmean"], None):
        ref = agb.front_apply_ref(flat, gates.reshape(S, -1), x2, dst.reshape(-1), dmean.reshape(-1) if dmean is not None else None)
        slips = [k for k in agb.FRONT_SLIPS if not (k == "no_dmean" and dmean is None) and not (k == "other_gate" and S == 1)]
        for off in (0, 1):
            x_d = shifted(s["x"], (3 * off) % 4)
            g_d = [shifted(g, (off + k * off) % 4) for k, g in enumerate(s["gs"])]
            runs = []
            for _ in range(2):
                buf, out = margins(s["x"].shape, off)
                got = at.channel_scale_multi_backward_apply(g_d, dev(gates), x_d, dev(dst), dev(dmean) if dmean is not None else None, out)
                assert got is out and untouched(buf, s["x"].shape, off), "written outside grad_x"
                runs.append(out.clone())
            assert torch.equal(runs[0], runs[1]), "two runs differ"
            what = f"channel_scale_multi_grad_apply {N},{C},{S},{hw} off={off} dmean={dmean is not None}"
            for kind in slips:
                _check_bound(_planes(runs[0]), ref[0], ref[1], agb.front_apply_ref(flat, gates.reshape(S, -1), x2, dst.reshape(-1),
                                                                                    dmean.reshape(-1) if dmean is not None else None, kind)[0], f"{what} {kind}")
            held("front apply", _planes(runs[0]), ref, what)
            if S == 1 and dmean is None:
                # 2 dsum is exact, so (2 dsum) x and dsum (2 x) round alike: the header's order allows the identity with the single-set entry
                one = gt.gct_scale_backward(g_d[0], x_d, dev(gates[0]), dev(dst), 1)
                assert torch.equal(one, runs[0]), f"{what}: not aoc_gct_scale_grad's bits"
    print(f"channel_scale_multi_grad_apply {N},{C},{S},{hw}: worst error / bound so far: {worst('front apply')}")


# ------------------------------------------------------------------------------------------ back: aoc_groupnorm_cat_relu_grad
def _back_device(s, off):
    """the case on the device, the sources at different misalignments, with what the forward leaves for the backward"""
    us = [shifted(u, (off + k * off) % 4) for k, u in enumerate(s["us"])]
    w, b = dev(s["weights"]), dev(s["biases"])
    tail = dev(s["tail"]) if s["tail"] is not None else None
    cat, sumsq, stats = at.groupnorm_cat_relu_forward(us, s["groups"], w, b, s["gn_eps"], tail)
    al, ga, be = dev(s["gct_alpha"]), dev(s["gct_gamma"]), dev(s["gct_beta"])
    gate = ops.gct_gate(sumsq, al, ga, be, s["gct_eps"], False)
    return dict(us=us, w=w, b=b, tail=tail, cat=cat, sumsq=sumsq, stats=stats, gate=gate, al=al, ga=ga, g=shifted(s["grad_out"], (2 * off) % 4))


def _back_call(s, d, **kw):
    return at.groupnorm_cat_relu_backward(d["g"], d["us"], d["stats"], s["groups"], d["w"], d["b"], d["tail"], d["sumsq"], d["gate"], d["al"], d["ga"],
                                          s["gct_eps"], **kw)


def _back_ref(s, d, slip=None):
    return agb.cat_grad_ref(_np(d["g"]), [_np(u) for u in d["us"]], _np(d["stats"]), s["groups"], s["weights"], s["biases"], s["tail"], _np(d["sumsq"]),
                            _np(d["gate"]), s["gct_alpha"], s["gct_gamma"], s["gct_eps"], slip=slip)


def _hold_back(ref, got, what, prefix="back "):
    gu, rest = got[0], got[1:]
    for k, g in enumerate(gu):
        if g is not None:
            held(prefix + "grad_u", _p3(g), ref["grad_u"][k], f"{what} grad_u[{k}]")
    for name, g in zip(agb.BACK_OUTS[1:], rest):
        if g is not None:
            held(prefix + name, g.reshape(ref[name][0].shape), ref[name], f"{what} {name}")


@pytest.mark.parametrize("key", sorted(agb.BACK_CASES), ids=lambda k: "-".join(map(str, k)))
def test_groupnorm_cat_relu_backward(key):
    N, C, groups, n_src, C_tail, hw = key
    s = agb.back_case(*key)
    C_total = n_src * C + C_tail
    small_shapes = dict(zip(agb.BACK_OUTS[1:], ((n_src, C), (n_src, C), (N, C_tail), (C_total,), (C_total,), (C_total,))))
    if not C_tail:
        del small_shapes["grad_tail"]
    for off in (0, 1):
        d = _back_device(s, off)
        ref, und = _back_ref(s, d)
        n_und = sum(int(u.sum()) for u in und)
        assert n_und <= agb.MASK_CAP * sum(u.numel() for u in und), f"{n_und} elements undecided"
        what = f"groupnorm_cat_relu_grad {key} off={off}"
        # the forward's saved tensors are the mirror's: the statistics and the concatenation in place of the workspace and of ops' own call
        cat2, sq2 = ops.groupnorm_cat_relu(d["us"], groups, d["w"], d["b"], 1e-5, d["tail"], True, want_plane_sumsq=True)
        assert torch.equal(cat2, d["cat"]) and torch.equal(sq2, d["sumsq"])
        runs = []
        for _ in range(2):
            bu = [margins(s["us"][0].shape, (off + 3 * k * off) % 4) for k in range(n_src)]
            bs = {k: margins(sh) for k, sh in small_shapes.items()}
            got = _back_call(s, d, out=dict({k: v for k, (_, v) in bs.items()}, grad_u=[v for _, v in bu]))
            assert all(g is v for g, (_, v) in zip(got[0], bu)) and all(untouched(b_, s["us"][0].shape, (off + 3 * k * off) % 4) for k, (b_, _) in enumerate(bu))
            assert all(untouched(bs[k][0], sh) for k, sh in small_shapes.items()), "written outside the small outputs"
            runs.append(([g.clone() for g in got[0]],) + tuple(g.clone() if g is not None else None for g in got[1:]))
        for a, b in zip(runs[0][0], runs[1][0]):
            assert torch.equal(a, b), "two runs differ"
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:])), "two runs differ"
        _hold_back(ref, runs[0], what)
        if hw > 1:
            for kind in agb.BACK_SLIPS:
                if kind == "tail_no_hw":
                    if C_tail:
                        _check_bound(_np(runs[0][3]), ref["grad_tail"][0], ref["grad_tail"][1], _back_ref(s, d, kind)[0]["grad_tail"][0], f"{what} {kind}")
                    continue
                bad = _back_ref(s, d, kind)[0]
                _check_bound(_p3(runs[0][0][-1]), ref["grad_u"][-1][0], ref["grad_u"][-1][1], bad["grad_u"][-1][0], f"{what} {kind} grad_u")
                _check_bound(_np(runs[0][2]), ref["grad_beta"][0], ref["grad_beta"][1], bad["grad_beta"][0], f"{what} {kind} grad_beta")
        # planted: gamma = beta = 0 on channel 1 of source 0 (mask off: A = B = 0 exactly), tail entries <= 0
        assert float(runs[0][1][0, 1]) == 0.0 and float(runs[0][2][0, 1]) == 0.0, "a channel whose z is 0 everywhere has a gamma / beta gradient"
        if C_tail:
            assert float(runs[0][3][0, 0]) == 0.0 and float(runs[0][3][-1, 1]) == 0.0, "a tail entry <= 0 has a gradient"
        assert bool((d["gate"][:, 2] == 1.0).all()), "GCT gamma = beta = 0: the gate is 1"
        if off == 0:                                                           # each optional output alone: the same bits
            for i in range(len(agb.BACK_OUTS)):
                if agb.BACK_OUTS[i] == "grad_tail" and not C_tail:
                    continue
                want = tuple(([k == n_src - 1 for k in range(n_src)] if j == 0 else True) if j == i else ([False] * n_src if j == 0 else False) for j in range(7))
                only = _back_call(s, d, want=want)
                if i == 0:
                    assert all(g is None for g in only[0][:-1]) and torch.equal(only[0][-1], runs[0][0][-1]) and all(g is None for g in only[1:])
                else:
                    assert all(g is None for g in only[0]) and all((g is None) == (j + 1 != i) for j, g in enumerate(only[1:]))
                    assert torch.equal(only[i], runs[0][i]), f"{what}: {agb.BACK_OUTS[i]} alone differs"
    print(f"groupnorm_cat_relu_grad {key}: worst error / bound so far: {worst('back ')}")


def test_rejected_calls_write_nothing():
    """wrong group count, hw = 0, n_set = 0 and 9, N above AOC_MAX_OBJECTS, a short workspace, overlapping outputs: an error code, and the
    outputs keep their NaNs (the argument checks themselves are walked through without a device in test_aspp_grad_host.py)"""
    L = _lib.lib()
    N, C, S, hw = 2, 8, 2, 35
    x, g = torch.randn(N, C, hw, device=DEV), torch.randn(N, C, hw, device=DEV)
    small = torch.randn(S, N, C, device=DEV)
    buf, out = margins((S, N, C))
    bx, gx = margins((N, C, hw))
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    two = (ctypes.c_void_p * 2)(g.data_ptr(), g.data_ptr())
    nine = (ctypes.c_void_p * 9)(*([g.data_ptr()] * 9))
    st = ops._stream()
    codes = [L.aoc_plane_dot_multi(p(x), two, 0, N * C, hw, p(out), st), L.aoc_plane_dot_multi(p(x), nine, 9, N * C, hw, p(out), st),
             L.aoc_plane_dot_multi(p(x), two, 2, N * C, 0, p(out), st),
             L.aoc_gct_gate_multi_grad(p(small), p(small), p(small), p(small), p(small), None, S, 31, C, 1e-5, 0, p(out), None, None, None, None, None, 0, st),
             L.aoc_gct_gate_multi_grad(p(small), p(small), p(small), p(small), p(small), None, 1, N, C, 1e-5, 0, p(out), None, None, None, None, None, 0, st),
             L.aoc_channel_scale_multi_grad_apply(two, p(small), p(x), p(small), None, 0, N * C, hw, p(gx), st),
             L.aoc_channel_scale_multi_grad_apply(two, p(small), p(gx), p(small), None, 2, N * C, hw, p(gx), st)]      # grad_x on x
    s = agb.back_case(2, 8, 2, 4, 4, 35)
    d = _back_device(s, 0)
    us = (ctypes.c_void_p * 4)(*[u.data_ptr() for u in d["us"]])
    bu, gu = margins((2, 8, 35))
    gus = (ctypes.c_void_p * 4)(gu.data_ptr(), None, None, None)
    ws = torch.empty(L.aoc_groupnorm_cat_relu_grad_workspace_bytes(4, 2, 8, 4, 2), dtype=torch.uint8, device=DEV)

    def back(n_src=4, N_=2, groups=2, hw_=35, nbytes=ws.numel(), gus_=gus):
        return L.aoc_groupnorm_cat_relu_grad(p(d["g"]), us, n_src, N_, 8, hw_, groups, p(d["stats"]), p(d["w"]), p(d["b"]), p(d["tail"]), 4, p(d["sumsq"]),
                                             p(d["gate"]), p(d["al"]), p(d["ga"]), 1e-5, gus_, None, None, None, None, None, None, p(ws), nbytes, st)
    on_input = (ctypes.c_void_p * 4)(d["us"][1].data_ptr(), None, None, None)
    codes += [back(groups=3), back(hw_=0), back(n_src=0), back(n_src=9), back(N_=31), back(nbytes=ws.numel() - 1), back(gus_=on_input)]
    torch.cuda.synchronize()
    assert codes == [-1, -1, -1, -4, -2, -1, -1, -1, -1, -1, -1, -4, -2, -1], codes
    assert untouched(buf, (S, N, C)) and bool(torch.isnan(out).all()) and untouched(bx, (N, C, hw)) and bool(torch.isnan(gx).all())
    assert untouched(bu, (2, 8, 35)) and bool(torch.isnan(gu).all()), "a rejected call wrote"
    assert back() == 0 and bool(torch.isfinite(gu).all())                     # the same call, accepted


# ------------------------------------------------------------------------------------------ the modules: every wrapper call on tape
class Tape(tgd.Tape):
    """tgd.Tape (the wrappers of gates_train and decoder_train) plus this module's four"""
    OURS = ("plane_dot_multi", "gct_gate_multi_backward", "channel_scale_multi_backward_apply", "groupnorm_cat_relu_backward")

    def __enter__(self):
        super().__enter__()
        self._ours = {n: getattr(at, n) for n in self.OURS}
        for n, f in self._ours.items():
            setattr(at, n, lambda *a, _n=n, _f=f, **k: self._note(_n, _f, a, k))
        return self

    def __exit__(self, *exc):
        for n, f in self._ours.items():
            setattr(at, n, f)
        super().__exit__(*exc)


UNDECIDED = []


def hold_call(name, a, k, res):
    """one recorded wrapper call against its float64 reference at the tensors it received"""
    if name == "plane_dot_multi":
        x, gs = a[0], a[1]
        S = len(gs)
        held("module dots", res.reshape(S, -1), agb.plane_dot_multi_ref(_planes(x), [_planes(g) for g in gs]), name)
    elif name == "gct_gate_multi_backward":
        ref = agb.gct_gate_multi_grad_ref(_np(a[0]), _np(a[1]), _np(a[2]), _np(a[3]), _np(a[4]), a[6], a[7])
        for g, n in zip(res, ("dsum_total", "dsum", "grad_alpha", "grad_gamma", "grad_beta")):
            if g is not None:
                held("module gate " + n, g, ref[n], n)
    elif name == "channel_scale_multi_backward_apply":
        gs, gates, x, dst, dmean = a[:5]
        ref = agb.front_apply_ref([_planes(g) for g in gs], _np(gates).reshape(len(gs), -1), _planes(x), _np(dst).reshape(-1),
                                  _np(dmean).reshape(-1) if dmean is not None else None)
        held("module front apply", _planes(res), ref, name)
    elif name == "groupnorm_cat_relu_backward":
        g, us, stats, groups, gamma, beta, tail, sumsq, gate, al, ga, eps = a[:12]
        ref, und = agb.cat_grad_ref(_p3(g), [_p3(u) for u in us], _np(stats), groups, _np(gamma), _np(beta), _np(tail), _np(sumsq), _np(gate),
                                    _np(al).reshape(-1), _np(ga).reshape(-1), eps)
        UNDECIDED.append(sum(int(u.sum()) for u in und))
        _hold_back(ref, res, name, prefix="module back ")
    elif name == "cond_scale_backward" and a[0] is None and a[4] is None:     # the plane mean's backward: nothing but dpx / hw, broadcast
        dpx, hw = agb.t64(_np(a[5])), a[2].shape[1]
        q = agb.E(dpx) / agb._const(hw)
        N, C = dpx.shape
        held("module mean", res.reshape(N, C, hw), (q.v.unsqueeze(2).expand(N, C, hw), q.e.unsqueeze(2).expand(N, C, hw)), "grad_x of the plane mean")
    else:
        with SummedBounds():
            tgd.hold_call(name, a, k, res)


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


def replayed(mirror, twin, records):
    """tgd.replayed for a module whose pooled 1 x 1 convolution is never called as a module (both arms read its weight for a [N, 512] x
    [512, 128] product): only the recorded convolutions are replaced"""
    mirror.load_state_dict(twin.state_dict())
    for n, m in list(mirror.named_modules()):
        if isinstance(m, torch.nn.Conv2d) and n in records:
            parent, _, child = n.rpartition(".")
            setattr(mirror.get_submodule(parent) if parent else mirror, child, tgd.Replay(n, *records[n]))
    return mirror.to(DEV)


def mirror_bits(twin, make_mirror, call):
    """call(module) under no_grad on the twin, then on the replaying mirror: the same bits"""
    records, hooks = tgd.record_convs(twin)
    with torch.no_grad():
        yt = call(twin)
    for hk in hooks:
        hk.remove()
    assert len(records) == 5, sorted(records)
    with torch.no_grad():
        ym = call(replayed(make_mirror(), twin, records))
    assert not yt.requires_grad and torch.equal(yt, ym), "without a graph the twin does not give the mirror's bits"


def _twin(seed, twin=True):
    torch.manual_seed(seed)
    net = (at if twin else aspp).ASPP()
    rs = np.random.RandomState([seed, 5])
    h16 = lambda v: torch.from_numpy(np.asarray(v, f32).astype(np.float16).astype(f32))
    with torch.no_grad():
        for name, p in net.named_parameters():
            leaf = name.split(".")[-1]
            if leaf == "alpha" or (leaf == "weight" and p.dim() == 1):
                p.copy_(h16(rs.uniform(0.5, 1.5, tuple(p.shape))))
            elif leaf in ("gamma", "beta") or leaf == "bias":
                p.copy_(h16(0.5 * rs.standard_normal(tuple(p.shape))))
            else:
                p.copy_(h16(p.detach().numpy()))
    return net.to(DEV)


def aspp_plain(x, sd):
    """aspp_bounds.aspp_torch with a graph: the reference's lines in plain torch on x's device and dtype, from a state_dict of that dtype"""
    outs = []
    for name, d in zip(ab.BRANCHES, ab.DILATIONS):
        w = sd[name + ".atrous_conv.weight"]
        y = F.conv2d(ab._gct_torch(x, sd, name + ".GCT."), w, None, 1, 0 if w.shape[2] == 1 else d, d)
        outs.append(torch.relu(F.group_norm(y, w.shape[0] // 4, sd[name + ".bn.weight"], sd[name + ".bn.bias"], 1e-5)))
    x5 = torch.relu(F.conv2d(F.adaptive_avg_pool2d(x, (1, 1)), sd["global_avg_pool.1.weight"]))
    x5 = F.interpolate(x5, size=outs[0].shape[2:], mode='bilinear', align_corners=True)
    y = F.conv2d(ab._gct_torch(torch.cat(outs + [x5], dim=1), sd, "GCT."), sd["conv1.weight"])
    return torch.relu(F.group_norm(y, 32, sd["bn1.weight"], sd["bn1.bias"], 1e-5))


def plain_gradients(net, x, gy, dtype, device):
    """-> (out, gradients by name: 'x' and every parameter) of aspp_plain in `dtype` on `device`"""
    sd = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in net.state_dict().items()}
    lx = x.detach().to(device=device, dtype=dtype).requires_grad_(True)
    with torch.enable_grad():
        out = aspp_plain(lx, sd)
        out.backward(gy.to(device=device, dtype=dtype))
    return out.detach(), dict({k: v.grad for k, v in sd.items()}, x=lx.grad)


FRONT_CHAIN = ["plane_dot_multi", "gct_gate_multi_backward", "channel_scale_multi_backward_apply"]
GN, GCT = ["groupnorm_relu_backward"], ["channel_scale_backward", "gct_gate_backward", "gct_scale_backward"]
CHAINS = {True: GN + ["groupnorm_cat_relu_backward", "film_gain_backward"] + FRONT_CHAIN,
          False: GN + GCT + ["film_gain_backward", "cond_scale_backward"] + 4 * (GN + GCT)}


@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("N,h,w", ((3, 5, 7), (3, 3, 4), (1, 2, 3)))
def test_aspp_backward(N, h, w, fused):
    net = _twin(100 + N * h)
    rs = agb.rng(N, h, w, 31)
    x = dev(rs.standard_normal((N, 512, h, w)).astype(f32).astype(np.float16).astype(f32))
    gy = dev(rs.standard_normal((N, 256, h, w)).astype(f32))
    mirror_bits(net, lambda: aspp.ASPP(), lambda m: m(x, fused=fused))     # without a graph: the mirror's bits
    records, hooks = tgd.record_convs(net)
    for p in net.parameters():
        p.grad = None
    lx = x.clone().requires_grad_(True)
    with Tape() as tape, torch.enable_grad():
        y = net(lx, fused=fused)
        y.backward(gy)
    for hk in hooks:
        hk.remove()
    del RHO[:], UNDECIDED[:]
    for c in tape.calls:
        hold_call(*c)
    rho = sum(RHO)
    with torch.no_grad():
        ym = replayed(aspp.ASPP(), net, records)(x, fused=fused)
    assert y.shape == ym.shape and torch.equal(y.detach(), ym), "the forward with a graph is not the mirror's at this fused flag"
    names = tape.names()
    if fused:
        assert names == CHAINS[True], names
        c = tape.calls
        seen = {n: out for n, (_, out) in records.items()}
        same = lambda u, v: u is v or (u.data_ptr() == v.data_ptr() and u.numel() == v.numel())
        # bn1: the cotangent and conv1's output; the back stage: the four convolution outputs in branch order
        assert torch.equal(c[0][1][0], gy) and torch.equal(c[0][1][1], seen["conv1"])
        assert all(torch.equal(u, seen[f"{b}.atrous_conv"]) for u, b in zip(c[1][1][1], ab.BRANCHES))
        with torch.no_grad():
            _, sumsq, mean = ops.plane_sum_sumsq(x, want_sum=False)
            wp = net.global_avg_pool[1].weight.view(128, 512)
            tail = ops.linear(mean, wp, None)
        assert torch.equal(c[1][1][6], tail), "the back stage's tail is not the pooled product before its ReLU"
        # the pooled product's backward: grad_tail at a unit gain, the plane means, the 1 x 1 weight
        assert same(c[2][1][0], c[1][3][3]) and bool((c[2][1][1] == 1).all()) and torch.equal(c[2][1][2], mean) and torch.equal(c[2][1][3], wp)
        # the front: x and four cotangents; their dots into the gates' backward with the forward's sums; the apply pass on dsum_total and dmean
        assert torch.equal(c[3][1][0], x) and len(c[3][1][1]) == 4 and c[4][1][0] is c[3][3] and torch.equal(c[4][1][2], sumsq)
        assert all(a_ is b_ for a_, b_ in zip(c[5][1][0], c[3][1][1])) and c[5][1][1] is c[4][1][1] and c[5][1][3] is c[4][3][0] and same(c[5][1][4], c[2][3][0])
        assert torch.equal(lx.grad, c[5][3]) and torch.equal(net.global_avg_pool[1].weight.grad.view(128, 512), c[2][3][1])
        for k, b in enumerate(ab.BRANCHES):
            m = getattr(net, b)
            assert torch.equal(m.GCT.alpha.grad.reshape(-1), c[4][3][2][k]) and torch.equal(m.GCT.beta.grad.reshape(-1), c[4][3][4][k])
            assert torch.equal(m.bn.weight.grad, c[1][3][1][k]) and torch.equal(m.bn.bias.grad, c[1][3][2][k])
        assert torch.equal(net.GCT.gamma.grad.reshape(-1), c[1][3][5])
    else:
        assert sorted(names) == sorted(CHAINS[False]), names
    assert sum(UNDECIDED) == 0, f"{sum(UNDECIDED)} elements within the float32 bound of a ReLU's z = 0: the comparison is not decided"
    # end to end against float64 autograd of the reference's lines (CPU).  The bound per tensor: what the same lines in plain float32 PyTorch
    # on this device are off the float64 gradients by, plus the kernels' own relative bounds summed over the taped calls times the tensor's
    # largest entry (the rule of test_decoder_final_and_predict_backward).
    out64, want = plain_gradients(net, x, gy, torch.float64, "cpu")
    out32, ref32 = plain_gradients(net, x, gy, torch.float32, DEV)
    got = dict({k: p.grad for k, p in net.named_parameters()}, x=lx.grad)
    ratio = 0.0
    for key in sorted(want):
        assert got[key] is not None and bool(torch.isfinite(got[key]).all()), key
        rec = want[key]
        scale = float(rec.abs().max())
        e_hip = float((got[key].detach().cpu().double().reshape(rec.shape) - rec).abs().max())
        e_ref = float((ref32[key].detach().cpu().double().reshape(rec.shape) - rec).abs().max())
        tol = e_ref + rho * scale
        ratio = max(ratio, e_hip / max(tol, 1e-300))
        print(f"  ASPP {N},{h}x{w} fused={fused} {key}: |hip - float64| {e_hip:.3e}, plain float32's own error {e_ref:.3e}, summed bounds {rho * scale:.3e}")
        assert e_hip <= tol, f"{key}: {e_hip:.3e} against {tol:.3e}"
    print(f"ASPP {N},{h}x{w} fused={fused}: worst error / bound so far: {worst('module ')}; end to end {ratio:.3f} of the bound, sum of rho {rho:.2e}")


@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("name", agb.ASPP_FIXTURES)
def test_aspp_backward_against_the_recorded_gradients(name, fused, golden):
    """End to end at the fixtures' shapes against the gradients recorded from the reference's OWN ASPP in float64
    (tests/golden/make_golden_aspp_grad.py), under the bound of test_aspp_backward: plain float32 PyTorch's own error plus the summed kernel bounds."""
    fx = golden(name)
    net = agb.load_fixture_parameters(at.ASPP(), fx).to(DEV)
    x, gy = dev(fx["in_x"].astype(f32)), dev(fx["in_weight"].astype(f32))
    lx = x.clone().requires_grad_(True)
    with Tape() as tape, torch.enable_grad():
        y = net(lx, fused=fused)
        y.backward(gy)
    del RHO[:], UNDECIDED[:]
    for c in tape.calls:
        hold_call(*c)
    rho = sum(RHO)
    assert sum(UNDECIDED) == 0, f"{sum(UNDECIDED)} elements within the float32 bound of a ReLU's z = 0: the comparison is not decided"
    assert abs(float((y.detach().double() * gy.double()).sum()) - float(fx["loss"])) <= 1e-4 * float((y.detach().abs().double() * gy.abs().double()).sum())
    _, ref32 = plain_gradients(net, x, gy, torch.float32, DEV)
    got = dict({k: p.grad for k, p in net.named_parameters()}, x=lx.grad)
    ratio = 0.0
    for key in sorted(k[5:] for k in fx if k.startswith("grad_")):
        rec = torch.from_numpy(fx["grad_" + key]).double()
        scale = float(rec.abs().max())
        view = lambda g: agb.recorded_view(key, g.detach().cpu().double()).reshape(rec.shape)
        e_hip, e_ref = float((view(got[key]) - rec).abs().max()), float((view(ref32[key]) - rec).abs().max())
        tol = e_ref + rho * scale
        ratio = max(ratio, e_hip / max(tol, 1e-300))
        print(f"  {name} fused={fused} {key}: |hip - recorded| {e_hip:.3e}, plain float32's own error {e_ref:.3e}, summed bounds {rho * scale:.3e}, largest entry {scale:.3e}")
        assert e_hip <= tol, f"{name} {key}: {e_hip:.3e} against {tol:.3e}"
    print(f"ASPP {name} fused={fused}: end to end {ratio:.3f} of the bound, sum of rho {rho:.2e}")


def test_frozen_parameters_ask_for_nothing_unwanted():
    net = _twin(7)
    for n, p in net.named_parameters():
        if ".GCT." in n or n.startswith("GCT.") or ".bn." in n:
            p.requires_grad_(False)
    x = torch.randn(2, 512, 3, 4, device=DEV)
    with Tape() as tape, torch.enable_grad():
        net(x).sum().backward()                                                # x wants nothing either: only the convolutions and bn1 train
    calls = {c[0]: c for c in tape.calls}
    back = calls["groupnorm_cat_relu_backward"][3]
    assert all(g is not None for g in back[0]) and back[3] is not None and all(g is None for g in (back[1], back[2], back[4], back[5], back[6]))
    assert "plane_dot_multi" not in calls and "channel_scale_multi_backward_apply" not in calls, "nothing of the front wants a gradient"
    assert calls["film_gain_backward"][3][0] is None and calls["film_gain_backward"][3][1] is not None
    assert all(p.grad is None for n, p in net.named_parameters() if not p.requires_grad) and net.conv1.weight.grad is not None
    lx = x.clone().requires_grad_(True)
    with Tape() as tape, torch.enable_grad():
        net(lx).sum().backward()
    gate = [c for c in tape.calls if c[0] == "gct_gate_multi_backward"][0][3]
    assert gate[0] is not None and all(g is None for g in gate[1:]) and lx.grad is not None


def test_mirror_raises_and_double_backward_raises():
    x = torch.randn(1, 512, 3, 4, device=DEV, requires_grad=True)
    with torch.enable_grad():
        with pytest.raises(_lib.AocHipError, match="inference-only.*aspp_train.ASPP is the differentiable form"):
            aspp.ASPP().to(DEV)(x)
        net = _twin(9)
        g, = torch.autograd.grad(net(x).sum(), x, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()


def test_aspp_peak_memory():
    N, h, w = 3, 31, 33
    net = _twin(11)
    rs = agb.rng(N, h, w, 9)
    x, gy = dev(rs.standard_normal((N, 512, h, w)).astype(f32)).requires_grad_(True), dev(rs.standard_normal((N, 256, h, w)).astype(f32))

    def run():
        with torch.enable_grad():
            y = net(x)
            y.backward(gy)
        return y.detach()
    run()                                                                      # warm-up: library, MIOpen and allocator
    x.grad = None
    for p in net.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    plane = N * h * w * 4
    output = 256 * plane
    # saved: x, the four gated copies (the convolutions' inputs), the four convolution outputs, the gated concatenation (conv1's input),
    # conv1's output (bn1's input); the small tensors
    saved = (512 + 4 * 512 + 4 * 128 + 640 + 256) * plane + (5 * N * 512 + 2 * N * 640 + N * 128 + 5 * N * 32 * 2) * 4
    grads = 512 * plane + sum(p.numel() for p in net.parameters()) * 4         # x's and the parameters'
    L = _lib.lib()
    work = L.aoc_groupnorm_cat_relu_workspace_bytes(4, N, 32) + L.aoc_groupnorm_cat_relu_grad_workspace_bytes(4, N, 128, 128, 32) + \
        L.aoc_groupnorm_relu_workspace_bytes(N, 32) + L.aoc_groupnorm_relu_grad_workspace_bytes(N, 256, 32) + L.aoc_gct_gate_multi_grad_workspace_bytes(4, N, 512)
    budget = output + saved + grads + work
    print(f"ASPP {N},{h}x{w}: peak {peak} bytes above the inputs, output + saved + gradients + workspaces {budget}")
    assert peak < 2 * budget, f"peak {peak} bytes, twice the accounted tensors is {2 * budget}"
    del y
