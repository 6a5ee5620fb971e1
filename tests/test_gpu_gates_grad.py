"""The differentiable calibration gates on the device: the six entry points of csrc/gate_grad.hip through their wrappers, and the four
twins of aoc_amd.gates_train through ``backward()``, against the float64 references and derived bounds of tests/gates_grad_bounds.py.
Every module test records what each wrapper received and returned during the backward and holds each call to its reference AT THOSE
TENSORS, and reads the wiring off the same tape (`wired`): every tensor a stage received is the module's input, the cotangent, a parameter,
the forward's saved tensor (recomputed through the mirror's calls and held to its float64 value) or the very tensor an earlier stage
returned, and mode, l1 and eps are the module's.  So no tolerance is added for the chain.  Each test prints its largest error / bound per entry before it asserts."""
import numpy as np
import pytest
import torch

import aoc_amd
import gates_grad_bounds as ggb
from aoc_amd import _lib, attention, conditioning_layer as cl, gates_train as gt, gct, ops
import float64_bounds as fb
from float64_bounds import _check_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, f64 = np.float32, np.float64
NAN = float("nan")
PAD = 8                                  # floats around a caller's output: a multiple of four keeps the view's alignment


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def shifted(a, off):
    """a device copy of `a` whose base sits `off` floats past a 16-byte boundary"""
    a = np.ascontiguousarray(a, f32)
    buf = torch.empty(a.size + 4, device=DEV)
    v = buf[off:off + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def margins(shape, off=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD + 4,), NAN, device=DEV)
    return buf, buf[PAD + off:PAD + off + n].view(*shape)


def untouched(buf, shape, off=0):
    n = int(np.prod(shape))
    return bool(torch.isnan(buf[:PAD + off]).all() and torch.isnan(buf[PAD + off + n:]).all())


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


WORST = {}


def note(entry, ratio):
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    return ratio


def held(entry, got, want_tol, what):
    want, tol = want_tol
    r = note(entry, ggb.check(_np(got), want, tol, what))
    assert r <= 1.0, f"{what}: error / bound {r:.3f}"
    return r


# ------------------------------------------------------------------------------------------ 1 aoc_channel_scale_grad
@pytest.mark.parametrize("planes,hw", ((1, 1), (5, 9), (6, 35), (3, 257), (3, 1023), (3, 1024), (2, 8209), (700, 3)))
def test_channel_scale_grad(planes, hw):
    rs = ggb.rng(planes, hw, 1)
    gy, x = rs.standard_normal((planes, 1, hw)).astype(f32), rs.standard_normal((planes, 1, hw)).astype(f32)
    gain = (1 + np.tanh(rs.standard_normal((planes, 1)))).astype(f32)
    ref = ggb.channel_scale_grad_ref(gy[:, 0], x[:, 0], gain[:, 0])
    slip = (ggb.channel_scale_grad_ref(gy[:, 0], x[:, 0], gain[:, 0], "prev_gain")[0][0], ggb.channel_scale_grad_ref(gy[:, 0], x[:, 0], gain[:, 0], "drop_last")[1][0])
    for off in (0, 1):                                                         # 1: every plane a float off the 16-byte grid (4-byte front)
        g_d, x_d, a_d = shifted(gy, off), shifted(x, off), dev(gain)
        runs = []
        for _ in range(2):
            bx, ox = margins(gy.shape, off)
            bg, og = margins(gain.shape)
            rx, rg = gt.channel_scale_backward(g_d, x_d, a_d, ox, og)
            assert rx is ox and rg is og and untouched(bx, gy.shape, off) and untouched(bg, gain.shape), "written outside the outputs"
            runs.append((ox.clone(), og.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
        what = f"channel_scale_grad {planes}x{hw} off={off}"
        _check_bound(_np(runs[0][0]).reshape(planes, hw), ref[0][0], ref[0][1], slip[0] if planes > 1 else ref[0][0] + 1, what + " grad_x")
        _check_bound(_np(runs[0][1]).reshape(planes), ref[1][0], ref[1][1], slip[1], what + " dgain")
        held("channel_scale_grad", runs[0][0].reshape(planes, hw), ref[0], what)
        held("channel_scale_grad", runs[0][1].reshape(planes), ref[1], what)
        only_x, none = gt.channel_scale_backward(g_d, None, a_d, want_gain=False)      # each half alone: the same bits
        none2, only_g = gt.channel_scale_backward(g_d, x_d, None, want_x=False)
        assert none is None and none2 is None and torch.equal(only_x, runs[0][0]) and torch.equal(only_g, runs[0][1])
    print(f"channel_scale_grad {planes}x{hw}: worst error / bound {WORST['channel_scale_grad']:.3f}")


# ------------------------------------------------------------------------------------------ 2 aoc_film_gain_grad
@pytest.mark.parametrize("O,c,D", ((1, 1, 1), (2, 5, 7), (3, 164, 400), (30, 4, 1025)))
def test_film_gain_grad(O, c, D):
    rs = ggb.rng(O, c, D, 2)
    dgain, head, W = (rs.standard_normal(s).astype(f32) for s in ((O, c), (O, D), (c, D)))
    gain = (1 + np.tanh(2 * rs.standard_normal((O, c)))).astype(f32)
    gain[0, 0] = 2.0 if c == 1 else 0.0                                        # a saturated gate: exactly no gradient through it
    ref = ggb.film_gain_grad_ref(dgain, gain, head, W)
    bad = ggb.film_gain_grad_ref(dgain, gain, head, W, "one_minus_t")
    shapes = ((O, D), (c, D), (c,))
    runs = []
    for _ in range(2):
        bufs = [margins(s) for s in shapes]
        got = gt.film_gain_backward(dev(dgain), dev(gain), dev(head), dev(W), *(v for _, v in bufs))
        assert all(g is v for g, (_, v) in zip(got, bufs)) and all(untouched(b, s) for (b, _), s in zip(bufs, shapes)), "written outside the outputs"
        runs.append([g.clone() for g in got])
    for k, name in enumerate(("grad_head", "grad_weight", "grad_bias")):
        assert torch.equal(runs[0][k], runs[1][k]), "two runs differ"
        slip = bad[k][0] if (O * c > 1) else ref[k][0] + 1
        _check_bound(_np(runs[0][k]), ref[k][0], ref[k][1], slip, f"film_gain_grad {O},{c},{D} {name}")
        held("film_gain_grad", runs[0][k], ref[k], name)
    assert float(runs[0][1][0].abs().max()) == 0.0 or O > 1, "a saturated channel of the only object has a weight gradient"
    gh, gw, gb = gt.film_gain_backward(dev(dgain), dev(gain), dev(head), dev(W), want=(False, True, False))
    assert gh is None and gb is None and torch.equal(gw, runs[0][1])
    print(f"film_gain_grad {O},{c},{D}: worst error / bound {WORST['film_gain_grad']:.3f}")


# ------------------------------------------------------------------------------------------ 3, 4 the GCT kernels
@pytest.mark.parametrize("l1", (False, True))
@pytest.mark.parametrize("N,C", ((1, 1), (3, 5), (3, 300), (1, 640), (30, 257)))
def test_gct_gate_grad(N, C, l1):
    rs = ggb.rng(N, C, int(l1), 3)
    dgate = rs.standard_normal((N, C)).astype(f32)
    gate = (1 + np.tanh(rs.standard_normal((N, C)))).astype(f32)
    s = (rs.standard_normal((N, C)) * 20).astype(f32) if l1 else (np.abs(rs.standard_normal((N, C))) * 30).astype(f32)
    if N * C > 1:
        s[0, 0] = 0.0                                                          # an all-zero plane: l2 stays finite through eps, l1 takes sign(0) = 0
    al, ga, be = rs.uniform(0.5, 1.5, C).astype(f32), rs.standard_normal(C).astype(f32), rs.standard_normal(C).astype(f32)
    ref = ggb.gct_gate_grad_ref(dgate, gate, s, al, ga, 1e-5, l1)
    bad = ggb.gct_gate_grad_ref(dgate, gate, s, al, ga, 1e-5, l1, "one_minus_t")
    no_dm = ggb.gct_gate_grad_ref(dgate, gate, s, al, ga, 1e-5, l1, "no_dM")
    shapes = ((N, C), (C,), (C,), (C,))
    runs = []
    for _ in range(2):
        bufs = [margins(sh) for sh in shapes]
        got = gt.gct_gate_backward(dev(dgate), dev(gate), dev(s), dev(al).view(1, C, 1, 1), dev(ga), dev(be), 1e-5, l1, *(v for _, v in bufs))
        assert all(g is v for g, (_, v) in zip(got, bufs)) and all(untouched(b, sh) for (b, _), sh in zip(bufs, shapes)), "written outside the outputs"
        runs.append([g.clone() for g in got])
    for k, name in enumerate(("dsum", "grad_alpha", "grad_gamma", "grad_beta")):
        assert torch.equal(runs[0][k], runs[1][k]), "two runs differ"
        assert np.isfinite(_np(runs[0][k])).all(), name
        held("gct_gate_grad", runs[0][k], ref[k], name)
        if C > 1 or k > 1:            # one channel: e norm depends neither on S nor on alpha; dsum and grad_alpha are rounding residue of a zero
            _check_bound(_np(runs[0][k]), ref[k][0], ref[k][1], bad[k][0], f"gct_gate_grad N={N} C={C} l1={l1} {name}")
    _check_bound(_np(runs[0][0]), ref[0][0], ref[0][1], no_dm[0][0], f"gct_gate_grad N={N} C={C} l1={l1} dsum against the dropped dM term")
    only = gt.gct_gate_backward(dev(dgate), dev(gate), dev(s), dev(al), dev(ga), dev(be), 1e-5, l1, want=(True, False, False, False))
    assert only[1] is None and only[2] is None and only[3] is None and torch.equal(only[0], runs[0][0])
    print(f"gct_gate_grad N={N} C={C} l1={l1}: worst error / bound {WORST['gct_gate_grad']:.3f}")


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("planes,hw", ((1, 1), (6, 35), (3, 1023), (2, 8209)))
def test_gct_scale_grad(planes, hw, mode):
    rs = ggb.rng(planes, hw, mode, 4)
    gy, x = rs.standard_normal((planes, 1, hw)).astype(f32), rs.standard_normal((planes, 1, hw)).astype(f32)
    x[0] = 0.0                                                                 # sign(0) = 0
    gate, dsum = (1 + np.tanh(rs.standard_normal((planes, 1)))).astype(f32), rs.standard_normal((planes, 1)).astype(f32)
    want, tol = ggb.gct_scale_grad_ref(gy[:, 0], x[:, 0], gate[:, 0], dsum[:, 0], mode)
    slip, _ = ggb.gct_scale_grad_ref(gy[:, 0], x[:, 0], gate[:, 0], dsum[:, 0], mode, True)
    if planes == 1 and mode != 0:
        slip = want + 1                                                        # the only plane is the zero plane: f' = 0 either way
    for off in (0, 1):
        runs = []
        for _ in range(2):
            buf, out = margins(gy.shape, off)
            got = gt.gct_scale_backward(shifted(gy, off), shifted(x, off), dev(gate), dev(dsum), mode, out)
            assert got is out and untouched(buf, gy.shape, off), "written outside grad_x"
            runs.append(out.clone())
        assert torch.equal(runs[0], runs[1]), "two runs differ"
        _check_bound(_np(runs[0]).reshape(planes, hw), want, tol, slip, f"gct_scale_grad {planes}x{hw} mode {mode} off={off}")
        held("gct_scale_grad", runs[0].reshape(planes, hw), (want, tol), "grad_x")
    print(f"gct_scale_grad {planes}x{hw} mode {mode}: worst error / bound {WORST['gct_scale_grad']:.3f}")


# ------------------------------------------------------------------------------------------ 5 aoc_cond_codes_grad
@pytest.mark.parametrize("N,C,D", ((1, 4, 7), (3, 24, 5), (30, 4, 9), (3, 32, 300), (3, 300, 12)))
def test_cond_codes_grad(N, C, D):
    rs = ggb.rng(N, C, D, 5)
    args = [rs.standard_normal(s).astype(f32) for s in ((N, 2 * C + D), (N, C), (N, C), (N, D), (C, C), (C, C), (D, D))]
    ref = ggb.cond_codes_grad_ref(*args)
    last, minus = ggb.cond_codes_grad_ref(*args, "drop_last"), ggb.cond_codes_grad_ref(*args, "no_minus")
    shapes = dict(zip(ggb.CODE_OUTS, ((N, C), (N, C), (N, D), (C, C), (C,), (C, C), (C,), (D, D), (D,))))
    runs = []
    for _ in range(2):
        bufs = {k: margins(s) for k, s in shapes.items()}
        got = gt.cond_codes_backward(*(dev(a) for a in args), out={k: v for k, (_, v) in bufs.items()})
        assert all(g is bufs[k][1] for g, k in zip(got, ggb.CODE_OUTS)) and all(untouched(bufs[k][0], s) for k, s in shapes.items())
        runs.append([g.clone() for g in got])
    for k, name in enumerate(ggb.CODE_OUTS):
        assert torch.equal(runs[0][k], runs[1][k]), "two runs differ"
        if N == 1 and name == "dpx":
            assert float(runs[0][k].abs().max()) == 0.0, "N = 1: dpx = dd - dd is exactly 0"
            continue
        if N == 1 and name == "grad_w2":
            assert float(runs[0][k].abs().max()) == 0.0, "N = 1: the forward's delta px - px is exactly 0"
            continue
        _check_bound(_np(runs[0][k]), ref[name][0], ref[name][1], last[name][0], f"cond_codes_grad {N},{C},{D} {name}")
        held("cond_codes_grad", runs[0][k], ref[name], name)
    if N > 1:
        _check_bound(_np(runs[0][1]), ref["dpx"][0], ref["dpx"][1], minus["dpx"][0], "cond_codes_grad dpx against the dropped - dd[n]")
    some = gt.cond_codes_backward(*(dev(a) for a in args), want=(True, False, False, False, False, True, False, False, False))
    assert [g is None for g in some] == [False, True, True, True, True, False, True, True, True] and torch.equal(some[0], runs[0][0]) and torch.equal(some[5], runs[0][5])
    # C = 0: one square linear's backward (conditioning_layer's mlp_layer)
    gh, gw, gb = (gt.cond_codes_backward(dev(args[0][:, 2 * C:].copy()), None, None, dev(args[3]), None, None, dev(args[6]))[i] for i in (2, 7, 8))
    assert torch.equal(gh, runs[0][2]) and torch.equal(gw, runs[0][7]) and torch.equal(gb, runs[0][8])
    print(f"cond_codes_grad {N},{C},{D}: worst error / bound {WORST['cond_codes_grad']:.3f}")


# ------------------------------------------------------------------------------------------ modules: every wrapper call on tape
WRAPPERS = ("channel_scale_backward", "film_gain_backward", "gct_gate_backward", "gct_scale_backward", "cond_codes_backward", "cond_scale_backward")


class Tape:
    """records (name, args, kwargs, result) of every wrapper call of gates_train while it is open"""

    def __enter__(self):
        self.calls, self._orig = [], {n: getattr(gt, n) for n in WRAPPERS}
        for n, f in self._orig.items():
            setattr(gt, n, lambda *a, _n=n, _f=f, **k: self._note(_n, _f, a, k))
        return self

    def _note(self, name, f, a, k):
        res = f(*a, **k)
        self.calls.append((name, a, k, res))
        return res

    def __exit__(self, *exc):
        for n, f in self._orig.items():
            setattr(gt, n, f)

    def names(self):
        return [c[0] for c in self.calls]


def _planes(t):
    return _np(t).reshape(t.shape[0] * t.shape[1], -1)


def hold_call(name, a, k, res):
    """one recorded wrapper call against its float64 reference at the tensors it received"""
    if name == "channel_scale_backward":
        gy, x, gain = a[0], a[1], a[2]
        P = gy.shape[0] * gy.shape[1]
        ref = ggb.channel_scale_grad_ref(_planes(gy), _planes(x) if x is not None else np.zeros_like(_planes(gy)),
                                         _np(gain).reshape(-1) if gain is not None else np.ones(P, f32))
        if res[0] is not None:
            held("channel_scale_grad", res[0].reshape(P, -1), ref[0], "grad_x")
        if res[1] is not None:
            held("channel_scale_grad", res[1].reshape(P), ref[1], "dgain")
    elif name == "film_gain_backward":
        ref = ggb.film_gain_grad_ref(*(_np(t) for t in a[:4]))
        for g, r, n in zip(res, ref, ("grad_head", "grad_weight", "grad_bias")):
            if g is not None:
                held("film_gain_grad", g, r, n)
    elif name == "gct_gate_backward":
        ref = ggb.gct_gate_grad_ref(_np(a[0]), _np(a[1]), _np(a[2]), _np(a[3]).reshape(-1), _np(a[4]).reshape(-1), a[6], a[7])
        for g, r, n in zip(res, ref, ("dsum", "grad_alpha", "grad_gamma", "grad_beta")):
            if g is not None:
                held("gct_gate_grad", g, r, n)
    elif name == "gct_scale_backward":
        held("gct_scale_grad", res.reshape(res.shape[0] * res.shape[1], -1),
             ggb.gct_scale_grad_ref(_planes(a[0]), _planes(a[1]), _np(a[2]).reshape(-1), _np(a[3]).reshape(-1), a[4]), "grad_x")
    elif name == "cond_codes_backward":
        dcode, gap, px, head, w1, w2, w3 = (_np(t) for t in a[:7])
        N, D = head.shape
        if gap is None:
            e = lambda *s: np.zeros(s, f32)
            gap, px, w1, w2 = e(N, 0), e(N, 0), e(0, 0), e(0, 0)
        ref = ggb.cond_codes_grad_ref(dcode, gap, px, head, w1, w2, w3)
        for g, n in zip(res, ggb.CODE_OUTS):
            if g is not None:
                held("cond_codes_grad", g, ref[n], n)
    elif name == "cond_scale_backward":
        gy, gain, scores, thr, dgap, dpx = a[:6]
        N, C = res.shape[:2]
        want, tol = ggb.cond_scale_grad_ref(_np(gy).reshape(N, C, -1) if gy is not None else None, _np(gain), _np(scores), _np(thr), _np(dgap), _np(dpx))
        held("cond_scale_grad", res.reshape(N, C, -1), (want, tol), "grad_x")
        bad, _ = ggb.cond_scale_grad_ref(_np(gy).reshape(N, C, -1) if gy is not None else None, _np(gain), _np(scores), _np(thr), _np(dgap), _np(dpx), slip=True)
        if dgap is not None and float(dgap.abs().min()) > 0:
            assert ((bad - want).abs() > tol).any(), "cond_scale_grad: >= in the mask stays inside the bound"


def FROM(call, out=None):
    """in a wiring list: this argument IS (the same object as) output `out` of taped call `call`"""
    return ("from", call, out)


def wired(tape, *specs):
    """The wiring of a backward, read off the tape: per taped call the leading positional arguments it must have received -- a tensor (equal
    element for element: a module input, the cotangent, a parameter, a saved forward tensor recomputed here through the mirror's own ops
    calls), FROM(...) (the very tensor an earlier stage returned), None, or a plain value (mode, l1, eps).  With each stage held to its
    float64 reference at the tensors it received (hold_call) and the saved forward tensors held to their float64 values, this pins the
    gradients a module returns to the reference's."""
    assert len(tape.calls) == len(specs)
    for (name, a, _, _), spec in zip(tape.calls, specs):
        for pos, want in enumerate(spec):
            got, where = a[pos], f"{name}, argument {pos}"
            if isinstance(want, tuple) and len(want) == 3 and want[0] == "from":
                src = tape.calls[want[1]][3]
                src = src if want[2] is None else src[want[2]]          # autograd may hand a stage's result on in a new tensor object over the same memory
                assert got is src or (got.data_ptr() == src.data_ptr() and got.shape == src.shape), where + ": not the tensor the earlier stage returned"
            elif want is None:
                assert got is None, where + ": expected None"
            elif torch.is_tensor(want):
                assert torch.is_tensor(got) and got.numel() == want.numel() and torch.equal(got.reshape(want.shape), want), where + ": another tensor"
            else:
                assert not torch.is_tensor(got) and got == want and type(got) is type(want), f"{where}: {got!r}, expected {want!r}"


def hold_forward(entry, got, want_tol, what):
    """a tensor the forward saved against its float64 value (the forward kernels' own bounds, tests/float64_bounds.py)"""
    want, tol = want_tol
    r = ggb.check(_np(got), want, tol, what)
    assert r <= 1.0, f"{what}: the saved {entry} is off its float64 value, error / bound {r:.3f}"


def film_gain_ref(head, weight, bias):
    """aoc_film_gain, the bound of tests/test_gpu_stream_kernels.py::test_film_gain"""
    h, w, b = ggb.t64(head), ggb.t64(weight), ggb.t64(bias)
    return 1.0 + torch.tanh(h @ w.t() + b), fb.gamma(-(-h.shape[1] // 64) + 7) * (h.abs() @ w.abs().t() + b.abs()) + 4 * fb.U


def backward_twice(module, inputs, grad_y, expect):
    """forward + backward of `module` twice on fresh leaves -> (leaves, parameter gradients) of the first run; checks the bits of the second,
    the wrapper calls of the first against their references and the order of those calls."""
    runs = []
    for rep in range(2):
        for p in module.parameters():
            p.grad = None
        leaves = [t.clone().requires_grad_(r) for t, r in inputs]
        with Tape() as tape, torch.enable_grad():
            y = module(*leaves)
            y.backward(grad_y)
        if rep == 0:
            assert tape.names() == list(expect), f"{type(module).__name__}: backward chain {tape.names()}"
            for c in tape.calls:
                hold_call(*c)
        runs.append((y.detach(), [l.grad for l in leaves], {n: (p.grad.clone() if p.grad is not None else None) for n, p in module.named_parameters()}))
    eq = lambda u, v: (u is None and v is None) or torch.equal(u, v)
    assert eq(runs[0][0], runs[1][0]) and all(eq(u, v) for u, v in zip(runs[0][1], runs[1][1])) and all(eq(runs[0][2][n], runs[1][2][n]) for n in runs[0][2]), \
        "two runs differ"
    return runs[0], tape


def same_forward(twin, mirror, *inputs):
    """the twin's forward with a graph against the mirror under no_grad, bit for bit"""
    mirror.load_state_dict(twin.state_dict())
    with torch.enable_grad():
        y = twin(*inputs)
    assert y.requires_grad and y.grad_fn is not None
    with torch.no_grad():
        ym = mirror.to(DEV)(*inputs)
        yt = twin(*inputs)
    assert torch.equal(y.detach(), ym) and torch.equal(yt, ym) and not yt.requires_grad, "the forward is not the mirror's"


IA_CASES = ((1, 1, 1, 1, 1), (2, 5, 7, 3, 3), (3, 164, 400, 5, 7), (30, 4, 1025, 3, 3), (2, 3, 5, 1, 257), (2, 3, 5, 3, 341), (2, 3, 5, 32, 32))


@pytest.mark.parametrize("O,c,D,h,w", IA_CASES)
def test_ia_gate_backward(O, c, D, h, w):
    rs = ggb.rng(O, c, D, h, w, 6)
    torch.manual_seed(O * 1000 + c)
    m = gt.IA_gate(D, c).to(DEV)
    x, head, gy = dev(rs.standard_normal((O, c, h, w)).astype(f32)), dev(rs.standard_normal((O, D)).astype(f32)), dev(rs.standard_normal((O, c, h, w)).astype(f32))
    same_forward(m, attention.IA_gate(D, c), x, head)
    chain = ("channel_scale_backward", "film_gain_backward")
    (y, (gx, gh), pg), tape = backward_twice(m, ((x, True), (head, True)), gy, chain)
    last = tape.calls
    assert torch.equal(gx, last[0][3][0]) and torch.equal(gh, last[1][3][0]) and torch.equal(pg["IA.weight"], last[1][3][1]) and torch.equal(pg["IA.bias"], last[1][3][2])
    W, b = m.IA.weight.detach(), m.IA.bias.detach()
    gain = ops.film_gain(head, W, b)
    hold_forward("gain", gain, film_gain_ref(head, W, b), "IA_gate")
    wired(tape, (gy, x, gain), (FROM(0, 1), gain, head, W))
    # x without a gradient while the parameters have one; a frozen bias; everything frozen but x
    (_, (gx2, gh2), pg2), t2 = backward_twice(m, ((x, False), (head, False)), gy, chain)
    assert gx2 is None and gh2 is None and t2.calls[0][3][0] is None and torch.equal(pg2["IA.weight"], pg["IA.weight"])
    wired(t2, (gy, x, gain), (FROM(0, 1), gain, head, W))
    m.IA.bias.requires_grad_(False)
    (_, _, pg3), t3 = backward_twice(m, ((x, True), (head, True)), gy, chain)
    assert pg3["IA.bias"] is None and t3.calls[1][3][2] is None and torch.equal(pg3["IA.weight"], pg["IA.weight"])
    m.requires_grad_(False)
    (_, (gx4, gh4), _), t4 = backward_twice(m, ((x, True), (head, False)), gy, ("channel_scale_backward",))
    assert torch.equal(gx4, gx) and gh4 is None and t4.calls[0][3][1] is None
    wired(t4, (gy, None, gain))
    print(f"IA_gate {O},{c},{D},{h}x{w}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def test_ia_gate_unaligned_view_and_saturated_gains():
    O, c, D, h, w = 2, 6, 5, 5, 7
    rs = ggb.rng(7)
    m = gt.IA_gate(D, c).to(DEV)
    with torch.no_grad():
        m.IA.bias[0], m.IA.bias[1] = 60.0, -60.0                              # tanhf saturates: gains exactly 2.0 and 0.0
    x, gy = (shifted(rs.standard_normal((O, c, h, w)).astype(f32), 1) for _ in range(2))   # contiguous views one float off the 16-byte grid
    head = dev((0.1 * rs.standard_normal((O, D))).astype(f32))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    same_forward(m, attention.IA_gate(D, c), x, head)
    (y, (gx, gh), pg), tape = backward_twice(m, ((x, True), (head, True)), gy, ("channel_scale_backward", "film_gain_backward"))
    gain = tape.calls[0][1][2]
    assert (gain[:, 0] == 2.0).all() and (gain[:, 1] == 0.0).all()
    wired(tape, (gy, x, ops.film_gain(head, m.IA.weight.detach(), m.IA.bias.detach())), (FROM(0, 1), gain, head, m.IA.weight.detach()))
    assert float(pg["IA.weight"][:2].abs().max()) == 0.0 and float(pg["IA.bias"][:2].abs().max()) == 0.0, "a saturated channel has a parameter gradient"
    dgain = tape.calls[1][1][0].clone()
    dgain[:, :2] = 0.0                                                          # ... and contributes exactly zero to grad_head
    assert torch.equal(gt.film_gain_backward(dgain, gain, head, m.IA.weight.detach())[0], gh)
    assert torch.equal(y[:, 1], torch.zeros_like(y[:, 1])) and torch.equal(gx[:, 1], torch.zeros_like(gx[:, 1]))


GCT_CASES = (("l2", False, 1, 1, 1, 1), ("l2", False, 3, 5, 5, 7), ("l2", False, 3, 300, 5, 7), ("l2", False, 1, 640, 31, 33), ("l1", False, 3, 5, 5, 7),
             ("l1", False, 1, 300, 1, 1), ("l1", True, 3, 640, 5, 7), ("l1", True, 3, 5, 31, 33))


@pytest.mark.parametrize("mode,after_relu,N,C,h,w", GCT_CASES)
def test_gct_backward(mode, after_relu, N, C, h, w):
    rs = ggb.rng(N, C, h, w, 8)
    m = gt.GCT(C, mode=mode, after_relu=after_relu).to(DEV)
    x = rs.standard_normal((N, C, h, w)).astype(f32)
    if after_relu:
        x = np.maximum(x, 0)
    if N * C > 1:
        x[0, 0] = 0.0                                                          # an all-zero plane
    x, gy = dev(x), dev(rs.standard_normal((N, C, h, w)).astype(f32))
    chain = ("channel_scale_backward", "gct_gate_backward", "gct_scale_backward")
    # the constructor's state, where training starts: the gate is exactly 1 and gamma still gets a gradient
    same_forward(m, gct.GCT(C, mode=mode, after_relu=after_relu), x)
    (y, (gx,), pg), tape = backward_twice(m, ((x, True),), gy, chain)
    assert torch.equal(y, x) and (tape.calls[1][1][1] == 1.0).all(), "gamma = beta = 0: the gate is not exactly 1"
    assert float(pg["gamma"].abs().max()) > 0 and torch.isfinite(gx).all() and all(torch.isfinite(g).all() for g in pg.values())
    with torch.no_grad():
        m.alpha.copy_(dev(rs.uniform(0.5, 1.5, (1, C, 1, 1)).astype(f32)))
        m.gamma.copy_(dev(rs.standard_normal((1, C, 1, 1)).astype(f32)))
        m.beta.copy_(dev((0.5 * rs.standard_normal((1, C, 1, 1))).astype(f32)))
    same_forward(m, gct.GCT(C, mode=mode, after_relu=after_relu), x)
    (y, (gx,), pg), tape = backward_twice(m, ((x, True),), gy, chain)
    assert torch.isfinite(gx).all() and all(torch.isfinite(g).all() and g.shape == (1, C, 1, 1) for g in pg.values())
    assert torch.equal(gx, tape.calls[2][3]) and torch.equal(pg["alpha"].reshape(-1), tape.calls[1][3][1])
    assert torch.equal(pg["gamma"].reshape(-1), tape.calls[1][3][2]) and torch.equal(pg["beta"].reshape(-1), tape.calls[1][3][3])
    reduce_mode, l1 = ggb.gct_mode(mode, after_relu)
    al, ga, be = m.alpha.detach(), m.gamma.detach(), m.beta.detach()
    sums = ops.plane_reduce(x, reduce_mode)
    gate = ops.gct_gate(sums, al, ga, be, m.epsilon, l1)
    hold_forward("plane sums", sums, fb.plane_reduce_ref(ggb.t64(x).reshape(N, C, -1), reduce_mode), f"GCT {mode}")
    hold_forward("gate", gate, fb.gct_gate_ref(ggb.t64(sums), *(ggb.t64(t).reshape(1, -1) for t in (al, ga, be)), m.epsilon, l1), f"GCT {mode}")
    wired(tape, (gy, x, None), (FROM(0, 1), gate, sums, al, ga, be, m.epsilon, l1), (gy, x, gate, FROM(1, 0), reduce_mode))
    if mode == "l1" and not after_relu and N * C > 1:
        assert torch.equal(gx[0, 0], gy[0, 0] * tape.calls[1][1][1][0, 0]), "sign(0) = 0: the zero plane's gradient is grad_y * gate alone"
    # the whole chain against float64 autograd's own answer is what tests/test_gates_grad_host.py holds the references to
    m.gamma.requires_grad_(False)
    (_, (gx2,), pg2), t2 = backward_twice(m, ((x, False),), gy, chain[:2])
    assert gx2 is None and pg2["gamma"] is None and t2.calls[1][3][0] is None and torch.equal(pg2["alpha"], pg["alpha"])
    wired(t2, (gy, x, None), (FROM(0, 1), gate, sums, al, ga, be, m.epsilon, l1))
    print(f"GCT {mode} {N},{C},{h}x{w}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _block(s, D):
    N, C = s["x"].shape[:2]
    m = gt.conditioning_block(C, D, s["beta"])
    p = s["p"]
    with torch.no_grad():
        m.CL_1.phi_layer.weight.copy_(torch.from_numpy(p["phi_w"]).view(1, C, 1, 1))
        m.CL_1.phi_layer.bias.copy_(torch.from_numpy(p["phi_b"]))
        for layer, (wk, bk) in ((m.CL_1.mlp_layer, ("w1", "b1")), (m.CL_2.mlp_layer, ("w2", "b2")), (m.CL_3.mlp_layer, ("w3", "b3")), (m.mlp_layer, ("wm", "bm"))):
            layer.weight.copy_(torch.from_numpy(p[wk]))
            layer.bias.copy_(torch.from_numpy(p[bk]))
    return m.to(DEV)


def _hold_mask(s, scores, thr):
    """the mask the kernels drew against the float64 scores, outside the pixels a float32 evaluation may decide either way"""
    N, C = s["x"].shape[:2]
    k = s["k_rank"]
    mask = _np(scores) > _np(thr)[:, None]
    if s["kind"] == "constant":
        assert not mask.any(), "constant planes: every score ties, the mask is empty"
        return
    assert (mask.sum(1) == k - 1).all(), "strict >: the pixels above the k-th largest score"
    if s["kind"] == "tie":
        sc = np.take_along_axis(_np(scores), s["tied"], 1)
        assert (sc[:, 0] == sc[:, 1]).all() and (sc[:, 0] == _np(thr)).all() and not np.take_along_axis(mask, s["tied"], 1).any(), "the strict > keeps a tied pixel"
        return
    _, _, mask64, near = ggb.mask_undecided(s["x"].reshape(N, C, -1), s["p"], k)
    assert float(near.double().mean(1).max()) <= ggb.MASK_CAP
    assert ((torch.from_numpy(mask) == mask64) | near).all(), "the mask differs from the float64 scores' where the float32 scores decide"


@pytest.mark.parametrize("case", ggb.COND_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conditioning_block_backward(case):
    s = ggb.cond_case(*case)
    N, C, D = case[:3]
    m = _block(s, D)
    x, head, gy = dev(s["x"]), dev(s["head"]), dev(s["grad_y"])
    same_forward(m, cl.conditioning_block(C, D, s["beta"]), x, head)
    chain = ("channel_scale_backward", "film_gain_backward", "cond_codes_backward", "cond_scale_backward")
    (y, (gx, gh), pg), tape = backward_twice(m, ((x, True), (head, True)), gy, chain)
    for i in (1, 2, 3):
        assert pg[f"CL_{i}.phi_layer.weight"] is None and pg[f"CL_{i}.phi_layer.bias"] is None, "phi_layer got a gradient (CLB:36 compares)"
    codes, apply = tape.calls[2][3], tape.calls[3]
    assert torch.equal(gx, apply[3]) and torch.equal(gh, codes[2]) and torch.equal(pg["CL_2.mlp_layer.weight"], codes[5])
    assert torch.equal(pg["mlp_layer.weight"], tape.calls[1][3][1]) and torch.equal(pg["CL_3.mlp_layer.bias"], codes[8])
    _hold_mask(s, apply[1][2], apply[1][3])
    # the wiring: the forward's saved tensors are what the mirror's own calls give at the module's inputs, each held to its float64 value
    prm = {k: dev(v) for k, v in s["p"].items()}
    gap, scores, thr, px = ops.cond_gate_pool(x, prm["phi_w"], prm["phi_b"], s["k_rank"], want_debug=True, want_plane_mean=True)
    code = ops.cond_codes(gap, px, head, *(prm[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3")))
    gain = ops.film_gain(code, prm["wm"], prm["bm"])
    z64 = ggb.t64(x).reshape(N, C, -1)
    hold_forward("gap", gap, fb.cond_gap_ref(z64, ggb.t64(scores) > ggb.t64(thr)[:, None]), "conditioning_block")
    hold_forward("plane means", px, fb.cond_plane_mean_ref(z64), "conditioning_block")
    hold_forward("code", code, fb.cond_codes_ref(ggb.t64(gap), ggb.t64(px), ggb.t64(head), *(ggb.t64(s["p"][k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3"))),
                 "conditioning_block")
    hold_forward("gain", gain, film_gain_ref(code, prm["wm"], prm["bm"]), "conditioning_block")
    wired(tape, (gy, x, None), (FROM(0, 1), gain, code, prm["wm"]), (FROM(1, 0), gap, px, head, prm["w1"], prm["w2"], prm["w3"]),
          (gy, gain, scores, thr, FROM(2, 0), FROM(2, 1)))
    for name, g in (("CL_1.mlp_layer.weight", codes[3]), ("CL_1.mlp_layer.bias", codes[4]), ("CL_2.mlp_layer.bias", codes[6]), ("CL_3.mlp_layer.weight", codes[7]),
                    ("mlp_layer.bias", tape.calls[1][3][2])):
        assert torch.equal(pg[name], g), name + ": not the gradient its stage returned"
    if N == 1:
        assert float(codes[1].abs().max()) == 0.0, "N = 1: the dpx term is not exactly 0"
    if s["kind"] == "constant" or s["k_rank"] == 1:
        gap = tape.calls[2][1][1]
        assert float(gap.abs().max()) == 0.0, "an empty mask: gap = 0"
        no_gap = gt.cond_scale_backward(apply[1][0], apply[1][1], apply[1][2], apply[1][3], None, apply[1][5])
        assert torch.equal(no_gap, gx), "an empty mask: dgap reaches a pixel"
    # frozen parameters, x without a gradient: only what is asked for is computed
    m.requires_grad_(False)
    m.mlp_layer.bias.requires_grad_(True)
    (_, (gx2, gh2), pg2), t2 = backward_twice(m, ((x, False), (head, False)), gy, chain[:2])
    assert gx2 is None and gh2 is None and t2.calls[1][3][0] is None and t2.calls[1][3][1] is None and torch.equal(pg2["mlp_layer.bias"], pg["mlp_layer.bias"])
    wired(t2, (gy, x, None), (FROM(0, 1), gain, code, prm["wm"]))
    print(f"conditioning_block {case}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("case", ggb.COND_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conditioning_layer_backward(case):
    s = ggb.cond_case(*case)
    N, C = case[:2]
    blk = _block(s, case[2])
    m = gt.conditioning_layer(C, s["beta"]).to(DEV)
    m.load_state_dict(blk.CL_1.state_dict())
    x, gy = dev(s["x"]), dev(ggb.rng(9).standard_normal((N, C)).astype(f32))
    same_forward(m, cl.conditioning_layer(C, s["beta"]), x)
    (y, (gx,), pg), tape = backward_twice(m, ((x, True),), gy, ("cond_codes_backward", "cond_scale_backward"))
    assert pg["phi_layer.weight"] is None and pg["phi_layer.bias"] is None
    assert torch.equal(gx, tape.calls[1][3]) and tape.calls[1][1][0] is None and tape.calls[1][1][5] is None, "conditioning_layer's own backward: dpx = NULL"
    _hold_mask(s, tape.calls[1][1][2], tape.calls[1][1][3])
    w1 = m.mlp_layer.weight.detach()
    gap, scores, thr = ops.cond_gate_pool(x, dev(s["p"]["phi_w"]), dev(s["p"]["phi_b"]), s["k_rank"], want_debug=True)
    hold_forward("gap", gap, fb.cond_gap_ref(ggb.t64(x).reshape(N, C, -1), ggb.t64(scores) > ggb.t64(thr)[:, None]), "conditioning_layer")
    wired(tape, (gy, None, None, gap, None, None, w1), (None, None, scores, thr, FROM(0, 2), None))
    assert tape.calls[1][2]["shape"] == tuple(x.shape)
    assert torch.equal(pg["mlp_layer.weight"], tape.calls[0][3][7]) and torch.equal(pg["mlp_layer.bias"], tape.calls[0][3][8])
    if s["kind"] == "constant" or s["k_rank"] == 1:
        assert float(gx.abs().max()) == 0.0, "an empty mask: dgap reaches a pixel"
    # the vector form: one linear
    v = dev(s["x"].reshape(N, C, -1)[:, :, 0].copy())
    same_forward(m, cl.conditioning_layer(C, s["beta"]), v)
    (_, (gv,), pv), tv = backward_twice(m, ((v, True),), gy, ("cond_codes_backward",))
    assert torch.equal(gv, tv.calls[0][3][2]) and torch.equal(pv["mlp_layer.weight"], tv.calls[0][3][7]) and torch.equal(pv["mlp_layer.bias"], tv.calls[0][3][8])
    wired(tv, (gy, None, None, v, None, None, w1))
    print(f"conditioning_layer {case}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def test_cond_scale_grad_direct():
    """the sixth entry through its wrapper with a caller's output in NaN margins, aligned and one float off"""
    s = ggb.cond_case(3, 5, 4, 9, 11, 0.3, 21)
    N, C, hw = 3, 5, 99
    x = dev(s["x"])
    gap, scores, thr = ops.cond_gate_pool(x, dev(s["p"]["phi_w"]), dev(s["p"]["phi_b"]), s["k_rank"], want_debug=True)
    rs = ggb.rng(22)
    gain, dgap, dpx = (rs.standard_normal((N, C)).astype(f32) for _ in range(3))
    gy = s["grad_y"]
    for args in ((gy, gain, dgap, dpx), (gy, gain, dgap, None), (gy, gain, None, None), (None, None, dgap, None)):
        gy3 = args[0].reshape(N, C, hw) if args[0] is not None else None
        want, tol = ggb.cond_scale_grad_ref(gy3, args[1], _np(scores), _np(thr), args[2], args[3])
        slip = ggb.cond_scale_grad_ref(gy3, args[1], _np(scores), _np(thr), args[2], args[3], slip=True)[0] if args[2] is not None else want + 1
        for off in (0, 1):
            runs = []
            for _ in range(2):
                buf, out = margins((N, C, 9, 11), off)
                a = [shifted(t, off) if t is not None and t.ndim == 4 else (dev(t) if t is not None else None) for t in args]
                got = gt.cond_scale_backward(a[0], a[1], scores, thr, a[2], a[3], shape=(N, C, 9, 11), grad_x=out)
                assert got is out and untouched(buf, (N, C, 9, 11), off), "written outside grad_x"
                runs.append(out.clone())
            assert torch.equal(runs[0], runs[1]), "two runs differ"
            _check_bound(_np(runs[0]).reshape(N, C, hw), want, tol, slip, f"cond_scale_grad off={off}")
            held("cond_scale_grad", runs[0].reshape(N, C, hw), (want, tol), "grad_x")
    print(f"cond_scale_grad: worst error / bound {WORST['cond_scale_grad']:.3f}")


def test_beta_rank_below_one_raises_as_the_mirror_does():
    x = torch.randn(2, 4, 1, 2, device=DEV, requires_grad=True)
    head = torch.randn(2, 6, device=DEV)
    for twin, mirror, args in ((gt.conditioning_layer(4), cl.conditioning_layer(4), (x,)), (gt.conditioning_block(4, 6), cl.conditioning_block(4, 6), (x, head))):
        with torch.enable_grad(), pytest.raises(IndexError, match="beta_rank == 0"):
            twin.to(DEV)(*args)
        with torch.no_grad(), pytest.raises(IndexError, match="beta_rank == 0"):
            mirror.to(DEV)(*args)


def test_double_backward_raises():
    m = gt.IA_gate(5, 3).to(DEV)
    x = torch.randn(2, 3, 4, 4, device=DEV, requires_grad=True)
    with torch.enable_grad():
        y = m(x, torch.randn(2, 5, device=DEV))
        g, = torch.autograd.grad((y * y).sum(), x, create_graph=True)       # the cotangent 2 y carries a graph into the backward
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()


def test_conditioning_block_peak_memory():
    N, C, D, h, w = 4, 100, 400, 31, 33
    s = ggb.cond_case(N, C, D, h, w, 0.3, 31)
    m = _block(s, D)
    x, head, gy = dev(s["x"]).requires_grad_(True), dev(s["head"]).requires_grad_(True), dev(s["grad_y"])

    def run():
        with torch.enable_grad():
            y = m(x, head)
            y.backward(gy)
        return y.detach()
    run()                                                                      # warm-up: library and allocator
    x.grad = head.grad = None
    for p in m.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    hw, code = h * w, 2 * C + D
    output = N * C * hw * 4
    saved = (N * hw + N + 4 * N * C + N * code) * 4                            # scores, threshold, gap, px, gain, dgain's twin; the code
    grads = N * C * hw * 4 + (N * D + 2 * (C * C + C) + D * D + D + C * code + C) * 4
    work = _lib.lib().aoc_cond_gate_pool_workspace_bytes(N, C, hw) + (N * C + N * code + 2 * N * C) * 4      # the pool's workspace; dgain, dcode, dgap, dpx
    budget = output + saved + grads + work
    print(f"conditioning_block {N},{C},{D},{h}x{w}: peak {peak} bytes above the inputs, output + saved + gradients + workspaces {budget}")
    assert peak < 2 * budget, f"peak {peak} bytes, twice the accounted tensors is {2 * budget}"
    del y
