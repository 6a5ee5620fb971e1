"""The differentiable DynamicPreHead on the device: aoc_prehead_grad through its wrapper and the twin of aoc_amd.prehead_train through
``backward()``, against the float64 reference and derived bounds of tests/prehead_grad_bounds.py.  No element is excluded from a comparison:
every case and seed here has no element near the ReLU's corner (tests/test_prehead_grad_host.py asserts it).  Each test prints its largest
error / bound per output before it asserts."""
import numpy as np
import pytest
import torch

import aoc_amd
import float64_bounds as fb
import prehead_grad_bounds as pgb
from aoc_amd import _lib, frontend_train as ft, hotpath, ops, prehead_train as pt
from conftest import load_golden
from test_gpu_gates_grad import DEV, dev, margins, shifted, untouched, _np

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
INVALID, WORKSPACE, UNSUPPORTED = "AOC_ERR_INVALID_ARG", "AOC_ERR_WORKSPACE", "AOC_ERR_UNSUPPORTED"
WORST = {}


def held(entry, got, want_tol, what):
    want, tol = want_tol
    r = pgb.check(_np(got), want, tol, what)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    print(f"{what}: error / bound {r:.3f}")
    assert r <= 1.0, f"{what}: error / bound {r:.3f}"
    return r


def worst(prefix):
    return ", ".join(f"{k[len(prefix):]} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith(prefix))


def on_device(s, key, off):
    """one case on the device, every buffer `off` floats past a 16-byte boundary: the forward through prehead_forward, then the positional
    arguments of prehead_backward (the statistics copied out of the forward's workspace to that misalignment too) and the forward's output"""
    O, n_in, n_out, groups, hw, C = key
    feat = shifted(s["feat"].reshape(O, n_in, hw, 1), off)
    w, b, gw, gb = (shifted(s[k], off) for k in ("weight", "bias", "gn_w", "gn_b"))
    emb = shifted(s["emb"].reshape(hw, 1, C), off) if C else None
    out, stats = pt.prehead_forward(feat, w, b, groups, gw, gb, 1e-5, emb)
    go = shifted(s["grad_out"].reshape(O, C + n_out, hw, 1), off)
    return [go, feat, shifted(_np(stats), off), w, b, groups, gw, gb, C], out


def out_shapes(key):
    O, n_in, n_out, groups, hw, C = key
    sh = {"grad_feat": (O, n_in, hw, 1), "grad_weight": (n_out, n_in), "grad_bias": (n_out,), "grad_gamma": (n_out,), "grad_beta": (n_out,)}
    if C:
        sh["grad_emb"] = (hw, 1, C)
    return sh


# ------------------------------------------------------------------------------------------ 1 the entry through its wrapper
@pytest.mark.parametrize("key", tuple(pgb.CASES))
def test_prehead_grad(key):
    O, n_in, n_out, groups, hw, C = key
    s = pgb.case(*key, pgb.CASES[key])
    ref, und = pgb.prehead_grad_ref(**pgb.ref_args(s, groups, C))
    assert int(und.sum()) == 0
    fwd = fb.prehead_ref(*(pgb.t64(s[k]) for k in ("feat", "weight", "bias")), groups, pgb.t64(s["gn_w"]), pgb.t64(s["gn_b"]), 1e-5)
    shapes = out_shapes(key)
    names = tuple(shapes)
    for off in (0, 1):
        args, out = on_device(s, key, off)
        what = f"prehead_grad {key} off={off}"
        held("fwd out", out[:, C:, :, 0], fwd, f"{what}: the forward's output")
        if C:
            assert torch.equal(out[:, :C, :, 0], dev(s["emb"]).t().unsqueeze(0).expand(O, C, hw)), "the embedding channels are copies"
        runs = []
        for _ in range(2):
            bufs = {k: margins(shape, off) for k, shape in shapes.items()}
            got = pt.prehead_backward(*args, want=tuple(k in shapes for k in pgb.OUTS), out={k: v for k, (_, v) in bufs.items()})
            assert all((g is bufs[k][1]) if k in bufs else g is None for g, k in zip(got, pgb.OUTS)), "the caller's buffers are returned"
            assert all(untouched(bufs[k][0], shapes[k], off) for k in shapes), "written outside the outputs"
            runs.append({k: g.clone() for g, k in zip(got, pgb.OUTS) if g is not None})
        for name in names:
            a, b = runs[0][name], runs[1][name]
            assert not bool(torch.isnan(a).any()), f"{what} {name}: an element was not written"
            assert torch.equal(a, b), f"{what} {name}: two runs differ"
            held("entry " + name, a, ref[name], f"{what} {name}")
            alone = pt.prehead_backward(*args, want=tuple(k == name for k in pgb.OUTS))                # each output alone: the same bits
            assert all((g is None) == (k != name) for g, k in zip(alone, pgb.OUTS)), f"{what}: asked for {name} alone"
            assert torch.equal(alone[pgb.OUTS.index(name)], a), f"{what}: {name} alone differs"
    print(f"prehead_grad {key}: worst error / bound so far: {worst('entry ')}; forward {WORST['fwd out']:.3f}")


# ------------------------------------------------------------------------------------------ 2 the mask is the forward's, bit for bit
@pytest.mark.parametrize("key", tuple(pgb.MASK_CASES))
def test_mask_identity(key):
    """With a cotangent of 1 on the pre-head's channels grad_beta[c] is the number of active elements of channel c: an integer, summed in
    double, equal to the count of out[:, C + c] > 0 in the forward's own output.  24, 26, 28 and a generic channel count."""
    O, n_in, n_out, groups, hw, C = key
    s = pgb.case(*key, pgb.MASK_CASES[key])
    s["grad_out"][:, C:] = 1.0
    for off in (0, 1):
        args, out = on_device(s, key, off)
        gb = pt.prehead_backward(*args, want=(False, False, False, False, True, False))[4]
        count = (out[:, C:] > 0).sum((0, 2, 3))
        assert torch.equal(gb.double(), count.double()), f"{key}: grad_beta is not the forward's own count on {int((gb.double() != count.double()).sum())} channels"
        assert 0 < int(count.sum()) < O * n_out * hw
    print(f"mask identity {key}: {int(count.sum())} of {O * n_out * hw} elements active, the counts equal")


# ------------------------------------------------------------------------------------------ 3 planted
def test_planted():
    """An object whose cotangent is all zero; channels that are never active (beta = -100): a whole group (0 .. 3), whose dy is then exactly 0,
    and channel 6 alone, whose dy is what its group's other channels leave (-rstd (c1 + xhat c2)): its grad_gamma and grad_beta are exactly 0
    and its grad_weight row is held to the reference like every other; gamma = 0 on channel 9."""
    key = pgb.PLANTED
    O, n_in, n_out, groups, hw, C = key
    s = pgb.planted_case()
    ref, und = pgb.prehead_grad_ref(**pgb.ref_args(s, groups, C))
    assert int(und.sum()) == 0
    args, out = on_device(s, key, 0)
    got = dict(zip(pgb.OUTS, pt.prehead_backward(*args)))
    for name in pgb.OUTS:
        held("planted " + name, got[name], ref[name], "planted " + name)
    assert float(got["grad_feat"][1].abs().max()) == 0.0, "an all-zero cotangent: grad_feat of that object is exactly 0"
    assert float(got["grad_feat"][0].abs().max()) > 0.0
    dead = [0, 1, 2, 3, 6]
    assert float(out[:, [C + c for c in dead]].abs().max()) == 0.0, "beta = -100: never active"
    assert float(got["grad_gamma"][dead].abs().max()) == 0.0 and float(got["grad_beta"][dead].abs().max()) == 0.0
    assert float(ref["grad_weight"][1][:4].max()) == 0.0 and float(got["grad_weight"][:4].abs().max()) == 0.0, "a dead group: the bound of 0 is 0"
    assert float(got["grad_bias"][:4].abs().max()) == 0.0
    assert bool(torch.isfinite(got["grad_feat"]).all())
    # one element per group (hw = 1, group size 1): xhat = 0 and gamma dz - c1 = 0, so grad_feat stays within the bound of 0
    key1 = (3, 32, 128, 128, 1, 100)
    s1 = pgb.case(*key1, pgb.CASES[key1])
    ref1, _ = pgb.prehead_grad_ref(**pgb.ref_args(s1, 128, 100))
    args1, _ = on_device(s1, key1, 0)
    gf = pt.prehead_backward(*args1, want=(True,) + (False,) * 5)[0]
    want, tol = ref1["grad_feat"]
    assert float(want.abs().max()) <= 1e-9 and bool((pgb.t64(gf).reshape(want.shape).abs() <= tol).all()), "one element per group: within the bound of 0"
    print(f"planted: {worst('planted ')}; one element per group: |grad_feat| <= {float(pgb.t64(gf).abs().max()):.3e} (bound {float(tol.max()):.3e})")


# ------------------------------------------------------------------------------------------ 4 rejections
def test_rejections():
    key = (2, 24, 64, 16, 35, 3)
    O, n_in, n_out, groups, hw, C = key
    s = pgb.case(*key, 0)
    args, _ = on_device(s, key, 0)
    go, feat, stats, w, b, _, gw, gb, _ = args
    shapes = out_shapes(key)
    L = _lib.lib()
    p = ops._p

    def call(n_obj=O, n_in=n_in, n_out=n_out, groups=groups, hw=hw, C=C, ws_bytes=None, emb_out=True):
        bufs = {k: margins(shape) for k, shape in shapes.items()}
        ws = ops._ws(L.aoc_prehead_grad_workspace_bytes(O, 24, 64, 16, 35), DEV)
        o = [bufs[k][1] for k in pgb.OUTS]
        rc = L.aoc_prehead_grad(p(go), p(feat), p(stats), p(w), p(b), p(gw), p(gb), n_obj, n_in, n_out, groups, hw, C, *(p(t) for t in o[:5]),
                                p(o[5]) if emb_out else None, p(ws), ws.numel() if ws_bytes is None else ws_bytes, ops._stream())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(b_).all()) for b_, _ in bufs.values()), "a rejected call wrote something"
        return _lib.STATUS[rc]
    # the forward's limits with the forward's codes
    assert call(n_in=33) == UNSUPPORTED and call(n_out=129, groups=3) == UNSUPPORTED and call(groups=5) == UNSUPPORTED and call(n_obj=65536) == UNSUPPORTED
    assert call(hw=0) == INVALID and call(n_obj=0) == INVALID and call(C=-1) == INVALID
    assert call(C=0) == UNSUPPORTED                                           # an embedding gradient asked for without embedding channels
    assert call(ws_bytes=64) == WORKSPACE
    with pytest.raises(ValueError, match="needs C > 0"):
        pt.prehead_backward(go[:, C:].contiguous(), feat, stats, w, b, groups, gw, gb, 0, want=(True,) * 6)
    with pytest.raises(ValueError, match="do not divide"):
        pt.prehead_backward(go, feat, stats, w, b, 5, gw, gb, C)
    with pytest.raises(ValueError, match=r"is not \[O, C \+ n_out"):
        pt.prehead_backward(go, feat, stats, w, b, groups, gw, gb, C + 1)
    with pytest.raises(ValueError, match="must be a contiguous float32 tensor of shape"):
        pt.prehead_backward(go, feat, stats, w, b, groups, gw, gb, C, out={"grad_bias": torch.empty(n_out + 1, device=DEV)})
    with pytest.raises(_lib.AocHipError, match="no CPU fallback"):
        pt.prehead_backward(go.cpu(), feat, stats, w, b, groups, gw, gb, C)
    with pytest.raises(_lib.AocHipError, match=UNSUPPORTED):
        pt.prehead_backward(torch.zeros(1, 3 + 132, 4, device=DEV), torch.zeros(1, 24, 4, device=DEV), torch.zeros(33, 2, device=DEV),
                            torch.zeros(132, 24, device=DEV), torch.zeros(132, device=DEV), 33, torch.zeros(132, device=DEV), torch.zeros(132, device=DEV), 3)


# ------------------------------------------------------------------------------------------ 5 the module
def _twin(z, cls=pt.DynamicPreHead):
    m = cls(in_dim=z["in_x"].shape[1], embed_dim=z["w_conv_w"].shape[0]).to(DEV)
    m.load_state_dict({"conv.weight": dev(z["w_conv_w"]), "conv.bias": dev(z["w_conv_b"]), "bn.weight": dev(z["w_gn_w"]), "bn.bias": dev(z["w_gn_b"])}, strict=True)
    assert m.bn.num_groups == int(z["groups"]) and abs(m.bn.eps - float(z["eps"])) < 1e-12
    return m


def _run(m, z):
    for p_ in m.parameters():
        p_.grad = None
    x = dev(z["in_x"]).requires_grad_(True)
    emb = dev(z["in_emb"]).requires_grad_(True) if "in_emb" in z else None
    with torch.enable_grad():
        out = m(x, emb.permute(1, 2, 0) if emb is not None else None)
        (out * dev(z["in_weight"])).sum().backward()
    return out.detach(), x.grad, emb.grad if emb is not None else None


@pytest.mark.parametrize("name", pgb.FIXTURES)
def test_module_against_the_recorded_gradients(name):
    """backward() at the fixtures against the gradients recorded from the reference's own class in float64, inside the derived bound (the
    float64 reference function, which carries the bound, agrees with the recorded values to 1e-10: tests/test_prehead_grad_host.py)."""
    z = load_golden(name)
    args, C = pgb.fixture_args(z)
    ref, und = pgb.prehead_grad_ref(**args)
    assert int(und.sum()) == 0
    twin, mirror = _twin(z), _twin(z, hotpath.DynamicPreHead)
    x = dev(z["in_x"])
    emb_hwc = dev(z["in_emb"]).permute(1, 2, 0) if C else None
    with torch.no_grad():
        want_out = mirror(x, emb_hwc)
        assert torch.equal(twin(x, emb_hwc), want_out) and torch.equal(twin(x), mirror(x)), "no gradient wanted: the mirror's result"
    out, gx, ge = _run(twin, z)
    assert torch.equal(out, want_out), "the twin's forward has the mirror's bits"
    recorded = {"grad_feat": z["grad_x"], "grad_weight": z["grad_conv_w"], "grad_bias": z["grad_conv_b"], "grad_gamma": z["grad_gn_w"], "grad_beta": z["grad_gn_b"]}
    got = {"grad_feat": gx, "grad_weight": twin.conv.weight.grad, "grad_bias": twin.conv.bias.grad, "grad_gamma": twin.bn.weight.grad, "grad_beta": twin.bn.bias.grad}
    if C:
        recorded["grad_emb"] = z["grad_emb"].reshape(C, -1).T
        got["grad_emb"] = ge.reshape(C, -1).t()
        assert ge.shape == z["in_emb"].shape
    first = {k: v.clone() for k, v in got.items()}
    for k in got:
        want = pgb.t64(recorded[k]).reshape(ref[k][0].shape)
        held("module " + k, got[k].reshape(ref[k][0].shape), (want, ref[k][1] + 1e-10 * max(float(want.abs().max()), 1.0)), f"{name} {k}")
    # a second backward: the same bits
    _, gx2, ge2 = _run(twin, z)
    again = {"grad_feat": gx2, "grad_weight": twin.conv.weight.grad, "grad_bias": twin.conv.bias.grad, "grad_gamma": twin.bn.weight.grad, "grad_beta": twin.bn.bias.grad}
    if C:
        again["grad_emb"] = ge2.reshape(C, -1).t()
    assert all(torch.equal(first[k], again[k]) for k in first), "two backward runs differ"
    # frozen conv, then frozen bn: no gradient for the frozen ones, the same bits for the others
    for frozen, live in ((twin.conv, twin.bn), (twin.bn, twin.conv)):
        for p_ in twin.parameters():
            p_.requires_grad_(True)
        for p_ in frozen.parameters():
            p_.requires_grad_(False)
        _, gx3, _ = _run(twin, z)
        assert all(p_.grad is None for p_ in frozen.parameters()) and all(p_.grad is not None for p_ in live.parameters())
        assert torch.equal(gx3, first["grad_feat"])
        names = ("grad_gamma", "grad_beta") if live is twin.bn else ("grad_weight", "grad_bias")
        assert torch.equal(live.weight.grad, first[names[0]]) and torch.equal(live.bias.grad, first[names[1]])
    for p_ in twin.parameters():
        p_.requires_grad_(True)
    with torch.enable_grad(), pytest.raises(_lib.AocHipError, match="prehead_train.DynamicPreHead is the differentiable form"):
        mirror(x.clone().requires_grad_(True), emb_hwc)
    xg = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out = twin(xg, emb_hwc)
        g, = torch.autograd.grad((out * out).sum(), xg, create_graph=True)      # a cotangent that itself depends on the input
        with pytest.raises(RuntimeError, match="once_differentiable"):     # the gradient kernels build no graph: a double backward raises
            g.sum().backward()
    print(f"module {name}: worst error / bound so far: {worst('module ')}")


# ------------------------------------------------------------------------------------------ 6 the wiring behind the front end
@pytest.mark.parametrize("h,w", ((9, 11), (31, 33)))
def test_wiring_behind_proto_mask_features(h, w):
    """aocnet.py:141-362 as two calls: frontend_train.proto_mask_features, then the twin with ``cur.permute(1, 2, 0)``.  Four objects, C = 100,
    six radii, loss (out * weight).sum().  The front end is handed ``cur.view_as(cur)`` -- the same memory, and a backward that is the identity
    -- so that autograd keeps what the front end alone sends to the embedding: the leaf's gradient is then ONE float32 addition of that and
    of the pre-head's embedding gradient, which is demanded bit for bit, and with it the bound of the sum (the pre-head's own bound, the front
    end's device value as it is, gamma(1) of the absolute terms)."""
    C, gt_id, radii = 100, 3, (2, 4, 6, 8, 10, 12)
    O = gt_id + 1
    rs = pgb.rng(h, w, C, gt_id, 21)
    embs = [dev((0.12 * rs.standard_normal((C, h, w))).astype(f32)).requires_grad_(True) for _ in range(3)]
    labs = [dev(rs.randint(0, O, (h, w)).astype(np.int32)) for _ in range(2)]
    bg, fg = (dev((0.1 * rs.standard_normal((1, 1, 1, 1))).astype(f32)).requires_grad_(True) for _ in range(2))
    torch.manual_seed(3)
    twin = pt.DynamicPreHead(in_dim=ft.aggregate_channels(2, len(radii)), embed_dim=64).to(DEV)
    with torch.no_grad():
        twin.bn.weight.copy_(dev((1 + 0.25 * rs.standard_normal(64)).astype(f32)))
        twin.bn.bias.copy_(dev((0.5 * rs.standard_normal(64)).astype(f32)))
    weight = dev(rs.standard_normal((O, C + 64, h, w)).astype(f32))
    cur = embs[2]
    np.random.seed(1)
    with torch.enable_grad():
        cur_front = cur.view_as(cur)
        cur_hwc = cur.permute(1, 2, 0)
        cur_front.retain_grad()
        cur_hwc.retain_grad()
        feat, head = ft.proto_mask_features(embs[0], embs[1], cur_front, labs[0], labs[1], gt_id, bg, fg, radii)
        feat.retain_grad()
        out = twin(feat, cur_hwc)
        (out * weight).sum().backward()
    assert feat.shape == (O, 24, h, w) and out.shape == (O, C + 64, h, w)
    # the cotangent that reaches proto_mask_features is prehead_backward's grad_feat, bit for bit
    conv, bn = twin.conv, twin.bn
    pars = [t.detach() for t in (conv.weight, conv.bias, bn.weight, bn.bias)]
    out2, stats = pt.prehead_forward(feat.detach(), pars[0], pars[1], bn.num_groups, pars[2], pars[3], bn.eps, cur.detach().permute(1, 2, 0))
    assert torch.equal(out2, out.detach())
    gf, gw_, gb_, gg_, gbe_, ge = pt.prehead_backward(weight, feat.detach(), stats, pars[0], pars[1], bn.num_groups, pars[2], pars[3], C)
    assert torch.equal(feat.grad, gf), "the cotangent handed to the front end is not prehead_backward's grad_feat"
    assert torch.equal(conv.weight.grad.reshape(64, 24), gw_) and torch.equal(conv.bias.grad, gb_) and torch.equal(bn.weight.grad, gg_) and torch.equal(bn.bias.grad, gbe_)
    assert torch.equal(cur_hwc.grad, ge) and ge.shape == (h, w, C)
    # the pre-head's embedding gradient inside its bound
    hw = h * w
    ref, _ = pgb.prehead_grad_ref(_np(weight).reshape(O, C + 64, hw), _np(feat).reshape(O, 24, hw), *(_np(t) for t in pars[:2]), bn.num_groups,
                                  _np(pars[2]), _np(pars[3]), bn.eps, C)
    e_want, e_tol = ref["grad_emb"]
    held("wiring grad_emb", ge.reshape(hw, C), (e_want, e_tol), f"{h}x{w} the pre-head's embedding gradient")
    # the leaf: one float32 addition of the two contributions
    front = cur_front.grad
    assert front is not None and float(front.abs().max()) > 0 and float(ge.abs().max()) > 0
    assert torch.equal(cur.grad, front + ge.permute(2, 0, 1)), "cur_emb.grad is not the float32 sum of the pre-head's and the front end's contributions"
    f64_front = pgb.t64(front).reshape(C, hw).t()
    want = e_want + f64_front
    tol = e_tol + pgb.gamma(1) * (e_want.abs() + e_tol + f64_front.abs())
    held("wiring cur_emb", cur.grad.reshape(C, hw).t(), (want, tol), f"{h}x{w} cur_emb.grad")
    assert all(e.grad is not None and float(e.grad.abs().max()) > 0 for e in embs) and bg.grad is not None and fg.grad is not None


# ------------------------------------------------------------------------------------------ 7 peak memory
def test_peak_memory():
    """One forward + backward of the twin at (4, 24, 64, 16, 31 x 33, 100): at most twice the sum of the output, what is saved, the gradients
    and the workspaces (the project's rule for a training twin)."""
    O, n_in, n_out, groups, h, w, C = 4, 24, 64, 16, 31, 33, 100
    hw = h * w
    s = pgb.case(O, n_in, n_out, groups, hw, C, 0)
    twin = pt.DynamicPreHead(in_dim=n_in, embed_dim=n_out).to(DEV)
    x = dev(s["feat"].reshape(O, n_in, h, w)).requires_grad_(True)
    emb = dev(s["emb"].reshape(h, w, C)).requires_grad_(True)
    go = dev(s["grad_out"].reshape(O, C + n_out, h, w))

    def run():
        for t in [x, emb] + list(twin.parameters()):
            t.grad = None
        with torch.enable_grad():
            twin(x, emb).backward(go)
    run()                                                                          # warm-up: library and allocator
    for t in [x, emb] + list(twin.parameters()):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    L = _lib.lib()
    output = O * (C + n_out) * hw * 4
    ws_fwd = L.aoc_prehead_workspace_bytes(O, n_out, n_out // groups, hw)          # kept: the statistics are a view of it
    saved = ws_fwd                                                                 # feat and the parameters are the caller's own tensors
    grads = O * n_in * hw * 4 + hw * C * 4 + (n_out * n_in + 3 * n_out) * 4
    ws_bwd = L.aoc_prehead_grad_workspace_bytes(O, n_in, n_out, groups, hw)
    limit = 2 * (output + saved + grads + ws_fwd + ws_bwd)
    print(f"peak above the inputs {peak} bytes; output {output}, saved {saved}, gradients {grads}, workspaces {ws_fwd} + {ws_bwd}; limit {limit}")
    assert peak <= limit
    assert x.grad is not None and emb.grad.shape == (h, w, C)
