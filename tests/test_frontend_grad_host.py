"""What can be checked without a GPU about the training-time front end (aoc_amd.frontend_train, csrc/frontend_grad.hip): the stated tie and
summation rules applied to planted inputs in the numpy restatements of tests/frontend_grad_bounds.py (and that the wrong rules give other
gradients there), the restatements against torch autograd in float64, the wrappers against the address / lifetime / dtype contract of
aoc_amd.ops with the library stubbed, the no-gradient path, the argument checks of the new entry points and the module's guards."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import aoc_amd
import frontend_grad_bounds as fgb
import local_grad_bounds as lgb
import match_grad_bounds as mgb
import ops_contract_cases as occ
from aoc_amd import _lib, frontend_train as ft, ops
from conftest import load_golden
from oracle import matching as om

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4
f32, f64 = np.float32, np.float64
ERRORS = occ.ERRORS + (_lib.AocHipError,)


# ------------------------------------------------------------------------------------------ the rules on planted inputs
def test_fg2bg_rule_on_planted_ties():
    dis, go = fgb.planted_fg2bg()
    o1, c1, o2, c2 = fgb.fg2bg_winners(dis)
    # exact tie of two objects; winner tied with the runner-up (other object AND own second channel); 3+; all +inf; +inf but one; tie-free
    assert list(zip(o1, c1)) == [(0, 0), (0, 0), (0, 0), (0, 0), (1, 1), (1, 0)]
    assert list(zip(o2, c2)) == [(1, 0), (1, 0), (1, 0), (1, 0), (0, 0), (2, 0)]
    gd = fgb.fg2bg_grad_np(go, dis)
    assert gd.dtype == f32 and gd[0, 0, 0] == f32(1.25) and gd[1, 0, 0] == f32(1.5) and gd[1, 1, 4] == f32(1.75) and gd[0, 0, 4] == f32(1.0)
    assert np.count_nonzero(gd) == 2 * dis.shape[2], "exactly two entries per column receive a gradient"
    assert np.array_equal(gd.sum((0, 1)).astype(f64), np.full(6, 2.75)), "nothing is lost: the gradients of a column add up to sum_o grad_out"
    hi = fgb.fg2bg_grad_np(go, dis, highest=True)
    down = fgb.fg2bg_grad_np(go, dis, descending=True)
    for col in range(5):                                             # every tied column tells the tie rules apart; the tie-free one does not
        assert not np.array_equal(hi[:, :, col], gd[:, :, col]), f"column {col}: 'highest index wins' gives the same gradient"
    assert np.array_equal(hi[:, :, 5], gd[:, :, 5])
    assert (down != gd).any() and down[0, 0, 0] == f32(1.25 + 2.0 ** -23), "'descending o' gives the same bits"


def test_aggregate_rule_on_planted_ties():
    src, prev, gfeat = fgb.planted_aggregate()
    feat = fgb.aggregate_np(*src, prev)
    lay = fgb.channel_layout(2, 2)
    assert lay["n_ch"] == feat.shape[1] == 1 + 2 + 1 + 2 + 2 + 1 + 2 + 1 and not np.isnan(feat).any()
    assert np.array_equal(feat[:, lay["global_bg"], 0], f32([0.25, 0.25, 0.25, 0.25, 0.25])), "a tied minimum is its own runner-up"
    assert np.array_equal(feat[:, lay["global_bg"], 4], f32([-0.25, 1.0, -0.25, -0.25, -0.25]))
    g = fgb.aggregate_grad_np(gfeat, feat, 2, 2)
    assert all(a.dtype == f32 for a in g)
    assert np.array_equal(g[0][:, 0, 0], f32([1.25, 1.5, 0, 0, 0])) and np.array_equal(g[0][:, 0, 3], f32([1.25, 1.5, 0, 0, 0]))
    assert np.array_equal(g[0][:, 0, 4], f32([1.0, 1.75, 0, 0, 0]))
    assert np.array_equal(g[1], gfeat[:, lay["cluster"]:lay["cluster"] + 2]) and np.array_equal(g[4], gfeat[:, lay["lproxy"]:lay["lproxy"] + 2])
    hi = fgb.aggregate_grad_np(gfeat, feat, 2, 2, highest=True)
    down = fgb.aggregate_grad_np(gfeat, feat, 2, 2, descending=True)
    for k in (0, 3):
        for col in range(4):
            assert not np.array_equal(hi[k][:, :, col], g[k][:, :, col]), f"source {k} column {col}: 'highest index wins' gives the same gradient"
        assert (down[k] != g[k]).any(), f"source {k}: 'descending o' gives the same bits"
    # background off: a plain split of the cotangent; one object: the two gradients added
    off = fgb.aggregate_grad_np(gfeat[:, :lay["mask"] + 1], feat[:, :lay["mask"] + 1], 2, 2, background=False)
    assert np.array_equal(off[0], gfeat[:, :1]) and np.array_equal(off[3], gfeat[:, lay["local"]:lay["local"] + 2])
    one = fgb.aggregate_grad_np(gfeat[:1], fgb.aggregate_np(*[s[:1] for s in src], prev[:1]), 2, 2)
    assert np.array_equal(one[0][:, 0], gfeat[:1, lay["glob"]] + gfeat[:1, lay["global_bg"]])


# ------------------------------------------------------------------------------------------ the restatements against autograd
@pytest.mark.parametrize("O,nc", ((2, 1), (3, 2), (17, 1), (30, 3)))
def test_fg2bg_restatement_against_autograd(O, nc):
    rs = fgb.rng(O, nc, 1)
    dis = rs.standard_normal((O, nc, 35)).astype(f32)
    go = rs.standard_normal((O, 35)).astype(f32)
    d = torch.from_numpy(dis.astype(f64)).requires_grad_(True)
    out = om.foreground2background(d, O)
    assert np.array_equal(out.detach().numpy().astype(f32), fgb.fg2bg_min_np(dis))
    (out[:, 0] * torch.from_numpy(go.astype(f64))).sum().backward()
    got = fgb.fg2bg_grad_np(go, dis)
    assert np.array_equal(got != 0, d.grad.numpy() != 0), "the restatement's winners are not torch.min's"
    assert fgb.check(got, d.grad.numpy(), fgb.fg2bg_grad_tol(go, dis), f"fg2bg restatement O={O} c={nc}") <= 1.0


@pytest.mark.parametrize("O,n_cluster,n_local,background", ((1, 2, 1, True), (2, 2, 6, True), (3, 6, 2, True), (17, 2, 8, True), (30, 2, 3, True),
                                                              (3, 2, 6, False)))
def test_aggregate_restatement_against_autograd(O, n_cluster, n_local, background):
    src, prev, gfeat = fgb.aggregate_case(5, 7, O, n_cluster, n_local, 2)
    lay = fgb.channel_layout(n_cluster, n_local, background)
    gfeat = gfeat[:, :lay["n_ch"]]
    feat = fgb.aggregate_np(*src, prev, background)
    ts = [torch.from_numpy(s.astype(f64)).requires_grad_(True) for s in src]
    want = fgb.aggregate_torch(ts,torch.from_numpy(prev.astype(f64)), O, background)
    assert np.array_equal(want.detach().numpy().astype(f32), feat), "the restated forward is not the reference's concatenation"
    (want * torch.from_numpy(gfeat.astype(f64))).sum().backward()
    got = fgb.aggregate_grad_np(gfeat, feat, n_cluster, n_local, background)
    for k, (g, t, tol) in enumerate(zip(got, ts, fgb.aggregate_grad_tol(gfeat, n_cluster, n_local, background))):
        assert fgb.check(g, t.grad.numpy(), tol, f"aggregate restatement O={O} source {k}") <= 1.0


@pytest.mark.parametrize("soft,with_neg", ((False, True), (True, True), (False, False)))
def test_pool_reference_against_autograd(soft, with_neg):
    O, C, h, w, eps = 3, 4, 5, 7, 1e-5
    lab, gpos, gneg = fgb.pool_case(h, w, O, C, 3, soft=soft, empty=None if soft else 1, with_neg=with_neg)
    want, tol = fgb.pool_grad_ref(lab, gpos, gneg, eps)
    emb = torch.randn(1, C, h, w, dtype=torch.float64, requires_grad=True)
    e, l = emb.expand(O, -1, -1, -1), torch.from_numpy(lab.astype(f64)).view(O, 1, h, w)
    pos_sum = torch.sum(e * l, dim=(2, 3))                                                     # ATT:136-142
    pos = pos_sum / (torch.sum(l, dim=(2, 3)) + fgb.eps32(eps))
    neg = (torch.sum(e, dim=(2, 3)) - pos_sum) / (torch.sum(1. - l, dim=(2, 3)) + fgb.eps32(eps))
    loss = (pos * torch.from_numpy(gpos.astype(f64))).sum()
    if with_neg:
        loss = loss + (neg * torch.from_numpy(gneg.astype(f64))).sum()
    loss.backward()
    auto = emb.grad[0].reshape(C, -1).numpy()
    assert np.abs(auto - want).max() <= 1e-12 * np.abs(auto).max()
    assert (tol > 0).all() and (tol <= 1e-4 * np.abs(want).max()).all(), "the bound is not a float32 rounding bound"


# ------------------------------------------------------------------------------------------ the references ARE the reference's functions
@pytest.mark.parametrize("name", fgb.HEAD_FIXTURES)
def test_pool_reference_reproduces_the_recorded_gradients(name):
    fx = load_golden(name)
    C = fx["in_ref"].shape[0]
    O = fx["in_ref_label"].shape[0]
    wt = fx["weight"]
    for emb, lab, grad, lo in (("in_ref", "in_ref_label", "grad_ref", 0), ("in_prev", "in_prev_label", "grad_prev", 2 * C)):
        l = fx[lab].reshape(O, -1).astype(f32)
        want, tol = fgb.pool_grad_ref(l, wt[:, lo:lo + C], wt[:, lo + C:lo + 2 * C], float(fx["epsilon"]))
        rec = fx[grad].reshape(C, -1)
        # the reference's autograd adds gneg / (Nn + eps) through sum(emb) and takes it back through pos_sum (ATT:138): where an object owns
        # every pixel those two float64 terms are 1e5 x the result and leave their rounding behind
        cancel = 8 * 2.0 ** -53 * np.abs(wt[:, lo + C:lo + 2 * C].astype(f64) / ((1.0 - l.astype(f64)).sum(1) + fgb.eps32(float(fx["epsilon"])))[:, None]).max()
        assert np.abs(want - rec).max() <= 1e-12 * np.abs(rec).max() + cancel, f"{name} {grad}: the float64 reference is not the reference's gradient"
        assert np.abs(rec).max() > 1e-3
    if O > 1:
        assert (fx["in_prev_label"].reshape(O, -1).sum(1) == 0).any(), "no object without a pixel"
    else:
        assert fx["in_ref_label"].all(), "the single object does not own every pixel"


@pytest.mark.parametrize("name", fgb.FG2BG_FIXTURES)
def test_fg2bg_restatement_reproduces_the_recorded_gradients(name):
    fx = load_golden(name)
    dis = fx["in_dis"].reshape(fx["in_dis"].shape[0], fx["in_dis"].shape[1], -1)
    go = fx["weight"].reshape(dis.shape[0], -1)
    assert np.array_equal(fgb.fg2bg_min_np(dis).astype(f64), fx["out"].reshape(dis.shape[0], 1, -1))
    got = fgb.fg2bg_grad_np(go, dis)
    rec = fx["grad_dis"].reshape(dis.shape)
    assert np.array_equal(got != 0, rec != 0)
    assert fgb.check(got, rec, fgb.fg2bg_grad_tol(go, dis), name) <= 1.0


# ------------------------------------------------------------------------------------------ saturated ties end to end
def _composed_leaf_gradients(s, highest):
    """aocnet.py:141-358 for one sample in float64, composed from the numpy references of the operators (match_grad_bounds,
    local_grad_bounds, frontend_grad_bounds: each is held to the reference's recorded autograd by its own host test), with the
    foreground2background winners of the aggregation chosen by the stated rule or by 'highest index wins'.  The cluster channels have no
    background channel and take their cotangent as a plain slice whatever the rule, so a constant stands in for them.
    -> (leaf gradients ref, prev, cur [m, C] and bias [O]; the cotangents that reach the global and the local matcher; their T)."""
    h, w, C = s["cur"].shape
    m, O, radii = h * w, s["bias"].size, s["radii"]
    q, ref, prev = (s[k].reshape(m, C) for k in ("cur", "ref", "prev"))
    l_ref, l_prev = (s[k].reshape(m, O).T.astype(f64) for k in ("lab_ref", "lab_prev"))
    eps = fgb.eps32(1e-5)
    rp = ((l_ref @ ref.astype(f64)) / (l_ref.sum(1) + eps)[:, None]).astype(f32)                # ATT:136-141
    pp = ((l_prev @ prev.astype(f64)) / (l_prev.sum(1) + eps)[:, None]).astype(f32)
    inst = (l_prev.T @ pp.astype(f64)).astype(f32).reshape(h, w, C)                             # aocnet.py:325
    fwd = mgb.dense_forward_ref(q, ref, l_ref.T, s["bias"])
    pT, ptol = mgb.proxy_forward_ref(q, rp, s["bias"])
    base = dict(in_query=s["cur"], in_labels=s["lab_prev"], in_bias=s["bias"], multi_local_distance=np.asarray(radii), ori_size=np.zeros(2),
                atrous_rate=1, allow_downsample=1)
    nr = len(radii)
    zero = np.zeros((1, h, w, O, nr))
    to_planes = lambda out: out[0].transpose(2, 3, 0, 1).reshape(O, -1, m).astype(f32)
    local = to_planes(lgb.fixture_ref(dict(base, in_prev=s["prev"], weight=zero))["out"])
    lproxy = to_planes(lgb.fixture_ref(dict(base, in_prev=inst, weight=zero))["out"])
    planes = [fwd["T"].astype(f32)[:, None], s["cluster"], pT.astype(f32)[:, None], local, lproxy]
    feat = fgb.aggregate_np(*planes, l_prev.astype(f32))
    go = fgb.aggregate_grad_np(s["w_feat"], feat, 2, nr, True, highest=highest)
    emitted = lambda g: g.reshape(O, -1, h, w).transpose(2, 3, 0, 1)[None]                       # planes -> [1, h, w, O, k]
    dg = mgb.dense_grad_ref(go[0][:, 0], fwd["T"], fwd["tol_T"], fwd["arg"], q, ref)
    pg = mgb.proxy_grad_ref(go[2][:, 0], pT, ptol, q, rp)
    lg = lgb.fixture_ref(dict(base, in_prev=s["prev"], weight=emitted(go[3])))
    lpg = lgb.fixture_ref(dict(base, in_prev=inst, weight=emitted(go[4])))
    wh = s["w_head"].astype(f64)
    g_ref = dg["grad_pool"] + fgb.pool_grad_ref(l_ref.astype(f32), pg["grad_proxies"] + wh[:, :C], wh[:, C:2 * C], 1e-5)[0].T
    g_pp = l_prev @ lpg["grad_prev"].reshape(m, C) + wh[:, 2 * C:3 * C]
    g_prev = lg["grad_prev"].reshape(m, C) + fgb.pool_grad_ref(l_prev.astype(f32), g_pp, wh[:, 3 * C:], 1e-5)[0].T
    g_cur = dg["grad_query"] + pg["grad_query"] + lg["grad_query"].reshape(m, C) + lpg["grad_query"].reshape(m, C)
    g_bias = dg["grad_bias"] + pg["grad_bias"] + lg["grad_bias"] + lpg["grad_bias"]
    return (g_ref, g_prev, g_cur, g_bias), (go[0], go[3]), (planes[0], planes[3])


def test_end_to_end_gradients_do_not_depend_on_the_winner_of_a_saturated_tie():
    """Only object 0 is labelled, in both frames: the maps of objects 1 and 2 are saturated (T == 1.0 exactly), so for object 0 the minimum
    over the OTHER objects is an exact tie, in the global map and in every local one.  'Lowest index wins' and 'highest index wins' then
    send object 0's background cotangent to different objects -- and every leaf gradient comes out the same, because the matcher behind
    either multiplies it by 1 - T^2 = 0."""
    h, w, C, O, radii = 11, 13, 8, 3, (2, 4)
    rs = fgb.rng(h, w, C, O, 77)
    emb = lambda: (0.35 * rs.standard_normal((h, w, C))).astype(f32)
    lab = np.zeros((h, w, O), f32)
    lab[:, :, 0] = 1.0
    n_ch = fgb.channel_layout(2, len(radii))["n_ch"]
    s = dict(ref=emb(), prev=emb(), cur=emb(), lab_ref=lab, lab_prev=lab.copy(), bias=(0.2 * rs.standard_normal(O)).astype(f32), radii=radii,
             cluster=np.tanh(rs.standard_normal((O, 2, h * w))).astype(f32), w_feat=rs.standard_normal((O, n_ch, h * w)).astype(f32),
             w_head=rs.standard_normal((O, 4 * C)).astype(f32))
    low, go_low, T = _composed_leaf_gradients(s, highest=False)
    high, go_high, _ = _composed_leaf_gradients(s, highest=True)
    for k, name in enumerate(("global", "local")):
        moved = go_low[k] != go_high[k]
        assert moved.any(), name + ": the two rules choose the same winners: the case has no tie"
        assert (T[k][moved] == 1.0).all(), name + ": the rules differ at an entry that is not saturated"
        assert (T[k][0] < 1.0).all() and (T[k][1:] == 1.0).all()
    for name, a, b in zip(("ref_emb", "prev_emb", "cur_emb", "bias"), low, high):
        assert np.abs(a).max() > 1e-3, name + ": the gradient vanishes"
        assert np.array_equal(a, b), f"{name}: the gradient depends on the winner of a saturated tie (by up to {np.abs(a - b).max():.3e})"


# ------------------------------------------------------------------------------------------ the tensor contract, library stubbed
def _t(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(f32))


def _cases():
    O, C, X, nc, nl = 3, 8, 12, 2, 3
    n_ch = ft.aggregate_channels(nc, nl)
    F, OUT = occ.F, occ.OUT

    def mk(builder):
        return lambda ops_, device: {k: v.to(device) for k, v in builder(np.random.RandomState(7)).items()}
    return [
        occ.Case("masked_mean_pool_backward", [], mk(lambda rs: dict(gpos=_t(rs, O, C), gneg=_t(rs, O, C), labels=_t(rs, O, X), grad_emb=torch.zeros(C, X))),
                 {"gpos": F, "gneg": F, "labels": F, "grad_emb": OUT},
                 lambda ops_, a: ft.masked_mean_pool_backward(a["gpos"], a["gneg"], a["labels"], 1e-5, False, a["grad_emb"]), None),
        occ.Case("fg2bg_backward", [], mk(lambda rs: dict(grad_out=_t(rs, O, 1, X), dis=_t(rs, O, nc, X), grad_dis=torch.zeros(O, nc, X))),
                 {"grad_out": F, "dis": F, "grad_dis": OUT},
                 lambda ops_, a: ft.fg2bg_backward(a["grad_out"], a["dis"], O, a["grad_dis"]), None),
        occ.Case("proto_aggregate", [], mk(lambda rs: dict(g=_t(rs, O, 1, X), c=_t(rs, O, nc, X), p=_t(rs, O, 1, X), l=_t(rs, O, nl, X), lp=_t(rs, O, nl, X),
                                                           prev=_t(rs, O, X), feat=torch.zeros(O, n_ch, X))),
                 {"g": F, "c": F, "p": F, "l": F, "lp": F, "prev": F, "feat": OUT},
                 lambda ops_, a: ft.proto_aggregate(a["g"], a["c"], a["p"], a["l"], a["lp"], a["prev"], True, a["feat"]), None),
        occ.Case("proto_aggregate_backward", [], mk(lambda rs: dict(grad_feat=_t(rs, O, n_ch, X), feat=_t(rs, O, n_ch, X))),
                 {"grad_feat": F, "feat": F},
                 lambda ops_, a: ft.proto_aggregate_backward(a["grad_feat"], a["feat"], nc, nl, True), None),
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
    src = inspect.getsource(ft)
    assert "data_ptr" not in src and "import ctypes" not in src
    import ast
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ("_p", "_addr"):
            assert not any(isinstance(sub, ast.Call) for arg in node.args for sub in ast.walk(arg)), f"line {node.lineno}: a call expression inside _p(...)"
    public = {n for n, v in vars(ops).items() if callable(v) and not n.startswith("_") and getattr(v, "__module__", None) == ops.__name__}
    assert not {"masked_mean_pool_backward", "fg2bg_backward", "proto_aggregate", "proto_aggregate_backward"} & public


# ------------------------------------------------------------------------------------------ the no-gradient path and the guards
def test_no_gradient_path_returns_the_mirrors_result_unchanged(monkeypatch):
    sentinel = object()
    seen = []
    monkeypatch.setattr(aoc_amd.matching, "foreground2background", lambda *a: seen.append(("fg2bg", a)) or sentinel)
    monkeypatch.setattr(aoc_amd.attention, "calculate_attention_head_p_m", lambda *a: seen.append(("p_m", a)) or sentinel)
    monkeypatch.setattr(aoc_amd.attention, "calculate_attention_head", lambda *a: seen.append(("head", a)) or sentinel)
    dis = torch.randn(3, 1, 4, 5)
    e, l = torch.randn(1, 4, 4, 5).expand(3, -1, -1, -1), torch.ones(3, 1, 4, 5)
    assert ft.foreground2background(dis, 3) is sentinel
    assert ft.calculate_attention_head_p_m(e, l, e, l, 1e-4) is sentinel and ft.calculate_attention_head(e, l, e, l) is sentinel
    assert seen[0][1] == (dis, 3) and seen[1][1][4] == 1e-4 and seen[2][1][4] == 1e-5 and seen[1][1][0] is e
    with torch.no_grad():                                           # autograd off: the same, whatever requires_grad says
        assert ft.foreground2background(dis.clone().requires_grad_(True), 3) is sentinel
    one = torch.randn(1, 1, 4, 5, requires_grad=True)
    assert ft.foreground2background(one, 1) is one                 # AEM:10-11


def test_guards_and_signatures(monkeypatch):
    e = torch.randn(1, 4, 4, 5, requires_grad=True)
    l = torch.ones(3, 1, 4, 5)
    with pytest.raises(_lib.AocHipError, match="no CPU fallback"):
        ft.calculate_attention_head_p_m(e.expand(3, -1, -1, -1), l, e.expand(3, -1, -1, -1), l)
    with pytest.raises(_lib.AocHipError, match="no CPU fallback"):
        ft.foreground2background(torch.randn(3, 1, 4, 5, requires_grad=True), 3)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_need_gpu", lambda *t: None)
        with pytest.raises(NotImplementedError, match="per-object embeddings"):
            ft.calculate_attention_head_p_m(torch.randn(3, 4, 4, 5, requires_grad=True), l, e.expand(3, -1, -1, -1), l)
    emb = torch.randn(4, 5, 6, requires_grad=True)
    with pytest.raises(_lib.AocHipError, match="use_float16"):
        ft.proto_mask_features(emb, emb, emb, torch.zeros(5, 6), torch.zeros(5, 6), 2, torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 1, 1), use_float16=True)
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(ft.foreground2background) == ["dis", "obj_num"]
    for f in (ft.calculate_attention_head, ft.calculate_attention_head_p_m):
        assert names(f) == ["ref_embedding", "ref_label", "prev_embedding", "prev_label", "epsilon"]
        assert inspect.signature(f).parameters["epsilon"].default == 1e-5
    assert names(ft.aggregate) == ["global_fg", "cluster_fg", "proxy_fg", "local_fg", "local_proxy_fg", "prev_label", "matching_background"]
    assert names(ft.proto_mask_features)[:8] == ["ref_emb", "prev_emb", "cur_emb", "ref_label", "prev_label", "gt_id", "bg_bias", "fg_bias"]
    with pytest.raises(_lib.AocHipError, match="frontend_train.foreground2background is the differentiable form"):
        aoc_amd.matching.foreground2background(torch.randn(3, 1, 4, 5, requires_grad=True), 3)
    with pytest.raises(_lib.AocHipError, match="frontend_train.calculate_attention_head_p_m is the differentiable form"):
        aoc_amd.attention.calculate_attention_head_p_m(e.expand(3, -1, -1, -1), l, e.expand(3, -1, -1, -1), l)


def test_aggregate_takes_the_matchers_layout_without_a_copy():
    """[O, k, h, w] planes -> the [1, h, w, O, k] the matchers return (matching_train._emit) -> _planes: the same storage, contiguous."""
    planes = torch.randn(3, 2, 4, 5)
    emitted = planes.view(6, 1, 4, 5).permute(2, 3, 0, 1).reshape(1, 4, 5, 3, 2)
    back = ft._planes(emitted, "x")
    assert back.is_contiguous() and back.data_ptr() == planes.data_ptr() and torch.equal(back, planes)
    assert ops._f32c(back).data_ptr() == planes.data_ptr()
    with pytest.raises(ValueError):
        ft._planes(planes, "x")


# ------------------------------------------------------------------------------------------ the C entry points before any launch
def test_entries_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(256)                         # never dereferenced: every call here returns before a launch
    need = L.aoc_masked_mean_pool_grad_workspace_bytes(4)
    assert need == 256 and L.aoc_masked_mean_pool_grad_workspace_bytes(0) == 0 and L.aoc_masked_mean_pool_grad_workspace_bytes(30) == 256

    def pool(gp=p, lab=p, hw=35, C=4, O=4, out=p, ws=p, nbytes=need):
        return L.aoc_masked_mean_pool_grad(gp, None, lab, hw, C, O, 0, 1e-5, out, ws, nbytes, None)
    assert pool(gp=None) == INVALID and pool(lab=None) == INVALID and pool(out=None) == INVALID
    assert pool(hw=0) == INVALID and pool(C=0) == INVALID and pool(O=0) == INVALID and pool(O=33, nbytes=1 << 12) == UNSUPPORTED
    assert pool(ws=None) == WORKSPACE and pool(nbytes=need - 1) == WORKSPACE

    def fg(go=p, gs=35, dis=p, O=3, nc=2, inner=35, ds=70, gd=p, gds=70):
        return L.aoc_fg2bg_grad(go, gs, dis, O, nc, inner, ds, gd, gds, None)
    assert fg(go=None) == INVALID and fg(dis=None) == INVALID and fg(gd=None) == INVALID
    assert fg(O=1) == INVALID and fg(nc=0) == INVALID and fg(inner=0) == INVALID and fg(ds=69) == INVALID and fg(gds=69) == INVALID and fg(gs=34) == INVALID

    assert L.aoc_proto_aggregate_channels(2, 6, 1) == 24 == ft.aggregate_channels(2, 6) and L.aoc_proto_aggregate_channels(2, 6, 0) == 17
    assert L.aoc_frame_channels(6, 1, 1) == 24, "the training tensor has the channels of the inference frame call"
    assert L.aoc_proto_aggregate_channels(6, 1, 1) == ft.aggregate_channels(6, 1) and L.aoc_proto_aggregate_channels(0, 6, 1) == INVALID

    def agg(g=p, c=p, px=p, l=p, lp=p, prev=p, O=3, hw=35, nc=2, nl=6, feat=p):
        return L.aoc_proto_aggregate(g, c, px, l, lp, prev, O, hw, nc, nl, 1, feat, None)
    for k in ("g", "c", "px", "l", "lp", "prev", "feat"):
        assert agg(**{k: None}) == INVALID, k
    assert agg(O=0) == INVALID and agg(hw=0) == INVALID and agg(nc=0) == INVALID and agg(nl=0) == INVALID

    def aggb(gf=p, f=p, O=3, hw=35, nc=2, nl=6):
        return L.aoc_proto_aggregate_grad(gf, f, O, hw, nc, nl, 1, p, p, p, p, p, None)
    assert aggb(gf=None) == INVALID and aggb(f=None) == INVALID and aggb(O=0) == INVALID and aggb(hw=0) == INVALID and aggb(nc=0) == INVALID
