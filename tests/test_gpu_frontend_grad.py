"""The training-time front end on the device: aoc_masked_mean_pool_grad, aoc_fg2bg_grad, aoc_proto_aggregate, aoc_proto_aggregate_grad and
aoc_amd.frontend_train against the restatements, float64 references and derived bounds of tests/frontend_grad_bounds.py."""
import numpy as np
import pytest
import torch

import aoc_amd
import cluster_grad_bounds as cgb
import frontend_grad_bounds as fgb
import local_grad_bounds as lgb
import match_grad_bounds as mgb
from aoc_amd import attention, cluster_train, frontend_train as ft, local_train, matching, matching_train, ops  # noqa: F401
from conftest import load_golden
from oracle import matching as om

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, f64 = np.float32, np.float64
NAN = float("nan")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def margins(shape, pad=5):
    """-> (buffer, view): a NaN-filled flat buffer with ``pad`` elements before and after a contiguous view of ``shape``; an odd pad also
    moves the view off a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), NAN, device=DEV)
    return buf, buf[pad:pad + n].view(*shape)


def untouched(buf, pad=5):
    return bool(torch.isnan(buf[:pad]).all() and torch.isnan(buf[-pad:]).all())


# ------------------------------------------------------------------------------------------ pooling gradient
def _pool_run(lab, gpos, gneg, pixel_major, pad):
    C, X = gpos.shape[1], lab.shape[1]
    buf, out = margins((C, X), pad)
    labels = dev(lab.T.copy() if pixel_major else lab)
    got = ft.masked_mean_pool_backward(dev(gpos), None if gneg is None else dev(gneg), labels, 1e-5, pixel_major, out)
    assert got is out and untouched(buf, pad), "written outside grad_emb"
    return out


@pytest.mark.parametrize("h,w", fgb.MAPS + fgb.MAPS_VEC)
def test_pool_grad_inside_the_bound(h, w):
    worst = 0.0
    for k, (O, C) in enumerate(zip(fgb.OBJECTS, (36, 4, 100, 128, 36))):
        for soft in (False, True):
            kind = dict(soft=True) if soft else (dict(empty=O - 1) if k % 2 == 0 else dict(full=0))
            lab, gpos, gneg = fgb.pool_case(h, w, O, C, k, with_neg=(k != 1), **kind)
            if not soft and O > 1:
                assert (lab.sum(1) == 0).any() or (lab.sum(1) == h * w).any(), "neither an empty object nor one that owns every pixel"
            want, tol = fgb.pool_grad_ref(lab, gpos, gneg, 1e-5)
            for pixel_major in (False, True):
                pad = 4 if (h * w) % 4 == 0 else 5                                   # a multiple of four keeps the view 16-byte aligned
                out = _pool_run(lab, gpos, gneg, pixel_major, pad)
                worst = max(worst, fgb.check(out.cpu().numpy(), want, tol, f"pool grad {h}x{w} O={O} C={C} soft={soft} pixel_major={pixel_major}"))
                again = _pool_run(lab, gpos, gneg, pixel_major, pad)
                assert torch.equal(out, again), "two runs differ"
                if pixel_major:
                    assert torch.equal(out, first), "the two label layouts differ"
                first = out
    print(f"pool grad {h}x{w}: worst error / bound {worst:.3f}")


def test_pool_grad_alignment_changes_no_bit():
    """hw a multiple of four: the 16-byte instantiation on an aligned buffer, the 4-byte one on a buffer moved by one float."""
    lab, gpos, gneg = fgb.pool_case(16, 20, 5, 100, 9, soft=True)
    a = _pool_run(lab, gpos, gneg, False, 4)
    b = _pool_run(lab, gpos, gneg, False, 5)
    assert torch.equal(a, b)


def test_heads_against_the_mirror_and_autograd_formula():
    h, w, C, O = 13, 9, 36, 3
    rs = fgb.rng(h, w, C, O)
    ref = dev((0.5 * rs.standard_normal((1, C, h, w))).astype(f32)).requires_grad_(True)
    prev = dev((0.5 * rs.standard_normal((1, C, h, w))).astype(f32)).requires_grad_(True)
    lr, lp = (dev(np.eye(O, dtype=f32)[rs.randint(0, O, (h, w))].transpose(2, 0, 1)[:, None].copy()) for _ in range(2))
    wt = dev(rs.standard_normal((O, 4 * C)).astype(f32))
    with torch.no_grad():
        plain = attention.calculate_attention_head_p_m(ref.expand(O, -1, -1, -1), lr, prev.expand(O, -1, -1, -1), lp)
    with torch.enable_grad():
        got = ft.calculate_attention_head_p_m(ref.expand(O, -1, -1, -1), lr, prev.expand(O, -1, -1, -1), lp)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), "the training forward differs from the mirror's bits"
        head = ft.calculate_attention_head(ref.expand(O, -1, -1, -1), lr, prev.expand(O, -1, -1, -1), lp)
        assert torch.equal(head, plain[0])
        (got[0] * wt).sum().backward()
    for t, lab, lo in ((ref, lr, 0), (prev, lp, 2 * C)):
        g = wt.cpu().numpy()
        want, tol = fgb.pool_grad_ref(lab.cpu().numpy().reshape(O, -1), g[:, lo:lo + C], g[:, lo + C:lo + 2 * C], 1e-5)
        assert t.grad.shape == t.shape
        fgb.check(t.grad.cpu().numpy().reshape(C, -1), want, tol, "head gradient")
    # only the positive proxies used: the negative term is left out, not multiplied by zero
    ref.grad = None
    with torch.enable_grad():
        out = ft.calculate_attention_head_p_m(ref.expand(O, -1, -1, -1), lr, prev.expand(O, -1, -1, -1), lp)
        (out[1] * wt[:, :C]).sum().backward()
    want, tol = fgb.pool_grad_ref(lr.cpu().numpy().reshape(O, -1), wt.cpu().numpy()[:, :C], None, 1e-5)
    fgb.check(ref.grad.cpu().numpy().reshape(C, -1), want, tol, "head gradient, positive half only")
    with torch.enable_grad():
        g = torch.autograd.grad(ft.calculate_attention_head(ref.expand(O, -1, -1, -1), lr, prev.expand(O, -1, -1, -1), lp).sum(), [ref], create_graph=True)
        with pytest.raises(RuntimeError):
            g[0].sum().backward()                                                  # once_differentiable: a double backward raises
        with pytest.raises(NotImplementedError):
            ft.calculate_attention_head(ref.expand(O, -1, -1, -1).contiguous(), lr, prev.expand(O, -1, -1, -1), lp)


@pytest.mark.parametrize("name", fgb.HEAD_FIXTURES)
def test_heads_against_the_recorded_reference(name):
    fx = load_golden(name)
    C, O = fx["in_ref"].shape[0], fx["in_ref_label"].shape[0]
    eps = float(fx["epsilon"])
    ref, prev = (dev(fx[k].astype(f32)).requires_grad_(True) for k in ("in_ref", "in_prev"))
    lr, lp = dev(fx["in_ref_label"], torch.float32), dev(fx["in_prev_label"], torch.float32)
    with torch.enable_grad():
        outs = ft.calculate_attention_head_p_m(ref.unsqueeze(0).expand(O, -1, -1, -1), lr, prev.unsqueeze(0).expand(O, -1, -1, -1), lp, eps)
        (outs[0] * dev(fx["weight"])).sum().backward()
    head = outs[0].detach().cpu().numpy()
    for t, emb, lab, grad, lo in ((ref, "in_ref", "in_ref_label", "grad_ref", 0), (prev, "in_prev", "in_prev_label", "grad_prev", 2 * C)):
        l = fx[lab].reshape(O, -1).astype(f32)
        tol_pos, tol_neg = fgb.pool_forward_tol(fx[emb].reshape(C, -1).astype(f32), l, eps)
        fgb.check(head[:, lo:lo + C], fx["out_head"][:, lo:lo + C], tol_pos, f"{name} {emb} positive head")
        fgb.check(head[:, lo + C:lo + 2 * C], fx["out_head"][:, lo + C:lo + 2 * C], tol_neg, f"{name} {emb} negative head")
        _, tol = fgb.pool_grad_ref(l, fx["weight"][:, lo:lo + C], fx["weight"][:, lo + C:lo + 2 * C], eps)
        fgb.check(t.grad.cpu().numpy().reshape(C, -1), fx[grad].reshape(C, -1), tol, f"{name} {grad}")


@pytest.mark.parametrize("name", fgb.FG2BG_FIXTURES)
def test_fg2bg_against_the_recorded_reference(name):
    fx = load_golden(name)
    O = fx["in_dis"].shape[0]
    d = dev(fx["in_dis"]).requires_grad_(True)
    with torch.enable_grad():
        out = ft.foreground2background(d, O)
        (out * dev(fx["weight"])).sum().backward()
    assert out.shape == fx["out"].shape and np.array_equal(out.detach().cpu().numpy().astype(f64), fx["out"])
    flat = lambda a: a.reshape(O, fx["in_dis"].shape[1], -1)
    fgb.check(flat(d.grad.cpu().numpy()), flat(fx["grad_dis"]), fgb.fg2bg_grad_tol(fx["weight"].reshape(O, -1), flat(fx["in_dis"])), name)


# ------------------------------------------------------------------------------------------ foreground2background
def _fg2bg_run(go, dis, pad):
    O, nc, X = dis.shape
    buf, out = margins(dis.shape, pad)
    got = ft.fg2bg_backward(dev(go).view(O, 1, X), dev(dis), O, out)
    assert got is out and untouched(buf, pad), "written outside grad_dis"
    return out.cpu().numpy()


@pytest.mark.parametrize("h,w", fgb.MAPS + fgb.MAPS_VEC)
def test_fg2bg_forward_bits_and_backward_against_restatement_and_bound(h, w):
    X = h * w
    for k, O in enumerate(fgb.OBJECTS[1:]):
        nc = (1, 2, 3, 1)[k]
        rs = fgb.rng(h, w, O, nc)
        dis = rs.standard_normal((O, nc, X)).astype(f32)
        go = rs.standard_normal((O, X)).astype(f32)
        d = dev(dis).requires_grad_(True)
        with torch.enable_grad():
            out = ft.foreground2background(d, O)
            (out * dev(go).view(O, 1, X)).sum().backward()
        with torch.no_grad():
            assert torch.equal(out.detach(), matching.foreground2background(d.detach(), O)), "the training forward differs from the mirror's bits"
        assert np.array_equal(out.detach().cpu().numpy(), fgb.fg2bg_min_np(dis))
        want = fgb.fg2bg_grad_np(go, dis)
        assert np.array_equal(d.grad.cpu().numpy(), want), f"O={O} c={nc}: grad_dis differs from the restatement"
        pad = 4 if X % 4 == 0 else 5
        assert np.array_equal(_fg2bg_run(go, dis, pad), want)
        if X % 4 == 0:
            assert np.array_equal(_fg2bg_run(go, dis, 5), want), "the 4-byte instantiation differs"
        dd = torch.from_numpy(dis.astype(f64)).requires_grad_(True)
        with torch.enable_grad():
            (om.foreground2background(dd, O)[:, 0] * torch.from_numpy(go.astype(f64))).sum().backward()
        fgb.check(d.grad.cpu().numpy(), dd.grad.numpy(), fgb.fg2bg_grad_tol(go, dis), f"fg2bg grad {h}x{w} O={O} c={nc}")


def test_fg2bg_planted_ties_come_out_by_the_rule():
    dis, go = fgb.planted_fg2bg()
    want = fgb.fg2bg_grad_np(go, dis)
    assert np.array_equal(_fg2bg_run(go, dis, 5), want)
    d4, g4 = np.tile(dis, (1, 1, 2)), np.tile(go, (1, 2))                           # 12 columns: the 16-byte instantiation
    assert np.array_equal(_fg2bg_run(g4, d4, 4), np.tile(want, (1, 1, 2)))
    assert not np.array_equal(want, fgb.fg2bg_grad_np(go, dis, highest=True)) and not np.array_equal(want, fgb.fg2bg_grad_np(go, dis, descending=True))


# ------------------------------------------------------------------------------------------ aggregation
def _emitted(planes, h, w):
    """[O, k, X] -> the [1, h, w, O, k] tensor a matcher returns."""
    O, k, _ = planes.shape
    return planes.view(O * k, 1, h, w).permute(2, 3, 0, 1).reshape(1, h, w, O, k)


def _mirror_composition(src, prev, O, h, w, background):
    """aocnet.py:341-358 by the existing inference mirrors: torch.cat, matching.foreground2background (aoc_fg2bg_min)."""
    glob, cluster, proxy, local, lproxy = (s.view(O, -1, h, w) for s in src)
    cat = [glob, cluster, proxy, local, lproxy, prev.view(O, 1, h, w)]
    if background:
        lbg = matching.foreground2background(local.permute(0, 2, 3, 1).unsqueeze(1), O)
        cat += [lbg.permute(0, 4, 2, 3, 1).squeeze(-1), matching.foreground2background(glob, O)]
    return torch.cat(cat, 1)


AGG_CASES = ((1, 1, 2, 1), (5, 7, 1, 2), (5, 7, 2, 2), (13, 9, 3, 6), (13, 9, 17, 2), (31, 33, 30, 2), (31, 33, 3, 2), (4, 8, 3, 6), (16, 20, 17, 2))


@pytest.mark.parametrize("h,w,O,n_cluster", AGG_CASES)
@pytest.mark.parametrize("ties", (False, True))
def test_aggregate_forward_bits_and_backward_against_restatement(h, w, O, n_cluster, ties):
    X = h * w
    n_local = 1 + (h + O) % 8
    background = not (h == 13 and O == 3)
    src, prev, gfeat = fgb.aggregate_case(h, w, O, n_cluster, n_local, 4, ties)
    lay = fgb.channel_layout(n_cluster, n_local, background)
    gfeat = gfeat[:, :lay["n_ch"]].copy()
    ts = [dev(s).requires_grad_(True) for s in src]
    with torch.enable_grad():
        feat = ft.aggregate(*[_emitted(t, h, w) for t in ts], dev(prev).view(O, 1, h, w), background)
        assert feat.shape == (O, lay["n_ch"], h, w)
        (feat * dev(gfeat).view(O, -1, h, w)).sum().backward()
    with torch.no_grad():
        want_feat = _mirror_composition([t.detach() for t in ts], dev(prev), O, h, w, background)
        assert torch.equal(feat.detach(), want_feat), "the forward differs from the composition of the mirrors"
        plain = ft.aggregate(*[_emitted(t.detach(), h, w) for t in ts], dev(prev).permute(1, 0).reshape(h, w, O), background)
        assert torch.equal(plain, want_feat) and not plain.requires_grad
    feat_np = fgb.aggregate_np(*src, prev, background)
    assert np.array_equal(feat.detach().cpu().numpy().reshape(feat_np.shape), feat_np)
    want = fgb.aggregate_grad_np(gfeat, feat_np, n_cluster, n_local, background)
    for k, (t, g) in enumerate(zip(ts, want)):
        assert np.array_equal(t.grad.cpu().numpy(), g), f"source {k}: gradient differs from the restatement"
    if not ties:
        t64 = [torch.from_numpy(s.astype(f64)).requires_grad_(True) for s in src]
        with torch.enable_grad():
            (fgb.aggregate_torch(t64, torch.from_numpy(prev.astype(f64)), O, background) * torch.from_numpy(gfeat.astype(f64))).sum().backward()
        for k, (t, r, tol) in enumerate(zip(ts, t64, fgb.aggregate_grad_tol(gfeat, n_cluster, n_local, background))):
            fgb.check(t.grad.cpu().numpy(), r.grad.numpy(), tol, f"aggregate grad {h}x{w} O={O} source {k}")


@pytest.mark.parametrize("pad", (4, 5))
def test_aggregate_margins_planted_ties_and_partial_wants(pad):
    src, prev, gfeat = fgb.planted_aggregate()
    src = [np.tile(s, (1, 1, 2)) for s in src]                                       # 12 columns: the 16-byte instantiation with pad 4
    prev, gfeat = np.tile(prev, (1, 2)), np.tile(gfeat, (1, 1, 2))
    O, n_ch, X = gfeat.shape
    buf, feat = margins((O, n_ch, X), pad)
    got = ft.proto_aggregate(*[dev(s) for s in src], dev(prev), True, feat)
    assert got is feat and untouched(buf, pad), "written outside feat"
    feat_np = fgb.aggregate_np(*src, prev)
    assert np.array_equal(feat.cpu().numpy(), feat_np) and not torch.isnan(feat).any()
    want = fgb.aggregate_grad_np(gfeat, feat_np, 2, 2)
    assert any(not np.array_equal(a, b) for a, b in zip(want, fgb.aggregate_grad_np(gfeat, feat_np, 2, 2, highest=True)))
    gbuf, g = margins((O, n_ch, X), pad)
    g.copy_(dev(gfeat))
    grads = ft.proto_aggregate_backward(g, feat, 2, 2, True)
    for k, (a, b) in enumerate(zip(grads, want)):
        assert np.array_equal(a.cpu().numpy(), b), f"source {k}: the planted ties do not come out by the rule"
    some = ft.proto_aggregate_backward(g, feat, 2, 2, True, (True, False, False, True, False))
    assert some[1] is None and some[2] is None and some[4] is None and torch.equal(some[0], grads[0]) and torch.equal(some[3], grads[3])
    again = ft.proto_aggregate_backward(g, feat, 2, 2, True)
    assert all(torch.equal(a, b) for a, b in zip(grads, again)), "two runs differ"


# ------------------------------------------------------------------------------------------ one training sample
def _sample(h, w, C, gt_id, seed, absent=None):
    rs = fgb.rng(h, w, C, gt_id, seed)
    O = gt_id + 1
    embs = [dev((0.12 * rs.standard_normal((C, h, w))).astype(f32)).requires_grad_(True) for _ in range(3)]
    labs = []
    for _ in range(2):
        l = rs.randint(0, O, (h, w))
        if absent is not None:
            l[l == absent] = 0
        labs.append(dev(l.astype(np.int32)))
    bg = dev((0.1 * rs.standard_normal((1, 1, 1, 1))).astype(f32)).requires_grad_(True)
    fg = dev((0.1 * rs.standard_normal((1, 1, 1, 1))).astype(f32)).requires_grad_(True)
    return embs, labs, bg, fg


def _by_hand(embs, labs, gt_id, bg, fg, radii, background, rows):
    """aocnet.py:141-358 written out line by line with the five differentiable matchers and the differentiable heads, and with torch's own
    cat for aocnet.py:355-358; foreground2background is written as a product with the one-hot of the FIRST minimum among the other objects
    (the value of torch.min, and the stated tie rule for its gradient), so autograd differentiates it without any of the new kernels."""
    ref_emb, prev_emb, cur_emb = embs
    O = gt_id + 1
    C, h, w = cur_emb.shape
    ids = torch.arange(O, device=DEV).int().view(-1, 1, 1, 1)
    bias = torch.cat([bg, fg.expand(gt_id, -1, -1, -1)], 0) if gt_id > 0 else bg
    cur, prev, ref = (e.permute(1, 2, 0) for e in (cur_emb, prev_emb, ref_emb))
    to_prev, to_ref = ((l.view(1, h, w) == ids).float() for l in (labs[1], labs[0]))
    sp, sr = to_prev.squeeze(1).permute(1, 2, 0), to_ref.squeeze(1).permute(1, 2, 0)
    g = matching_train.global_matching(ref, cur, sr, 1, bias, None, 1, False)
    c = cluster_train.global_matching_cluster2(ref, cur, sr, 1, bias, None, 1, False, 0, init_rows=rows)
    l = local_train.local_matching(prev, cur, sp, bias, radii, None, 1, False, True, True)
    head, rp, _, pp, _ = ft.calculate_attention_head_p_m(ref_emb.unsqueeze(0).expand(O, -1, -1, -1), to_ref, prev_emb.unsqueeze(0).expand(O, -1, -1, -1),
                                                         to_prev, 1e-5)
    p = matching_train.global_matching_proxy(rp, cur, sr, 1, bias, None, 1, False)
    lp = local_train.local_matching_proxy(torch.matmul(sp, pp), cur, sp, bias, radii, None, 1, False, True, True)
    planes = [t.squeeze(0).permute(2, 3, 0, 1) for t in (g, c, p, l, lp)]
    cat = [planes[0], planes[1], planes[2], planes[3], planes[4], to_prev]
    if background:
        bgs = []
        for src in (planes[3], planes[0]):
            if O == 1:
                bgs.append(src)
                continue
            per = []
            for o in range(O):
                others = torch.cat([src[:o], src[o + 1:]], 0)                           # AEM:13-19
                hit = others.detach() == others.detach().min(0, keepdim=True)[0]
                first = (hit & (hit.cumsum(0) == 1)).float()
                per.append((others * first).sum(0))                                     # one non-zero term: the exact value of AEM:20
            bgs.append(torch.stack(per))
        cat += bgs
    return torch.cat(cat, 1), head


@pytest.mark.parametrize("gt_id,absent,background,radii", ((3, None, True, (2, 4, 6)), (0, None, True, (2, 4)), (3, 2, True, (4,)), (2, None, False, (2, 4, 6, 8))))
def test_proto_mask_features_wiring(gt_id, absent, background, radii):
    """The matchers and the heads have their own references and bounds; what proto_mask_features adds is the wiring and the aggregation.
    It is held to the same lines written out by hand (_by_hand), forward and backward, bit for bit: with an integer cotangent on the tensor
    the aggregation's sums are exact whichever way they are added, and everything behind them is the same graph.  A no-gradient mirror of
    the cluster call draws its k-means rows itself, so the rows are drawn once here and passed to both."""
    h, w, C = 11, 13, 36
    embs, labs, bg, fg = _sample(h, w, C, gt_id, 7, absent)
    O = gt_id + 1
    with torch.no_grad():
        sr = (labs[0].view(1, h, w) == torch.arange(O, device=DEV).view(-1, 1, 1)).float().permute(1, 2, 0)
        pool, labels_flat = matching._flatten_pool([embs[0].detach().permute(1, 2, 0)], [sr], h, w, 1, 0)
        cp = matching.cluster_proxies(pool, labels_flat, 16, None, np.random.RandomState(3))
    rows = cp["init_rows"]
    wt = None
    grads = []
    outs = []
    for fn in ("new", "hand"):
        for t in embs + [bg, fg]:
            t.grad = None
        with torch.enable_grad():
            if fn == "new":
                feat, head = ft.proto_mask_features(embs[0], embs[1], embs[2], labs[0], labs[1], gt_id, bg, fg, radii, matching_background=background,
                                                    init_rows=rows)
            else:
                feat, head = _by_hand(embs, labs, gt_id, bg, fg, list(radii), background, rows)
            if wt is None:
                gen = torch.Generator(DEV).manual_seed(5)
                # small integers on feat: every sum of at most O + 1 of them is exact in float32, whatever order autograd adds them in
                wt = (torch.randint(-4, 5, feat.shape, device=DEV, generator=gen).float(), torch.randn(head.shape, device=DEV, generator=gen))
            ((feat * wt[0]).sum() + (head * wt[1]).sum()).backward()
        outs.append((feat.detach(), head.detach()))
        grads.append([None if t.grad is None else t.grad.clone() for t in embs + [bg, fg]])
    lay = fgb.channel_layout(2, len(radii), background)
    assert outs[0][0].shape == (O, lay["n_ch"], h, w) and outs[0][1].shape == (O, 4 * C)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the forward differs from the hand-written lines"
    if absent is not None:
        assert (outs[0][0][absent, lay["glob"]] == 1.0).all() and (outs[0][1][absent, :C] == 0).all()
    if background and O > 1:
        assert not torch.equal(outs[0][0][:, lay["global_bg"]], outs[0][0][:, lay["glob"]])
    # the gradients that reach the five matchers are exact sums on both sides and the graph behind them is the same: the same bits
    for name, a, b in zip(("ref_emb", "prev_emb", "cur_emb", "bg_bias", "fg_bias"), grads[0], grads[1]):
        if name == "fg_bias" and gt_id == 0:
            assert a is None and b is None                                          # aocnet.py:146: one object never reads fg_bias
            continue
        assert float(b.abs().max()) > 0, name + ": the hand-written gradient vanishes"
        assert torch.equal(a, b), f"{name}: |new - hand| up to {float((a - b).abs().max()):.3e} at a gradient scale of {float(b.abs().max()):.3e}"
    # no gradient wanted: no graph, and the inference mirrors' results in the same wiring (at C = 36 the mirrors' local and dense kernels
    # are not the training forwards' bit for bit, so the comparison is with the hand-written lines under no_grad, not with the run above)
    with torch.no_grad():
        feat, head = ft.proto_mask_features(embs[0], embs[1], embs[2], labs[0], labs[1], gt_id, bg, fg, radii, matching_background=background, init_rows=rows)
        feat_hand, head_hand = _by_hand(embs, labs, gt_id, bg, fg, list(radii), background, rows)
    assert not feat.requires_grad and not head.requires_grad and torch.equal(feat, feat_hand) and torch.equal(head, head_hand)
    assert torch.equal(head, outs[0][1])                                            # the heads are one kernel either way


def _np(t):
    return t.detach().cpu().numpy()


def _record(monkeypatch, rec):
    """Wraps the five matchers and the heads as proto_mask_features reaches them: notes the arguments each receives and its result, and has
    autograd keep the gradient of every result and of every argument that is not a leaf (the pooled heads, the per-pixel proxy map)."""
    def wrap(mod, name, key):
        real = getattr(mod, name)

        def f(*a, **k):
            out = real(*a, **k)
            for t in (out if isinstance(out, tuple) else (out,)) + tuple(a[:2]):
                if torch.is_tensor(t) and t.requires_grad and not t.is_leaf:
                    t.retain_grad()
            rec[key] = (a, k, out)
            return out
        monkeypatch.setattr(mod, name, f)
    wrap(matching_train, "global_matching", "dense")
    wrap(matching_train, "global_matching_proxy", "proxy")
    wrap(cluster_train, "global_matching_cluster2", "cluster")
    wrap(local_train, "local_matching", "local")
    wrap(local_train, "local_matching_proxy", "lproxy")
    wrap(ft, "calculate_attention_head_p_m", "heads")


def _sum_check(got, parts, what, extra_adds=0):
    """A float32 sum of the contributions [(reference, bound), ...] each of which the device holds within its bound: the references add up
    to `want`, the bounds add up, and the len(parts) - 1 + extra_adds additions give gamma(.) x the absolute terms."""
    want = sum(p for p, _ in parts)
    tol = sum(t for _, t in parts)
    mag = sum(np.abs(p) + t for p, t in parts)
    return fgb.check(got, want, tol + fgb.gamma(max(len(parts) - 1 + extra_adds, 1)) * mag, what)


@pytest.mark.parametrize("gt_id,absent,background,radii,seed", ((3, None, True, (2, 4, 6), 7), (0, None, True, (2, 4), 7), (3, 2, True, (4,), 7),
                                                                  (2, None, False, (2, 4, 6, 8), 7)))
def test_proto_mask_features_against_the_float64_references(monkeypatch, gt_id, absent, background, radii, seed):
    """proto_mask_features end to end against the float64 references of its operators, composed link by link: every operator inside the
    chain is held to ITS float64 reference (the numpy references of match_grad_bounds, cluster_grad_bounds, local_grad_bounds and
    frontend_grad_bounds, which the host tests hold to the reference's recorded autograd) evaluated at the float32 tensors it actually
    received in the chain, inside ITS OWN bound; a leaf's gradient is the float32 sum of its operators' contributions, so its bound is the sum
    of theirs plus gamma(additions) x the absolute terms.  Because each reference is taken at the operator's actual inputs, no error has to
    be carried from one operator into the next and no tolerance is added: pre_to_cat, attention_head and the five leaf gradients are
    covered, and so are the arguments, label layouts and biases each operator is wired to."""
    h, w, C = 11, 13, 36
    embs, labs, bg, fg = _sample(h, w, C, gt_id, seed, absent)
    O, m, nr = gt_id + 1, h * w, len(radii)
    with torch.no_grad():
        sr = (labs[0].view(1, h, w) == torch.arange(O, device=DEV).view(-1, 1, 1)).float().permute(1, 2, 0)
        pool, labels_flat = matching._flatten_pool([embs[0].detach().permute(1, 2, 0)], [sr], h, w, 1, 0)
        cp = matching.cluster_proxies(pool, labels_flat, 16, None, np.random.RandomState(3))
    rec = {}
    _record(monkeypatch, rec)
    gen = torch.Generator(DEV).manual_seed(5)
    with torch.enable_grad():
        feat, head = ft.proto_mask_features(embs[0], embs[1], embs[2], labs[0], labs[1], gt_id, bg, fg, radii, matching_background=background,
                                            init_rows=cp["init_rows"])
        w_feat, w_head = torch.randn(feat.shape, device=DEV, generator=gen), torch.randn(head.shape, device=DEV, generator=gen)
        ((feat * w_feat).sum() + (head * w_head).sum()).backward()
    assert set(rec) == {"dense", "proxy", "cluster", "local", "lproxy", "heads"}
    ids = np.arange(O)
    lab_ref, lab_prev = ((_np(l)[:, :, None] == ids).astype(f32) for l in labs)                 # [h, w, O], aocnet.py:154, 166
    bias = np.concatenate([_np(bg).reshape(-1)] + [_np(fg).reshape(-1)] * gt_id).astype(f32)    # aocnet.py:143-146
    ref_hwc, prev_hwc, cur_hwc = (_np(e).transpose(1, 2, 0).copy() for e in embs)
    wh = _np(w_head)

    # what each operator received is what aocnet.py:170-337 hands it
    for key, e0, lab in (("dense", ref_hwc, lab_ref), ("cluster", ref_hwc, lab_ref), ("local", prev_hwc, lab_prev)):
        a = rec[key][0]
        assert np.array_equal(_np(a[0]), e0) and np.array_equal(_np(a[1]), cur_hwc) and np.array_equal(_np(a[2]), lab), key + ": operands"
    for key in ("dense", "cluster", "proxy"):
        assert np.array_equal(_np(rec[key][0][4]).reshape(-1), bias) and np.array_equal(_np(rec[key][0][2]), lab_ref), key + ": bias / labels"
    for key in ("local", "lproxy"):
        a = rec[key][0]
        assert np.array_equal(_np(a[3]).reshape(-1), bias) and list(a[4]) == list(radii) and np.array_equal(_np(a[2]), lab_prev), key + ": bias / radii / labels"
    _, rp, rn, pp, pn = rec["heads"][2]
    assert rec["proxy"][0][0] is rp and np.array_equal(_np(rec["proxy"][0][1]), cur_hwc)
    prev_inst = rec["lproxy"][0][0]
    assert np.array_equal(_np(prev_inst), _np(pp)[_np(labs[1]).astype(np.int64)]), "aocnet.py:325: every pixel carries its object's previous-frame proxy"

    # the heads, forward: ATT:134-153 in float64
    got_head = _np(head)
    for k, (e, lab) in enumerate(((_np(embs[0]), lab_ref), (_np(embs[1]), lab_prev))):
        l = lab.reshape(m, O).T.astype(f64)
        e2 = e.reshape(C, m).astype(f64)
        pos = (l @ e2.T) / (l.sum(1) + fgb.eps32(1e-5))[:, None]
        neg = (e2.sum(1)[None] - l @ e2.T) / ((1.0 - l).sum(1) + fgb.eps32(1e-5))[:, None]
        tol_pos, tol_neg = fgb.pool_forward_tol(e.reshape(C, m), l, 1e-5)
        fgb.check(got_head[:, 2 * k * C:(2 * k + 1) * C], pos, tol_pos, f"head {k} positive")
        fgb.check(got_head[:, (2 * k + 1) * C:(2 * k + 2) * C], neg, tol_neg, f"head {k} negative")
    assert np.array_equal(got_head, np.concatenate([_np(t) for t in (rp, rn, pp, pn)], 1))

    # the five matchers at the tensors they received: forward and the three gradients each
    outs = {k: rec[k][2] for k in ("dense", "cluster", "proxy", "local", "lproxy")}
    go = {k: _np(v.grad) for k, v in outs.items()}
    base = dict(in_query=cur_hwc, in_bias=bias, atrous_rate=1, atrous_obj_pixel_num=0, multi_local_distance=np.asarray(radii), ori_size=np.zeros(2),
                allow_downsample=1)
    fwd, dg = mgb.fixture_ref(dict(base, in_ref=ref_hwc, in_labels=lab_ref, weight=go["dense"]))
    fgb.check(_np(outs["dense"]).reshape(m, O).T, fwd["T"], fwd["tol_T"], "global_fg")
    (pT, ptol), pgr = mgb.fixture_proxy_ref(dict(base, in_ref=_np(rp), weight=go["proxy"]))
    fgb.check(_np(outs["proxy"]).reshape(m, O).T, pT, ptol, "proxy_fg")
    offs = cp["seg_offsets"].cpu().numpy()
    km_l = [cp["labels"][offs[o]:offs[o + 1]].cpu().numpy() if cp["seg_k"][o] else None for o in range(O)]
    km_c = [cp["centroids"][o, :cp["seg_k"][o]].cpu().numpy() if cp["seg_k"][o] else None for o in range(O)]
    cg = cgb.cluster_match_ref(cur_hwc.reshape(m, C), ref_hwc.reshape(m, C), lab_ref.reshape(m, O).astype(f64), bias, [16], km_l, km_c,
                               go["cluster"].reshape(m, 2 * O).T)
    fgb.check(_np(outs["cluster"]).reshape(m, 2 * O).T, cg["planes"], cg["tol_planes"], "cluster_fg")
    lg = lgb.fixture_ref(dict(base, in_prev=prev_hwc, in_labels=lab_prev, weight=go["local"]))
    fgb.check(_np(outs["local"]), lg["out"], lg["tol_out"], "local_fg")
    lpg = lgb.fixture_ref(dict(base, in_prev=_np(prev_inst), in_labels=lab_prev, weight=go["lproxy"]))
    fgb.check(_np(outs["lproxy"]), lpg["out"], lpg["tol_out"], "local_proxy_fg")

    # pre_to_cat is aocnet.py:341-358 of those five outputs, and the cotangent reaches them by the stated rule: both exactly
    planes = [_np(outs[k])[0].transpose(2, 3, 0, 1).reshape(O, -1, m) for k in ("dense", "cluster", "proxy", "local", "lproxy")]
    prev_planes = lab_prev.reshape(m, O).T.copy()
    feat_np = fgb.aggregate_np(*planes, prev_planes, background)
    assert np.array_equal(_np(feat).reshape(feat_np.shape), feat_np), "pre_to_cat is not the concatenation of the five outputs"
    want_go = fgb.aggregate_grad_np(_np(w_feat).reshape(feat_np.shape), feat_np, 2, nr, background)
    for k, g in zip(("dense", "cluster", "proxy", "local", "lproxy"), want_go):
        assert np.array_equal(go[k][0].transpose(2, 3, 0, 1).reshape(g.shape), g), k + ": the cotangent that reaches it"

    # the non-leaf links: the pooled heads' gradients and the per-pixel proxy map's
    fgb.check(_np(prev_inst.grad).reshape(m, C), lpg["grad_prev"].reshape(m, C), lpg["tol_prev"].reshape(m, C), "grad of matmul(label, prev_head_pos)")
    _sum_check(_np(rp.grad), [(pgr["grad_proxies"], pgr["tol_proxies"]), (wh[:, :C].astype(f64), 0.0)], "grad of ref_head_pos")
    gi = _np(prev_inst.grad).reshape(m, C).astype(f64)
    l_prev = lab_prev.reshape(m, O).astype(f64)
    n_o = np.maximum(l_prev.sum(0), 1.0)[:, None]                                               # torch's matmul adds an object's pixels in some order
    _sum_check(_np(pp.grad), [(l_prev.T @ gi, fgb.gamma(n_o) * (l_prev.T @ np.abs(gi))), (wh[:, 2 * C:3 * C].astype(f64), 0.0)], "grad of prev_head_pos")

    # the leaves
    pool_ref, tol_pool_ref = fgb.pool_grad_ref(lab_ref.reshape(m, O).T.copy(), _np(rp.grad), wh[:, C:2 * C], 1e-5)
    _sum_check(_np(embs[0].grad).reshape(C, m), [(dg["grad_pool"].T, dg["tol_pool"].T), (cg["grad_pool"].T, cg["tol_pool"].T), (pool_ref, tol_pool_ref)],
               "grad ref_emb")
    pool_prev, tol_pool_prev = fgb.pool_grad_ref(prev_planes, _np(pp.grad), wh[:, 3 * C:], 1e-5)
    _sum_check(_np(embs[1].grad).reshape(C, m), [(lg["grad_prev"].reshape(m, C).T, lg["tol_prev"].reshape(m, C).T), (pool_prev, tol_pool_prev)],
               "grad prev_emb")
    _sum_check(_np(embs[2].grad).reshape(C, m),
               [(dg["grad_query"].T, dg["tol_query"].T), (cg["grad_query"].T, cg["tol_query"].T), (pgr["grad_query"].T, pgr["tol_query"].T),
                (lg["grad_query"].reshape(m, C).T, lg["tol_query"].reshape(m, C).T), (lpg["grad_query"].reshape(m, C).T, lpg["tol_query"].reshape(m, C).T)],
               "grad cur_emb")
    b_parts = [(r["grad_bias"], r["tol_bias"]) for r in (dg, cg, pgr, lg, lpg)]
    _sum_check(_np(bg.grad).reshape(-1), [(p[:1], t[:1]) for p, t in b_parts], "grad bg_bias")
    if gt_id > 0:                                                                              # expand's backward adds the gt_id objects' sums
        _sum_check(_np(fg.grad).reshape(-1), [(p[o:o + 1], t[o:o + 1]) for o in range(1, O) for p, t in b_parts], "grad fg_bias")
    else:
        assert fg.grad is None                                                                 # aocnet.py:146: one object never reads fg_bias
    if absent is not None:
        assert (_np(outs["dense"])[..., absent, :] == 1.0).all() and (got_head[absent, :C] == 0).all()


def test_proto_mask_features_peak_memory():
    h, w, C, gt_id = 31, 33, 100, 3
    O, radii = gt_id + 1, (2, 4, 6, 8, 10, 12)
    embs, labs, bg, fg = _sample(h, w, C, gt_id, 11)
    ref_l = [l for l in labs]

    def run():
        np.random.seed(1)
        with torch.enable_grad():
            feat, head = ft.proto_mask_features(embs[0], embs[1], embs[2], ref_l[0], ref_l[1], gt_id, bg, fg, radii)
            (feat.sum() + head.sum()).backward()
        return feat
    run()                                                                          # warm-up: library and allocator
    for t in embs + [bg, fg]:
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    feat = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    m, nl, kmax = h * w, len(radii), 16
    H2, W2 = h // 2 + 1, w // 2 + 1
    m2 = H2 * W2
    n_ch = ft.aggregate_channels(2, nl)
    output = O * n_ch * m * 4 + O * 4 * C * 4
    # what the operators keep for their backward (their own tests hold each of them to these terms)
    dense = 2 * m * C * 4 + 2 * O * m * 4                                          # query, pool, T, arg
    cluster = 2 * m * C * 4 + 2 * m * 2 * O * 4 + O * 2 * kmax * C * 4 + (2 * m + O + 2) * 4
    proxy = m * C * 4 + O * C * 4 + O * m * 4
    local = 2 * (2 * m2 * C * 4 + 2 * O * nl * m2 * 4)                              # both local calls: q, p at half size, T, arg
    pooling = 2 * O * m * 4                                                         # the labels of both frames: all the heads keep
    mix = m * O * 4 + O * C * 4                                                     # matmul(label, prev_head_pos) keeps its operands
    saved = dense + cluster + proxy + local + pooling + mix + O * n_ch * m * 4      # ... and feat, all the aggregation keeps
    sources = (1 + 2 + 1 + 2 * nl) * O * m * 4                                      # the five matching outputs / their gradients
    grads = (3 * C * m * 4 + 2 * 4                                                  # the leaves
             + sources + O * 4 * C * 4                                              # what reaches the matchers and the heads
             + 5 * m * C * 4 + 2 * m * C * 4 + O * 2 * kmax * C * 4                 # per matcher its query gradient; dense and cluster their pool gradient
             + 2 * 2 * m2 * C * 4 + 4 * m * C * 4                                   # both local calls at half size, and resized back by torch
             + 2 * m * C * 4 + m * C * 4 + 2 * O * C * 4)                           # the pooling gradients of both frames; matmul's two
    output += sources                                                              # the matchers' outputs live until the aggregation has read them
    import cluster_grad_bounds as cgb
    ws = cgb.set_grad_workspace_bytes(m, C, 2 * O * kmax) + cgb.centroid_grad_workspace_bytes(O, kmax) + 256
    print(f"peak above the inputs {peak} bytes; output {output}, saved {saved}, gradients {grads}, workspace {ws}; limit {2 * (output + saved + grads + ws)}")
    assert feat.shape == (O, n_ch, h, w)
    assert peak <= 2 * (output + saved + grads + ws)
