"""The training-time cluster matching on the device: aoc_proxy_set_match_argmin, aoc_proxy_set_match_grad, aoc_centroid_avg_grad and
aoc_amd.cluster_train against the float64 references and derived bounds of tests/cluster_grad_bounds.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aoc_amd
import cluster_grad_bounds as cgb
from aoc_amd import cluster_train, matching, ops
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ------------------------------------------------------------------------------------------ argmin
def _run_argmin(inp, m, transform, pixel_major, use_norms=True, with_corr=True):
    n_set = len(inp["size"])
    pad = 7                                                      # oversized, NaN-filled: nothing outside the addressed elements is written
    if pixel_major:
        stride, offs, shape = n_set + 1, list(range(n_set)), (m + pad, n_set + 1)
    else:
        stride, offs, shape = 1, [s * (m + pad) for s in range(n_set)], (n_set, m + pad)
    q, p = dev(inp["query"]), dev(inp["proxies"])
    sq = dev(inp["sqnorm"]) if use_norms else None
    bias = dev(inp["bias"])
    out = torch.full(shape, float("nan"), device=DEV)
    arg = torch.full(shape, -7, dtype=torch.int32, device=DEV)
    ops.proxy_set_match_argmin(q, p, sq, inp["begin"], inp["size"], offs, bias, out, arg, stride, transform)
    want = None
    if with_corr:
        want = torch.full(shape, float("nan"), device=DEV)
        ops.proxy_corr_min(q, p, sq, inp["begin"], inp["size"], offs, bias, want, stride, transform)
    view = (lambda t: t[:m, :n_set].T) if pixel_major else (lambda t: t[:, :m])
    return out, arg, want, view


@pytest.mark.parametrize("C", cgb.ARGMIN_C)
def test_argmin_values_equal_proxy_corr_min_and_slots_the_float64_argmin(C):
    for k, m in enumerate(cgb.ARGMIN_M):
        transform, pixel_major, use_norms = bool(k % 2 == 0), bool(k % 3 == 1), k != 3
        inp, fwd = cgb.argmin_case_ref(C, m, 0, True, use_norms)
        out, arg, want, view = _run_argmin(inp, m, transform, pixel_major, use_norms)
        assert np.array_equal(out.cpu().numpy(), want.cpu().numpy(), equal_nan=True), f"C={C} m={m}: values differ from aoc_proxy_corr_min"
        got_arg = view(arg).cpu().numpy()
        assert np.array_equal(got_arg, fwd["arg"]), f"C={C} m={m}: {int((got_arg != fwd['arg']).sum())} slots differ from the float64 argmin"
        untouched = arg.clone()
        view(untouched).fill_(-7)
        assert (untouched == -7).all(), "arg written outside the addressed elements"
        n = len(cgb.ARGMIN_SIZES)
        dead = [n, n + 1] if use_norms else [n]                     # the empty set and (where the norms carry its +inf marks) the all-ignored one
        assert (got_arg[dead] == -1).all()
        vals = view(out).cpu().numpy()
        if transform:
            assert (vals[dead] == 1.0).all()
            cgb.check(vals, fwd["T"], fwd["tol_T"], f"argmin T C={C} m={m}")
        else:
            assert (vals[dead] == f32(cgb.PAD)).all()
            cgb.check(vals, fwd["raw"], fwd["tol_raw"], f"argmin raw C={C} m={m}")


def test_argmin_more_than_64_sets_in_one_call():
    inp, fwd = cgb.argmin_case_ref(36, 65, 70, True, True)
    assert len(inp["size"]) > 64
    out, arg, want, view = _run_argmin(inp, 65, True, False)
    assert np.array_equal(out.cpu().numpy(), want.cpu().numpy(), equal_nan=True)
    assert np.array_equal(view(arg).cpu().numpy(), fwd["arg"])


@pytest.mark.parametrize("C", (36, 100, 256))
def test_argmin_ties_go_to_the_lower_slot(C):
    inp = cgb.argmin_case_inputs(C, 65, ties=True)
    out, arg, want, view = _run_argmin(inp, 65, True, False)
    assert np.array_equal(out.cpu().numpy(), want.cpu().numpy(), equal_nan=True)
    got = view(arg).cpu().numpy()
    for s, (lo, hi) in enumerate(cgb.TIE_SLOTS):
        assert (got[s] == lo).all(), f"slots ({lo}, {hi}): got {np.unique(got[s])}"


# ------------------------------------------------------------------------------------------ set gradient
def _run_grad(inp, fwd, T32, want=(True, True, True)):
    m = inp["query"].shape[0]
    n_set = len(inp["size"])
    offs = [s * m for s in range(n_set)]
    arg = fwd["arg"].astype(np.int32)
    return ops.proxy_set_match_backward(dev(inp["grad_out"]), dev(T32), dev(arg), 1, dev(inp["query"]), dev(inp["proxies"]), inp["begin"], inp["size"],
                                        offs, inp["bias_index"], inp["n_bias"], *want)


def _check_grad(inp, fwd, T32, grad, what):
    gq, gp, gb = _run_grad(inp, fwd, T32)
    r = [cgb.check(gq.cpu().numpy(), grad["grad_query"], grad["tol_query"], what + " grad_query"),
         cgb.check(gp.cpu().numpy(), grad["grad_proxies"], grad["tol_proxies"], what + " grad_proxies"),
         cgb.check(gb.cpu().numpy(), grad["grad_bias"], grad["tol_bias"], what + " grad_bias")]
    gpn = gp.cpu().numpy()
    assert (gpn[grad["chosen"] == 0] == 0.0).all(), what + ": a row nobody chose is not zero"
    gq2, gp2, gb2 = _run_grad(inp, fwd, T32)
    assert torch.equal(gq, gq2) and torch.equal(gp, gp2) and torch.equal(gb, gb2), what + ": two runs differ"
    return max(r)


@pytest.mark.parametrize("C", cgb.GRAD_C)
def test_set_grad_inside_the_bound(C):
    for m in cgb.GRAD_M:
        inp, fwd, T32, grad = cgb.grad_case_ref(C, m, 3)
        assert (fwd["arg"][3] == -1).all()                                       # an arg = -1 column
        _check_grad(inp, fwd, T32, grad, f"C={C} m={m} O=3")


@pytest.mark.parametrize("n_obj", cgb.GRAD_OBJECTS)
def test_set_grad_object_counts(n_obj):
    inp, fwd, T32, grad = cgb.grad_case_ref(36, 65, n_obj)
    _check_grad(inp, fwd, T32, grad, f"O={n_obj}")


def test_set_grad_more_than_64_sets_in_one_call():
    inp, fwd, T32, grad = cgb.grad_case_ref(36, 65, 33)                           # 66 sets: two launches, the second adds to the first's outputs
    assert len(inp["size"]) > cgb.CG_SETS
    _check_grad(inp, fwd, T32, grad, "O=33")


@pytest.mark.parametrize("C", (100, 256))
def test_set_grad_one_proxy_chosen_by_every_pixel(C):
    inp, fwd, T32, grad = cgb.grad_case_ref(C, 257, 3, "hot")
    assert (fwd["arg"] == 1).all() and grad["chosen"].max() == 257 and (grad["chosen"] == 0).sum() >= 12
    _check_grad(inp, fwd, T32, grad, f"hot C={C}")


def test_set_grad_each_output_null_in_turn():
    inp, fwd, T32, grad = cgb.grad_case_ref(36, 65, 3)
    full = _run_grad(inp, fwd, T32)
    for k in range(3):
        want = [True] * 3
        want[k] = False
        got = _run_grad(inp, fwd, T32, tuple(want))
        assert got[k] is None
        for j in range(3):
            if j != k:
                assert torch.equal(got[j], full[j])


# ------------------------------------------------------------------------------------------ mean pull-back
@pytest.mark.parametrize("levels", (1, 2))
def test_centroid_avg_grad(levels):
    c = cgb.pullback_case(levels)
    gp64 = c["grad_proxies"].astype(np.float64)
    want, tol, _ = cgb.centroid_grad_ref(gp64, np.zeros_like(gp64), c["fg_rows"], c["n_fg"], c["seg_offsets"], c["seg_k"], c["labels"], c["pool_rows"])
    fg = np.full(c["pool_rows"], -1, np.int32)
    fg[:c["n_fg"]] = c["fg_rows"]
    args = (dev(c["grad_proxies"]), dev(fg), dev(np.asarray([c["n_fg"]], np.int32)), dev(c["seg_offsets"]), dev(c["seg_k"]), dev(c["labels"]),
            c["pool_rows"])
    got = ops.centroid_avg_backward(*args)
    g = got.cpu().numpy()
    must_be_zero = np.ones(c["pool_rows"], bool)
    must_be_zero[c["fg_rows"][:300]] = False
    assert (g[must_be_zero] == 0.0).all() and must_be_zero.sum() == 100
    assert np.abs(g[~must_be_zero]).min() > 0
    cgb.check(g, want, tol, f"centroid_avg_grad levels={levels}")
    assert torch.equal(got, ops.centroid_avg_backward(*args)), "two runs differ"


# ------------------------------------------------------------------------------------------ end to end
def _fixture_tensors(fx, bias_form="O111"):
    ref = dev(fx["in_ref"]).requires_grad_(True)
    q = dev(fx["in_query"]).requires_grad_(True)
    lab = dev(fx["in_labels"], torch.float32)
    if bias_form == "O111":
        b = dev(fx["in_bias"]).view(-1, 1, 1, 1).requires_grad_(True)
    else:
        b = dev(fx["in_bias"]).requires_grad_(True)
    return ref, q, lab, b


def _fixture_call(fx, ref, q, lab, b, rows, **kw):
    return cluster_train.global_matching_cluster2(ref, q, lab, int(fx["n_chunks"]), b, kw.pop("ori_size", None), int(fx["atrous_rate"]), False,
                                                  int(fx["atrous_obj_pixel_num"]), init_rows=rows, **kw)


@pytest.mark.parametrize("name", cgb.FIXTURES)
def test_end_to_end_against_the_recorded_gradients(name):
    fx = load_golden(name)
    want = cgb.fixture_ref_by_name(name)
    km_labels, km_cents, rows = cgb.fixture_km(fx)
    ref, q, lab, b = _fixture_tensors(fx)
    lab_before = lab.clone()
    # the device k-means chain reproduces the recorded clustering bit for bit
    h, w, _ = fx["in_query"].shape
    with torch.no_grad():
        labels = matching._train_twin_labels(lab, h, w, int(fx["atrous_rate"]), int(fx["atrous_obj_pixel_num"]))
        pool, labels_flat = matching._flatten_pool([ref.detach()], [labels], h, w, 1, 0)
        cp = matching.cluster_proxies(pool, labels_flat, 16, rows)
    offs = cp["seg_offsets"].cpu().numpy()
    for o, (l, c) in enumerate(zip(km_labels, km_cents)):
        if l is None:
            assert cp["seg_k"][o] == 0
            continue
        assert np.array_equal(cp["labels"][offs[o]:offs[o + 1]].cpu().numpy(), l), f"object {o}: labels differ from the km log"
        assert np.array_equal(cp["centroids"][o, :c.shape[0]].cpu().numpy(), c), f"object {o}: code book differs from the km log"
    with torch.enable_grad():
        out = _fixture_call(fx, ref, q, lab, b, rows)
        assert out.shape == fx["out"].shape
        (out * dev(fx["weight"])).sum().backward()
    assert torch.equal(lab, lab_before), "the caller's label tensor was written"
    cgb.check(out.detach().cpu().numpy(), fx["out"], want["tol_out"], name + " out")
    cgb.check(q.grad.cpu().numpy().reshape(-1, q.shape[2]), fx["grad_query"].reshape(-1, q.shape[2]), want["tol_query"], name + " grad_query")
    cgb.check(ref.grad.cpu().numpy(), fx["grad_ref"], want["tol_ref"], name + " grad_ref")
    cgb.check(b.grad.cpu().numpy().reshape(-1), fx["grad_bias"], want["tol_bias"], name + " grad_bias")
    if name == "cluster_grad_absent":
        assert (out.detach()[..., 2, :] == 1.0).all() and b.grad.reshape(-1)[2] == 0.0


def test_end_to_end_no_grad_bits_double_backward_and_bias_forms():
    fx = load_golden("cluster_grad_C36_O3")
    _, _, rows = cgb.fixture_km(fx)
    ref, q, lab, b = _fixture_tensors(fx)
    with torch.enable_grad():
        out = _fixture_call(fx, ref, q, lab, b, rows)
        g = torch.autograd.grad((out * dev(fx["weight"])).sum(), [ref, q, b], create_graph=True)
        with pytest.raises(RuntimeError):
            g[1].sum().backward()                                             # once_differentiable: a double backward raises
    with torch.no_grad():
        plain = matching.global_matching_for_eval_cluster([ref.detach()], q.detach(), [lab], 3, b.detach(), None, 1, False, 0, rows, 16)
        same = _fixture_call(fx, ref, q, lab, b, rows)
        np.random.seed(5)
        a = cluster_train.global_matching_cluster2(ref, q, lab, 3, b, None, 1, False, 0)
        np.random.seed(5)
        a2 = matching.global_matching_cluster2(ref, q, lab, 3, b, None, 1, False, 0)
    assert torch.equal(same, plain) and torch.equal(out.detach(), plain), "the training forward differs from the mirror's bits"
    assert torch.equal(a, a2)
    # a one-element bias tensor and a float
    b1 = torch.tensor([0.25], device=DEV, requires_grad=True)
    bO = torch.full((3, 1, 1, 1), 0.25, device=DEV, requires_grad=True)
    with torch.enable_grad():
        o1 = _fixture_call(fx, ref, q, lab, b1, rows)
        o1.sum().backward()
        oO = _fixture_call(fx, ref, q, lab, bO, rows)
        oO.sum().backward()
        oF = _fixture_call(fx, ref, q, lab, 0.25, rows)
    assert torch.equal(o1, oO) and torch.equal(oF, oO) and b1.grad.shape == (1,) and bO.grad.shape == (3, 1, 1, 1)
    assert abs(float(b1.grad) - float(bO.grad.sum())) <= 1e-5 * float(bO.grad.abs().sum())


def test_end_to_end_ori_size_and_levels():
    fx = load_golden("cluster_grad_C36_O3")
    _, _, rows = cgb.fixture_km(fx)
    h, w, C = fx["in_query"].shape
    ref, q, lab, b = _fixture_tensors(fx)
    H, W = 2 * h + 1, 2 * w - 3
    wt = torch.randn(1, H, W, 3, 2, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    with torch.enable_grad():
        base = _fixture_call(fx, ref, q, lab, b, rows)
        big = _fixture_call(fx, ref, q, lab, b, rows, ori_size=(H, W))
        (big * wt).sum().backward()
    assert big.shape == (1, H, W, 3, 2)
    x = base.detach()[0].permute(2, 3, 0, 1).reshape(6, 1, h, w).requires_grad_(True)
    with torch.enable_grad():
        y = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True)
        assert torch.equal(y.view(3, 2, H, W).permute(2, 3, 0, 1).reshape(1, H, W, 3, 2), big.detach())
        (y * wt[0].permute(2, 3, 0, 1).reshape(6, 1, H, W)).sum().backward()
    # the gradient that reaches the planes is torch's; from there on the reference at that grad_out, whose error is the resize's fp32 sums
    go = x.grad.view(3, 2, h * w).reshape(6, h * w).cpu().numpy().astype(np.float64)
    k = (2 * -(-H // (h - 1)) + 2) * (2 * -(-W // (w - 1)) + 2)
    with torch.enable_grad():
        xa = torch.zeros(6, 1, h, w, device=DEV, dtype=torch.float64, requires_grad=True)
        (F.interpolate(xa, size=(H, W), mode="bilinear", align_corners=True) * wt[0].permute(2, 3, 0, 1).reshape(6, 1, H, W).abs().double()).sum().backward()
    e_go = cgb.gamma(k) * xa.grad.view(6, h * w).cpu().numpy()
    km_labels, km_cents, _ = cgb.fixture_km(fx)
    lab_flat = fx["in_labels"].reshape(-1, 3).astype(np.float64)
    want = cgb.cluster_match_ref(fx["in_query"].reshape(-1, C), fx["in_ref"].reshape(-1, C), lab_flat, fx["in_bias"], [16], km_labels, km_cents, go, e_go)
    cgb.check(q.grad.cpu().numpy().reshape(-1, C), want["grad_query"], want["tol_query"], "ori_size grad_query")
    cgb.check(ref.grad.cpu().numpy().reshape(-1, C), want["grad_pool"], want["tol_pool"], "ori_size grad_ref")
    cgb.check(b.grad.cpu().numpy().reshape(-1), want["grad_bias"], want["tol_bias"], "ori_size grad_bias")
    # levels [8, 16]: [1, h, w, O, 4]; the level-16 planes are the single-level call's, the level-8 planes follow the float64 reference
    with torch.no_grad():
        labels = matching._train_twin_labels(lab, h, w, 1, 0)
        pool, labels_flat = matching._flatten_pool([ref.detach()], [labels], h, w, 1, 0)
        cp = matching.cluster_proxies(pool, labels_flat, [8, 16], [None, rows])
    for t in (ref, q, b):
        t.grad = None
    wt4 = torch.randn(1, h, w, 3, 4, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    with torch.enable_grad():
        two = cluster_train.global_matching_cluster2(ref, q, lab, 3, b, None, 1, False, 0, init_rows=cp["init_rows"], cluster_num=[8, 16])
        (two * wt4).sum().backward()
    assert two.shape == (1, h, w, 3, 4) and torch.equal(two.detach()[..., 2:], base.detach())
    offs = cp["seg_offsets"].cpu().numpy()
    kl = [cp["labels"][offs[s]:offs[s + 1]].cpu().numpy() for s in range(6)]
    kc = [cp["centroids"][s, :cp["seg_k"][s // 3][s % 3]].cpu().numpy() for s in range(6)]
    go4 = wt4.reshape(h * w, 12).T.cpu().numpy().astype(np.float64)
    want = cgb.cluster_match_ref(fx["in_query"].reshape(-1, C), fx["in_ref"].reshape(-1, C), lab_flat, fx["in_bias"], [8, 16], kl, kc, go4)
    live = want["fwd"]["arg"] >= 0
    assert (want["fwd"]["gap"][live] >= cgb.GAP_FACTOR * want["fwd"]["e_best"][live]).all(), "the level-8 clustering puts a pixel near a tie"
    cgb.check(two.detach().cpu().numpy().reshape(h * w, 12).T, want["planes"], want["tol_planes"], "levels out")
    cgb.check(q.grad.cpu().numpy().reshape(-1, C), want["grad_query"], want["tol_query"], "levels grad_query")
    cgb.check(ref.grad.cpu().numpy().reshape(-1, C), want["grad_pool"], want["tol_pool"], "levels grad_ref")
    cgb.check(b.grad.cpu().numpy().reshape(-1), want["grad_bias"], want["tol_bias"], "levels grad_bias")


def test_end_to_end_peak_memory():
    h, w, C, O = 31, 33, 100, 4
    rs = np.random.RandomState(11)
    ref = dev((0.12 * rs.standard_normal((h, w, C))).astype(f32)).requires_grad_(True)
    q = dev((0.12 * rs.standard_normal((h, w, C))).astype(f32)).requires_grad_(True)
    lab = dev(np.eye(O, dtype=f32)[rs.randint(0, O, (h, w))])
    b = torch.zeros(O, 1, 1, 1, device=DEV, requires_grad=True)
    np.random.seed(1)
    with torch.enable_grad():
        cluster_train.global_matching_cluster2(ref, q, lab, 3, b, None, 1, False, 0).sum().backward()      # warm-up: library and allocator
    for t in (ref, q, b):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    np.random.seed(1)
    with torch.enable_grad():
        out = cluster_train.global_matching_cluster2(ref, q, lab, 3, b, None, 1, False, 0)
        out.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    m, n_set, kmax = h * w, 2 * O, 16
    output = m * n_set * 4
    saved = 2 * m * C * 4 + 2 * m * n_set * 4 + O * 2 * kmax * C * 4 + (m + m + O + 2) * 4      # q, pool, T, arg, proxies, labels, fg_rows, offsets
    grads = 2 * m * C * 4 + O * 4 + O * 2 * kmax * C * 4
    ws = cgb.set_grad_workspace_bytes(m, C, n_set * kmax) + cgb.centroid_grad_workspace_bytes(O, kmax)
    print(f"peak above the inputs {peak} bytes; output {output}, saved {saved}, gradients {grads}, workspace {ws}")
    assert peak <= 2 * (output + saved + grads + ws)
