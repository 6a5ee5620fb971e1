"""The training-time global matching on the MI355X: aoc_dense_match_argmin against aoc_dense_match_min (bit for bit) and the float64 argmin,
aoc_dense_match_grad / aoc_proxy_match_grad against the float64 references under the derived bounds of tests/match_grad_bounds.py, and
aoc_amd.matching_train end to end against the gradients the reference's own autograd recorded (tests/golden/match_grad_*.npz).

The autouse fixture of conftest.py wraps GPU tests in torch.no_grad(); the tests that need a graph open torch.enable_grad() themselves.
Every check prints its worst error / bound before it asserts; a module fixture prints the largest per quantity after the last test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aoc_amd
import match_grad_bounds as mgb
from aoc_amd import ops
from conftest import load_golden
from float64_bounds import U, gamma

pytestmark = pytest.mark.gpu
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _print_worst_ratios():
    """After the module's last test: the largest error / bound per quantity among the checks that ran (STATUS.md quotes a full run's)."""
    yield
    worst = {}
    for what, r in REPORT:
        key = what.split()[-1] if "proxy" not in what else "proxy " + what.split()[-1]
        worst[key] = max(worst.get(key, 0.0), r)
    for key in sorted(worst):
        print(f"match_grad worst error / bound, {key}: {worst[key]:.3f}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def layout(case_layout, m, n_obj, gap=False):
    """-> (pixel stride, object stride, buffer elements, named [O, m] flat indices); views start at element 2.  gap: every other slot unused."""
    ps, os_ = (1, m) if case_layout == "planes" else (n_obj, 1)
    if gap:
        ps, os_ = 2 * ps, 2 * os_
    named = 2 + ps * np.arange(m)[None, :] + os_ * np.arange(n_obj)[:, None]
    return ps, os_, int(named.max()) + 8, named


def place(values, named, size, fill, dtype):
    buf = np.full(size, fill, dtype)
    buf[named.ravel()] = np.asarray(values, dtype).ravel()
    return dev(buf)


def forward(inp, case_layout, transform=True, gap=False):
    """aoc_dense_match_argmin and aoc_dense_match_min into NaN / -7 filled oversized buffers -> (out buffer, arg buffer, min's buffer, named, prep)."""
    m, n_obj = inp["query"].shape[0], inp["labels"].shape[1]
    ps, os_, size, named = layout(case_layout, m, n_obj, gap)
    q, p = dev(inp["query"]), dev(inp["pool"])
    prep = ops.label_prep(dev(inp["labels"]))
    bias = dev(inp["bias"])
    out = torch.full((size,), float("nan"), device="cuda")
    arg = torch.full((size,), -7, dtype=torch.int32, device="cuda")
    plain = torch.full((size,), float("nan"), device="cuda")
    ops.dense_match_argmin(q, p, prep, bias, out[2:], arg[2:], ps, os_, transform)
    ops.dense_match_min(q, p, prep, bias, plain[2:], ps, os_, transform)
    return out, arg, plain, named, (ps, os_, q, p)


ALL_DENSE = [c.name for c in mgb.DENSE_GRAD_CASES] + [mgb.NO_ROWS.name, mgb.TIES.name]


@pytest.mark.parametrize("name", ALL_DENSE)
def test_argmin_forward_equals_dense_match_min_and_the_float64_argmin(name):
    case = mgb.DENSE_BY_NAME[name]
    inp, fwd, _ = mgb.dense_case_ref(name)
    for transform in (True, False):
        out, arg, plain, named, _ = forward(inp, case.layout, transform)
        assert torch.equal(out.view(torch.int32), plain.view(torch.int32)), f"{name}: values differ from aoc_dense_match_min (transform={transform})"
        a = arg.cpu().numpy()
        mask = np.zeros(a.size, bool)
        mask[named.ravel()] = True
        assert (a[~mask] == -7).all(), f"{name}: arg was written outside its layout"
        assert np.isnan(out.cpu().numpy()[~mask]).all(), f"{name}: out was written outside its layout"
        wrong = int((a[named] != fwd["arg"]).sum())
        assert wrong == 0, f"{name}: {wrong} of {named.size} minimisers differ from the float64 argmin"
        got = out.cpu().numpy()[named]
        if transform:
            if case.n_fg == 0:
                assert (got == 1.0).all() and (a[named] == -1).all()
            else:
                mgb.check(got, fwd["T"], fwd["tol_T"], f"{name} T", REPORT)
            assert (got[a[named] < 0] == 1.0).all(), "T is exactly 1 where there is no minimiser"
    if case.absent is not None:
        assert (a[named][case.absent] == -1).all()


def test_planted_ties_go_to_the_lowest_pool_row():
    inp, fwd, grad = mgb.dense_case_ref(mgb.TIES.name)
    out, arg, _, named, (ps, os_, q, p) = forward(inp, "planes")
    a = arg.cpu().numpy()[named]
    for r, later in inp["dup"]:
        assert (a == r).any() and not np.isin(a, later).any(), "a later copy of a duplicated row won"
    go = place(inp["grad_out"], named, out.numel(), np.nan, np.float32)
    _, gp, _ = ops.dense_match_backward(go[2:], out[2:], arg[2:], ps, os_, q, p, 3, want_query=False, want_bias=False)
    gp = gp.cpu().numpy()
    for r, later in inp["dup"]:
        assert (gp[later] == 0.0).all() and np.abs(gp[r]).max() > 0


def _backward_checks(name, got, grad, n_obj):
    gq, gp, gb = (t.cpu().numpy() for t in got)
    mgb.check(gq, grad["grad_query"], grad["tol_query"], f"{name} grad_query", REPORT)
    mgb.check(gp, grad["grad_pool"], grad["tol_pool"], f"{name} grad_pool", REPORT)
    mgb.check(gb, grad["grad_bias"], grad["tol_bias"], f"{name} grad_bias", REPORT)
    assert (gp[grad["counts"] == 0] == 0.0).all(), f"{name}: a row nobody chose has a gradient"


@pytest.mark.parametrize("name", [c.name for c in mgb.DENSE_GRAD_CASES])
def test_dense_backward_within_the_derived_bound_and_deterministic(name):
    case = mgb.DENSE_BY_NAME[name]
    inp, fwd, grad = mgb.dense_case_ref(name)
    out, arg, _, named, (ps, os_, q, p) = forward(inp, case.layout)
    go = place(inp["grad_out"], named, out.numel(), np.nan, np.float32)
    first = ops.dense_match_backward(go[2:], out[2:], arg[2:], ps, os_, q, p, case.n_obj)
    _backward_checks(name, first, grad, case.n_obj)
    kept, _ = mgb.labels_to_bits(inp["labels"])
    unkept = np.setdiff1d(np.arange(inp["pool"].shape[0]), kept)
    assert unkept.size and (first[1].cpu().numpy()[unkept] == 0.0).all(), "an unkept row has a gradient"
    again = ops.dense_match_backward(go[2:], out[2:], arg[2:], ps, os_, q, p, case.n_obj)
    for a, b, what in zip(first, again, ("grad_query", "grad_pool", "grad_bias")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two runs give different bits for {what}"
    if case.kind == "hot":
        assert grad["counts"].max() > mgb.MG_LIST


def test_dense_backward_no_rows_and_zero_grad_out():
    inp, fwd, grad = mgb.dense_case_ref(mgb.NO_ROWS.name)
    out, arg, _, named, (ps, os_, q, p) = forward(inp, "planes")
    go = place(inp["grad_out"], named, out.numel(), np.nan, np.float32)
    for t in ops.dense_match_backward(go[2:], out[2:], arg[2:], ps, os_, q, p, 3):
        assert (t == 0).all(), "nothing is labelled: every gradient is zero"
    name = "C100_m257_O3"
    inp, fwd, grad = mgb.dense_case_ref(name)
    out, arg, _, named, (ps, os_, q, p) = forward(inp, "planes")
    zero = place(np.zeros_like(inp["grad_out"]), named, out.numel(), np.nan, np.float32)
    for t in ops.dense_match_backward(zero[2:], out[2:], arg[2:], ps, os_, q, p, 3):
        assert (t == 0).all(), "grad_out of zeros"


@pytest.mark.parametrize("case_layout", ["planes", "pixels"])
def test_dense_backward_strided_buffers(case_layout):
    """grad_out, T and arg in buffers with every other slot unused (NaN / -7 there): non-contiguous, and nothing outside the layout is read."""
    name = "C36_m99_O17"
    inp, fwd, grad = mgb.dense_case_ref(name)
    out, arg, _, named, (ps, os_, q, p) = forward(inp, case_layout, gap=True)
    go = place(inp["grad_out"], named, out.numel(), np.nan, np.float32)
    got = ops.dense_match_backward(go[2:], out[2:], arg[2:], ps, os_, q, p, 17)
    _backward_checks(f"{name} strided {case_layout}", got, grad, 17)


@pytest.mark.parametrize("name", [c.name for c in mgb.WIDE_GRAD_CASES])
def test_dense_backward_above_the_forward_width(name):
    """C = 256: wider than aoc_dense_match_argmin takes, so T (the float32 rounding of the reference's) and arg come from the reference."""
    case = mgb.DENSE_BY_NAME[name]
    inp, fwd, T32, grad = mgb.wide_case_ref(name)
    ps, os_, size, named = layout(case.layout, case.m, case.n_obj)
    T = place(T32, named, size, np.nan, np.float32)
    arg = place(fwd["arg"], named, size, -7, np.int32)
    go = place(inp["grad_out"], named, size, np.nan, np.float32)
    q, p = dev(inp["query"]), dev(inp["pool"])
    first = ops.dense_match_backward(go[2:], T[2:], arg[2:], ps, os_, q, p, case.n_obj)
    _backward_checks(name, first, grad, case.n_obj)
    again = ops.dense_match_backward(go[2:], T[2:], arg[2:], ps, os_, q, p, case.n_obj)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two runs give different bits"


@pytest.mark.parametrize("want", ["query", "pool", "bias"])
def test_dense_backward_subsets_leave_unwanted_buffers_alone(want):
    name = "C100_m99_O30"
    case = mgb.DENSE_BY_NAME[name]
    inp, fwd, grad = mgb.dense_case_ref(name)
    out, arg, _, named, (ps, os_, q, p) = forward(inp, case.layout)
    go = place(inp["grad_out"], named, out.numel(), np.nan, np.float32)
    bufs = dict(query=torch.full_like(q, float("nan")), pool=torch.full_like(p, float("nan")), bias=torch.full((30,), float("nan"), device="cuda"))
    got = ops.dense_match_backward(go[2:], out[2:], arg[2:], ps, os_, q, p, 30, want == "query", want == "pool", want == "bias",
                                   grad_query=bufs["query"], grad_pool=bufs["pool"], grad_bias=bufs["bias"])
    for key, t in zip(("query", "pool", "bias"), got):
        if key == want:
            mgb.check(t.cpu().numpy(), grad["grad_" + key], grad["tol_" + key], f"{name} only grad_{key}", REPORT)
        else:
            assert t is None and torch.isnan(bufs[key]).all(), f"grad_{key} was not wanted but its buffer was written"


@pytest.mark.parametrize("name", [c[0] for c in mgb.PROXY_GRAD_CASES + mgb.PROXY_WIDE_CASES])
def test_proxy_backward_within_the_derived_bound_and_deterministic(name):
    inp, (T, tol_T), grad = mgb.proxy_case_ref(name)
    n_obj, m = T.shape
    q, p, bias = dev(inp["query"]), dev(inp["proxies"]), dev(inp["bias"])
    for case_layout in ("planes", "pixels"):
        ps, os_, size, named = layout(case_layout, m, n_obj)
        out = torch.full((size,), float("nan"), device="cuda")
        ops.proxy_corr_min(q, p, None, list(range(n_obj)), [1] * n_obj, [2 + o * os_ for o in range(n_obj)], bias, out, ps, True)
        mgb.check(out.cpu().numpy()[named], T, tol_T, f"{name} T", REPORT)
        go = place(inp["grad_out"], named, size, np.nan, np.float32)
        first = ops.proxy_match_backward(go[2:], out[2:], ps, os_, q, p)
        for t, key in zip(first, ("query", "proxies", "bias")):
            mgb.check(t.cpu().numpy(), grad["grad_" + key], grad["tol_" + key], f"{name} proxy grad_{key}", REPORT)
        again = ops.proxy_match_backward(go[2:], out[2:], ps, os_, q, p)
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two runs give different bits"
    only = ops.proxy_match_backward(go[2:], out[2:], ps, os_, q, p, want_query=False, want_bias=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1], first[1])


# ------------------------------------------------------------------------------------------ end to end through matching_train
def _leaf(a):
    return dev(np.asarray(a, np.float32)).requires_grad_(True)


def _slack(ref, recorded):
    """The recorded values are the yardstick; the bound was derived around the numpy reference, which reproduces them to 1e-12."""
    return np.abs(np.asarray(ref, np.float64) - np.asarray(recorded, np.float64).reshape(np.shape(ref)))


@pytest.mark.parametrize("name", mgb.FIXTURES_DENSE)
def test_matching_train_against_the_reference_recorded_gradients(name):
    fx = load_golden(name)
    h, w, C = fx["in_query"].shape
    n_obj = fx["in_labels"].shape[2]
    fwd, grad = mgb.fixture_ref(fx)
    ref, q = _leaf(fx["in_ref"]), _leaf(fx["in_query"])
    bias = _leaf(fx["in_bias"].reshape(-1, 1, 1, 1))
    labels = dev(fx["in_labels"].astype(np.float32))
    before = labels.clone()
    with torch.enable_grad():
        out = aoc_amd.matching_train.global_matching(ref, q, labels, int(fx["n_chunks"]), bias, None, int(fx["atrous_rate"]), False,
                                                     int(fx["atrous_obj_pixel_num"]))
        (out * dev(fx["weight"])).sum().backward()
    assert torch.equal(labels, before), "the labels were written into"
    assert out.shape == (1, h, w, n_obj, 1)
    T_rec = fx["out"].reshape(h * w, n_obj).T
    mgb.check(out.detach().cpu().numpy().reshape(h * w, n_obj).T, T_rec, fwd["tol_T"] + _slack(fwd["T"], T_rec), f"{name} out", REPORT)
    rec_q, rec_r = fx["grad_query"].reshape(-1, C), fx["grad_ref"].reshape(-1, C)
    mgb.check(q.grad.cpu().numpy().reshape(-1, C), rec_q, grad["tol_query"] + _slack(grad["grad_query"], rec_q), f"{name} grad_query", REPORT)
    mgb.check(ref.grad.cpu().numpy().reshape(-1, C), rec_r, grad["tol_pool"] + _slack(grad["grad_pool"], rec_r), f"{name} grad_ref", REPORT)
    assert bias.grad.shape == bias.shape
    mgb.check(bias.grad.cpu().numpy().reshape(-1), fx["grad_bias"], grad["tol_bias"] + _slack(grad["grad_bias"], fx["grad_bias"]),
              f"{name} grad_bias", REPORT)
    with torch.no_grad():
        same = aoc_amd.matching_train.global_matching(ref, q, labels, 1, bias, None, int(fx["atrous_rate"]), False, int(fx["atrous_obj_pixel_num"]))
        mirror = aoc_amd.matching.global_matching(ref, q, labels, 1, bias, None, int(fx["atrous_rate"]), False, int(fx["atrous_obj_pixel_num"]))
    assert torch.equal(same, mirror), "without a graph the twin must return the mirror's bits"


def test_matching_train_unlabelled_is_the_constant_without_a_graph():
    fx = load_golden(mgb.FIXTURE_UNLABELLED)
    h, w, _ = fx["in_query"].shape
    ref, q = _leaf(fx["in_ref"]), _leaf(fx["in_query"])
    labels = dev(fx["in_labels"].astype(np.float32))
    with torch.enable_grad():
        out = aoc_amd.matching_train.global_matching(ref, q, labels, 1, _leaf(fx["in_bias"].reshape(-1, 1, 1, 1)), (2 * h, 2 * w), 1, False, 0)
        prox = aoc_amd.matching_train.global_matching_proxy(_leaf(fx["in_ref"].reshape(-1, fx["in_ref"].shape[2])[:3]), q, labels, 1, 0., None, 1, False, 0)
    for t in (out, prox):
        assert t.shape == (1, h, w, 3, 1) and (t == 1).all() and not t.requires_grad     # AEM:666-667, 385-386: (h, w) even with ori_size
    assert np.array_equal(out.cpu().numpy(), fx["out"])


def test_matching_train_proxy_against_the_reference_recorded_gradients():
    fx = load_golden(mgb.FIXTURE_PROXY)
    h, w, C = fx["in_query"].shape
    n_obj = fx["in_ref"].shape[0]
    (T, tol_T), grad = mgb.fixture_proxy_ref(fx)
    prox, q, bias = _leaf(fx["in_ref"]), _leaf(fx["in_query"]), _leaf(fx["in_bias"].reshape(-1, 1, 1, 1))
    labels = dev(fx["in_labels"].astype(np.float32))
    with torch.enable_grad():
        out = aoc_amd.matching_train.global_matching_proxy(prox, q, labels, 2, bias, None, 1, False, 0)
        (out * dev(fx["weight"])).sum().backward()
    T_rec = fx["out"].reshape(h * w, n_obj).T
    mgb.check(out.detach().cpu().numpy().reshape(h * w, n_obj).T, T_rec, tol_T + _slack(T, T_rec), "proxy out", REPORT)
    rec_q = fx["grad_query"].reshape(-1, C)
    mgb.check(q.grad.cpu().numpy().reshape(-1, C), rec_q, grad["tol_query"] + _slack(grad["grad_query"], rec_q), "proxy fixture grad_query", REPORT)
    mgb.check(prox.grad.cpu().numpy(), fx["grad_ref"], grad["tol_proxies"] + _slack(grad["grad_proxies"], fx["grad_ref"]), "proxy fixture grad_ref", REPORT)
    mgb.check(bias.grad.cpu().numpy().reshape(-1), fx["grad_bias"], grad["tol_bias"] + _slack(grad["grad_bias"], fx["grad_bias"]),
              "proxy fixture grad_bias", REPORT)
    with torch.no_grad():
        assert torch.equal(aoc_amd.matching_train.global_matching_proxy(prox, q, labels, 2, bias, None, 1, False, 0),
                           aoc_amd.matching.global_matching_proxy(prox, q, labels, 2, bias, None, 1, False, 0))


def test_matching_train_one_element_bias_and_wanted_subsets():
    """A one-element dis_bias expanded to O objects: its gradient has one element, the sum over the objects.  A float dis_bias and a
    reference that wants no gradient get none."""
    fx = load_golden("match_grad_dense_C36_O4")
    h, w, C = fx["in_query"].shape
    n_obj = 4
    b1 = np.float32(0.2)
    lab = fx["in_labels"].reshape(-1, n_obj)
    q32, p32 = fx["in_query"].reshape(-1, C).astype(np.float32), fx["in_ref"].reshape(-1, C).astype(np.float32)
    fwd = mgb.dense_forward_ref(q32, p32, lab, np.full(n_obj, b1, np.float32))
    mgb.check_case_conditions("one-element bias", fwd)
    grad = mgb.dense_grad_ref(fx["weight"].reshape(h * w, n_obj).T, fwd["T"], fwd["tol_T"], fwd["arg"], q32, p32)
    ref, q, bias = dev(fx["in_ref"]), _leaf(fx["in_query"]), _leaf(np.asarray([b1]))
    labels = dev(fx["in_labels"].astype(np.float32))
    with torch.enable_grad():
        out = aoc_amd.matching_train.global_matching(ref, q, labels, 1, bias, None, 1, False, 0)
        (out * dev(fx["weight"])).sum().backward()
    assert bias.grad.shape == (1,) and ref.grad is None
    # the expanded gradient is summed by torch: O - 1 more float32 additions of the per-object sums
    tol = grad["tol_bias"].sum() + gamma(n_obj) * (np.abs(grad["grad_bias"]) + grad["tol_bias"]).sum()
    mgb.check(bias.grad.cpu().numpy(), np.asarray([grad["grad_bias"].sum()]), np.asarray([tol]), "one-element bias grad", REPORT)
    mgb.check(q.grad.cpu().numpy().reshape(-1, C), grad["grad_query"], grad["tol_query"], "one-element bias grad_query", REPORT)
    q2 = _leaf(fx["in_query"])
    with torch.enable_grad():
        out2 = aoc_amd.matching_train.global_matching(ref, q2, labels, 1, float(b1), None, 1, False, 0)
        out2.sum().backward()
    assert torch.equal(out2.detach(), out.detach()) and q2.grad is not None


def test_matching_train_ori_size_through_torch_interpolate():
    """ori_size = (2h - 1, 2w - 1): the source coordinate of every output pixel is a multiple of 1/2, exact in float32, so torch's bilinear
    weights are exactly 0, 1/2 or 1 and their products with a value are exact.  Forward: a sum of at most four such terms, gamma(4), on
    top of the interpolated forward bound.  Backward: an element of grad_planes is a float32 sum of at most nine weighted output gradients
    (one rounding for the product with the incoming gradient, additions in any order: gamma(16) covers both); that error enters g as e_go."""
    fx = load_golden("match_grad_dense_C36_O4")
    h, w, C = fx["in_query"].shape
    n_obj, H, W = 4, 2 * h - 1, 2 * w - 1
    fwd, _ = mgb.fixture_ref(fx)
    rs = np.random.RandomState(5)
    weight = rs.standard_normal((1, H, W, n_obj, 1)).astype(np.float32)

    def through(planes, wgt):
        t = torch.from_numpy(np.ascontiguousarray(planes, np.float64)).view(n_obj, 1, h, w).requires_grad_(True)
        with torch.enable_grad():
            o = F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True).permute(2, 3, 0, 1).reshape(1, H, W, n_obj, 1)
            (o * torch.from_numpy(wgt.astype(np.float64))).sum().backward()
        return o.detach().numpy(), t.grad.numpy().reshape(n_obj, h * w)

    out_ref, go = through(fwd["T"], weight)
    _, go_abs = through(fwd["T"], np.abs(weight))
    tol_out = through(fwd["tol_T"], weight)[0] + gamma(4) * through(np.abs(fwd["T"]) + fwd["tol_T"], weight)[0]
    q32, p32 = fx["in_query"].reshape(-1, C).astype(np.float32), fx["in_ref"].reshape(-1, C).astype(np.float32)
    grad = mgb.dense_grad_ref(go, fwd["T"], fwd["tol_T"], fwd["arg"], q32, p32, e_go=gamma(16) * go_abs)
    ref, q, bias = _leaf(fx["in_ref"]), _leaf(fx["in_query"]), _leaf(fx["in_bias"].reshape(-1, 1, 1, 1))
    labels = dev(fx["in_labels"].astype(np.float32))
    with torch.enable_grad():
        out = aoc_amd.matching_train.global_matching(ref, q, labels, 1, bias, (H, W), 1, False, 0)
        (out * dev(weight)).sum().backward()
    assert out.shape == (1, H, W, n_obj, 1)
    mgb.check(out.detach().cpu().numpy(), out_ref, tol_out, "ori_size out", REPORT)
    mgb.check(q.grad.cpu().numpy().reshape(-1, C), grad["grad_query"], grad["tol_query"], "ori_size grad_query", REPORT)
    mgb.check(ref.grad.cpu().numpy().reshape(-1, C), grad["grad_pool"], grad["tol_pool"], "ori_size grad_ref", REPORT)
    mgb.check(bias.grad.cpu().numpy().reshape(-1), grad["grad_bias"], grad["tol_bias"], "ori_size grad_bias", REPORT)


def test_matching_train_refuses_what_has_no_backward():
    fx = load_golden("match_grad_dense_C4_O2")
    ref, q, labels = _leaf(fx["in_ref"]), _leaf(fx["in_query"]), dev(fx["in_labels"].astype(np.float32))
    with torch.enable_grad():
        with pytest.raises(aoc_amd._lib.AocHipError, match="use_float16"):
            aoc_amd.matching_train.global_matching(ref, q, labels, 1, 0., None, 1, True, 0)
        with pytest.raises(aoc_amd._lib.AocHipError, match="not yet differentiable"):
            aoc_amd.matching_train.global_matching_cluster2(ref, q, labels, 1, 0., None, 1, False, 0)
        with pytest.raises(aoc_amd._lib.AocHipError, match="not yet differentiable"):
            aoc_amd.matching_train.local_matching(ref, q, labels, 0., [2], None, 1, False)
        with pytest.raises(aoc_amd._lib.AocHipError, match="inference-only"):
            aoc_amd.matching.global_matching(ref, q, labels, 1, 0., None, 1, False, 0)
        # the gradient kernels build no graph: a second derivative must raise, not come back as a constant
        out = aoc_amd.matching_train.global_matching(ref, q, labels, 1, 0., None, 1, False, 0)
        (gq,) = torch.autograd.grad((out * out).sum(), q, create_graph=True)        # grad_out = 2 out is itself part of the graph
        with pytest.raises(RuntimeError, match="once_differentiable"):
            gq.sum().backward()
