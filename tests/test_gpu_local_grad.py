"""The training-time local matching on the MI355X: aoc_local_window_match_argmin against the float64 argmin (array_equal), the derived
forward bound and, at C = 100 / 128, aoc_local_window_match_ex bit for bit; aoc_local_match_grad against the float64 references under the
derived bounds of tests/local_grad_bounds.py; and aoc_amd.local_train end to end against the gradients the reference's own autograd
recorded (tests/golden/local_grad_*.npz).

End to end the bound widens by the rounding of torch's float32 interpolate (local_grad_bounds.fixture_ref): operands off by
gamma(6) W|x|, which goes into the distance as 2 sum_c |q_c - p_c| (dq_c + dp_c) + sum (dq_c + dp_c)^2; the interpolation's own backward
by gamma(k + 3) |W|^T |grad| + |W|^T tol, k the most non-zeros in a column of W.  The fixtures' sizes make every weight a float32 value
(the host test checks it), so torch's float32 weights are the float64 matrices' exactly.  Bit-for-bit repeatability is claimed and
tested for the two entries only: torch's interpolate backward adds atomically.

Outputs sit in NaN / -7 filled, oversized buffers between sentinels.  The autouse fixture of conftest.py wraps GPU tests in
torch.no_grad(); the tests that need a graph open torch.enable_grad() themselves.  Every check prints its worst error / bound before it
asserts; a module fixture prints the largest per quantity after the last test."""
import itertools

import numpy as np
import pytest
import torch

import aoc_amd
import local_grad_bounds as lgb
from aoc_amd import ops
from conftest import load_golden
from float64_bounds import gamma

pytestmark = pytest.mark.gpu
REPORT = []
GUARD = 8                     # sentinel elements on either side of an output


@pytest.fixture(scope="module", autouse=True)
def _print_worst_ratios():
    """After the module's last test: the largest error / bound per quantity among the checks that ran (STATUS.md quotes a full run's)."""
    yield
    worst = {}
    for what, r in REPORT:
        key = ("end to end " if what.startswith("e2e") else "") + what.split()[-1]
        worst[key] = max(worst.get(key, 0.0), r)
    for key in sorted(worst):
        print(f"local_grad worst error / bound, {key}: {worst[key]:.3f}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(shape, dtype, fill):
    """-> (whole buffer, the view of `shape` that starts GUARD elements in)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf, what):
    edge = torch.cat([buf[:GUARD], buf[-GUARD:]])
    ok = torch.isnan(edge).all() if buf.dtype == torch.float32 else (edge == -7).all()
    assert ok, f"{what}: written outside the buffer"


def forward(case, inp, transform=True):
    q, p, bits, bias = dev(inp["query"]), dev(inp["prev"]), dev(inp["bits"].view(np.int32)), dev(inp["bias"])
    shape = (case.n_obj, len(case.radii), case.H, case.W)
    obuf, out = guarded(shape, torch.float32, float("nan"))
    abuf, arg = guarded(shape, torch.int32, -7)
    ops.local_window_match_argmin(q, p, bits, list(case.radii), bias, case.n_obj, transform, atrous_rate=case.rate, out=out, arg=arg)
    guards_intact(obuf, case.name + " out")
    guards_intact(abuf, case.name + " arg")
    return out, arg, (q, p, bits, bias)


def backward(case, inp, out, arg, q, p, wants=(True, True, True)):
    go = dev(inp["grad_out"])
    bufs = [guarded((case.H, case.W, case.C), torch.float32, float("nan")), guarded((case.H, case.W, case.C), torch.float32, float("nan")),
            guarded((case.n_obj,), torch.float32, float("nan"))]
    got = ops.local_match_backward(go, out, arg, q, p, lgb.window(case), *wants, grad_query=bufs[0][1], grad_prev=bufs[1][1], grad_bias=bufs[2][1])
    for (whole, view), want, t, key in zip(bufs, wants, got, ("grad_query", "grad_prev", "grad_bias")):
        guards_intact(whole, f"{case.name} {key}")
        if not want:
            assert t is None and torch.isnan(view).all(), f"{case.name}: {key} was not wanted but its buffer was written"
    return got


ENTRY_CASES = [c.name for c in lgb.CASES] + [lgb.PLANTED.name, lgb.PLANTED_LDS.name]


@pytest.mark.parametrize("name", ENTRY_CASES)
def test_argmin_forward_equals_the_float64_argmin_and_the_inference_kernel(name):
    case = lgb.BY_NAME[name]
    inp, fwd, _ = lgb.case_ref(name)
    for transform in (True, False):
        out, arg, (q, p, bits, bias) = forward(case, inp, transform)
        a, got = arg.cpu().numpy(), out.cpu().numpy()
        wrong = int((a != fwd["arg"]).sum())
        assert wrong == 0, f"{name}: {wrong} of {a.size} minimisers differ from the float64 argmin (transform={transform})"
        if transform:
            lgb.check(got, fwd["T"], fwd["tol_T"], f"{name} T", REPORT)
            assert (got[a < 0] == 1.0).all(), "T is exactly 1 where there is no minimiser"
        else:
            lgb.check(got, fwd["raw"], fwd["tol_raw"], f"{name} raw", REPORT)
            assert (got[a < 0] == np.float32(lgb.PAD)).all()
        if case.C in (100, 128):
            plain = ops.local_window_match(q, p, bits, list(case.radii), bias, case.n_obj, transform, atrous_rate=case.rate)
            assert torch.equal(out.view(torch.int32), plain.view(torch.int32)), f"{name}: values differ from aoc_local_window_match_ex (transform={transform})"


@pytest.mark.parametrize("name", ENTRY_CASES)
def test_backward_within_the_derived_bounds_and_deterministic(name):
    case = lgb.BY_NAME[name]
    inp, fwd, grad = lgb.case_ref(name)
    out, arg, (q, p, _, _) = forward(case, inp)
    first = backward(case, inp, out, arg, q, p)
    gq, gp, gb = (t.cpu().numpy() for t in first)
    lgb.check(gq.reshape(-1, case.C), grad["grad_query"], grad["tol_query"], f"{name} grad_query", REPORT)
    lgb.check(gp.reshape(-1, case.C), grad["grad_prev"], grad["tol_prev"], f"{name} grad_prev", REPORT)
    lgb.check(gb, grad["grad_bias"], grad["tol_bias"], f"{name} grad_bias", REPORT)
    assert (gp.reshape(-1, case.C)[grad["counts"] == 0] == 0.0).all(), f"{name}: a pixel nobody chose has a gradient"
    again = backward(case, inp, out, arg, q, p)
    for x, y, what in zip(first, again, ("grad_query", "grad_prev", "grad_bias")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{name}: two runs give different bits for {what}"
    out2, arg2, _ = forward(case, inp)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(arg, arg2), f"{name}: two forward runs differ"


@pytest.mark.parametrize("name", [lgb.PLANTED.name, lgb.PLANTED_LDS.name])
def test_planted_structure(name):
    case = lgb.BY_NAME[name]
    inp, fwd, grad = lgb.case_ref(name)
    out, arg, (q, p, _, _) = forward(case, inp)
    a = arg.cpu().numpy().reshape(case.n_obj, len(case.radii), -1)
    T = out.cpu().numpy().reshape(case.n_obj, len(case.radii), -1)
    px = lambda rc: rc[0] * case.W + rc[1]
    single, lo, hi, qi = px(lgb.SINGLE), px(lgb.DUP_LO), px(lgb.DUP_HI), px(lgb.DUP_QUERY)
    # one labelled pixel of object 1: everybody within R chooses it; small windows that do not reach it are empty
    ys, xs = np.divmod(np.arange(case.H * case.W), case.W)
    within = np.maximum(np.abs(ys - lgb.SINGLE[0]), np.abs(xs - lgb.SINGLE[1])) <= lgb.window(case)
    assert (a[1, 0][within] == single).all() and (a[1, 0][~within] == -1).all()
    small_empty = (a[1, 1] == -1) & (a[1, 0] == single)
    assert small_empty.any() and (T[1, 1][small_empty] == 1.0).all() and (T[1, 0][small_empty] < 1.0).all()
    # two bit-equal pixels of object 2: the lower index where both are in the window, the inner pixel in the small windows
    assert a[2, 0, qi] == lo and a[2, 1, qi] == hi and a[2, 2, qi] == hi and T[2, 0, qi] == T[2, 1, qi]
    # object 3 is absent
    assert (a[3] == -1).all() and (T[3] == 1.0).all()
    # grad_prev seen through one object at a time: grad_out zero elsewhere
    for o, rows in ((1, [single]), (2, [lo, hi])):
        only = dict(inp, grad_out=np.where(np.arange(case.n_obj)[:, None, None, None] == o, inp["grad_out"], 0).astype(np.float32))
        gq, gp, gb = (t.cpu().numpy() for t in backward(case, only, out, arg, q, p))
        ref = lgb.grad_ref(only["grad_out"], fwd["T"], fwd["tol_T"], fwd["arg"], inp["query"], inp["prev"])
        gp = gp.reshape(-1, case.C)
        lgb.check(gp, ref["grad_prev"], ref["tol_prev"], f"{name} object {o} grad_prev", REPORT)
        others = np.setdiff1d(np.arange(gp.shape[0]), rows)
        assert (gp[others] == 0.0).all() and all(np.abs(gp[r]).max() > 0 for r in rows), "only the chosen pixels have a gradient"
        assert (np.delete(gb, o) == 0.0).all() and gb[o] != 0.0
    assert grad["counts"][single] >= int((fwd["arg"][1] == single).sum()) > 100      # up to (2 R + 1)^2 n_radii terms in one row
    gb = backward(case, inp, out, arg, q, p, (False, False, True))[2].cpu().numpy()
    assert gb[3] == 0.0, "an absent object has a zero grad_bias entry"


def test_null_outputs_write_only_what_was_asked_for():
    name = "C100_15x17_r3"
    case = lgb.BY_NAME[name]
    inp, fwd, grad = lgb.case_ref(name)
    out, arg, (q, p, _, _) = forward(case, inp)
    full = backward(case, inp, out, arg, q, p)
    for wants in itertools.product((False, True), repeat=3):
        got = backward(case, inp, out, arg, q, p, wants)              # asserts that unwanted buffers keep their NaNs
        for want, t, ref in zip(wants, got, full):
            assert (t is None) == (not want)
            if want:
                assert torch.equal(t.view(torch.int32), ref.view(torch.int32)), f"wants={wants}: an output depends on which others were asked for"


# ------------------------------------------------------------------------------------------ end to end through local_train
def _leaf(a):
    return dev(np.asarray(a, np.float32)).requires_grad_(True)


def _slack(ref, recorded):
    """The recorded values are the yardstick; the bound was derived around the numpy reference, which reproduces them to 1e-10."""
    return np.abs(np.asarray(ref, np.float64) - np.asarray(recorded, np.float64).reshape(np.shape(ref)))


def _call(fx, prev, q, labels, bias, fn=None):
    radii, ori, rate, down = lgb.fixture_args(fx)
    fn = fn or aoc_amd.local_train.local_matching
    return fn(prev, q, labels, bias, radii, ori, rate, False, down, True)


@pytest.mark.parametrize("name", lgb.FIXTURES)
def test_local_train_against_the_reference_recorded_gradients(name):
    fx = load_golden(name)
    ref = lgb.fixture_ref(fx)
    prev, q, bias = _leaf(fx["in_prev"]), _leaf(fx["in_query"]), _leaf(fx["in_bias"].reshape(-1, 1, 1, 1))
    labels = dev(fx["in_labels"].astype(np.float32))
    before = labels.clone()
    with torch.enable_grad():
        out = _call(fx, prev, q, labels, bias)
        (out * dev(fx["weight"])).sum().backward()
    assert torch.equal(labels, before), "the labels were written into"
    assert out.shape == fx["out"].shape
    lgb.check(out.detach().cpu().numpy(), fx["out"], ref["tol_out"] + _slack(ref["out"], fx["out"]), f"e2e {name} out", REPORT)
    lgb.check(q.grad.cpu().numpy(), fx["grad_query"], ref["tol_query"] + _slack(ref["grad_query"], fx["grad_query"]), f"e2e {name} grad_query", REPORT)
    lgb.check(prev.grad.cpu().numpy(), fx["grad_prev"], ref["tol_prev"] + _slack(ref["grad_prev"], fx["grad_prev"]), f"e2e {name} grad_prev", REPORT)
    assert bias.grad.shape == bias.shape
    lgb.check(bias.grad.cpu().numpy().reshape(-1), fx["grad_bias"], ref["tol_bias"] + _slack(ref["grad_bias"], fx["grad_bias"]),
              f"e2e {name} grad_bias", REPORT)
    with torch.no_grad():
        same = _call(fx, prev, q, labels, bias)
        mirror = _call(fx, prev, q, labels, bias, aoc_amd.matching.local_matching)
    assert torch.equal(same, mirror), "without a graph the twin must return the mirror's bits"


def test_local_train_unlabelled_previous_frame():
    fx = load_golden(lgb.FIXTURE_UNLABELLED)
    prev, q, bias = _leaf(fx["in_prev"]), _leaf(fx["in_query"]), _leaf(fx["in_bias"].reshape(-1, 1, 1, 1))
    with torch.enable_grad():
        out = _call(fx, prev, q, dev(fx["in_labels"].astype(np.float32)), bias)
        (out * dev(fx["weight"])).sum().backward()
    assert np.array_equal(out.detach().cpu().numpy(), fx["out"]) and (out == 1).all()
    assert (q.grad == 0).all() and (prev.grad == 0).all() and (bias.grad == 0).all()


def test_local_train_second_derivative_raises():
    fx = load_golden("local_grad_absent")
    prev, q = _leaf(fx["in_prev"]), _leaf(fx["in_query"])
    with torch.enable_grad():
        out = _call(fx, prev, q, dev(fx["in_labels"].astype(np.float32)), 0.)
        (gq,) = torch.autograd.grad((out * out).sum(), q, create_graph=True)        # grad_out = 2 out is itself part of the graph
        with pytest.raises(RuntimeError, match="once_differentiable"):
            gq.sum().backward()


@pytest.mark.parametrize("only", ["query", "prev", "bias", "one_element_bias"])
def test_local_train_wanted_subsets(only):
    name = "local_grad_down_O3"
    fx = load_golden(name)
    n_obj = fx["in_labels"].shape[2]
    b1 = np.float32(0.2)
    ref = lgb.fixture_ref(fx, bias=np.full(n_obj, b1, np.float32)) if only == "one_element_bias" else lgb.fixture_ref(fx)
    if only == "one_element_bias":
        lgb.check_conditions("one-element bias", ref["fwd"])
    prev = _leaf(fx["in_prev"]) if only == "prev" else dev(fx["in_prev"])
    q = _leaf(fx["in_query"]) if only == "query" else dev(fx["in_query"])
    bias = {"bias": _leaf(fx["in_bias"].reshape(-1, 1, 1, 1)), "one_element_bias": _leaf(np.asarray([b1]))}.get(only, dev(fx["in_bias"].reshape(-1, 1, 1, 1)))
    with torch.enable_grad():
        out = _call(fx, prev, q, dev(fx["in_labels"].astype(np.float32)), bias)
        (out * dev(fx["weight"])).sum().backward()
    assert (prev.grad is not None) == (only == "prev") and (q.grad is not None) == (only == "query") and (bias.grad is not None) == ("bias" in only)
    if only == "query":
        lgb.check(q.grad.cpu().numpy(), ref["grad_query"], ref["tol_query"], f"e2e only grad_query", REPORT)
    elif only == "prev":
        lgb.check(prev.grad.cpu().numpy(), ref["grad_prev"], ref["tol_prev"], f"e2e only grad_prev", REPORT)
    elif only == "bias":
        lgb.check(bias.grad.cpu().numpy().reshape(-1), ref["grad_bias"], ref["tol_bias"], f"e2e only grad_bias", REPORT)
    else:
        # the expanded gradient is summed by torch: O - 1 more float32 additions of the per-object sums
        assert bias.grad.shape == (1,)
        tol = ref["tol_bias"].sum() + gamma(n_obj) * (np.abs(ref["grad_bias"]) + ref["tol_bias"]).sum()
        lgb.check(bias.grad.cpu().numpy(), np.asarray([ref["grad_bias"].sum()]), np.asarray([tol]), "e2e one-element grad_bias", REPORT)


def test_local_matching_proxy_with_the_heads_as_the_leaf():
    """aocnet.py:325-328: prev_frame_embedding = matmul(labels, heads) stays the caller's torch op.  Every pixel of an object then carries
    the same vector: which of them wins a window is a tie, but the query's gradient and the heads' (the sum over an object's pixels) do not
    depend on it.  Bound of grad_heads: grad_prev's rows with every pair of the map as the count of additions (a tie moves pairs between the
    rows of one object; their sum over the object stays), through the down-sample's backward, then labels^T grad_prev, a float32 matrix
    product of h w terms per element."""
    fx = load_golden("local_grad_down_O3")
    radii, ori, rate, down = lgb.fixture_args(fx)
    h, w, C = fx["in_query"].shape
    n_obj = fx["in_labels"].shape[2]
    heads = ((1.0 / np.sqrt(C)) * np.random.RandomState(11).standard_normal((n_obj, C))).astype(np.float32)
    lab = fx["in_labels"].astype(np.float32)
    L = lab.reshape(-1, n_obj).astype(np.float64)
    ref = lgb.fixture_ref(dict(fx, in_prev=(L @ heads.astype(np.float64)).astype(np.float32).reshape(h, w, C)))     # one-hot rows: exact
    g, Wd = ref["grad"], np.abs(ref["Wd"])
    n_pairs = g["g"].size
    tol_rows = g["e_prev"] + gamma(n_pairs) * g["mag_prev"]
    k = int((Wd != 0).sum(0).max())
    tol_full = gamma(k + 3) * (Wd.T @ np.abs(g["grad_prev"])) + Wd.T @ tol_rows
    full = ref["grad_prev"].reshape(-1, C)
    want = L.T @ full
    tol = L.T @ tol_full + gamma(h * w) * (L.T @ (np.abs(full) + tol_full))
    heads_t, q, labels = _leaf(heads), _leaf(fx["in_query"]), dev(lab)
    with torch.enable_grad():
        prev = torch.matmul(labels, heads_t)
        out = aoc_amd.local_train.local_matching_proxy(prev, q, labels, dev(fx["in_bias"].reshape(-1, 1, 1, 1)), radii, ori, rate, False, down, True)
        (out * dev(fx["weight"])).sum().backward()
    lgb.check(out.detach().cpu().numpy(), ref["out"], ref["tol_out"], "e2e proxy out", REPORT)
    lgb.check(q.grad.cpu().numpy(), ref["grad_query"], ref["tol_query"], "e2e proxy grad_query", REPORT)
    lgb.check(heads_t.grad.cpu().numpy(), want, tol, "e2e proxy grad_heads", REPORT)
    assert np.abs(want).max() > 1e-2


def test_memory_stays_at_the_size_of_the_outputs():
    """31 x 33, C = 100, R = 12, four objects, no resize: forward + backward may allocate, above the inputs, at most twice the bytes of the
    output, the saved tensors (T, arg; the two maps are the inputs themselves), the incoming gradient, the three gradients and the
    workspace, all computed from the shapes.  The reference's unfolded operand alone is 31 33 100 625 4 B = 256 MB there."""
    case = lgb.MEMORY
    inp, _, _ = lgb.case_ref(case.name)
    H, W, C, n_obj, nr = case.H, case.W, case.C, case.n_obj, len(case.radii)
    labels = np.zeros((H * W, n_obj), np.float32)
    for o in range(n_obj):
        labels[:, o] = (inp["bits"] >> o) & 1
    prev, q, bias = _leaf(inp["prev"]), _leaf(inp["query"]), _leaf(inp["bias"].reshape(-1, 1, 1, 1))
    labels, weight = dev(labels.reshape(H, W, n_obj)), dev(inp["grad_out"].transpose(2, 3, 0, 1).reshape(1, H, W, n_obj, nr).copy())
    planes = n_obj * nr * H * W * 4
    ws = aoc_amd._lib.lib().aoc_local_match_grad_workspace_bytes(H, W, C, nr, n_obj)
    assert ws <= 2 * planes + 4096
    limit = 2 * (planes + 2 * planes + planes + 2 * H * W * C * 4 + n_obj * 4 + ws)
    assert limit < 8 << 20 and H * W * C * (2 * 12 + 1) ** 2 * 4 > 255_000_000
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.enable_grad():
        out = aoc_amd.local_train.local_matching(prev, q, labels, bias, list(case.radii), None, 1, False, False, True)
        (out * weight).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"memory: peak above the inputs {peak} bytes, limit {limit} bytes (the unfolded operand: {H * W * C * 625 * 4} bytes)")
    assert peak <= limit
    assert q.grad is not None and prev.grad is not None and bias.grad is not None
