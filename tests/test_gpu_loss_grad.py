"""The training criterion on the device: the entry points of csrc/loss_grad.hip through their wrappers, and aoc_amd.loss_train through
``backward()``, against the float64 references and derived bounds of tests/loss_grad_bounds.py.  Every output goes into a margined buffer
(NaN around floats, a sentinel around integers and bytes) whose margins must stay untouched; every case runs twice and must give the same
bits; each optional output must have the same bits alone as with the others.  The preconditions the comparisons rest on (a decided rank-k
loss, a decided argmax) are asserted for these cases and seeds by tests/test_loss_grad_host.py.  Each test prints its largest error / bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aoc_amd  # noqa: F401
import loss_grad_bounds as lgb
import test_loss_grad_host as tlh
from aoc_amd import _lib, loss_train as lt
from test_gpu_gates_grad import DEV, PAD, dev, margins, untouched, _np

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
WORST = {}
FILL = {torch.int32: -7, torch.uint8: 9}


def held(entry, got, want_tol, what):
    want, tol = want_tol
    r = lgb.check(_np(got), want, tol, what)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, f"{what}: error / bound {r:.3f}"
    return r


def imargins(n, dtype):
    buf = torch.full((n + 2 * PAD,), FILL[dtype], dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def iuntouched(buf, n):
    fill = FILL[buf.dtype]
    return bool((buf[:PAD] == fill).all() and (buf[PAD + n:] == fill).all())


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


FWD_DTYPES = dict(loss=torch.float32, lse=torch.float32, argmax=torch.int32, valid_partial=torch.int32, bad=torch.int32)


def run_forward(pred, labels, size, names, ignore_index=lgb.IGNORE):
    """the named outputs of aoc_upsample_ce_forward out of margined buffers -> {name: clone}"""
    n = size[0] * size[1]
    sizes = dict(loss=n, lse=n, argmax=n, valid_partial=(n + 255) // 256, bad=1)
    held_bufs, out = {}, {}
    for name in names:
        held_bufs[name], out[name] = margins((sizes[name],)) if FWD_DTYPES[name] == torch.float32 else imargins(sizes[name], FWD_DTYPES[name])
    res = lt.upsample_ce_forward(pred, labels, size, ignore_index, want=(False,) * 5, out=out)
    for name, r in zip(lt._FWD_OUTS, res):
        assert (r is out[name]) if name in names else (r is None)
    for name in names:
        ok = untouched(held_bufs[name], (sizes[name],)) if FWD_DTYPES[name] == torch.float32 else iuntouched(held_bufs[name], sizes[name])
        assert ok, f"{name}: written outside the output"
    return {name: out[name].clone() for name in names}


def run_backward(pred, labels, lse, mask, grad_out, size, **kw):
    buf, g = margins(tuple(pred.shape))
    r = lt.upsample_ce_backward(pred, labels, lse, mask, grad_out, size, grad_pred=g, **kw)
    assert r is g and untouched(buf, tuple(pred.shape)), "grad_pred: written outside the output"
    return g.clone()


# ------------------------------------------------------------------------------------------ 1 the forward and the gradient entries
@pytest.mark.parametrize("case", lgb.CASES, ids=str)
def test_forward_and_gradient_entries(case):
    C, h, w, H, W = case
    n = H * W
    pred, labels = lgb.make_case(*case)
    fw = lgb.forward_ref(pred, labels, (H, W))
    pd, ld = dev(pred), dev(labels)
    runs = [run_forward(pd, ld, (H, W), lt._FWD_OUTS) for _ in range(2)]
    for name in lt._FWD_OUTS:
        assert torch.equal(bits(runs[0][name]), bits(runs[1][name])), f"{case} {name}: two runs differ"
        alone = run_forward(pd, ld, (H, W), (name,))[name]
        assert torch.equal(bits(alone), bits(runs[0][name])), f"{case} {name}: alone it has other bits"
    got = runs[0]
    held("forward lse", got["lse"], fw["lse"], f"{case} lse")
    held("forward loss", got["loss"], fw["loss"], f"{case} loss")
    assert float(got["loss"].min()) >= 0.0 and not bool(torch.signbit(got["loss"][~fw["valid"].to(DEV)]).any()), "loss is never negative; +0.0 where not valid"
    assert torch.equal(got["argmax"].cpu().long(), fw["argmax"]), f"{case}: argmax"
    assert int(got["valid_partial"].sum()) == fw["n_valid"] and int(got["bad"]) == 0
    want_partial = np.add.reduceat(fw["valid"].numpy().astype(np.int64), np.arange(0, n, 256))
    assert np.array_equal(_np(got["valid_partial"]), want_partial)
    if (h, w) == (H, W):
        raw = torch.logsumexp(torch.from_numpy(pred).double().reshape(C, -1), 0)
        assert float(fw["x_tol"].max()) == 0.0 and float((fw["lse"][0] - raw).abs().max()) < 1e-12, "the identity geometry: lse of the raw logits, no interpolation term"
    # the gradient entry with the lse the forward wrote and the reference's mask (ties by the lowest index), at k < n and k = n
    go = np.float32(0.75)
    for k in sorted({max(1, n // 3), n}):
        mask = lgb.topk_ref(fw["loss"][0].numpy(), k)["mask"]
        md, gd = dev(mask.astype(np.uint8)), dev(np.array([go], f32))
        g2 = [run_backward(pd, ld, got["lse"], md, gd, (H, W), k=k) for _ in range(2)]
        assert torch.equal(bits(g2[0]), bits(g2[1])), f"{case} k={k}: two gradient runs differ"
        ref = lgb.grad_ref(pred, labels, _np(got["lse"]).astype(f64), np.zeros(n), mask, (H, W), k, go)
        held("gradient", g2[0], ref, f"{case} k={k} grad_pred")
        reached = np.outer(lgb.tap_matrix(lgb.taps32(h, H), h).numpy().sum(0) != 0, lgb.tap_matrix(lgb.taps32(w, W), w).numpy().sum(0) != 0)
        if not reached.all():
            assert float(g2[0][:, torch.from_numpy(~reached).to(DEV)].abs().max()) == 0.0, "coarse pixels no fine pixel reaches are written as 0"
    if case == (4, 6, 6, 3, 4):
        assert int((~reached).sum()) > 0, "the downsampling case leaves coarse pixels unreached"
    # n_valid read from the device: the reduction='mean' branch
    vm = lt.valid_mask(ld, C)
    assert np.array_equal(_np(vm).astype(bool), fw["valid"].numpy())
    if fw["n_valid"]:
        nv = dev(np.array([fw["n_valid"]], np.int32))
        g = run_backward(pd, ld, got["lse"], vm, dev(np.array([go], f32)), (H, W), n_valid=nv)
        held("gradient", g, lgb.grad_ref(pred, labels, _np(got["lse"]).astype(f64), np.zeros(n), fw["valid"].numpy(), (H, W), fw["n_valid"], go), f"{case} mean mode")
    print(f"{case}: worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("mode", ("all_ignored", "none_ignored", "out_of_range"))
def test_label_cases(mode):
    case = (4, 5, 7, 17, 25)
    C, h, w, H, W = case
    n = H * W
    pred, labels = lgb.make_case(*case, ignored=0.0 if mode != "all_ignored" else 2.0)
    if mode == "out_of_range":
        labels[[3, 77, 400]] = (C, -1, 31)
    fw = lgb.forward_ref(pred, labels, (H, W))
    assert fw["n_valid"] == {"all_ignored": 0, "none_ignored": n, "out_of_range": n - 3}[mode] and fw["bad"] == (3 if mode == "out_of_range" else 0)
    pd, ld = dev(pred), dev(labels)
    got = run_forward(pd, ld, (H, W), lt._FWD_OUTS)
    held("forward loss", got["loss"], fw["loss"], mode + " loss")
    assert int(got["bad"]) == fw["bad"] and int(got["valid_partial"].sum()) == fw["n_valid"]
    mean, nv = lt.valid_mean(got["loss"], got["valid_partial"])
    assert int(nv) == fw["n_valid"]
    (want, tol), _ = lgb.valid_mean_ref(_np(got["loss"]), fw["valid"].numpy())
    assert bool(torch.isnan(mean).all()) if mode == "all_ignored" else abs(float(mean) - want) <= tol
    # every pixel selected: ignored and out-of-range pixels still contribute nothing
    ones, gd = torch.ones(n, dtype=torch.uint8, device=DEV), torch.ones(1, device=DEV)
    g = run_backward(pd, ld, got["lse"], ones, gd, (H, W), k=n)
    held("gradient", g, lgb.grad_ref(pred, labels, _np(got["lse"]).astype(f64), np.zeros(n), np.ones(n, bool), (H, W), n), mode + " grad_pred")
    if mode == "all_ignored":
        assert float(g.abs().max()) == 0.0
    crit = lt.Concat_CrossEntropyLoss(0.15, 100000, check_labels=True)
    lab4 = torch.from_numpy(labels).long().view(1, H, W).to(DEV)
    if mode == "out_of_range":
        with pytest.raises(ValueError, match="3 labels"):
            crit.sample(pd[None], lab4, 0, (H, W))
        loss, _ = lt.Concat_CrossEntropyLoss(0.15, 100000).sample(pd[None], lab4, 0, (H, W))      # the asynchronous default: loss 0 there
        assert abs(float(loss) - float(fw["loss"][0].sum()) / n) <= float(fw["loss"][1].max()) + lgb.gamma(n + 3) * float(fw["loss"][0].sum()) / n
    else:
        crit.sample(pd[None], lab4, 0, (H, W))


def test_tensor_contract():
    """a strided pred, a wide dtype, or an output one element short raises before the library is called: the buffers stay untouched"""
    pred, labels = lgb.make_case(3, 4, 5, 6, 7)
    pd, ld = dev(pred), dev(labels)
    buf, out = margins((42,))
    calls = []
    real = _lib.lib()

    class Spy:
        def __getattr__(self, name):
            if name.startswith("aoc_upsample_ce_forward") or name.startswith("aoc_upsample_ce_grad") or name.startswith("aoc_topk"):
                calls.append(name)
            return getattr(real, name)

    orig = _lib.lib
    _lib.lib = lambda: Spy()
    try:
        for bad_pred in (dev(np.ascontiguousarray(pred.transpose(0, 2, 1))).transpose(1, 2), pd.double(), pd.half()):
            with pytest.raises(ValueError):
                lt.upsample_ce_forward(bad_pred, ld, (6, 7), out=dict(loss=out))
        assert calls == []
        with pytest.raises(ValueError):
            lt.upsample_ce_forward(pd, ld, (6, 7), out=dict(loss=out[:-1]))
        with pytest.raises(ValueError):
            lt.upsample_ce_forward(pd, ld, (6, 7), out=dict(lse=out.double()))
        with pytest.raises(ValueError):
            lt.upsample_ce_forward(pd, ld, (6, 7), out=dict(argmax=out))
        with pytest.raises(ValueError):
            lt.topk_mean(out.double(), 3)
        with pytest.raises(ValueError):
            lt.topk_select_mask(torch.zeros(42, device=DEV), 3, torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                                mask=torch.zeros(41, dtype=torch.uint8, device=DEV))
        lse, mask, go = torch.zeros(42, device=DEV), torch.ones(42, dtype=torch.uint8, device=DEV), torch.ones(1, device=DEV)
        with pytest.raises(ValueError):
            lt.upsample_ce_backward(pd, ld, lse, mask, go, (6, 7), k=3, grad_pred=torch.zeros(3, 4, 4, device=DEV))
        with pytest.raises(ValueError):
            lt.upsample_ce_backward(pd, ld, lse, mask.int(), go, (6, 7), k=3)
        with pytest.raises(ValueError):
            lt.upsample_ce_backward(pd, ld, lse[::1].double(), mask, go, (6, 7), k=3)
        assert [c for c in calls if not c.endswith("_partials") and not c.endswith("workspace_bytes")] == [], calls
    finally:
        _lib.lib = orig
    assert untouched(buf, (42,)) and bool(torch.isnan(out).all())
    assert lt.upsample_ce_forward(pd, torch.from_numpy(labels).long().to(DEV), (6, 7))[0] is not None, "int64 labels are converted"


# ------------------------------------------------------------------------------------------ 2 the top-k mean and the mask alone
def run_topk(vd, k):
    n = vd.numel()
    (bm, mean), (bt, thr) = margins((1,)), margins((1,))
    bn, n_gt = imargins(1, torch.int32)
    bk, mask = imargins(n, torch.uint8)
    lt.topk_mean(vd, k, mean, thr, n_gt)
    lt.topk_select_mask(vd, k, thr, n_gt, mask)
    assert untouched(bm, (1,)) and untouched(bt, (1,)) and iuntouched(bn, 1) and iuntouched(bk, n), "written outside the outputs"
    return mean.clone(), thr.clone(), n_gt.clone(), mask.clone()


@pytest.mark.parametrize("n", lgb.TOPK_N)
def test_topk_mean_and_mask(n):
    worst = 0.0
    for kind in lgb.TOPK_DATA:
        v = lgb.topk_data(kind, n)
        vd = dev(v)
        for k in lgb.topk_ks(n):
            what = f"n={n} {kind} k={k}"
            a, b = run_topk(vd, k), run_topk(vd, k)
            assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), what + ": two runs differ"
            mean, thr, n_gt, mask = a
            ref = lgb.topk_ref(v, k)
            want_thr = torch.topk(torch.from_numpy(v), k).values[-1]
            assert int(bits(thr.cpu())) == int(bits(want_thr.reshape(1))), what + f": thr {float(thr)} is not torch.topk's {float(want_thr)}"
            assert int(n_gt) == ref["n_gt"], what + ": n_gt"
            assert np.array_equal(_np(mask).astype(bool), ref["mask"]) and int(mask.sum()) == k, what + ": the mask is not the lowest-index rule's"
            want, tol = ref["mean"]
            if np.isfinite(want):
                r = abs(float(mean) - want) / tol if tol > 0 else (0.0 if float(mean) == want else np.inf)
                worst = max(worst, r)
                assert r <= 1.0, what + f": mean {float(mean)} against {want}, error / bound {r:.3f}"
            else:
                assert float(mean) == want, what
            for i in range(3):                                                      # each output alone: the same bits
                only = lt.topk_mean(vd, k, want=tuple(j == i for j in range(3)))
                assert [o is None for o in only] == [j != i for j in range(3)] and torch.equal(bits(only[i]), bits(a[i])), what + ": an output alone differs"
    print(f"topk n={n}: worst mean error / bound {worst:.3f}")


@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_topk_nan_gives_nan(sign):
    v = lgb.topk_data("random", 8209)
    v[4000] = np.copysign(np.nan, sign)
    for k in (1, 1000, 8209):
        mean, _, _ = lt.topk_mean(dev(v), k)
        assert bool(torch.isnan(mean).all()), (sign, k)


# ------------------------------------------------------------------------------------------ 3 the module
def module_run(pred, labels, size, top_k, mining_step, step, weight=1.0):
    pd = dev(pred)[None].requires_grad_(True)
    lab = torch.from_numpy(np.asarray(labels)).long().view(1, *size).to(DEV)
    crit = lt.Concat_CrossEntropyLoss(top_k, mining_step)
    with torch.enable_grad():
        loss, arg = crit.sample(pd, lab, step, size)
        assert loss.dim() == 0 and loss.is_cuda and arg.shape == (1,) + tuple(size) and arg.dtype == torch.int64
        (loss * weight).backward()
    return loss.detach(), pd.grad[0].clone(), arg


@pytest.mark.parametrize("name", tlh.FIXTURES)
def test_module_at_the_fixtures(name):
    fx = tlh.load_fixture(name)
    labels = fx["labels"].astype(np.int32).reshape(-1)
    ref = lgb.criterion_ref(fx["pred"], labels, fx["size"], fx["k"])
    runs = [module_run(fx["pred"], labels, fx["size"], fx["top_k"], int(fx["hard_example_mining_step"]), int(fx["step"])) for _ in range(2)]
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(runs[0][:2], runs[1][:2])), name + ": two runs differ"
    loss, grad, arg = runs[0]
    r1 = held("module loss", loss, (fx["loss"].astype(f64).reshape(()), np.float64(ref["loss"][1]).reshape(())), name + " loss against the recorded value")
    r2 = held("module grad", grad, (fx["grad_pred"], ref["grad"][1]), name + " grad_pred against the recorded value")
    assert np.array_equal(_np(arg[0]), fx["all_pred"].astype(np.int64))
    print(f"{name}: loss error / bound {r1:.3f}, grad_pred {r2:.3f}")


@pytest.mark.parametrize("case", lgb.COMPOSED, ids=str)
def test_module_composed(case):
    """the whole criterion where the kernels choose the k pixels themselves, at every step and in the reduction='mean' branch"""
    pred, labels = lgb.make_case(*case)
    for step in lgb.STEPS + (None,):
        _, _, ref = tlh.reference(case, step)
        top_k = None if step is None else lgb.TOP_K
        loss, grad, arg = module_run(pred, labels, case[3:], top_k, lgb.MINING_STEP, step or 0, weight=0.5)
        half = lgb.criterion_ref(pred, labels, case[3:], tlh.case_k(case, step), grad_out=0.5)
        held("module loss", loss, tuple(np.float64(v).reshape(()) for v in ref["loss"]), f"{case} step {step} loss")
        held("module grad", grad, half["grad"], f"{case} step {step} grad_pred")
        assert torch.equal(arg.cpu().reshape(-1), ref["argmax"])
    print(f"{case}: worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith("module")))


def test_batch_of_two_and_the_torch_arm():
    """upsampled_criterion over two samples with different C equals Concat_CrossEntropyLoss fed torch's own float32 upsampled logits, within
    the sum of both bounds: the fused arm's, and the identity arm's bound at the logits torch's float32 upsample produced (whose float64
    criterion is off the coarse logits' by what torch's own upsample rounding moved it: computed, not bounded)."""
    cases, step = ((4, 5, 7, 17, 25), (2, 5, 7, 17, 25)), lgb.STEPS[1]
    size = (17, 25)
    data = [lgb.make_case(*c) for c in cases]
    crit = lt.Concat_CrossEntropyLoss(lgb.TOP_K, lgb.MINING_STEP)
    preds = [dev(p)[None].requires_grad_(True) for p, _ in data]
    labs = [torch.from_numpy(l).float().view(1, *size).to(DEV) for _, l in data]             # the reference's float label maps
    with torch.enable_grad():
        losses, all_pred = lt.upsampled_criterion(crit, preds, labs, step, size)
        assert losses.shape == (2,) and all_pred.shape == (2,) + size and all_pred.dtype == torch.int64
        losses.sum().backward()
        ups = [F.interpolate(dev(p)[None], size=size, mode="bilinear", align_corners=True) for p, _ in data]
        plain = crit(ups, [l.long() for l in labs], step)
    k = lgb.top_k_pixels(lgb.TOP_K, lgb.MINING_STEP, step, size[0] * size[1])
    for i, (c, (p, l)) in enumerate(zip(cases, data)):
        ref = lgb.criterion_ref(p, l, size, k)
        held("module loss", losses[i], tuple(np.float64(v).reshape(()) for v in ref["loss"]), f"sample {i} loss")
        held("module grad", preds[i].grad[0], ref["grad"], f"sample {i} grad_pred")
        assert torch.equal(all_pred[i].cpu().reshape(-1), ref["argmax"])
        own = lgb.criterion_ref(_np(ups[i][0]), l, size, k)                                   # identity geometry at torch's float32 logits
        allowed = ref["loss"][1] + own["loss"][1] + abs(own["loss"][0] - ref["loss"][0])
        assert abs(float(losses[i]) - float(plain[i])) <= allowed, f"sample {i}: fused {float(losses[i])} against the torch arm {float(plain[i])}"


@pytest.mark.parametrize("case", ((4, 5, 7, 17, 25), (3, 17, 33, 65, 129), (3, 7, 5, 7, 5)), ids=str)
def test_one_call_forward_has_the_separate_entries_bits(case):
    C, h, w, H, W = case
    pred, labels = lgb.make_case(*case)
    pd, ld = dev(pred), dev(labels)
    loss, lse, arg, valid, bad = lt.upsample_ce_forward(pd, ld, (H, W), want=(True,) * 5)
    for k in (None, 1, (H * W) // 7, H * W):
        mean, lse1, arg1, mask1, nv1, bad1 = lt.criterion_forward(pd, ld, (H, W), k, want_bad=True)
        if k is None:
            want_mean, nv = lt.valid_mean(loss, valid)
            want_mask = lt.valid_mask(ld, C)
            assert torch.equal(nv1, nv)
        else:
            want_mean, thr, n_gt = lt.topk_mean(loss, k)
            want_mask = lt.topk_select_mask(loss, k, thr, n_gt)
            assert nv1 is None
        assert torch.equal(bits(mean), bits(want_mean)) and torch.equal(bits(lse1), bits(lse)) and torch.equal(arg1, arg) and torch.equal(mask1, want_mask)
        assert torch.equal(bad1, bad)
        lean = lt.criterion_forward(pd, ld, (H, W), k, want_backward=False)
        assert torch.equal(bits(lean[0]), bits(mean)) and torch.equal(lean[2], arg) and lean[1] is None and lean[3] is None and lean[5] is None


def test_no_gradient_wanted_and_double_backward():
    pred, labels = lgb.make_case(4, 5, 7, 17, 25)
    lab = torch.from_numpy(labels).long().view(1, 17, 25).to(DEV)
    crit = lt.Concat_CrossEntropyLoss(0.15, 100000)
    calls = []
    orig = lt.upsample_ce_backward, lt.criterion_forward
    lt.upsample_ce_backward = lambda *a, **k: (calls.append("grad"), orig[0](*a, **k))[1]
    lt.criterion_forward = lambda *a, **k: (calls.append("mask") if k["want_backward"] else None, orig[1](*a, **k))[1]
    try:
        with torch.enable_grad():
            loss, _ = crit.sample(dev(pred)[None], lab, 60000, (17, 25))
            assert not loss.requires_grad and calls == [], "requires_grad=False: no mask is built and nothing is saved"
            pd = dev(pred)[None].requires_grad_(True)
            loss2, _ = crit.sample(pd, lab, 60000, (17, 25))
            assert torch.equal(bits(loss2.detach().reshape(1)), bits(loss.reshape(1)))
            g, = torch.autograd.grad(loss2 * loss2, pd, create_graph=True)
            assert calls == ["mask", "grad"]
            with pytest.raises(RuntimeError, match="once_differentiable"):
                g.sum().backward()
        with torch.no_grad():
            assert not crit.sample(pd, lab, 60000, (17, 25))[0].requires_grad and calls == ["mask", "grad"]
    finally:
        lt.upsample_ce_backward, lt.criterion_forward = orig


def test_deterministic_algorithms_allowed():
    pred, labels = lgb.make_case(4, 5, 7, 17, 25)
    torch.use_deterministic_algorithms(True)
    try:
        module_run(pred, labels, (17, 25), 0.15, 100000, 60000)
    finally:
        torch.use_deterministic_algorithms(False)


# ------------------------------------------------------------------------------------------ 4 peak memory
def test_peak_memory_stays_below_the_upsampled_logits():
    C, h, w, H, W = 31, 8, 9, 117, 117
    n = H * W
    pred, labels = lgb.make_case(C, h, w, H, W)
    pd = dev(pred)[None].requires_grad_(True)
    lab = torch.from_numpy(labels).long().view(1, H, W).to(DEV)
    crit = lt.Concat_CrossEntropyLoss(0.15, 100000)
    L = _lib.lib()
    with torch.enable_grad():
        crit.sample(pd, lab, 60000, (H, W))[0].backward()                                     # warm: the allocator's pools, the library
        pd.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, arg = crit.sample(pd, lab, 60000, (H, W))
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    outputs = 4 + 4 * n + 8 * n                                   # the loss; argmax as the kernel writes it and as int64 for all_pred
    saved = 4 * n + 4 * n + n                                     # the int32 labels, lse, the mask
    gradient = 4 * C * h * w + 4                                  # grad_pred, the grad_out word
    workspaces = 4 * n + L.aoc_criterion_forward_workspace_bytes(n)      # the loss plane; the histograms, chunk sums, tie counts, thr and n_gt
    allowed = 2 * (outputs + saved + gradient + workspaces)
    upsampled = 4 * C * n
    print(f"peak above the inputs {peak} bytes, allowed {allowed}, the upsampled logits alone {upsampled}")
    assert allowed < upsampled == 1697436, "the rule must exclude a kernel that forms the upsampled logits"
    assert peak <= allowed, f"peak {peak} bytes above the inputs, allowed {allowed}"
