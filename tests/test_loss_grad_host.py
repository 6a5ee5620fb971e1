"""What can be checked without a GPU about the training criterion (aoc_amd.loss_train, csrc/loss_grad.hip): the float64 references of
tests/loss_grad_bounds.py against torch's float64 autograd of the reference's lines (F.interpolate + cross_entropy + topk + mean) and against
losses and gradients recorded from the reference's own Concat_CrossEntropyLoss; that every slipped twin leaves its bound; the reference's k at
the steps where it changes; the tie rules of the mask; the PRECONDITIONS of the GPU file (asserted for every case and seed it uses, never
skipped): a decided rank-k loss and a decided argmax; the module's surface, the wrappers' tensor contract and the entry points' rejections."""
import ctypes
import functools
import inspect
import os

import numpy as np
import pytest
import torch

import aoc_amd
import loss_grad_bounds as lgb
from aoc_amd import _lib, loss_train as lt

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("loss_grad_half", "loss_grad_C2", "loss_grad_mean", "loss_grad_mining0", "loss_grad_past")
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4


def case_k(case, step):
    """k of a case at a step (None: the reduction='mean' branch)"""
    return None if step is None else lgb.top_k_pixels(lgb.TOP_K, lgb.MINING_STEP, step, case[3] * case[4])


# every case at every step, but for the one-pixel crop past step 0: there the reference's k is int(0.575) = 0, its loss the mean of nothing,
# and the module rejects the call (test_wrappers_reject_before_the_library)
RUNS = tuple((c, s) for c in lgb.CASES for s in lgb.STEPS + (None,) if case_k(c, s) != 0)
assert len(RUNS) == 4 * len(lgb.CASES) - 2


@functools.lru_cache(maxsize=None)
def reference(case, step):
    pred, labels = lgb.make_case(*case)
    return pred, labels, lgb.criterion_ref(pred, labels, case[3:], case_k(case, step))


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        d = {k: z[k] for k in z.files}
    p = float(d["top_k_percent_pixels"])
    d["top_k"] = None if np.isnan(p) else p
    d["pred"] = d["pred"].astype(f32)
    d["size"] = tuple(int(s) for s in d["size"])
    d["k"] = None if d["top_k"] is None else lgb.top_k_pixels(d["top_k"], int(d["hard_example_mining_step"]), int(d["step"]), d["size"][0] * d["size"][1])
    return d


def close(got, want, what, rel):
    got, want = lgb.t64(got), lgb.t64(want)
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= rel * scale, f"{what}: {err:.3e} against a largest value of {scale:.3e}"


# ------------------------------------------------------------------------------------------ 1 the references
@pytest.mark.parametrize("case,step", RUNS, ids=str)
def test_reference_equals_float64_autograd(case, step):
    pred, labels, ref = reference(case, step)
    k = case_k(case, step)
    loss, grad, arg = lgb.torch_criterion(pred, labels, case[3:], k)
    if k is None and ref["fw"]["n_valid"] == 0:
        assert np.isnan(ref["loss"][0]) and bool(torch.isnan(loss))
        return
    close(ref["loss"][0], loss, f"{case} step {step}: loss", 1e-12)
    close(ref["grad"][0], grad, f"{case} step {step}: grad_pred", 1e-12)
    assert torch.equal(ref["argmax"].reshape(arg.shape), arg)
    assert int(ref["mask"].sum()) == (k if k is not None else ref["fw"]["n_valid"])


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_equals_recorded(name):
    fx = load_fixture(name)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 250000
    ref = lgb.criterion_ref(fx["pred"], fx["labels"].astype(np.int32).reshape(-1), fx["size"], fx["k"])
    close(ref["loss"][0], fx["loss"], name + ": loss", 1e-10)
    close(ref["grad"][0], fx["grad_pred"], name + ": grad_pred", 1e-10)
    assert np.array_equal(ref["argmax"].reshape(fx["size"]).numpy(), fx["all_pred"])
    assert ref["k_gap"] > 1.0 and float(lgb.argmax_margin(ref["fw"]).min()) > 1.0, "a fixture the GPU cannot be held to"


def test_fixture_cases_are_the_listed_ones():
    fx = {n: load_fixture(n) for n in FIXTURES}
    assert fx["loss_grad_half"]["pred"].shape == (4, 9, 11) and fx["loss_grad_half"]["size"] == (33, 41)
    assert int(fx["loss_grad_half"]["step"]) * 2 == int(fx["loss_grad_half"]["hard_example_mining_step"])
    assert fx["loss_grad_C2"]["pred"].shape[0] == 2 and fx["loss_grad_mean"]["top_k"] is None
    assert int(fx["loss_grad_mining0"]["hard_example_mining_step"]) == 0
    assert int(fx["loss_grad_past"]["step"]) > int(fx["loss_grad_past"]["hard_example_mining_step"]) > 0


# ------------------------------------------------------------------------------------------ 2 the slipped twins
SLIP_CASES = ((4, 5, 7, 17, 25), (5, 9, 11, 33, 41))


@pytest.mark.parametrize("case", SLIP_CASES, ids=str)
@pytest.mark.parametrize("slip", ("align_false", "no_onehot", "one_over_n", "ignored_grad", "drop_clamped"))
def test_slips_leave_the_bound(case, slip):
    step = lgb.STEPS[0] if slip == "ignored_grad" else lgb.STEPS[1]          # ignored pixels (loss 0) are selected only when k is every pixel
    pred, labels, ref = reference(case, step)
    k = case_k(case, step)
    bad = lgb.criterion_ref(pred, labels, case[3:], k, slip=slip)
    grad, tol = ref["grad"]
    assert bool(((bad["grad"][0] - grad).abs() > tol).any()), f"{slip}: the slipped gradient stays inside the bound"
    if slip == "align_false":
        lv, ltol = ref["fw"]["loss"]
        assert bool(((bad["fw"]["loss"][0] - lv).abs() > ltol).any()) and bool(((bad["fw"]["lse"][0] - ref["fw"]["lse"][0]).abs() > ref["fw"]["lse"][1]).any())
        assert abs(bad["loss"][0] - ref["loss"][0]) > ref["loss"][1]


def test_bounds_are_small():
    """the analysis gives a float32 loss error of a few 1e-6 at logits 3 randn: what the precondition compares the gaps with"""
    for case in lgb.CASES:
        _, _, ref = reference(case, 0)
        assert float(ref["fw"]["loss"][1].max()) < 2e-5 and float(ref["fw"]["x_tol"].max()) < 1e-5, case


# ------------------------------------------------------------------------------------------ 3 k
def test_k_is_the_references_formula():
    n, ms = 465 * 465, 100000
    want = {0: 216225, 1: 216223, ms // 2: 124329, ms - 1: 32435, ms: 32433, 2 * ms: 32433}
    for step, k in want.items():
        assert lt.top_k_pixels(0.15, ms, step, n) == k == lgb.top_k_pixels(0.15, ms, step, n), step
        ratio = min(1.0, step / float(ms))
        assert k == int((ratio * 0.15 + (1.0 - ratio)) * float(n))
    assert lt.top_k_pixels(0.15, 0, 12345, n) == int(0.15 * float(n)) == 32433


# ------------------------------------------------------------------------------------------ 4 ties
def test_tie_rules():
    v = np.array([0.5, 2.0, 0.5, 0.5, 3.0, 0.5, 0.25], f32)
    lo, hi, al = (lgb.topk_ref(v, 4, t) for t in ("lowest", "highest", "all"))
    assert lo["thr"] == 0.5 and lo["n_gt"] == 2 and lo["mean"][0] == (2.0 + 3.0 + 2 * 0.5) / 4
    assert lo["mask"].tolist() == [True, True, True, False, True, False, False]
    assert hi["mask"].tolist() == [False, True, False, True, True, True, False]
    assert al["mask"].tolist() == [True, True, True, True, True, True, False]
    assert lo["mask"].sum() == hi["mask"].sum() == 4 and al["mask"].sum() == 6


def test_planted_ties_change_the_gradient():
    """identical pixels (the same logits, the same label) have identical losses: lowest and highest take different ones"""
    C, h, w = 3, 4, 6
    pred = np.repeat((3.0 * lgb.rng(5).standard_normal((C, h, 1))).astype(f32), w, axis=2)
    labels = np.repeat(lgb.rng(6).randint(0, C, (h, 1)), w, axis=1).reshape(-1).astype(np.int32)
    k = 2 * w + 2
    lo, hi = (lgb.criterion_ref(pred, labels, (h, w), k, tie=t) for t in ("lowest", "highest"))
    assert lo["loss"][0] == hi["loss"][0] and lo["mask"].sum() == hi["mask"].sum() == k
    assert not np.array_equal(lo["mask"], hi["mask"])
    assert bool(((lo["grad"][0] - hi["grad"][0]).abs() > lo["grad"][1] + hi["grad"][1]).any())


# ------------------------------------------------------------------------------------------ 5 the GPU file's preconditions
@pytest.mark.parametrize("case,step", RUNS, ids=str)
def test_gpu_preconditions(case, step):
    """the argmax at every shape; the rank-k gap wherever the GPU file lets the kernels choose the k pixels (lgb.COMPOSED, every step).  The
    other shapes meet the gradient entry with the reference's mask: one coarse pixel or one channel ties every loss by construction."""
    _, _, ref = reference(case, step)
    if case in lgb.COMPOSED:
        assert ref["k_gap"] > 1.0, f"{case} step {step}: the losses of rank k and k + 1 differ by {ref['k_gap']:.3f} x twice the forward bound; change the seed"
    margin = float(lgb.argmax_margin(ref["fw"]).min())
    assert margin > 1.0, f"{case}: the two largest logits of a pixel differ by {margin:.3f} x twice the logit bound; change the seed"


# ------------------------------------------------------------------------------------------ 6 the surface and the contract
def test_criterion_surface():
    sig = inspect.signature(lt.Concat_CrossEntropyLoss.__init__)
    assert list(sig.parameters)[:3] == ["self", "top_k_percent_pixels", "hard_example_mining_step"]
    assert sig.parameters["top_k_percent_pixels"].default is None and sig.parameters["hard_example_mining_step"].default == 100000
    for bad in (0, 1, 1.5, -0.1):
        with pytest.raises(AssertionError):
            lt.Concat_CrossEntropyLoss(bad)
    c = lt.Concat_CrossEntropyLoss(0.15, 1000)
    assert c.top_k_percent_pixels == 0.15 and c.hard_example_mining_step == 1000 and c.check_labels is False
    assert "loss_train" in aoc_amd.__all__ and not hasattr(lt, "Concat_BCEWithLogitsLoss")
    assert list(inspect.signature(c.forward).parameters) == ["dic_tmp", "y", "step"]


def test_wrappers_reject_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    pred, labels = torch.zeros(3, 4, 5), torch.zeros(6 * 7, dtype=torch.int32)
    with pytest.raises(ValueError):
        lt.upsample_ce_forward(pred.transpose(1, 2), labels, (6, 7))              # a strided pred
    with pytest.raises(ValueError):
        lt.upsample_ce_forward(pred.double(), labels, (6, 7))                      # a wide dtype
    with pytest.raises(ValueError):
        lt.upsample_ce_forward(torch.zeros(32, 4, 5), labels, (6, 7))              # 32 channels
    with pytest.raises(ValueError):
        lt.upsample_ce_forward(pred, labels[:-1], (6, 7))
    with pytest.raises(ValueError):
        lt.upsample_ce_forward(pred, labels.float(), (6, 7))
    for k in (0, 43):
        with pytest.raises(ValueError):
            lt.topk_mean(torch.zeros(42), k)
        with pytest.raises(ValueError):
            lt.topk_select_mask(torch.zeros(42), k, torch.zeros(1), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        lt.upsample_ce_backward(pred, labels, torch.zeros(41), torch.zeros(42, dtype=torch.uint8), torch.ones(1), (6, 7), k=3)      # lse one short
    with pytest.raises(ValueError):
        lt.upsample_ce_backward(pred, labels, torch.zeros(42), torch.zeros(42, dtype=torch.uint8), torch.ones(1), (6, 7))            # no divisor
    with pytest.raises(ValueError):
        lt.Concat_CrossEntropyLoss(0.15, 0).sample(torch.zeros(1, 3, 2, 2), torch.zeros(4, dtype=torch.int64), 0)                   # k = 0


def test_wrappers_need_a_device():
    with pytest.raises(_lib.AocHipError):
        lt.topk_mean(torch.zeros(42), 3)
    with pytest.raises(_lib.AocHipError):
        lt.upsample_ce_forward(torch.zeros(3, 4, 5), torch.zeros(42, dtype=torch.int64), (6, 7))


def test_entry_points_reject():
    """a rejection returns before anything is enqueued: no device is needed, and the pointers are never read"""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    fwd = lambda C, h=2, w=2, H=4, W=4, pred=p: L.aoc_upsample_ce_forward(pred, p, C, h, w, H, W, 255, p, p, p, p, p, None)
    assert fwd(0) == INVALID and fwd(32) == UNSUPPORTED and fwd(3, h=0) == INVALID and fwd(3, pred=None) == INVALID
    assert fwd(3, H=1 << 16, W=1 << 15) == UNSUPPORTED
    ws = L.aoc_topk_mean_workspace_bytes(1000)
    assert ws > 0 and L.aoc_topk_mean_workspace_bytes(0) == 0 and L.aoc_topk_select_mask_workspace_bytes(1000) > 0
    assert L.aoc_topk_mean_workspace_bytes(1 << 20) <= 1 << 16
    assert L.aoc_upsample_ce_partials(257) == 2
    for k in (0, 1001, -1):
        assert L.aoc_topk_mean(p, 1000, k, p, p, p, p, ws, None) == INVALID
        assert L.aoc_topk_select_mask(p, 1000, k, p, p, p, p, ws, None) == INVALID
    assert L.aoc_topk_mean(p, 1000, 5, p, p, p, p, ws - 1, None) == WORKSPACE and L.aoc_topk_mean(p, 1000, 5, p, p, p, None, ws, None) == WORKSPACE
    assert L.aoc_topk_mean(p, 1 << 31, 5, p, p, p, p, ws, None) == UNSUPPORTED and L.aoc_topk_mean(None, 1000, 5, p, p, p, p, ws, None) == INVALID
    assert L.aoc_valid_mean(p, 1000, None, 4, p, p, p, ws, None) == INVALID and L.aoc_valid_mean(p, 1000, p, 4, p, p, p, 0, None) == WORKSPACE
    assert L.aoc_topk_select_mask(p, 1000, 5, p, p, p, p, 0, None) == WORKSPACE
    assert L.aoc_valid_mask(p, 1000, 32, 255, p, None) == UNSUPPORTED and L.aoc_valid_mask(p, 1000, 0, 255, p, None) == INVALID
    grad = lambda C, k=3, nv=p, g=p: L.aoc_upsample_ce_grad(p, p, p, p, g, k, nv, C, 2, 2, 4, 4, 255, p, None)
    assert grad(32) == UNSUPPORTED and grad(0) == INVALID and grad(3, k=0, nv=None) == INVALID and grad(3, k=17) == INVALID and grad(3, g=None) == INVALID
    assert grad(3, k=-1) == INVALID
    cws = L.aoc_criterion_forward_workspace_bytes(16)
    crit = lambda C=3, k=3, loss=p, mean=p, ws=cws: L.aoc_criterion_forward(p, p, C, 2, 2, 4, 4, 255, k, loss, p, p, p, mean, p, p, p, ws, None)
    assert cws >= L.aoc_topk_mean_workspace_bytes(16) + L.aoc_topk_select_mask_workspace_bytes(16) and L.aoc_criterion_forward_workspace_bytes(0) == 0
    assert crit(C=32) == UNSUPPORTED and crit(C=0) == INVALID and crit(k=17) == INVALID and crit(k=-1) == INVALID and crit(loss=None) == INVALID
    assert crit(mean=None) == INVALID and crit(ws=cws - 1) == WORKSPACE
    assert bytes(buf) == bytes(1 << 16), "a rejected call writes nothing"
