"""The training update without a GPU (aoc_amd.optim_train, csrc/optim.hip; tests/optim_bounds.py holds the references and the bounds):

  - the float32 restatement of the kernels AND torch-CPU's clip_grad_norm_ + optim.SGD, each against the float64 reference taken at the state
    its own step received, over three steps (the first, a clipped one, an unclipped one) in five modes;
  - every slipped twin of the reference leaves the bound;
  - the chunk prefix and the owner search against a count made one element at a time;
  - adjust_learning_rate and get_trainable_params against what the reference's own file gave (tests/golden/optim_schedule.json);
  - a state_dict round trip with torch.optim.SGD, both ways;
  - what the constructor, the wrappers and the C entries reject, the entries before they would enqueue anything (no device is needed to be refused).
"""
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import aoc_amd
import optim_bounds as ob
from aoc_amd import _lib, ops
from aoc_amd import optim_train as ot

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_schedule.json")
LR, MAX_NORM = 0.01, 5.0
GRAD_SCALES = (1.0, 0.5, 1e-3)          # the first step and a second one above MAX_NORM (clipped), a third one below it (unclipped)


def _torch_step(params, opt, grads, max_norm):
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    return float(norm)


def _bufs(opt, params):
    return [None if opt.state[p].get("momentum_buffer") is None else opt.state[p]["momentum_buffer"].numpy().copy() for p in params]


@pytest.mark.parametrize("mode", sorted(ob.MODES))
def test_restatement_and_torch_cpu_are_inside_the_bound(mode):
    m = ob.MODES[mode]
    sizes = ob.HOST_SIZES
    wds = [m["wd"] if i % 3 else 0.0 for i in range(len(sizes))]                   # every third tensor a `beta`: no decay
    _, p0 = ob.make_list(sizes, 11)
    tparams = [nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    topt = torch.optim.SGD([{"params": [p], "weight_decay": wd} for p, wd in zip(tparams, wds)], lr=LR, momentum=m["momentum"], dampening=m["dampening"],
                           nesterov=m["nesterov"])
    mine_p, mine_b = [p.copy() for p in p0], [None] * len(sizes)
    worst = 0.0
    for step, scale in enumerate(GRAD_SCALES):
        grads, _ = ob.make_list(sizes, 100 + step, scale)
        # torch, from ITS state
        tp = [p.detach().numpy().copy() for p in tparams]
        tb = _bufs(topt, tparams) if step else [None] * len(sizes)
        N, dN, coef, ref = ob.clip_sgd_ref(grads, tp, tb, wds, [LR] * len(sizes), MAX_NORM, m["momentum"], m["dampening"], m["nesterov"])
        assert (coef.v < 1.0) == (step < 2), "the steps are a clipped first one, a clipped one and an unclipped one"
        tnorm = _torch_step(tparams, topt, grads, MAX_NORM)
        assert abs(tnorm - N) <= dN
        for p, (pe, be), buf in zip(tparams, ref, _bufs(topt, tparams)):
            worst = max(worst, ob.check(p.detach().numpy(), pe.v, pe.e))
            if be is not None:
                worst = max(worst, ob.check(buf, be.v, be.e))
        # the restatement, from ITS state
        N, dN, coef, ref = ob.clip_sgd_ref(grads, mine_p, mine_b, wds, [LR] * len(sizes), MAX_NORM, m["momentum"], m["dampening"], m["nesterov"])
        norm32, coef32 = ob.finish64(ob.partials32(grads), MAX_NORM)
        assert abs(float(norm32) - N) <= dN and abs(float(coef32) - coef.v) <= coef.e
        assert (coef32 == 1.0) == (step == 2)
        for i, (g, (pe, be)) in enumerate(zip(grads, ref)):
            mine_p[i], mine_b[i] = ob.step32(g, mine_p[i], mine_b[i], coef32, wds[i], LR, m["momentum"], m["dampening"], m["nesterov"])
            worst = max(worst, ob.check(mine_p[i], pe.v, pe.e))
            assert (be is None) == (mine_b[i] is None)
            if be is not None:
                worst = max(worst, ob.check(mine_b[i], be.v, be.e))
        # from the same state (the first step) the two implementations are therefore within twice the bound of each other
        if step == 0:
            for p, q, (pe, _) in zip(tparams, mine_p, ref):
                assert ob.check(p.detach().numpy(), q, 2 * pe.e) <= 1.0
    assert worst <= 1.0, f"{mode}: {worst:.3f} of the bound"


def _slip_case(slip):
    """kwargs of clip_sgd_ref: a small situation in which the mistake changes a value"""
    sizes = (257, 33)
    g, p = ob.make_list(sizes, 21)
    b = [x.astype(np.float32) for x in ob.make_list(sizes, 22)[0]]
    base = dict(grads=g, params=p, bufs=b, wds=[1e-4, 1e-4], lrs=[LR, LR], max_norm=MAX_NORM, momentum=0.9, dampening=0.0, nesterov=True)
    if slip == "unclamped":
        base["grads"] = ob.make_list(sizes, 21, 1e-3)[0]                            # norm below max_norm: the true coefficient is exactly 1
    elif slip == "no_eps":
        base.update(grads=ob.make_list(sizes, 21, 1e-5)[0], max_norm=1e-4, bufs=[None, None])    # norm near 2e-4: 1e-6 is half a percent of it; the first
                                                                                                    # step's buffer is d itself and shows it
    elif slip == "dampening_first":
        base.update(bufs=[None, None], dampening=0.1, nesterov=False)
    elif slip == "dampening_dropped":
        base.update(dampening=0.1, nesterov=False)
    return base


@pytest.mark.parametrize("slip", ob.SLIPS)
def test_every_slip_leaves_the_bound(slip):
    kw = _slip_case(slip)
    _, _, coef, ref = ob.clip_sgd_ref(**kw)
    _, _, _, bad = ob.clip_sgd_ref(slip=slip, **kw)
    norm32, coef32 = ob.finish64(ob.partials32(kw["grads"]), kw["max_norm"])
    ratio_bad, ratio_good = 0.0, 0.0
    for g, p, b, (pe, be), (pb, bb) in zip(kw["grads"], kw["params"], kw["bufs"], ref, bad):
        p32, b32 = ob.step32(g, p, b, coef32, 1e-4, LR, kw["momentum"], kw["dampening"], kw["nesterov"])
        ratio_good = max(ratio_good, ob.check(p32, pe.v, pe.e), ob.check(b32, be.v, be.e))
        ratio_bad = max(ratio_bad, ob.check(pb.v, pe.v, pe.e), ob.check(bb.v, be.v, be.e))
    assert ratio_good <= 1.0, f"the restatement is at {ratio_good:.3f} of the bound"
    assert ratio_bad > 4.0, f"{slip} is at {ratio_bad:.3f} of the bound: the bound would not notice it"


def _owner_by_search(begins, n_chunks):
    """csrc/optim.hip mt_find: the LAST record with chunk_begin <= c"""
    out = []
    for c in range(n_chunks):
        lo, hi = 0, len(begins) - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if begins[mid] <= c:
                lo = mid
            else:
                hi = mid - 1
        out.append(lo)
    return out


@pytest.mark.parametrize("sizes", [(0,), (1,), (4096,), (4097,), (0, 0, 5, 0), (5, 0, 0), (0, 4096, 0, 4097, 0, 1, 12288, 0), ob.SIZES, ob.HOST_SIZES,
                                   tuple([3] * 700)])
def test_chunk_prefix_against_a_brute_force_count(sizes):
    owner = ob.chunk_owner_brute(sizes)
    begins, n_chunks = ot.chunk_prefix(sizes)
    assert (begins, n_chunks) == ob.chunk_prefix(sizes) and n_chunks == len(owner)
    assert begins == [sum(1 for o in owner if o < i) for i in range(len(sizes))]
    assert _owner_by_search(begins, n_chunks) == owner
    L = _lib.lib()
    assert [L.aoc_mt_chunks(n) for n in sizes] == [owner.count(i) for i in range(len(sizes))] and L.aoc_mt_chunks(-3) == 0
    assert ot.CHUNK == ob.CHUNK == 4096
    with pytest.raises(ValueError):
        ot.chunk_prefix([3, -1])


# ------------------------------------------------------------------------------------------ utils/learning.py
class _Groups:
    def __init__(self):
        self.param_groups = [{"lr": None}, {"lr": None, "weight_decay": 0.0}]


def test_schedule_against_the_reference():
    gold = json.load(open(GOLDEN))
    assert {s["itr"] for s in gold["schedule"]} == {0, 1, 999, 1000, 1001, 25000, 49999, 50000}
    assert {s["is_cosine_decay"] for s in gold["schedule"]} == {False, True}
    assert any(s["floored"] and s["min_lr"] for s in gold["schedule"]) and any(not s["floored"] for s in gold["schedule"])
    for s in gold["schedule"]:
        opt = _Groups()
        kw = {} if s["min_lr"] is None else {"min_lr": s["min_lr"]}
        lr = ot.adjust_learning_rate(opt, s["base_lr"], s["p"], s["itr"], s["max_itr"], s["warm_up_steps"], s["is_cosine_decay"], **kw)
        assert lr == float.fromhex(s["lr_hex"]), s
        assert all(g["lr"] == lr for g in opt.param_groups)
    # the reference's defaults: warm-up 1000, polynomial, min_lr 1e-5
    want = [s for s in gold["schedule"] if not s["is_cosine_decay"] and s["min_lr"] is None]
    for s in want:
        assert ot.adjust_learning_rate(_Groups(), s["base_lr"], s["p"], s["itr"], s["max_itr"]) == float.fromhex(s["lr_hex"])


def _toy(spec):
    """a module whose named_parameters() are the recorded names, shapes and requires_grad flags, in the recorded order"""
    root = nn.Module()
    for name, shape, req in spec:
        mod, parts = root, name.split(".")
        for part in parts[:-1]:
            if part not in mod._modules:
                mod.add_module(part, nn.Module())
            mod = mod._modules[part]
        mod.register_parameter(parts[-1], nn.Parameter(torch.zeros(shape), requires_grad=req))
    assert [n for n, _ in root.named_parameters()] == [s[0] for s in spec]
    return root


def test_trainable_groups_against_the_reference():
    gold = json.load(open(GOLDEN))
    toy = _toy(gold["toy"])
    names = {id(p): n for n, p in toy.named_parameters()}
    assert any("beta" in s[0] for s in gold["toy"]) and any(not s[2] for s in gold["toy"])
    for beta_wd in (True, False):
        got = ot.get_trainable_params(toy, gold["base_lr"], gold["weight_decay"], beta_wd)
        got = [dict(names=[names[id(p)] for p in g["params"]], weight_decay=g["weight_decay"], lr=g["lr"]) for g in got]
        assert got == gold["groups"][str(beta_wd)]
    assert ot.get_trainable_params(toy, 0.1, 0.2) == ot.get_trainable_params(toy, 0.1, 0.2, True)         # the default keeps the betas' decay
    opt = ot.SGD(ot.get_trainable_params(toy, 0.01, 1e-4, False), lr=0.01, momentum=0.9, nesterov=True, clip_grad_norm=5.0)
    assert len(opt.param_groups) == sum(1 for s in gold["toy"] if s[2])
    assert ot.adjust_learning_rate(opt, 0.01, 0.9, 500, 50000) == 0.005 and all(g["lr"] == 0.005 for g in opt.param_groups)


# ------------------------------------------------------------------------------------------ checkpoints
def _cpu_model(seed):
    torch.manual_seed(seed)
    return [nn.Parameter(torch.randn(s)) for s in ((3, 4), (5,), (2, 2, 2))]


def _torch_sgd(params):
    return torch.optim.SGD([{"params": [p], "weight_decay": wd} for p, wd in zip(params, (1e-4, 0.0, 1e-4))], lr=LR, momentum=0.9, nesterov=True)


def _backward(params, seed):
    torch.manual_seed(seed)
    for p in params:
        p.grad = torch.randn_like(p)


def _through_a_file(state_dict):
    """torch.save / torch.load, as a checkpoint travels (state_dict() itself hands out the live buffers)"""
    buf = io.BytesIO()
    torch.save(state_dict, buf)
    buf.seek(0)
    return torch.load(buf)


def test_state_dict_round_trip_with_torch_sgd():
    a = _cpu_model(1)
    topt = _torch_sgd(a)
    _backward(a, 2)
    topt.step()
    saved = _through_a_file(topt.state_dict())
    # torch -> here
    b = [nn.Parameter(p.detach().clone()) for p in a]
    mine = ot.SGD([{"params": [p], "weight_decay": wd} for p, wd in zip(b, (1e-4, 0.0, 1e-4))], lr=0.5, momentum=0.9, nesterov=True, clip_grad_norm=5.0)
    mine.load_state_dict(saved)
    assert [g["lr"] for g in mine.param_groups] == [LR] * 3 and [g["weight_decay"] for g in mine.param_groups] == [1e-4, 0.0, 1e-4]
    for p, q in zip(a, b):
        assert torch.equal(topt.state[p]["momentum_buffer"], mine.state[q]["momentum_buffer"])
    assert set(mine.state_dict()["state"][0]) == {"momentum_buffer"}
    # here -> torch: a fresh torch optimiser that loads this module's checkpoint continues as the original does
    c = [nn.Parameter(p.detach().clone()) for p in a]
    again = _torch_sgd(c)
    again.load_state_dict(_through_a_file(mine.state_dict()))
    _backward(a, 3)
    _backward(c, 3)
    topt.step()
    again.step()
    for p, q in zip(a, c):
        assert torch.equal(p, q) and torch.equal(topt.state[p]["momentum_buffer"], again.state[q]["momentum_buffer"])


# ------------------------------------------------------------------------------------------ rejections
def test_constructor_rejections():
    p = nn.Parameter(torch.zeros(4, 3))
    for kw in (dict(maximize=True), dict(differentiable=True), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1), dict(momentum=-0.1),
               dict(weight_decay=-1.0), dict(clip_grad_norm=0.0), dict(clip_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            ot.SGD([p], lr=0.1, **kw)
    with pytest.raises(ValueError):
        ot.SGD([p], lr=-0.1)
    with pytest.raises(ValueError):
        ot.SGD([nn.Parameter(torch.zeros(3, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError):
        ot.SGD([nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))], lr=0.1)
    with pytest.raises(ValueError):
        ot.SGD([nn.Parameter(torch.zeros(4, 3).t())], lr=0.1)                        # not contiguous
    with pytest.raises(ValueError):
        ot.SGD([p, nn.Parameter(torch.zeros(3, device="meta"))], lr=0.1)             # another device
    opt = ot.SGD([p], lr=0.1, momentum=0.9)
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [nn.Parameter(torch.zeros(3, device="meta"))]})
    assert opt.table_uploads == 0 and opt.total_norm is None and opt.step() is None   # no gradient anywhere: nothing to do, nothing raised


def test_no_cpu_fallback_and_the_module_is_exported():
    p = nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.ones(4, 3)
    opt = ot.SGD([p], lr=0.1, momentum=0.9, clip_grad_norm=1.0)
    with pytest.raises(_lib.AocHipError):
        opt.step()
    with pytest.raises(_lib.AocHipError):
        opt.zero_grad(set_to_none=False)
    with pytest.raises(_lib.AocHipError):
        ot.clip_grad_norm_([p], 1.0)
    assert torch.equal(p.detach(), torch.zeros(4, 3)) and torch.equal(p.grad, torch.ones(4, 3)) and not opt.state[p]
    with pytest.raises(ValueError):
        ot.clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(ValueError):
        ot.clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    p.grad = torch.ones(3, 4).t()
    with pytest.raises(ValueError):
        opt.step()                                                                   # a gradient that is not contiguous
    opt.zero_grad()
    assert p.grad is None
    g1, g2 = ot.SGD([{"params": [p]}, {"params": [nn.Parameter(torch.zeros(2))], "momentum": 0.5}], lr=0.1, momentum=0.9), None
    g1.param_groups[0]["params"][0].grad = torch.ones(4, 3)
    with pytest.raises(ValueError):
        g1.step()                                                                    # momentum differs between the groups
    assert "optim_train" in aoc_amd.__all__ and aoc_amd.optim_train is ot
    for name in ("sgd_step", "clip_sgd_step", "grad_sumsq_partials", "grad_norm_finish", "multi_tensor_scale", "multi_tensor_zero"):
        assert hasattr(ot, name) and not hasattr(ops, name)


def _host_table(sizes, begins=None, param=0x1000, grad=0x2000, momentum=0x3000):
    arr = (ot._MtTensor * len(sizes))()
    for i, (rec, n) in enumerate(zip(arr, sizes)):
        rec.param, rec.grad, rec.momentum, rec.n, rec.weight_decay, rec.flags = param, grad, momentum, n, 0.0, 0
        rec.chunk_begin = (begins if begins is not None else ot.chunk_prefix([max(s, 0) for s in sizes])[0])[i]
    return arr


def test_entries_reject_before_they_enqueue():
    """AOC_ERR_INVALID_ARG from the host checks alone: none of these calls reaches a launch, so none needs a device (the pointers are never
    followed).  The record layout is the C compiler's."""
    L = _lib.lib()
    assert ctypes.sizeof(ot._MtTensor) == 48 and ot._MtTensor.n.offset == 24 and ot._MtTensor.chunk_begin.offset == 32
    assert ot._MtTensor.weight_decay.offset == 40 and ot._MtTensor.flags.offset == 44
    dev = ctypes.c_void_p(0x10000)                             # stands for the device table: a rejected call never reads it
    word = ctypes.c_void_p(0x20000)
    INVALID = -1

    def step(arr, n_chunks, momentum=0.9, dampening=0.0, nesterov=1, n_tensors=None):
        return L.aoc_sgd_step(dev, ctypes.addressof(arr), len(arr) if n_tensors is None else n_tensors, n_chunks, None, 0.1, None, momentum, dampening,
                              nesterov, 0, None)

    good = _host_table((5, 0, 4097))
    assert step(good, 3, momentum=-0.5, nesterov=0) == INVALID
    assert step(good, 3, momentum=float("nan"), nesterov=0) == INVALID
    assert step(good, 3, momentum=0.0, nesterov=1) == INVALID
    assert step(good, 3, momentum=0.9, dampening=0.1, nesterov=1) == INVALID
    assert step(good, 2) == INVALID and step(good, 4) == INVALID                    # n_chunks is not the table's total
    assert step(good, -1) == INVALID and step(good, 3, n_tensors=-1) == INVALID
    assert step(_host_table((5, -1, 4097)), 3) == INVALID                           # a negative size
    assert step(_host_table((5, 0, 4097), begins=[0, 1, 2]), 3) == INVALID          # the empty tensor was given a chunk
    assert step(_host_table((5, 0, 4097), begins=[0, 0, 1]), 3) == INVALID          # the first tensor's chunk is not counted
    assert step(_host_table((5, 0, 4097), param=0), 3) == INVALID                   # a gradient without a parameter
    assert step(_host_table((5, 0, 4097), momentum=0), 3) == INVALID                # momentum != 0 without a buffer
    huge = _host_table((2 ** 31 * 4096,))
    assert step(huge, 2 ** 31) == INVALID                                           # n_chunks beyond int32
    assert L.aoc_sgd_step(None, ctypes.addressof(good), 3, 3, None, 0.1, None, 0.9, 0.0, 1, 0, None) == INVALID
    for arr, n_chunks in ((_host_table((5, -1)), 1), (_host_table((5, 7), begins=[1, 2]), 2), (huge, 2 ** 31)):
        a = ctypes.addressof(arr)
        assert L.aoc_grad_sumsq_partials(dev, a, len(arr), n_chunks, word, None) == INVALID
        assert L.aoc_multi_tensor_scale(dev, a, len(arr), n_chunks, word, None) == INVALID
        assert L.aoc_multi_tensor_zero(dev, a, len(arr), n_chunks, None) == INVALID
        assert L.aoc_clip_sgd_step(dev, a, len(arr), n_chunks, 5.0, word, 0.1, None, 0.9, 0.0, 1, 0, word, 1 << 20, None) == INVALID
    a = ctypes.addressof(good)
    assert L.aoc_grad_sumsq_partials(dev, a, 3, 3, None, None) == INVALID
    assert L.aoc_grad_sumsq_partials(dev, a, 3, 3, ctypes.c_void_p(0x20004), None) == INVALID          # partial is read and written as doubles
    assert L.aoc_multi_tensor_scale(dev, a, 3, 3, None, None) == INVALID
    assert L.aoc_grad_norm_finish(None, 3, 5.0, word, word, None) == INVALID
    assert L.aoc_grad_norm_finish(word, -1, 5.0, word, word, None) == INVALID
    assert L.aoc_grad_norm_finish(word, 3, 5.0, None, None, None) == INVALID
    assert L.aoc_clip_sgd_step(dev, a, 3, 3, 5.0, None, 0.1, None, 0.9, 0.0, 1, 0, word, 1 << 20, None) == INVALID
    assert L.aoc_clip_sgd_step(dev, a, 3, 3, 5.0, word, 0.1, None, 0.9, 0.0, 1, 0, None, 0, None) == INVALID
    assert L.aoc_clip_sgd_step(dev, a, 3, 3, 5.0, word, 0.1, None, 0.9, 0.0, 1, 0, word, 8, None) == -2   # AOC_ERR_WORKSPACE
    assert L.aoc_clip_sgd_step_workspace_bytes(3) == 3 * 8 + 16 and L.aoc_clip_sgd_step_workspace_bytes(-1) == 0
    assert all(rec.flags == 0 for rec in good), "a rejected call has set a flag in the host mirror"
