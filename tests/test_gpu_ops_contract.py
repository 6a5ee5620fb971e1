"""The tensor contract of aoc_amd.ops on the device (tests/ops_contract_cases.py; the host half is tests/test_ops_contract_host.py).

Every variant of every tensor argument is first run under the recording stub with device tensors -- nothing is launched -- and held to the host
rule.  A variant that breaks the rule fails THERE and is never launched: no misread list or short buffer reaches a kernel.  A variant the
front-end converts is then run for real and must give the bits of the canonical call (the converted values are the same values); a variant the
front-end refuses must raise on the device too and leave the caller's buffers untouched."""
import numpy as np
import pytest
import torch

import ops_contract_cases as occ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()
    return aoc_amd


def _gate(monkeypatch, ops, case, a, errors):
    with monkeypatch.context() as mp:
        rec = occ.install(mp, ops)
        err, _ = occ.run_recorded(ops, case, a, errors)
    return rec, err


def _whole(t):
    return t._base if t._base is not None else t


@pytest.mark.parametrize("name", sorted(occ.CASES))
def test_contract_on_the_device(aoc, monkeypatch, name):
    ops, case = aoc.ops, occ.CASES[name]
    errors = occ.ERRORS + (aoc._lib.AocHipError,)
    a0 = case.build(ops, "cuda")
    rec, err = _gate(monkeypatch, ops, case, a0, errors)
    assert err is None and rec.calls, f"{name}: the canonical call under the stub: {err!r}"
    canon = rec.records
    want = [t.clone() for t in case.collect(case.call(ops, a0), a0)]
    torch.cuda.synchronize()
    assert want, f"{name}: no output is compared"
    for k, t in enumerate(want):
        assert t.numel() < 2 or float(t.double().min()) != float(t.double().max()), f"{name}: canonical output {k} {tuple(t.shape)} is constant"
    failed, ran = [], 0
    for label, transforms, role in occ.variants_of(case):
        a = occ.apply_variant(case.build(ops, "cuda"), transforms)
        if label.endswith(":strided") and all(a[n].is_contiguous() for n in transforms):
            continue
        rec, err = _gate(monkeypatch, ops, case, a, errors)
        bad = occ.check_rule(canon, rec, err, role, "cuda")
        if bad:
            failed.append(f"({name}, {label}) NOT LAUNCHED: {'; '.join(bad)}")
            continue
        ran += 1
        if err is None:                                                   # rule (b): converted -> the canonical bits
            got = case.collect(case.call(ops, a), a)
            torch.cuda.synchronize()
            for k, (g, w) in enumerate(zip(got, want)):
                if g.shape != w.shape or not torch.equal(g, w):
                    failed.append(f"({name}, {label}): output {k} differs from the canonical call's")
        else:                                                             # rule (a): refused on the device too, nothing written
            before = {n: _whole(t).clone() for n, t in a.items() if case.roles.get(n) == occ.OUT}
            with pytest.raises(errors):
                case.call(ops, a)
            torch.cuda.synchronize()
            for n, snap in before.items():
                if not torch.equal(_whole(a[n]), snap):
                    failed.append(f"({name}, {label}): the refused call wrote into {n}")
    assert ran, f"{name}: no variant was run"
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("N,C,D", [(3, 24, 400), (5, 65, 129)])
def test_cond_codes_with_float64_weights(aoc, N, C, D):
    """The reuse case itself: all six weights in float64, so each is read from a converted copy.  Taken inline, each copy was freed as soon
    as its address had been read and the next conversion could be handed the same block (b1's values at the start of W1); bound to names they
    all live across the launch.  Against the float64 reference and bound of test_cond_codes; b1 is far from the first row of W1, and
    test_ops_contract_host.py::test_cond_codes_misread_leaves_the_bound shows that the misread leaves this bound."""
    import float64_bounds as fb
    a = occ.cond_codes_args(N, C, D)
    dev = {k: (v.double() if k[0] in "wb" else v).cuda() for k, v in a.items()}
    got = aoc.ops.cond_codes(*[dev[k] for k in occ.COND_ROLES]).cpu()
    args = [a[k].double() for k in occ.COND_ROLES]
    want, tol = fb.cond_codes_ref(*args)
    for kind in ("no_minus", "drop_head"):
        fb._check_bound(got, want, tol, fb.cond_codes_ref(*args, slip=kind)[0], f"cond_codes float64 weights N={N} C={C} D={D} slip={kind}")
    assert torch.equal(got, aoc.ops.cond_codes(*[a[k].cuda() for k in occ.COND_ROLES]).cpu()), "float64 weights give other bits than their float32 values"


def test_calibration_gates_after_double(aoc):
    """hotpath.CalibrationGates.forward_batched keeps descriptors with raw pointers of the weights and, for weights that are not contiguous
    float32, converted copies.  After module.double() the next call must rebuild and give the float32 module's bits (float32 -> float64 ->
    float32 is exact) or raise -- and an in-place update of the float64 weights must be seen, not served from the stale copies."""
    hot = aoc.hotpath
    errors = occ.ERRORS + (aoc._lib.AocHipError,)
    torch.manual_seed(6)
    gates = hot.CalibrationGates(hot.MatchingConfig()).cuda()
    O, h, w = 2, 17, 23
    g = torch.Generator().manual_seed(10)
    acts = [torch.randn(O, c, hh, ww, generator=g).cuda() for (_, c, hh, ww, _) in gates.plan(h, w)]
    head = torch.randn(O, 400, generator=g).cuda()
    want = [t.clone() for t in gates.forward_batched(acts, head)]
    gates.double()
    try:
        got = [t.clone() for t in gates.forward_batched(acts, head)]
    except errors:
        return
    torch.cuda.synchronize()
    for name, a, b in zip([p[0] for p in gates.plan(h, w)], got, want):
        assert torch.equal(a, b), f"{name}: float64 parameters give other bits than the float32 module"
    with torch.no_grad():
        gates.IA1.IA.weight.mul_(0.5)                       # in place: same storage, new values (exact in either precision)
        gates.CLB2.CL_1.mlp_layer.bias.mul_(0.5)
    first = want
    got = [t.clone() for t in gates.forward_batched(acts, head)]
    gates.float()
    want = gates.forward_batched(acts, head)
    torch.cuda.synchronize()
    assert not torch.equal(want[0], first[0]) and not torch.equal(want[1], first[1]), "the update changes the first two gates' outputs"
    for name, a, b in zip([p[0] for p in gates.plan(h, w)], got, want):
        assert torch.equal(a, b), f"{name}: the batch served stale copies of float64 weights that were updated in place"
