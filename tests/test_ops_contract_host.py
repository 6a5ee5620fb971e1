"""The tensor contract of aoc_amd.ops on the host: no GPU, no library.  A stub stands in for libaoc_hip.so and _p / _addr are wrapped, so every
address that would reach the library is seen together with the tensor behind it (tests/ops_contract_cases.py).  Each registry case runs in its
canonical form and with every variant of every tensor argument; a variant passes when it raises before the library is called, or when every
pointer position receives a contiguous tensor of the canonical dtype, at least the canonical size, on the input's device, that is still
alive when the library function is entered."""
import ast
import inspect

import numpy as np
import pytest
import torch

import aoc_amd
from aoc_amd import _lib, ops

import ops_contract_cases as occ

ERRORS = occ.ERRORS + (_lib.AocHipError,)


def run_case(monkeypatch, case, device, narrow=True):
    """-> (canonical records, [(variant label, complaints)])."""
    with monkeypatch.context() as mp:
        rec = occ.install(mp, ops)
        err, _ = occ.run_recorded(ops, case, case.build(ops, device), ERRORS)
    assert err is None, f"{case.name}: the canonical call raised {err!r}"
    assert rec.calls and rec.records, f"{case.name}: the canonical call never reached the library"
    canon = rec.records
    assert all(r.shape is None or (r.contiguous and r.alive) for r in canon), f"{case.name}: the canonical call hands over a dead or strided tensor"
    results = []
    for label, transforms, role in occ.variants_of(case, narrow=narrow):
        a = occ.apply_variant(case.build(ops, device), transforms)
        if label.endswith(":strided") and all(a[n].is_contiguous() for n in transforms):
            continue                                    # one element along the last axis: every second element of two IS contiguous
        with monkeypatch.context() as mp:
            rec = occ.install(mp, ops)
            err, _ = occ.run_recorded(ops, case, a, ERRORS)
        results.append((label, occ.check_rule(canon, rec, err, role, device)))
    return canon, results


@pytest.mark.parametrize("name", sorted(occ.CASES))
def test_contract_on_the_host(monkeypatch, name):
    case = occ.CASES[name]
    _, results = run_case(monkeypatch, case, "cpu")
    assert results, f"{name}: no variant was run"
    failed = [f"({name}, {label}): {'; '.join(bad)}" for label, bad in results if bad]
    assert not failed, "\n".join(failed)


def test_every_public_callable_is_listed():
    """A condition, not a target: every public callable of ops has a registry case or stands in the exemption table with its reason, and
    nothing that takes a device tensor is exempt (an exempt callable, run under the recorder, takes no address)."""
    public = {n for n, v in vars(ops).items() if callable(v) and not n.startswith("_") and getattr(v, "__module__", None) == ops.__name__}
    covered = {c for case in occ.CASES.values() for c in case.covers}
    assert not (covered & set(occ.EXEMPT)), "a callable is both covered and exempt"
    missing = public - covered - set(occ.EXEMPT)
    assert not missing, f"public callables of ops in neither table: {sorted(missing)}"
    stale = (covered | set(occ.EXEMPT)) - public
    assert not stale, f"listed but not in ops: {sorted(stale)}"
    structures = [n for n, v in vars(ops).items() if inspect.isclass(v) and issubclass(v, __import__("ctypes").Structure) and v.__module__ == ops.__name__]
    assert structures and all(n.startswith("_") for n in structures), "the ctypes.Structure classes are private: they carry addresses, never tensors"
    for n in occ.EXEMPT:
        src = inspect.getsource(getattr(ops, n))
        assert "_p(" not in src and "_addr(" not in src and "data_ptr" not in src, f"{n} is exempt but takes a tensor's address"


def test_exempt_callables_take_no_address(monkeypatch):
    rec = occ.install(monkeypatch, ops)
    monkeypatch.setattr(ops._lib, "check", lambda rc, what: None)
    ops.kmeans_init_rows_draw(np.random.RandomState(0), [5, 7], [2], 1)
    assert ops.split_record_bytes(100) == 448
    ops.dense_prune_stats()
    ops.set_stream_cus(0)
    ops.inference_only("x", torch.zeros(1))
    assert not rec.records


def _source_patterns():
    tree = ast.parse(inspect.getsource(ops))
    inline, stray = [], []
    parents = {}
    for node in ast.walk(tree):
        for child in ast.iter_child_nodes(node):
            parents[child] = node
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ("_p", "_addr"):
            if any(isinstance(sub, ast.Call) for arg in node.args for sub in ast.walk(arg)):
                inline.append(node.lineno)
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "data_ptr":
            up, fn, compared = node, None, False
            while up in parents:
                up = parents[up]
                compared = compared or isinstance(up, ast.Compare)
                if isinstance(up, ast.FunctionDef):
                    fn = up.name
                    break
            if fn not in ("_p", "_addr") and not compared:
                stray.append(node.lineno)
    return inline, stray


def test_no_inline_conversion_and_no_stray_data_ptr():
    """Two patterns in the source of ops.py: a call expression as the argument of _p / _addr (its result dies as soon as the address is read),
    and a .data_ptr() outside the two helpers (comparisons of addresses excepted)."""
    inline, stray = _source_patterns()
    assert not inline, f"ops.py lines {inline}: a call expression inside _p(...) / _addr(...)"
    assert not stray, f"ops.py lines {stray}: .data_ptr() outside _p / _addr"


def test_conversion_helpers():
    t = torch.arange(6, dtype=torch.int64).reshape(2, 3)
    c = ops._i32c(t[:, ::2])
    assert c.dtype == torch.int32 and c.is_contiguous() and c.tolist() == [[0, 2], [3, 5]]
    same = torch.zeros(3, dtype=torch.int32)
    assert ops._i32c(same) is same and ops._f32c(torch.zeros(2)).dtype == torch.float32
    bits = torch.tensor([-2147483648 + 5], dtype=torch.int64)              # a label-bit pattern with bit 31 set, sign-extended
    assert ops._i32c(bits).view(torch.int32).item() == -2147483648 + 5
    ok = torch.zeros(2, 3)
    assert ops._out("x", ok, (2, 3)) is ok and ops._span("x", ok, 6) is ok
    for bad in (ok.double(), torch.zeros(2, 6)[:, ::2], torch.zeros(6)[:5]):
        with pytest.raises(ValueError):
            ops._out("x", bad, (2, 3))
        with pytest.raises(ValueError):
            ops._span("x", bad, 6)
    assert ops._addr(None) is None and ops._addr(ok) == ok.data_ptr() and ops._p(ok).value == ok.data_ptr()


def test_cond_codes_misread_leaves_the_bound():
    """What the freed-copy reuse in cond_codes would have computed: b1's values at the start of W1.  With the weights of the registry case the
    float64 reference evaluated that way leaves test_cond_codes' bound by orders of magnitude at both shapes the device test runs, so that
    test cannot pass on misread weights."""
    from float64_bounds import cond_codes_ref
    for N, C, D in ((3, 24, 400), (5, 65, 129)):
        a = {k: v.double() for k, v in occ.cond_codes_args(N, C, D).items()}
        want, tol = cond_codes_ref(*[a[k] for k in occ.COND_ROLES])
        w1 = a["w1"].clone()
        w1.view(-1)[:C] = a["b1"]
        wrong, _ = cond_codes_ref(a["gap"], a["plane_means"], a["head"], w1, *[a[k] for k in ("b1", "w2", "b2", "w3", "b3")])
        assert float((a["b1"] - a["w1"][0]).abs().min()) > 1.0
        assert bool(((wrong - want).abs() > 100 * tol).any()), (N, C, D)
