"""The window kernels of csrc/local_match.hip called directly (ops.local_window_match / ops.local_window_match_pair) and compared with the
plain float64 reference of tests/local_match_bounds.py under the bound derived there from the kernels' float32 expressions: raw distances
(transform = 0) in every case, transformed outputs with a bias of mixed signs in one case per kernel and mode.  right_bits are built in
numpy (a tenth of the pixels carry bits at or above n_obj and bit 31), never through label_bits.  Every comparison goes through
_check_bound once per slip of local_slips(case): the same reference with one deliberate mistake must leave the bound.
test_local_match_host.py proves without a GPU that the reference is the oracle's local_matching, that float32 restatements of both kernels
lie inside the bound and that every slip leaves it, at every case of this file.

C = 100 / 128 take local_window_reg_kernel, every other C local_window_kernel<32> (the LDS-image kernel): the two kernels the file has."""
import ctypes

import numpy as np
import pytest
import torch

import local_match_bounds as lb
from local_match_bounds import LOCAL_CASES, LOCAL_LDS_CASES, check_bound

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED = 0, -1, -4


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    return aoc_amd


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _run(aoc, case, inp, transform):
    """-> {map name: kernel output [n_obj, n_radii, H, W] as numpy}"""
    q, p, bits = dev(inp["query"]), dev(inp["prev"]), dev(inp["bits"])
    bias = dev(inp["bias"]) if transform else None
    if case.pair:
        out = aoc.ops.local_window_match_pair(q, p, dev(inp["prev_b"]), bits, case.radii, bias, case.n_obj, transform=transform)
        return {"prev": out[0].cpu().numpy(), "prev_b": out[1].cpu().numpy()}
    out = aoc.ops.local_window_match(q, p, bits, case.radii, bias, case.n_obj, transform=transform, atrous_rate=case.rate, float16=case.f16)
    return {"prev": out.cpu().numpy()}


def _compare(aoc, case):
    inp = lb.local_inputs(case)
    maps = ["prev", "prev_b"] if case.pair else ["prev"]
    refs = {m: lb.local_case_ref(case.name, m) for m in maps}
    raw = _run(aoc, case, inp, False)
    tr = _run(aoc, case, inp, True) if case.transformed else None
    for m in maps:
        want, tol, slips = refs[m]
        slips = dict(slips)
        if m == "prev_b":
            slips["other_map"] = refs["prev"][0]
        want_t = tol_t = None
        if case.transformed:
            want_t, tol_t = lb.local_transform_ref(want, tol, inp["bias"])
        lb.check_conditions(case, want, want_t)
        err = np.abs(raw[m].astype(np.float64) - want)
        print(f"{case.name} {m}: raw worst error {err.max():.3e}, worst error / bound {(err / np.where(tol > 0, tol, 1.0)).max():.3f}, "
              f"bound up to {tol.max():.3e}")
        rings = [r // case.rate for r in case.radii]
        chan = lambda i: 0 if i == len(rings) - 1 else i + 1
        for i in range(1, len(rings)):
            if rings[i] == rings[i - 1]:      # radii that collapse onto one ring after // rate: the same nested window, the same bits
                assert np.array_equal(raw[m][:, chan(i)], raw[m][:, chan(i - 1)]), f"{case.name}: radii {case.radii[i - 1]} and {case.radii[i]} differ"
        for kind, slip in slips.items():
            check_bound(raw[m], want, tol, slip, f"{case.name} {m} raw, slip {kind}")
            if case.transformed:
                check_bound(tr[m], want_t, tol_t, lb.local_transform_ref(slip, np.zeros_like(slip), inp["bias"])[0],
                            f"{case.name} {m} transformed, slip {kind}")


@pytest.mark.parametrize("case", LOCAL_CASES, ids=lambda c: c.name)
def test_local_window_match(aoc, case):
    _compare(aoc, case)


@pytest.mark.parametrize("case", LOCAL_LDS_CASES, ids=lambda c: c.name)
def test_largest_lds_request(aoc, case):
    """The LDS-image kernel with more than 64 KB of dynamic LDS (66 560 and 104 448 bytes; the entry accepts up to 150 KB): the call returns
    AOC_OK (ops raises otherwise) and meets the bound."""
    assert lb.lds_image_bytes(case.C, case.radii, case.rate, case.n_obj) > 64 * 1024
    _compare(aoc, case)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ rejections: return codes only, nothing is launched
def _call(aoc, C=36, H=3, W=5, radii=(1, 2), n_obj=3, rate=1, pair=False, null_prev_b=False):
    L = aoc._lib.lib()
    hw = max(H, 1) * W
    q = torch.zeros(hw * C, dtype=torch.float32, device="cuda")
    p = torch.zeros_like(q)
    bits = torch.zeros(hw, dtype=torch.int32, device="cuda")
    out = torch.zeros(2 * n_obj * len(radii) * hw, dtype=torch.float32, device="cuda")
    r = np.ascontiguousarray(np.asarray(radii, np.int32))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rp = r.ctypes.data_as(ctypes.c_void_p)
    st = aoc.ops._stream()
    if pair:
        return L.aoc_local_window_match_pair(ptr(q), ptr(p), None if null_prev_b else ptr(p), ptr(bits), H, W, C, rp, len(radii), None, n_obj,
                                             ptr(out), ptr(out[out.numel() // 2:]), 0, st)
    return L.aoc_local_window_match_ex(ptr(q), ptr(p), ptr(bits), H, W, C, rp, len(radii), None, n_obj, ptr(out), 0, rate, 0, st)


REJECTIONS = [
    ("C132", dict(C=132), UNSUPPORTED), ("C6", dict(C=6), UNSUPPORTED), ("R32", dict(radii=(32,)), UNSUPPORTED),
    ("nine_radii", dict(radii=tuple(range(1, 10))), UNSUPPORTED), ("31_objects", dict(n_obj=31), UNSUPPORTED),
    ("radii_not_increasing", dict(radii=(3, 3)), INVALID_ARG), ("negative_radius", dict(radii=(-1, 3)), INVALID_ARG),
    ("rate0", dict(rate=0), INVALID_ARG), ("H0", dict(H=0), INVALID_ARG), ("pair_null_prev_b", dict(pair=True, null_prev_b=True), INVALID_ARG),
]


def test_the_call_of_the_rejection_tests_is_accepted(aoc):
    """The call that test_rejections spoils one argument of, unspoilt (a 3 x 5 map of zeros without labels)."""
    assert _call(aoc) == OK and _call(aoc, pair=True) == OK
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,kw,code", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_rejections(aoc, name, kw, code):
    assert _call(aoc, **kw) == code
