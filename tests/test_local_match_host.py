"""The reference and bounds of tests/local_match_bounds.py checked without a GPU.

1. The plain float64 reference is oracle.matching.local_matching (the restatement of AEM:968-1060 that the goldens trust).  The oracle is not
   a float64 function even on float64 tensors: its dot product is taken after `.float()` and its result ends in `.float()` (AEM:1052).  So the
   features of this comparison sit on the grid 2^-8 (every product and sum of the dot product is then exact in float32, and both sides
   compute the same real numbers), and the transformed reference is rounded to float32 as the oracle's last line does.  After that the two
   agree to 1e-12.
2. numpy float32 restatements of the two kernels' order of operations lie inside the bound at every case of the GPU test.  The register
   kernel: lane g holds the float4 pieces g, g + 4, ... of a pixel (and channel 16 NP + g at C = 100), four fmaf chains per lane, the
   (s0 + s1) + (s2 + s3) fold, the two shuffle adds.  The LDS-image kernel: lane kq holds channels kq, kq + 4, ... of the query (a
   sequential sum, two shuffle adds); a candidate's norm is one sequential sum, kq-major.  In both the dot product is a k-ordered chain of
   rounded products (what the order of the matrix instruction really is, is not documented: the bound does not depend on it).  float16
   mode has np.float16 round trips where the kernels have aoc_h.  fmaf is restated as in test_decoder_bounds_host.py: the float32 rounding
   of the float64 sum of the exact product and the addend.
3. Every slip named by local_slips(case) leaves the bound at every case, and the conditions on the reference hold at every case."""
import numpy as np
import pytest
import torch

import local_match_bounds as lb
from local_match_bounds import LOCAL_CASES, LOCAL_LDS_CASES, check_bound

f32 = np.float32


# ------------------------------------------------------------------------------------------ 1. the reference is the oracle
ORACLE_CASES = [(100, 9, 14, (2, 4, 6), 1, 4), (36, 8, 11, (3, 4, 9), 2, 7), (128, 10, 13, (3, 7, 12), 3, 7), (100, 5, 7, (0, 3), 1, 7)]


@pytest.mark.parametrize("C,H,W,radii,rate,n_obj", ORACLE_CASES)
def test_reference_is_the_oracle(C, H, W, radii, rate, n_obj):
    from oracle import matching as om
    case = lb._case(f"oracle_{C}_{H}x{W}_rate{rate}", C, H, W, radii, rate=rate, n_obj=n_obj)
    inp = lb.local_inputs(case)
    grid = lambda a: (np.round(a.astype(np.float64) * 256.0) / 256.0).astype(f32)
    query, prev = grid(inp["query"]), grid(inp["prev"])
    want_raw, tol_raw = lb.local_window_ref(query, prev, inp["bits"], radii, rate, n_obj)
    want, _ = lb.local_transform_ref(want_raw, tol_raw, None)
    planes = lb.object_planes(inp["bits"], n_obj).reshape(n_obj, H, W)
    labels = torch.from_numpy(planes.astype(np.float64)).permute(1, 2, 0).contiguous()
    got = om.local_matching(torch.from_numpy(prev).double(), torch.from_numpy(query).double(), labels, dis_bias=0.0,
                            multi_local_distance=radii, atrous_rate=rate, allow_downsample=False)
    got = got[0].permute(2, 3, 0, 1).double().numpy()                      # [1, H, W, O, R] -> [O, R, H, W]
    assert got.shape == want.shape
    lb.check_conditions(case, want_raw, want)
    assert np.abs(want.astype(f32).astype(np.float64) - got).max() <= 1e-12


# ------------------------------------------------------------------------------------------ 2. float32 restatements of the kernels
def _h(x):
    return np.asarray(x, f32).astype(np.float16).astype(f32)


def _fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _reg_lane_channels(C, g):
    """The channels local_window_reg_kernel's lane (j, g) holds, in the order of its registers v[0 .. TMAX - 1]."""
    tmax = C // 4
    ch = [16 * u + 4 * g + e for u in range(tmax // 4) for e in range(4)]
    if tmax % 4:
        ch.append(16 * (tmax // 4) + g)
    return ch


def _reg_sq_norm(x, f16):
    C = x.shape[1]
    tmax = C // 4
    lanes = []
    for g in range(4):
        v = x[:, _reg_lane_channels(C, g)]
        s = [np.zeros(x.shape[0], f32) for _ in range(4)]
        for t in range(0, tmax - 3, 4):
            for e in range(4):
                s[e] = s[e] + _h(v[:, t + e] * v[:, t + e]) if f16 else _fmaf(v[:, t + e], v[:, t + e], s[e])
        if tmax % 4:
            s[0] = s[0] + _h(v[:, -1] * v[:, -1]) if f16 else _fmaf(v[:, -1], v[:, -1], s[0])
        lanes.append((s[0] + s[1]) + (s[2] + s[3]))
    s = (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])
    assert s.dtype == f32
    return _h(s) if f16 else s


def _lds_query_sq_norm(x, f16):
    C = x.shape[1]
    parts = []
    for kq in range(4):
        part = np.zeros(x.shape[0], f32)
        for t in range(C // 4):
            a = x[:, 4 * t + kq]
            part = part + (_h(a * a) if f16 else a * a)
        parts.append(part)
    s = (parts[0] + parts[1]) + (parts[2] + parts[3])
    return _h(s) if f16 else s


def _lds_cand_sq_norm(x, f16):
    C = x.shape[1]
    s = np.zeros(x.shape[0], f32)
    for kq in range(4):
        for t in range(C // 4):
            a = x[:, 4 * t + kq]
            s = s + (_h(a * a) if f16 else a * a)
    return _h(s) if f16 else s


def _dot_chain(q, p, order):
    acc = np.zeros((q.shape[0], p.shape[0]), f32)
    for c in order:
        acc = acc + q[:, c][:, None] * p[:, c][None, :]
    assert acc.dtype == f32
    return acc


def emulate_raw(case, query, prev, bits):
    """The kernel's raw output [n_obj, n_radii, H, W], float32 step by step."""
    C, f16 = case.C, case.f16
    q, p = query.reshape(-1, C), prev.reshape(-1, C)
    if f16:
        q, p = _h(q), _h(p)
    if lb.kernel_of(C) == "reg":
        q2, y2 = _reg_sq_norm(q, f16), _reg_sq_norm(p, f16)
        order = [_reg_lane_channels(C, g)[t] for t in range(C // 4) for g in range(4)]
    else:
        q2, y2 = _lds_query_sq_norm(q, f16), _lds_cand_sq_norm(p, f16)
        order = list(range(C))
    assert sorted(order) == list(range(C))
    acc = _dot_chain(q, p, order)
    if f16:
        d = _h(_h(q2[:, None] + y2[None, :]) - f32(2) * _h(acc))
    else:
        d = (q2[:, None] + y2[None, :]) - f32(2) * acc
    assert d.dtype == f32
    ring = lb.pair_rings(case.H, case.W, case.rate)
    planes = lb.object_planes(bits, case.n_obj)
    got, _ = lb.nested_min(d.astype(np.float64), np.zeros(d.shape), ring, planes, list(case.radii), case.rate, lb.PAD_H if f16 else lb.PAD)
    return lb.kernel_order(got).reshape(case.n_obj, len(case.radii), case.H, case.W).astype(f32)


def emulate_transform(raw, bias):
    """aoc_proto_transform in float32."""
    with np.errstate(under="ignore"):
        t = raw + bias.reshape(-1, 1, 1, 1)
        s = f32(1) / (f32(1) + np.exp(-t))
        out = (s - f32(0.5)) * f32(2)
    assert out.dtype == f32
    return out


@pytest.mark.parametrize("case", LOCAL_CASES + LOCAL_LDS_CASES, ids=lambda c: c.name)
def test_bound_holds_the_emulation_and_sheds_the_slips(case):
    inp = lb.local_inputs(case)
    maps = ["prev", "prev_b"] if case.pair else ["prev"]
    refs = {m: lb.local_case_ref(case.name, m) for m in maps}
    for m in maps:
        want, tol, slips = refs[m]
        assert (tol[want == (lb.PAD_H if case.f16 else lb.PAD)] == 0).all()
        slips = dict(slips)
        if case.pair and m == "prev_b":
            slips["other_map"] = refs["prev"][0]
        got = emulate_raw(case, inp["query"], inp[m], inp["bits"])
        want_t = tol_t = got_t = None
        if case.transformed:
            want_t, tol_t = lb.local_transform_ref(want, tol, inp["bias"])
            got_t = emulate_transform(got, inp["bias"])
        lb.check_conditions(case, want, want_t)
        assert set(slips) >= set(lb.local_slips(case))
        for kind, slip in slips.items():
            check_bound(got, want, tol, slip, f"{case.name} {m} raw, slip {kind}")
            if case.transformed:
                check_bound(got_t, want_t, tol_t, lb.local_transform_ref(slip, np.zeros_like(slip), inp["bias"])[0],
                            f"{case.name} {m} transformed, slip {kind}")


def test_raw_bound_is_of_the_size_of_float32():
    """|q - p|^2 of O(1) at C = 100: the bound is a few hundred float32 roundings, not a fitted 5e-6; and the lists hold what the GPU test
    says they hold: both kernels, both modes, a transformed case of each, the pair entry, and two requests above 64 KB."""
    want, tol, _ = lb.local_case_ref("reg_model_C100")
    assert 0 < tol.max() < 1e-4 and np.median(want[want < lb.PAD]) < 2.0
    for kern in ("reg", "lds"):
        for f16 in (False, True):
            assert any(lb.kernel_of(c.C) == kern and c.f16 == f16 and c.transformed for c in LOCAL_CASES), (kern, f16)
        assert any(lb.kernel_of(c.C) == kern and c.pair for c in LOCAL_CASES)
    assert [lb.lds_image_bytes(c.C, c.radii, c.rate, c.n_obj) for c in LOCAL_LDS_CASES] == [66560, 104448]
    for c in LOCAL_CASES:
        assert lb.kernel_of(c.C) == "reg" or lb.lds_image_bytes(c.C, c.radii, c.rate, c.n_obj) <= 64 * 1024, c.name
