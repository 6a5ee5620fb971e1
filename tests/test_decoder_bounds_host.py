"""The bounds of tests/float64_bounds.py checked without a GPU: numpy restatements of aoc_groupnorm_relu and aoc_prehead that follow the
kernels' order of operations with np.float32 arithmetic step by step (float64 where the kernels use double) must lie inside the bound, and
every slip the GPU tests use (test_gpu_decoder_kernels.py) must lie outside it.  The float64 folds of the kernels (lanes, waves, chunks)
are plain float64 sums here: their order changes the result by parts in 2^53, which the bounds do not count.  fmaf is restated as the
float32 rounding of the float64 sum of the exact product and the addend: the same value except for double roundings at exact ties."""
import numpy as np
import pytest
import torch

from float64_bounds import (_check_bound, eps32, gct_gate_ref, gn_inputs, gn_slips, groupnorm_ref, groupnorm_slip, ph_inputs, ph_slips, prehead_ref, prehead_slip,
                            t64)

f32 = np.float32


def gn_emulate(x, groups, w, b, eps, res, relu):
    N, C, hw = x.shape
    gc = C // groups
    n = gc * hw
    xg = x.reshape(N * groups, n)
    stats = np.zeros((N * groups, 2), f32)
    t = np.arange(256)
    for g in range(N * groups):
        s = np.zeros(256, np.float64)
        q = np.zeros(256, np.float64)
        i = t.copy()
        while True:
            full = i + 7 * 256 < n
            if not full.any():
                break
            ii = i[full]
            ps = np.zeros(ii.size, f32)
            pq = np.zeros(ii.size, f32)
            for u in range(8):
                v = xg[g, ii + u * 256]
                ps = ps + v
                pq = pq + v * v
            s[full] += ps
            q[full] += pq
            i = np.where(full, i + 8 * 256, i)
        live = i < n
        while live.any():
            v = xg[g, i[live]].astype(np.float64)
            s[live] += v
            q[live] += v * v
            i = np.where(live, i + 256, i)
            live = i < n
        mean = s.sum() / n
        var = max(q.sum() / n - mean * mean, 0.0)
        stats[g] = f32(mean), f32(1.0 / np.sqrt(var + np.float64(f32(eps))))
    mean = np.repeat(stats[:, 0].reshape(N, groups), gc, 1)[:, :, None]
    rstd = np.repeat(stats[:, 1].reshape(N, groups), gc, 1)[:, :, None]
    a = rstd * (w[None, :, None] if w is not None else f32(1))
    bb = (b[None, :, None] if b is not None else f32(0)) - mean * a
    v = x * a + bb
    if res is not None:
        v = v + res
    assert v.dtype == f32
    return np.maximum(v, f32(0)) if relu else v


GN_HOST_CASES = [(3, 64, 32, 391), (1, 4, 4, 1), (2, 6, 3, 2047), (2, 6, 3, 2048), (2, 6, 3, 2049), (2, 12, 1, 1025), (5, 8, 2, 7),
                 (1, 16, 2, 1291)]


@pytest.mark.parametrize("offset", [0.0, 3.0])
@pytest.mark.parametrize("N,C,groups,hw", GN_HOST_CASES)
def test_groupnorm_bound_holds_the_emulation_and_sheds_the_slips(N, C, groups, hw, offset):
    rng = np.random.RandomState(N * 1000 + C + hw)
    for affine, residual, relu in ((True, True, True), (False, True, True), (True, False, False)):
        x, w, b, res = gn_inputs(rng, N, C, groups, hw, offset, affine, residual)
        got = gn_emulate(x, groups, w, b, 1e-5, res, relu)
        args = (t64(x), groups, t64(w), t64(b), 1e-5, t64(res), relu)
        want, tol = groupnorm_ref(*args)
        for kind in gn_slips(N, C, groups, hw, offset):
            _check_bound(torch.from_numpy(got), want, tol, groupnorm_slip(kind, *args), f"groupnorm emulation {N}x{C}x{hw} G={groups} "
                         f"offset={offset} affine={affine} residual={residual} slip={kind}")


def test_groupnorm_bound_is_of_the_size_of_float32():
    """Zero-mean unit-variance data: the bound is a few float32 roundings of the output, not a fitted 1e-5."""
    rng = np.random.RandomState(0)
    x, w, b, res = gn_inputs(rng, 2, 6, 3, 2049, 0.0)
    _, tol = groupnorm_ref(t64(x), 3, t64(w), t64(b), 1e-5, t64(res), True)
    assert float(tol.max()) < 1e-5


def ph_emulate(feat, w, b, n_groups, gw, gb, eps):
    O, n_in, hw = feat.shape
    n_out = w.shape[0]
    gs = n_out // n_groups
    y = np.broadcast_to(b[None, :, None], (O, n_out, hw)).astype(f32)
    for k in range(n_in):
        y = (w[None, :, k, None].astype(np.float64) * feat[:, None, k, :].astype(np.float64) + y.astype(np.float64)).astype(f32)
    yg = y.reshape(O, n_groups, gs, hw)
    s1 = np.zeros((O, n_groups, hw), f32)
    s2 = np.zeros((O, n_groups, hw), f32)
    for c in range(gs):
        s1 = s1 + yg[:, :, c]
        s2 = s2 + yg[:, :, c] * yg[:, :, c]
    cnt = float(gs) * float(hw)
    mean = s1.astype(np.float64).sum(2) / cnt
    var = np.maximum(s2.astype(np.float64).sum(2) / cnt - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + np.float64(f32(eps)))).astype(f32)
    mean = mean.astype(f32)
    m_c, r_c = np.repeat(mean, gs, 1)[:, :, None], np.repeat(rstd, gs, 1)[:, :, None]
    v = (y - m_c) * r_c * gw[None, :, None] + gb[None, :, None]
    assert v.dtype == f32
    return np.maximum(v, f32(0))


PH_HOST_CASES = [(1, 24, 64, 16, 391), (3, 26, 64, 16, 257), (1, 28, 64, 16, 255), (3, 1, 128, 64, 1), (1, 7, 128, 128, 257),
                 (3, 32, 128, 128, 1), (1, 24, 128, 64, 256)]


@pytest.mark.parametrize("n_obj,n_in,n_out,n_groups,hw", PH_HOST_CASES)
def test_prehead_bound_holds_the_emulation_and_sheds_the_slips(n_obj, n_in, n_out, n_groups, hw):
    rng = np.random.RandomState(n_in * 100 + n_groups + hw)
    feat, w, b, gw, gb = ph_inputs(rng, n_obj, n_in, n_out, hw)
    got = ph_emulate(feat, w, b, n_groups, gw, gb, 1e-5)
    args = (t64(feat), t64(w), t64(b), n_groups, t64(gw), t64(gb), 1e-5)
    want, tol = prehead_ref(*args)
    kinds = ph_slips(n_in, n_out, n_groups, hw)
    assert kinds
    for kind in kinds:
        _check_bound(torch.from_numpy(got), want, tol, prehead_slip(kind, *args), f"prehead emulation O={n_obj} {n_in}->{n_out} G={n_groups} "
                     f"hw={hw} slip={kind}")


@pytest.mark.parametrize("mode,after_relu", [("l2", False), ("l1", False), ("l1", True)])
def test_gct_gate_ref_is_gct_forward(mode, after_relu):
    """The reference of gct_gate_ref (the gate from the plane sums) is the gate of oracle.calibration.gct_forward, both in float64."""
    from oracle import calibration as ocal
    rng = np.random.RandomState(len(mode) + after_relu)
    N, C, hw = 2, 300, 57
    x = torch.from_numpy(rng.standard_normal((N, C, hw)))
    if after_relu:
        x = x.clamp_min(0.125)
    alpha, gam, beta = (torch.from_numpy(rng.standard_normal(C)) for _ in range(3))
    v = lambda a: a.view(1, C, 1, 1)
    gate = ocal.gct_forward(x.view(N, C, hw, 1), v(alpha), v(gam), v(beta), eps32(1e-5), mode, after_relu).view(N, C, hw) / x
    sums = (x * x).sum(2) if mode == "l2" else x.abs().sum(2)
    ref, _ = gct_gate_ref(sums, alpha, gam, beta, 1e-5, mode == "l1")
    assert float((gate - ref.unsqueeze(2)).abs().max()) < 64 * 2.0 ** -53 * 2       # a handful of float64 roundings of a value below 2
