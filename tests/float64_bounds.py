"""Shared pieces of the float64-reference tests (test_gpu_stream_kernels.py, test_gpu_decoder_kernels.py, test_decoder_bounds_host.py).

U = 2^-24 is the unit roundoff of float32; gamma(n) = n U / (1 - n U) bounds the relative error of a value that went through n roundings,
and of a sum whose every term went through at most n additions.  _check_bound compares a kernel's result with a float64 reference under
an elementwise bound and demands that a deliberately slipped reference leaves that bound.

The second half holds, for every decoder-side kernel of calibration.hip (the ones that run after the proto-mask tensor is built), a pure
function of the float32 inputs widened to float64 that returns (want, tol): the float64 result and the bound on |kernel - want| that follows
from the kernel's float32 expressions.  The library is built with -ffp-contract=off, so every product and every sum rounds once; sqrtf and
the float division are the correctly rounded ones (one rounding); only the pre-head's 1x1 convolution uses explicit fmaf (one rounding per
step).  tanhf follows the convention of test_film_gain: within 2 ulp plus the final addition, 4 U.  No constant here is fitted to output.
The *_slip functions are the same references with one deliberate mistake; the tests demand that each leaves the bound."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def _check_bound(got, want, tol, slip, what):
    """got within tol of the float64 reference `want`; the slipped reference must leave the bound somewhere."""
    got, want, slip = (torch.as_tensor(v).double() for v in (got, want, slip))
    tol = torch.as_tensor(tol, dtype=torch.float64)
    err = (got - want).abs()
    bad = ~(err <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the bound, worst excess {float((err - tol).max()):.3e}"
    assert ((slip - want).abs() > tol).any(), f"{what}: the slipped reference stays inside the bound (bound too loose)"


def eps32(eps):
    """The kernels take eps as a float argument: the reference uses the value they get."""
    return float(np.float32(eps))


def _cdiv(a, b):
    return -(-a // b)


def _prod_err(a, da, b, db):
    """|a^ b^ - a b| for |a^ - a| <= da, |b^ - b| <= db (a, b magnitudes)."""
    return a * db + b * da + da * db


def _rstd_err(var, dvar, eps):
    """rstd = 1 / sqrt(var + eps) of a variance known to dvar (the kernel clamps its variance at 0, the true one is >= 0): the larger of the
    two one-sided changes, evaluated, not linearised; then its rounding to float32."""
    r = 1.0 / torch.sqrt(var + eps)
    hi = 1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + eps)
    lo = 1.0 / torch.sqrt(var + dvar + eps)
    dr = torch.maximum(hi - r, r - lo)
    return r, dr + U * (r + dr)


# ------------------------------------------------------------------------------------------ GroupNorm (+ residual) (+ ReLU)
def _gn_stats(x, groups):
    N, C, hw = x.shape
    xg = x.reshape(N, groups, -1)
    return xg.mean(2), xg.var(2, unbiased=False)


def _gn_finish(x, mean_c, r_c, weight, bias, residual, relu):
    C = x.shape[1]
    g = weight.view(1, C, 1) if weight is not None else 1.0
    b = bias.view(1, C, 1) if bias is not None else 0.0
    v = (x - mean_c) * r_c * g + b
    if residual is not None:
        v = v + residual
    return torch.relu(v) if relu else v


def _per_channel(t, C):
    """[N, groups] -> [N, C, 1]"""
    return t.repeat_interleave(C // t.shape[1], dim=1).unsqueeze(2)


def groupnorm_ref(x, groups, weight, bias, eps, residual=None, relu=True):
    """aoc_groupnorm_relu.  x, residual [N, C, hw]; weight, bias [C] or None.

    gn_stats_kernel: a thread sums blocks of 8 values in float32 (8 additions; the squares one rounding each and 8 additions); everything
    after that (the per-thread totals, the lane, wave and final sums, mean, E[x^2] - mean^2, 1 / sqrt(var + eps)) is float64, whose own
    roundings (2^-53) are not counted.  So the mean is off by at most dm = gamma(8) E|x| and the variance by
        dvar = gamma(9) E[x^2] + 2 |m| dm + dm^2;
    mean and rstd are rounded to float32 once each, rstd's error is carried through 1 / sqrt(var -+ dvar + eps) (_rstd_err).
    gn_apply_kernel: a = fl(rstd g), b = fl(beta - fl(mean a)), v = fl(fl(x a) + b), then fl(v + residual): one rounding per operation, each
    bounded by U times the magnitude of its (perturbed) result.  ReLU is 1-Lipschitz: the bound passes through it."""
    eps = eps32(eps)
    N, C, hw = x.shape
    xg = x.reshape(N, groups, -1)
    n = xg.shape[2]
    m, var = _gn_stats(x, groups)
    # element i = t + 256 u + 2048 j belongs to thread t's j-th block of 8, which is summed in float32 only while t + 2048 j + 7 * 256 < n;
    # what is left goes through the tail loop, whose sums and squares are float64: the E|x| and E[x^2] of the docstring run over the float32
    # part only (a group of fewer than 2048 elements has exact statistics)
    i = torch.arange(n)
    f32 = ((i % 256 + 2048 * (i // 2048) + 7 * 256) < n).double()
    dm0 = gamma(8) * (xg.abs() * f32).mean(2)
    dvar = gamma(9) * (xg * xg * f32).mean(2) + 2 * m.abs() * dm0 + dm0 * dm0
    r, dr = _rstd_err(var, dvar, eps)
    dm = dm0 + U * (m.abs() + dm0)
    m_c, dm_c, r_c, dr_c = (_per_channel(t, C) for t in (m, dm, r, dr))
    g = weight.abs().view(1, C, 1) if weight is not None else torch.ones(1, C, 1, dtype=torch.float64)
    be = bias.abs().view(1, C, 1) if bias is not None else torch.zeros(1, C, 1, dtype=torch.float64)
    a = r_c * g
    da = g * dr_c + U * (a + g * dr_c)
    e_ma = _prod_err(m_c.abs(), dm_c, a, da)
    ma = m_c.abs() * a + e_ma                                  # bound on |mean^ a^|
    db = e_ma + U * ma + U * (be + ma * (1 + U))
    want_b = (bias.view(1, C, 1) if bias is not None else 0.0) - m_c * r_c * (weight.view(1, C, 1) if weight is not None else 1.0)
    xa = x.abs() * (a + da)                                    # bound on |x a^|
    dv = x.abs() * da + U * xa + db + U * (xa * (1 + U) + want_b.abs() + db)
    want_v = _gn_finish(x, m_c, r_c, weight, bias, None, False)
    if residual is not None:
        want_v = want_v + residual
        dv = dv + U * (want_v.abs() + dv)
    return (torch.relu(want_v) if relu else want_v), dv


def groupnorm_slip(kind, x, groups, weight, bias, eps, residual=None, relu=True):
    """The reference with wrong statistics:
    unbiased     the variance divided by n - 1;
    per_channel  mean and variance of each channel instead of each group;
    tail         the last n mod 2048 elements of the group (what the 8 x 256 loop of gn_stats_kernel leaves to its tail loop) left out of the
                 statistics; where that is nothing or the whole group, the group's last channel is left out instead;
    next_group   the statistics of the next group of the sample (for groups of one element, whose output does not depend on the variance
                 and whose unbiased variance does not exist)."""
    eps = eps32(eps)
    N, C, hw = x.shape
    gc = C // groups
    n = gc * hw
    xg = x.reshape(N, groups, n)
    if kind == "unbiased":
        m, var = xg.mean(2), xg.var(2, unbiased=True)
    elif kind == "per_channel":
        m_c, var_c = x.mean(2, keepdim=True), x.var(2, unbiased=False, keepdim=True)
        return _gn_finish(x, m_c, 1.0 / torch.sqrt(var_c + eps), weight, bias, residual, relu)
    elif kind == "tail":
        keep = n - n % 2048
        if keep == n or keep == 0:
            keep = (gc - 1) * hw
        m, var = xg[:, :, :keep].mean(2), xg[:, :, :keep].var(2, unbiased=False)
    elif kind == "next_group":
        m, var = (t.roll(-1, dims=1) for t in _gn_stats(x, groups))
    else:
        raise ValueError(kind)
    return _gn_finish(x, _per_channel(m, C), _per_channel(1.0 / torch.sqrt(var + eps), C), weight, bias, residual, relu)


# ------------------------------------------------------------------------------------------ pre-head
def _prehead_conv(feat, w, b):
    return torch.einsum("ck,okp->ocp", w, feat) + b.view(1, -1, 1)


def _prehead_finish(y, m, r, n_groups, gn_w, gn_b):
    n_out = y.shape[1]
    v = (y - _per_channel(m, n_out)) * _per_channel(r, n_out) * gn_w.view(1, -1, 1) + gn_b.view(1, -1, 1)
    return torch.relu(v)


def prehead_ref(feat, w, b, n_groups, gn_w, gn_b, eps):
    """aoc_prehead without the embedding channels (those are copies).  feat [O, n_in, hw], w [n_out, n_in]; want is
    oracle.calibration.dynamic_prehead on the float64 tensors.

    y = b + sum_k w_k x_k is an fmaf chain of n_in steps: dy = gamma(n_in) (|b| + sum |w x|).
    prehead_stats_kernel: a thread adds the group_size values of y^ and of fl(y^ y^) of its pixel in float32 (group_size additions; the
    squares one rounding more); lanes, waves, chunks, mean, variance and rstd are float64 (not counted).  With E[] the mean over the group:
        dm   = E[dy] + gamma(gs) E[|y| + dy]
        dq   = E[2 |y| dy + dy^2] + gamma(gs + 1) E[(|y| + dy)^2]
        dvar = dq + 2 |m| dm + dm^2,
    rstd through _rstd_err, mean and rstd rounded to float32 once.
    prehead_apply_kernel: fl(fl(fl(fl(y^ - mean^) rstd^) g) + beta), one rounding per operation; ReLU passes the bound through."""
    from oracle import calibration as ocal
    eps = eps32(eps)
    O, n_in, hw = feat.shape
    n_out = w.shape[0]
    gs = n_out // n_groups
    want = ocal.dynamic_prehead(feat.unsqueeze(2), w, b, gn_w, gn_b, n_groups, eps).squeeze(2)
    y = _prehead_conv(feat, w, b)
    dy = gamma(n_in) * (torch.einsum("ck,okp->ocp", w.abs(), feat.abs()) + b.abs().view(1, -1, 1))
    E = lambda t: t.reshape(O, n_groups, -1).mean(2)
    ya = y.abs()
    m = E(y)
    var = (E(y * y) - m * m).clamp_min(0.0)
    dm0 = E(dy) + gamma(gs) * E(ya + dy)
    dq = E(2 * ya * dy + dy * dy) + gamma(gs + 1) * E((ya + dy) ** 2)
    dvar = dq + 2 * m.abs() * dm0 + dm0 * dm0
    r, dr = _rstd_err(var, dvar, eps)
    dm = dm0 + U * (m.abs() + dm0)
    m_c, dm_c, r_c, dr_c = (_per_channel(t, n_out) for t in (m, dm, r, dr))
    t1 = (y - m_c).abs()
    d1 = dy + dm_c
    d1 = d1 + U * (t1 + d1)
    t2 = t1 * r_c
    d2 = _prod_err(t1, d1, r_c, dr_c)
    d2 = d2 + U * (t2 + d2)
    g = gn_w.abs().view(1, -1, 1)
    t3 = t2 * g
    d3 = d2 * g
    d3 = d3 + U * (t3 + d3)
    t4 = ((y - m_c) * r_c * gn_w.view(1, -1, 1) + gn_b.view(1, -1, 1)).abs()
    tol = d3 + U * (t4 + d3)
    return want, tol


def prehead_slip(kind, feat, w, b, n_groups, gn_w, gn_b, eps):
    """drop_in      the last input channel dropped from the convolution;
    first_chunk  group statistics over the first chunk of 256 pixels (the first workgroup's partial) only;
    group_wrap   groups 32 and above use the statistics of group g - 32 (the slots of the first trip of the group loop)."""
    eps = eps32(eps)
    if kind == "drop_in":
        feat, w = feat[:, :-1], w[:, :-1]
    y = _prehead_conv(feat, w, b)
    O, n_out, hw = y.shape
    ys = y[:, :, :256] if kind == "first_chunk" else y
    yg = ys.reshape(O, n_groups, -1)
    m, var = yg.mean(2), yg.var(2, unbiased=False)
    if kind == "group_wrap":
        idx = torch.arange(n_groups)
        idx = torch.where(idx >= 32, idx - 32, idx)
        m, var = m[:, idx], var[:, idx]
    return _prehead_finish(y, m, 1.0 / torch.sqrt(var + eps), n_groups, gn_w, gn_b)


# ------------------------------------------------------------------------------------------ plane_reduce, gct_gate
def _plane_f(x, mode):
    return x * x if mode == 1 else (x.abs() if mode == 2 else x)


def plane_reduce_ref(x, mode):
    """aoc_plane_reduce.  x [N, C, hw]: a thread adds ceil(hw / 256) terms (the squares of mode 1 one rounding more), then 6 wave-sum
    levels and the two levels of (w0 + w1) + (w2 + w3)."""
    hw = x.shape[2]
    f = _plane_f(x, mode)
    depth = _cdiv(hw, 256) + 6 + 2 + (1 if mode == 1 else 0)
    return f.sum(2), gamma(depth) * f.abs().sum(2)


def plane_reduce_slip(kind, x, mode):
    """as_mode0   the plain sum (what mode 2 gives without its fabsf);
    tail       the elements after the last full 2048 (the kernel's tail loop) dropped; where hw is a multiple of 2048 there is no tail
               and the last of the eight unrolled loads, the last 256 elements, is dropped instead."""
    hw = x.shape[2]
    if kind == "as_mode0":
        return x.sum(2)
    keep = hw - hw % 2048 if hw % 2048 else hw - 256
    return _plane_f(x[:, :, :keep], mode).sum(2)


def gct_gate_ref(s, alpha, gam, beta, eps, l1, mean_slip=None):
    """aoc_gct_gate from the plane sums s [N, C] (gct.py:17-36; the lines of oracle.calibration.gct_forward after its plane sums).

    l2: e = fl(sqrtf(fl(s + eps)) alpha): three roundings, the first under the square root: de = gamma(3) |e|; fl(e e) is within gamma(7)
    of e^2.  l1: e = fl(s alpha): de = U |e|, |e| exact.  The mean over the channels adds ceil(C / 256) additions per thread, 6 wave-sum
    levels, 2 cross-wave levels and the division: k = ceil(C / 256) + 9, dm = gamma(7 + k) m (l2) or gamma(1 + k) m (l1).
    The denominator D = fl(m + eps) is off by dD = dm + U (D + dm); norm = gam / sqrt(D) (l2, two roundings) or gam / D (l1, one) is
    evaluated at D - dD, the side on which it moves more, not linearised.  Then fl(fl(e norm) + beta), and tanh' <= 1; tanhf: 4 U."""
    eps = eps32(eps)
    N, C = s.shape
    k = _cdiv(C, 256) + 9
    if l1:
        e = s * alpha
        de = U * e.abs()
        t = e.abs()
        nm = 1 + k
    else:
        e = torch.sqrt(s + eps) * alpha
        de = gamma(3) * e.abs()
        t = e * e
        nm = 7 + k
    if mean_slip == "first256":
        m = t[:, :256].sum(1, keepdim=True) / C
    elif mean_slip == "drop_last":
        m = t[:, :-1].sum(1, keepdim=True) / C
    else:
        m = t.mean(1, keepdim=True)
    D = m + eps
    dD = gamma(nm) * m
    dD = dD + U * (D + dD)
    if l1:
        norm, lo, nr = gam / D, gam.abs() / (D - dD), 1
    else:
        norm, lo, nr = gam / torch.sqrt(D), gam.abs() / torch.sqrt(D - dD), 2
    dn = lo - norm.abs()
    dn = dn + gamma(nr) * (norm.abs() + dn)
    prod = e * norm
    dp = _prod_err(e.abs(), de, norm.abs(), dn)
    dp = dp + U * (prod.abs() + dp)
    arg = prod + beta
    darg = dp + U * (arg.abs() + dp)
    return 1.0 + torch.tanh(arg), darg + 4 * U


# ------------------------------------------------------------------------------------------ object_logit
def object_logit_ref(x, w, b):
    """aoc_object_logit.  x [N, C, hw], w [N, C], b [N]; want is oracle.calibration.ia_logit with a head that hands the rows of [w | b]
    through unchanged (identity head, the rows as the Linear's weight, zero bias: exact in float64).  One rounding per product, C
    sequential additions and the bias share the budget of C + 1 additions: gamma(C + 1) (sum |w x| + |b|)."""
    from oracle import calibration as ocal
    N, C, hw = x.shape
    wb = torch.cat([w, b.view(N, 1)], 1)
    want = ocal.ia_logit(x.view(N, C, 1, hw), torch.eye(N, dtype=torch.float64), wb.t().contiguous(), torch.zeros(C + 1, dtype=torch.float64))
    tol = gamma(C + 1) * (torch.einsum("nc,ncp->np", w.abs(), x.abs()) + b.abs().view(N, 1))
    return want.view(N, hw), tol


def object_logit_slip(kind, x, w, b):
    """tail_channels  the channels after the last multiple of 8 dropped;  prev_object  object n read with object n - 1's weights and bias."""
    N, C, hw = x.shape
    if kind == "tail_channels":
        c = C - C % 8
        return torch.einsum("nc,ncp->np", w[:, :c], x[:, :c]) + b.view(N, 1)
    return torch.einsum("nc,ncp->np", w.roll(1, 0), x) + b.roll(1, 0).view(N, 1)


# ------------------------------------------------------------------------------------------ cond_codes, head_delta, plane_mean
def _wave_dot_tol(xa, dx, wa, ba, dim):
    """One wave per output: ceil(dim / 64) products and additions per lane, 6 wave-sum levels and the bias: ceil(dim / 64) + 8 roundings
    on the way of any term; dx is what the inputs of the dot product are already off by."""
    return dx @ wa.t() + gamma(_cdiv(dim, 64) + 8) * ((xa + dx) @ wa.t() + ba)


def cond_codes_ref(gap, px, head, w1, b1, w2, b2, w3, b3, slip=None):
    """aoc_cond_codes: the three F.linear calls and the sum(0) - px of oracle.calibration.conditioning_block (w1, w2 [C, C], w3 [D, D]).  The
    middle block's input
    tot - px[n] is N sequential additions and a subtraction: gamma(N + 1) (sum_m |px[m]| + |px[n]|).
    slip: 'no_minus' the middle block without - px[n]; 'drop_head' the last head dimension dropped."""
    N, C = gap.shape
    D = head.shape[1]
    delta = px.sum(0, keepdim=True).expand_as(px) - (0.0 if slip == "no_minus" else px)
    if slip == "drop_head":
        head, w3 = head[:, :-1], w3[:, :-1]
    want = torch.cat([F.linear(gap, w1, b1), F.linear(delta, w2, b2), F.linear(head, w3, b3)], 1)
    dd = gamma(N + 1) * (px.abs().sum(0, keepdim=True) + px.abs())
    z = torch.zeros_like
    tol = torch.cat([_wave_dot_tol(gap.abs(), z(gap), w1.abs(), b1.abs(), C), _wave_dot_tol(delta.abs(), dd, w2.abs(), b2.abs(), C),
                     _wave_dot_tol(head.abs(), z(head), w3.abs(), b3.abs(), D)], 1)
    return want, tol


def head_delta_ref(px, slip=False):
    """The delta half of aoc_head_delta: n_obj sequential additions (the first to 0 is exact) and the subtraction: gamma(n_obj) sum |px|.
    slip: without - px[o]."""
    n_obj = px.shape[0]
    want = px.sum(0, keepdim=True) - (0.0 if slip else px)
    return want.expand_as(px), (gamma(n_obj) * px.abs().sum(0, keepdim=True)).expand_as(px)


def plane_mean_ref(x):
    """aoc_plane_mean (plane_mean4_kernel).  x [P, hw]: 4 additions per float4 (three inside it, one into the accumulator), at most
    ceil(ceil(hw / 4) / 256) float4 per thread, the scalar head and tail additions before them (2), 6 wave-sum levels, 3 cross-wave
    additions and the division."""
    hw = x.shape[1]
    depth = 4 + _cdiv(_cdiv(hw, 4), 256) + 2 + 6 + 3 + 1
    return x.mean(1), gamma(depth) * x.abs().mean(1)


def plane_mean_slip(x, base_phase=0):
    """The scalar tail dropped: plane i starts (base_phase + i hw) mod 4 floats into a 16-byte line, its head is the floats up to the next
    line and its tail what is left after the float4 body; a plane whose tail is empty loses its last float4 instead."""
    P, hw = x.shape
    out = torch.empty(P, dtype=torch.float64)
    for i in range(P):
        head = min((4 - (base_phase + i * hw) % 4) % 4, hw)
        tail = (hw - head) % 4
        keep = hw - tail if tail else max(hw - 4, 0)
        out[i] = x[i, :keep].sum() / hw
    return out


# ------------------------------------------------------------------------------------------ cond_gate_pool
def cond_scores_ref(z, phi_w, phi_b, k_rank, skip_chunk=None):
    """The scores, threshold, mask and gap of oracle.calibration.conditioning_gate_stats for the k_rank-th largest score.  z [N, C, hw].
    Within a 32-channel chunk the scores are summed channel by channel, then the chunks in order, then + b: a term goes through at most
    C + n_chunks + 1 roundings with its product: gamma(C + n_chunks + 1) (sum |w z| + |b|).   skip_chunk: that 32-channel chunk left out."""
    from oracle import calibration as ocal
    N, C, hw = z.shape
    if skip_chunk is not None:
        phi_w = phi_w.clone()
        phi_w[32 * skip_chunk:32 * skip_chunk + 32] = 0.0
    s, thr, mask, gap = ocal.conditioning_gate_stats(z.view(N, C, 1, hw), phi_w, phi_b, beta_percentage=(k_rank + 0.5) / hw)
    tol = gamma(C + _cdiv(C, 32) + 1) * (torch.einsum("c,ncp->np", phi_w.abs(), z.abs()) + phi_b.abs())
    return s, thr, mask, gap, tol


def cond_gap_ref(z, mask):
    """gap = mean over ALL pixels of z * mask (cond_masked_gap_fused_kernel): ceil(hw / 256) additions per thread, 6 wave-sum levels, 3
    cross-wave additions and the division.  mask [N, hw] bool."""
    hw = z.shape[2]
    zm = z * mask.unsqueeze(1)
    return zm.mean(2), gamma(_cdiv(hw, 256) + 10) * zm.abs().mean(2)


def cond_plane_mean_ref(z, drop_last_tile=False):
    """The fused plane means of aoc_cond_gate_pool_ex: 8 additions per thread in its 2048-pixel tile, 6 wave-sum levels, 2 cross-wave levels,
    the n_tiles sequential additions of the tile partials and the division.  drop_last_tile: the slip."""
    hw = z.shape[2]
    n_tiles = _cdiv(hw, 2048)
    tol = gamma(8 + 6 + 2 + n_tiles + 1) * z.abs().mean(2)
    if drop_last_tile:
        return z[:, :, :2048 * (n_tiles - 1)].sum(2) / hw, tol
    return z.mean(2), tol


# ------------------------------------------------------------------------------------------ inputs and slip choices shared by the host and GPU tests
f32 = np.float32


def gn_inputs(rng, N, C, groups, hw, offset, with_affine=True, with_residual=True):
    """Unit noise + 0.5 x (channel index within the group) [+ offset]; gamma in [0.5, 1.5], beta ~ N(0, 1); residual O(1), mixed sign."""
    gc = C // groups
    x = rng.standard_normal((N, C, hw)) + 0.5 * (np.arange(C) % gc)[None, :, None] + offset
    w = rng.uniform(0.5, 1.5, C).astype(f32) if with_affine else None
    b = rng.standard_normal(C).astype(f32) if with_affine else None
    res = (1.5 * rng.standard_normal((N, C, hw))).astype(f32) if with_residual else None
    return x.astype(f32), w, b, res


def gn_slips(N, C, groups, hw, offset):
    """Which slips a case uses: unbiased variance for zero-offset groups of at most 4096 elements (in the float64 bound the n - 1 slip drowns
    for larger groups and for a mean of several sigma); wrong-scope statistics otherwise; groups of one element take their neighbour's."""
    n = C // groups * hw
    if n == 1:
        return ["next_group"]
    if offset == 0.0 and n <= 4096:
        return ["unbiased"]
    return ["per_channel", "tail"]


def ph_inputs(rng, n_obj, n_in, n_out, hw):
    """Proto-mask-like features in [0, 1], convolution weights ~ N(0, 1) / sqrt(n_in), bias up to +-2 (group means are not zero)."""
    feat = rng.uniform(0, 1, (n_obj, n_in, hw)).astype(f32)
    w = (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(f32)
    b = rng.uniform(-2, 2, n_out).astype(f32)
    gw = rng.uniform(0.5, 1.5, n_out).astype(f32)
    gb = (0.5 * rng.standard_normal(n_out)).astype(f32)
    return feat, w, b, gw, gb


def ph_slips(n_in, n_out, n_groups, hw):
    """drop_in wherever the output depends on the convolution beyond its group mean (one channel per group over one pixel does not);
    first_chunk where there is a second chunk; group_wrap where the group loop takes a second trip."""
    kinds = []
    if hw > 1 or n_out // n_groups > 1:
        kinds.append("drop_in")
    if hw > 256:
        kinds.append("first_chunk")
    if n_groups > 32:
        kinds.append("group_wrap")
    return kinds


def t64(a):
    return None if a is None else torch.from_numpy(np.asarray(a)).double()
