"""float64 references and float32 bounds shared by test_aspp_host.py and test_gpu_aspp.py (conventions of float64_bounds.py: U, gamma, tanhf
within 4 U with the addition of 1).  No constant here is fitted to output.

Plane statistics (aoc_plane_sum_sumsq; also torch's own CPU reductions, whatever their order):
    a sum of hw terms in any order          gamma(hw) sum |x|        (hw - 1 additions on the way of any term)
    the sum of squares                      gamma(hw + 1) sum x^2    (one more rounding for the square)
    the mean                                the plane-sum bound / hw, plus U of the quotient (the division rounds once)

A GCT whose plane sums are themselves off (gct_stage_ref): with s^ = s + ds, r_c = ds_c / (s_c + eps) is the relative change of s_c + eps and
of e_c^2 = (s_c + eps) alpha_c^2; the mean m of e_c^2 moves by at most mean(r_c e_c^2), m + eps by the relative r_m = that / (m + eps),
1 / sqrt(m + eps) by at most (1 - r_m)^-1/2 - 1 = r_n, and the argument of tanh, e_c norm_c + beta_c, by |e_c norm_c| (sqrt(1 + r_c) (1 + r_n) - 1)
-- evaluated, not linearised.  tanh' <= 1.  On top comes float64_bounds.gct_gate_ref's bound for the float32 evaluation, which is taken at the
exact sums: every magnitude it is built from (|e|, m, |norm|, |e norm|) moves by at most the relative change rho = max_c of the factor above,
products of two of them by (1 + rho)^2 - 1 <= 3 rho, so the bound is scaled by 1 + 4 rho."""
import torch
import torch.nn.functional as F

from float64_bounds import U, _gn_stats, _per_channel, _prod_err, _rstd_err, eps32, gamma, gct_gate_ref, groupnorm_ref, groupnorm_slip


# ------------------------------------------------------------------------------------------ plane statistics
def plane_stats_ref(x):
    """x [P, hw] float64 -> {name: (want, tol)} for sum, sumsq, mean."""
    hw = x.shape[1]
    s, a = x.sum(1), x.abs().sum(1)
    q = (x * x).sum(1)
    ds = gamma(hw) * a
    return {"sum": (s, ds), "sumsq": (q, gamma(hw + 1) * q), "mean": (s / hw, ds / hw + U * (s.abs() + ds) / hw)}


def plane_stats_slip(x):
    """The three references with the last quarter of every plane (at least one element) left out: what a reduction that combines three of
    its four waves, or stops a trip early, would give.  The any-order bound of a long plane's sum is wide (gamma(hw) sum |x| grows like
    hw^2 U); a few dropped elements would stay inside it."""
    hw = x.shape[1]
    k = x[:, :hw - max(1, hw // 4)]
    return {"sum": k.sum(1), "sumsq": (k * k).sum(1), "mean": k.sum(1) / hw}


# ------------------------------------------------------------------------------------------ GCT with its statistics and its product
def gct_stage_ref(y, dy, alpha, gam, beta, eps, sums_exact_to=None):
    """GCT (l2) of y [N, C, hw] that is itself known to dy (a tensor or 0.0): -> (gated want, tol, gate want, gate tol).
    The plane sums of squares are off by what dy does to them, sum(2 |y| dy + dy^2), and by their own float32 summation in any order,
    gamma(hw + 1) sum (|y| + dy)^2 (sums_exact_to: use this ds instead, e.g. zeros when the sums are given).  alpha, gam, beta [C]."""
    eps = eps32(eps)
    N, C, hw = y.shape
    dy = torch.as_tensor(dy, dtype=torch.float64).expand_as(y)
    s = (y * y).sum(2)
    ds = (2 * y.abs() * dy + dy * dy).sum(2) + gamma(hw + 1) * ((y.abs() + dy) ** 2).sum(2) if sums_exact_to is None else sums_exact_to
    gate, tol32 = gct_gate_ref(s, alpha.view(1, C), gam.view(1, C), beta.view(1, C), eps, False)
    e2 = (s + eps) * alpha.view(1, C) ** 2
    m = e2.mean(1, keepdim=True)
    r_c = ds / (s + eps)
    r_m = (r_c * e2).mean(1, keepdim=True) / (m + eps)
    assert float(r_m.max()) < 0.5, "the perturbation analysis needs a small relative change of the mean"
    r_n = (1.0 - r_m) ** -0.5 - 1.0
    factor = torch.sqrt(1.0 + r_c) * (1.0 + r_n) - 1.0
    en = (torch.sqrt(e2) * gam.view(1, C).abs() / torch.sqrt(m + eps))
    dgate = en * factor + tol32 * (1.0 + 4.0 * float(factor.max()))
    want = gate.unsqueeze(2) * y
    spread = _prod_err(gate.abs().unsqueeze(2), dgate.unsqueeze(2), y.abs(), dy)
    return want, spread + U * (want.abs() + spread), gate, dgate


def scale_ref(x, gain):
    """aoc_channel_scale(_multi) from given gains: one rounding."""
    want = gain.unsqueeze(2) * x
    return want, U * want.abs()


# ------------------------------------------------------------------------------------------ GroupNorm + ReLU into the concatenation
def _f32_stats_slack(x, groups, weight, eps):
    """What a GroupNorm whose group statistics are float32 sums of all n = C / groups x hw terms in any order (torch's CPU kernel, not
    gn_stats_kernel, whose partial sums of more than 8 terms are float64) adds to groupnorm_ref's bound: the mean off by
    dm = gamma(n) E|x|, the variance by gamma(n + 1) E[x^2] + 2 |m| dm + dm^2, rstd through _rstd_err; the output moves by
    |g| (r dm + |x - m| dr + dm dr).  It applies ONLY where the value under test is a recording of torch's CPU GroupNorm (the fixtures in
    test_aspp_host.py, and the recording's side of test_merge_golden); aoc_groupnorm_cat_relu itself is held to groupnorm_ref's bound alone."""
    eps = eps32(eps)
    N, C, hw = x.shape
    xg = x.reshape(N, groups, -1)
    n = xg.shape[2]
    m, var = _gn_stats(x, groups)
    dm = gamma(n) * xg.abs().mean(2)
    dvar = gamma(n + 1) * (xg * xg).mean(2) + 2 * m.abs() * dm + dm * dm
    r, dr = _rstd_err(var, dvar, eps)
    m_c, dm_c, r_c, dr_c = (_per_channel(t, C) for t in (m, dm, r, dr))
    g = weight.abs().view(1, C, 1) if weight is not None else 1.0
    return g * (r_c * dm_c + (x - m_c).abs() * dr_c + dm_c * dr_c)


def cat_ref(xs, groups, weights, biases, eps, tail, relu=True, order=None, slip=None, f32_stats=False):
    """aoc_groupnorm_cat_relu: xs: n_src tensors [N, C_src, hw]; weights, biases: lists of [C_src] or None; tail [N, C_tail] or None ->
    (want [N, C_total, hw], tol): float64_bounds.groupnorm_ref per source, the tail exact.  order: a permutation of the parts (the tail is
    part n_src) for a slipped concatenation; slip: a groupnorm_slip kind for every source, or 'tail_first_pixel' (the tail only at pixel 0);
    f32_stats: the value under test comes from a GroupNorm with float32 statistics (_f32_stats_slack)."""
    N, _, hw = xs[0].shape
    parts, tols = [], []
    for k, x in enumerate(xs):
        w = weights[k] if weights is not None else None
        b = biases[k] if biases is not None else None
        want, tol = groupnorm_ref(x, groups, w, b, eps, None, relu)
        if f32_stats:
            tol = tol + _f32_stats_slack(x, groups, w, eps)
        if slip is not None and slip != "tail_first_pixel":
            want = groupnorm_slip(slip, x, groups, w, b, eps, None, relu)
        parts.append(want)
        tols.append(tol)
    if tail is not None:
        t = (torch.relu(tail) if relu else tail).unsqueeze(2).expand(-1, -1, hw).clone()
        if slip == "tail_first_pixel":
            t[:, :, 1:] = 0.0
        parts.append(t)
        tols.append(torch.zeros_like(t))
    if order is not None:
        parts = [parts[i] for i in order]
    return torch.cat(parts, 1), torch.cat(tols, 1)


def plane_sumsq_of(y):
    """plane_sumsq of aoc_groupnorm_cat_relu against the float32 y it returned: [N, C, hw] -> (want, tol) [N, C]."""
    q = (y * y).sum(2)
    return q, gamma(y.shape[2] + 1) * q


# ------------------------------------------------------------------------------------------ the module in plain torch
BRANCHES = ("aspp1", "aspp2", "aspp3", "aspp4")
DILATIONS = (1, 6, 12, 18)


def _gct_torch(x, sd, prefix, eps=1e-5):
    a, g, b = sd[prefix + "alpha"], sd[prefix + "gamma"], sd[prefix + "beta"]
    embedding = (x.pow(2).sum((2, 3), keepdim=True) + eps).pow(0.5) * a
    norm = g / (embedding.pow(2).mean(dim=1, keepdim=True) + eps).pow(0.5)
    return x * (1. + torch.tanh(embedding * norm + b))


def aspp_torch(x, state_dict, dtype):
    """A plain-torch restatement of aspp.py:56-70 with functional convolutions, on the CPU in `dtype`, from a reference-style state_dict."""
    sd = {k: v.detach().cpu().to(dtype) for k, v in state_dict.items()}
    x = x.detach().cpu().to(dtype)
    outs = []
    for name, d in zip(BRANCHES, DILATIONS):
        w = sd[name + ".atrous_conv.weight"]
        y = _gct_torch(x, sd, name + ".GCT.")
        y = F.conv2d(y, w, None, 1, 0 if w.shape[2] == 1 else d, d)
        y = F.group_norm(y, w.shape[0] // 4, sd[name + ".bn.weight"], sd[name + ".bn.bias"], 1e-5)
        outs.append(torch.relu(y))
    x5 = torch.relu(F.conv2d(F.adaptive_avg_pool2d(x, (1, 1)), sd["global_avg_pool.1.weight"]))
    x5 = F.interpolate(x5, size=outs[0].shape[2:], mode='bilinear', align_corners=True)
    y = torch.cat(outs + [x5], dim=1)
    y = _gct_torch(y, sd, "GCT.")
    y = F.conv2d(y, sd["conv1.weight"])
    return torch.relu(F.group_norm(y, 32, sd["bn1.weight"], sd["bn1.bias"], 1e-5))
