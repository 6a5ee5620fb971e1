"""References and bounds for the training-time ASPP (csrc/aspp_grad.hip, aoc_amd.aspp_train), shared by tests/test_aspp_grad_host.py and
tests/test_gpu_aspp_grad.py.

Every *_ref is a pure function of the tensors an entry point receives, widened to float64; it returns the float64 results and, for each,
an elementwise bound on |kernel - reference|.  The bound is a running error analysis of the kernel's own float32 expressions carried by
``gates_grad_bounds.E`` (a value and what a float32 evaluation of it is off by at most; -ffp-contract=off, so every operation rounds once,
U = 2^-24).  The back stage reads the forward's statistics, plane sums of squares and gate: they are inputs of the entry point and enter the
reference as given, exactly.  The summation depths are the kernels':

    plane sums       gates_grad_bounds.dot_depth(hw): 4 ceil(ceil(hw / 4) / T) + 2 per thread, 6 butterfly levels, T / 64 wave sums
    GCT sums over c  ceil(C / 256) per thread, 6 butterfly levels, 2 cross-wave levels (gates_grad_bounds.gct_gate_grad_ref)
    dsum_total       serial over the sets;   s1, s2   serial over the C_src / groups channels of a group;   grad_gamma, grad_beta   serial over N

No constant is fitted to output.  A = G P2 + 2 ds P4 (and B likewise) is a two-term combination in which the terms may cancel: its bound
comes out of the two products' own bounds, which are built from the absolute plane sums (sum |g|, sum cat ...), never from |A|.

ReLU makes the gradient discontinuous at z = 0: ``undecided`` marks the elements whose float64 z lies within the float32 bound of the
forward's z (the backward recomputes z with the forward's expression, so that bound is the backward's too).  Either branch is legitimate
there: such an element gets the magnitude of what the mask selects added to its own bound and to the sums it enters.  The random cases
below use seeds for which no element is undecided (the host test asserts it); MASK_CAP of gates_grad_bounds caps the share where a shape
cannot avoid them.  Every reference has slipped twins (its ``slip`` argument) which the tests demand to leave the bound.

Called with float64 tensors that are NOT float32-representable (the host tests do, to compare with float64 autograd) the values are plain
float64 mathematics; the bounds then mean nothing and are ignored."""
import numpy as np
import torch
import torch.nn.functional as F

from float64_bounds import U, gamma, eps32, _cdiv, _per_channel  # noqa: F401
from gates_grad_bounds import E, t64, rng, check, dot_depth, MASK_CAP, channel_scale_grad_ref, gct_gate_grad_ref, gct_gate64  # noqa: F401

f32, f64 = np.float32, np.float64
FRONT_SLIPS = ("ds_not_doubled", "no_dmean", "other_gate")
BACK_SLIPS = ("ds_not_doubled", "no_P4_P5", "tail_no_hw", "other_gate")
BACK_OUTS = ("grad_u", "grad_gamma", "grad_beta", "grad_tail", "grad_gct_alpha", "grad_gct_gamma", "grad_gct_beta")


def _cat_E(parts, dim):
    return E(torch.cat([p.v for p in parts], dim), torch.cat([p.e for p in parts], dim))


def _const(v):
    return E(torch.full((1,), float(v), dtype=torch.float64))


# ------------------------------------------------------------------------------------------ front 1: aoc_plane_dot_multi
def plane_dot_multi_ref(x, gs, slip=None):
    """x [P, hw], gs: n_set arrays [P, hw] -> (dots [n_set, P], tol): aoc_channel_scale_grad's dot per set.  slip 'drop_last': the dots without
    their last element; 'other_set': set k dotted with g_{k+1}."""
    gs = list(gs)
    if slip == "other_set":
        gs = gs[1:] + gs[:1]
    ones = torch.ones(t64(x).shape[0], dtype=torch.float64)                  # the gain half of channel_scale_grad_ref is not used
    per = [channel_scale_grad_ref(g, x, ones, "drop_last" if slip == "drop_last" else None)[1] for g in gs]
    return torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per])


# ------------------------------------------------------------------------------------------ the GCT gate's backward with an inexact dgate
def _gct_gate_grad_E(dgate, gate, s, alpha, gam, eps, slip=None):
    """gates_grad_bounds.gct_gate_grad_ref (l2 mode) with dgate an E: the plane sums P1 the back stage's gate launch reads are themselves float32
    sums.  -> E's dsum [N, C], grad_alpha, grad_gamma, grad_beta [C]."""
    gate, s = t64(gate), t64(s)
    al, ga = E(t64(alpha).reshape(1, -1)), E(t64(gam).reshape(1, -1))
    N, C = s.shape
    eps_e = E(torch.full((1, 1), eps32(eps), dtype=torch.float64))
    Cf = E(torch.full((1, 1), float(C), dtype=torch.float64))
    kc = _cdiv(C, 256) + 8
    one = E(torch.ones_like(gate))
    t = E(gate) - one
    du = dgate * (one - t * t)
    root = (E(s) + eps_e).sqrt()
    e = root * al
    M = (e * e).sum(1, kc, keepdim=True) / Cf
    num = ((du * e) * ga).sum(1, kc, keepdim=True)
    q = M + eps_e
    r = q.sqrt()
    dM = num.scale(-0.5) / (r * q)
    chain = (e.scale(2.0) * dM) / Cf
    if slip == "no_dM":
        chain = E(torch.zeros_like(e.v))
    de = du * (ga / r) + chain
    dsum = (de * al) / root.scale(2.0)
    return dsum, (de * root).sum(0, N), ((du * e) / r).sum(0, N), du.sum(0, N)


# ------------------------------------------------------------------------------------------ front 2: aoc_gct_gate_multi_grad
def gct_gate_multi_grad_ref(dgate, gate, s, alpha, gam, eps, l1=False, slip=None):
    """dgate, gate [S, N, C]; s [N, C]; alpha, gam [S, C] -> dict dsum_total [N, C], dsum [S, N, C], grad_alpha, grad_gamma, grad_beta [S, C] ->
    (want, tol): gates_grad_bounds.gct_gate_grad_ref per set, dsum_total their sum in ascending set order.  slip 'other_gate': set k with the
    saved gate of set k + 1; 'no_dM', 'one_minus_t', 'drop_last' as gct_gate_grad_ref's."""
    S = np.asarray(dgate).shape[0]
    gate_of = (lambda k: gate[(k + 1) % S]) if slip == "other_gate" else (lambda k: gate[k])
    inner = slip if slip in ("no_dM", "one_minus_t", "drop_last") else None
    per = [gct_gate_grad_ref(dgate[k], gate_of(k), s, alpha[k], gam[k], eps, l1, inner) for k in range(S)]
    stack = lambda i: (torch.stack([p[i][0] for p in per]), torch.stack([p[i][1] for p in per]))
    ds = E(*stack(0))
    tot = ds.sum(0, S)
    out = {"dsum_total": (tot.v, tot.e), "dsum": stack(0), "grad_alpha": stack(1), "grad_gamma": stack(2), "grad_beta": stack(3)}
    return out


# ------------------------------------------------------------------------------------------ front 3: aoc_channel_scale_multi_grad_apply
def front_apply_ref(gs, gates, x, dsum_total, dmean, slip=None):
    """gs: n_set arrays [P, hw]; gates [n_set, P]; x [P, hw]; dsum_total, dmean (or None) [P] -> (grad_x, tol), the header's expression order.
    slip 'ds_not_doubled': dsum_total in place of 2 dsum_total; 'no_dmean': the mean's share dropped; 'other_gate': set k scaled by the gate of
    set k + 1."""
    xx = E(t64(x))
    P, hw = xx.v.shape
    gt = t64(gates).reshape(len(gs), P, 1)
    if slip == "other_gate":
        gt = torch.roll(gt, -1, 0)
    acc = E(t64(gs[0])) * E(gt[0])
    for k in range(1, len(gs)):
        acc = acc + E(t64(gs[k])) * E(gt[k])
    ds2 = E(t64(dsum_total).reshape(P, 1)).scale(1.0 if slip == "ds_not_doubled" else 2.0)
    out = acc + ds2 * xx
    if dmean is not None and slip != "no_dmean":
        out = out + E(t64(dmean).reshape(P, 1)) / _const(hw)
    return out.v, out.e


# ------------------------------------------------------------------------------------------ back: aoc_groupnorm_cat_relu_grad
def back_saved64(us, groups, weights, biases, gn_eps, tail, gct_alpha, gct_gamma, gct_beta, gct_eps):
    """What the forward leaves for the backward, in float64: us n_src x [N, C_src, hw] -> dict stats [n_src, N * groups, 2] (mean, rstd), cat
    [N, C_total, hw], plane_sumsq, gate [N, C_total], out = gate * cat."""
    us = [t64(u) for u in us]
    N, C, hw = us[0].shape
    stats, parts = [], []
    for k, u in enumerate(us):
        ug = u.reshape(N, groups, -1)
        m, var = ug.mean(2), ug.var(2, unbiased=False)
        r = 1.0 / torch.sqrt(var + eps32(gn_eps))
        stats.append(torch.stack([m.reshape(-1), r.reshape(-1)], 1))
        w = t64(weights[k]).reshape(1, C, 1) if weights is not None else 1.0
        b = t64(biases[k]).reshape(1, C, 1) if biases is not None else 0.0
        parts.append(torch.relu((u - _per_channel(m, C)) * _per_channel(r, C) * w + b))
    if tail is not None:
        parts.append(torch.relu(t64(tail)).reshape(N, -1, 1).expand(-1, -1, hw))
    cat = torch.cat(parts, 1)
    sq = (cat * cat).sum(2)
    gate = gct_gate64(sq, gct_alpha, gct_gamma, gct_beta, gct_eps, False)
    return dict(stats=torch.stack(stats), cat=cat, plane_sumsq=sq, gate=gate, out=cat * gate.unsqueeze(2))


def cat_grad_ref(grad_out, us, stats, groups, weights, biases, tail, plane_sumsq, gate, gct_alpha, gct_gamma, gct_eps, slip=None):
    """The backward of out = gate * cat(relu(GN(u_k) w_k + b_k) ..., relu(tail) broadcast) with gate = GCT_l2(plane sums of squares of cat).
    grad_out [N, C_total, hw]; us: n_src arrays [N, C_src, hw]; stats [n_src, N * groups, 2] the forward's (mean, rstd); weights, biases
    [n_src, C_src] or None; tail [N, C_tail] or None; plane_sumsq, gate [N, C_total]; gct_alpha, gct_gamma [C_total].
    -> (dict over BACK_OUTS -> (want, tol), grad_u a list of n_src pairs; undecided: a list of n_src bool arrays [N, C_src, hw]).
    The expressions and their order are aspp_grad.hip's.  slip: 'ds_not_doubled' (ds where 2 ds belongs), 'no_P4_P5' (A = G P2, B = G P3),
    'tail_no_hw' (grad_tail's second term without the hw factor), 'other_gate' (every plane gated by the next channel's G)."""
    g_all = t64(grad_out)
    us = [t64(u) for u in us]
    n_src = len(us)
    N, C, hw = us[0].shape
    gc = C // groups
    n_aff = n_src * C
    C_total = g_all.shape[1]
    C_tail = C_total - n_aff
    st = t64(stats).reshape(n_src, N, groups, 2)
    G_all = t64(gate).reshape(N, C_total, 1)
    if slip == "other_gate":
        G_all = torch.roll(G_all, -1, 1)
    depth = dot_depth(hw)
    zero = torch.zeros(())
    per = []                                                                  # per source what the apply pass needs again
    P1, P2, P3, P4, P5 = [], [], [], [], []
    undecided = []
    for k, u in enumerate(us):
        mean, rstd = E(_per_channel(st[k, :, :, 0], C)), E(_per_channel(st[k, :, :, 1], C))
        gam = E(t64(weights[k]).reshape(1, C, 1)) if weights is not None else E(torch.ones(1, C, 1, dtype=torch.float64))
        bet = E(t64(biases[k]).reshape(1, C, 1)) if biases is not None else E(torch.zeros(1, C, 1, dtype=torch.float64))
        a = rstd * gam                                                       # ag_plane: a = rstd gamma, b = beta - mean a
        bb = bet - mean * a
        z = E(u) * a + bb
        mask = z.v > 0
        und = (z.v.abs() <= z.e) & (z.e > 0)
        cat = E(torch.relu(z.v), z.e)                                        # 1-Lipschitz
        xhat = (E(u) - mean) * rstd
        g = E(g_all[:, k * C:(k + 1) * C])
        sel = lambda t, mask=mask, und=und: E(torch.where(mask, t.v, zero), torch.where(mask, t.e, zero) + torch.where(und, t.v.abs() + t.e, zero))
        P1.append((g * cat).sum(2, depth, keepdim=True))
        P2.append(sel(g).sum(2, depth, keepdim=True))
        P3.append(sel(g * xhat).sum(2, depth, keepdim=True))
        P4.append(cat.sum(2, depth, keepdim=True))
        P5.append((cat * xhat).sum(2, depth, keepdim=True))
        per.append((mean, rstd, gam, cat, xhat, g, sel))
        undecided.append(und)
    p1_all = list(P1)
    Sg = rt = None
    if C_tail:
        Sg = E(g_all[:, n_aff:]).sum(2, depth, keepdim=True)
        rt = E(torch.relu(t64(tail)).reshape(N, C_tail, 1))
        p1_all.append(rt * Sg)
    p1 = _cat_E(p1_all, 1)
    ds, g_al, g_ga, g_be = _gct_gate_grad_E(E(p1.v[:, :, 0], p1.e[:, :, 0]), gate, plane_sumsq, gct_alpha, gct_gamma, gct_eps)
    d2_all = E(ds.v.unsqueeze(2), ds.e.unsqueeze(2)).scale(1.0 if slip == "ds_not_doubled" else 2.0)
    Mf = E(torch.full((1, 1, 1), float(gc * hw), dtype=torch.float64))
    out = {"grad_u": [], "grad_gct_alpha": (g_al.v, g_al.e), "grad_gct_gamma": (g_ga.v, g_ga.e), "grad_gct_beta": (g_be.v, g_be.e)}
    gg_rows, gb_rows = [], []
    for k in range(n_src):
        mean, rstd, gam, cat, xhat, g, sel = per[k]
        G = E(G_all[:, k * C:(k + 1) * C])
        d2 = E(d2_all.v[:, k * C:(k + 1) * C], d2_all.e[:, k * C:(k + 1) * C])
        if slip == "no_P4_P5":
            A, B = G * P2[k], G * P3[k]
        else:
            A, B = G * P2[k] + d2 * P4[k], G * P3[k] + d2 * P5[k]

        def group_sum(t):                                                    # [N, C, 1] -> per channel the sum over its group, ascending c
            t = gam * t
            s = E(t.v.reshape(N, groups, gc), t.e.reshape(N, groups, gc)).sum(2, gc)
            return E(_per_channel(s.v, C), _per_channel(s.e, C))
        c1, c2 = group_sum(A) / Mf, group_sum(B) / Mf
        dz = sel(g * G + d2 * cat)
        gu = rstd * ((gam * dz - c1) - xhat * c2)
        out["grad_u"].append((gu.v, gu.e))
        gg, gb = B.sum(0, N), A.sum(0, N)
        gg_rows.append((gg.v.reshape(C), gg.e.reshape(C)))
        gb_rows.append((gb.v.reshape(C), gb.e.reshape(C)))
    out["grad_gamma"] = tuple(torch.stack([r[i] for r in gg_rows]) for i in (0, 1))
    out["grad_beta"] = tuple(torch.stack([r[i] for r in gb_rows]) for i in (0, 1))
    if C_tail:
        G = E(G_all[:, n_aff:])
        d2 = E(d2_all.v[:, n_aff:], d2_all.e[:, n_aff:])
        tv = t64(tail).reshape(N, C_tail, 1)
        second = d2 * E(tv) if slip == "tail_no_hw" else (d2 * _const(hw)) * E(tv)
        gt = G * Sg + second
        on = tv > 0
        out["grad_tail"] = (torch.where(on, gt.v, zero).reshape(N, C_tail), torch.where(on, gt.e, zero).reshape(N, C_tail))
    else:
        out["grad_tail"] = None
    return out, undecided


# ------------------------------------------------------------------------------------------ the two stages in float64 torch (for autograd)
def gct64(x, alpha, gam, beta, eps):
    """gct.py:17-36, mode 'l2', written out on [N, C, hw]"""
    emb = (x.pow(2).sum(2, keepdim=True) + eps32(eps)).pow(0.5) * alpha.reshape(1, -1, 1)
    norm = gam.reshape(1, -1, 1) / (emb.pow(2).mean(dim=1, keepdim=True) + eps32(eps)).pow(0.5)
    return x * (1.0 + torch.tanh(emb * norm + beta.reshape(1, -1, 1)))


def front_forward64(x, alphas, gammas, betas, eps):
    """aspp.py:19 for every branch and :46: x [N, C, hw] -> ([GCT_k(x)], plane means [N, C])"""
    return [gct64(x, a, g, b, eps) for a, g, b in zip(alphas, gammas, betas)], x.mean(2)


def back_forward64(us, groups, weights, biases, gn_eps, tail, gct_alpha, gct_gamma, gct_beta, gct_eps):
    """aspp.py:21-23 for every branch, :61-65: GroupNorm + ReLU, the broadcast relu(tail) behind them, GCT(C_total) -> [N, C_total, hw]"""
    parts = [torch.relu(F.group_norm(u, groups, w, b, eps32(gn_eps))) for u, w, b in zip(us, weights, biases)]
    if tail is not None:
        parts.append(torch.relu(tail).unsqueeze(2).expand(-1, -1, us[0].shape[2]))
    return gct64(torch.cat(parts, 1), gct_alpha, gct_gamma, gct_beta, gct_eps)


def front_chain(x, gs, dmean, alphas, gammas, betas, eps):
    """The front's backward composed of the three references (values only): -> dict grad_x [N, C, hw], grad_alpha, grad_gamma, grad_beta [S, C]"""
    x = t64(x)
    N, C, hw = x.shape
    S = len(gs)
    sq = (x * x).sum(2)
    al, ga, be = (torch.stack([t64(p).reshape(-1) for p in ps]) for ps in (alphas, gammas, betas))
    gates = torch.stack([gct_gate64(sq, al[k], ga[k], be[k], eps, False) for k in range(S)])
    flat = lambda t: t64(t).reshape(N * C, hw)
    dots, _ = plane_dot_multi_ref(flat(x), [flat(g) for g in gs])
    small = gct_gate_multi_grad_ref(dots.reshape(S, N, C), gates, sq, al, ga, eps)
    gx, _ = front_apply_ref([flat(g) for g in gs], gates.reshape(S, N * C), flat(x), small["dsum_total"][0].reshape(-1),
                            t64(dmean).reshape(-1) if dmean is not None else None)
    return dict(grad_x=gx.reshape(N, C, hw), grad_alpha=small["grad_alpha"][0], grad_gamma=small["grad_gamma"][0], grad_beta=small["grad_beta"][0])


# ------------------------------------------------------------------------------------------ inputs shared by the host and the GPU tests
HWS = (1, 35, 257, 1023, 1024, 1025, 8209, 61 * 107)


def front_case(N, C, S, hw, seed=1):
    """float32 inputs of one front backward: x, the S cotangents [N, C, hw], dmean [N, C], and S GCT parameter rows [S, C]"""
    rs = rng(N, C, S, hw, seed)
    n = lambda *s: rs.standard_normal(s).astype(f32)
    x = (n(N, C, hw) * (0.5 + rs.rand(1, C, 1)) + 0.3 * n(1, C, 1)).astype(f32)
    return dict(x=x, gs=[n(N, C, hw) for _ in range(S)], dmean=n(N, C), alpha=rs.uniform(0.5, 1.5, (S, C)).astype(f32), gamma=n(S, C),
                beta=(0.5 * n(S, C)).astype(f32))


# (N, C_src, groups, n_src, C_tail, hw) -> the seed of the case: the first of 0, 1, 2, ... for which no element is undecided
# (test_aspp_grad_host asserts the count is zero)
BACK_CASES = {(1, 8, 2, 1, 0, 1): 0, (1, 8, 2, 1, 0, 35): 0, (2, 8, 2, 4, 4, 35): 0, (2, 8, 2, 4, 4, 257): 0, (2, 8, 2, 4, 4, 1023): 0,
              (2, 8, 2, 4, 4, 1024): 0, (2, 8, 2, 4, 4, 1025): 0, (2, 8, 2, 4, 4, 8209): 0, (1, 8, 2, 1, 0, 61 * 107): 0,
              (3, 128, 32, 4, 128, 31 * 33): 0,
              (30, 8, 2, 2, 4, 35): 0}                # AOC_MAX_OBJECTS samples: the serial sums over n at their longest


def back_case(N, C, groups, n_src, C_tail, hw, seed=None, planted=True):
    """float32 inputs of one back-stage backward.  planted (where the shape has room): gamma = beta = 0 on channel 1 of source 0 (z == 0: the
    mask is off), a constant group (group 1 of the last source, sample 0), a tail entry <= 0 and one exactly 0, and GCT gamma = beta = 0 on
    channel 2 (its gate is exactly 1)."""
    seed = BACK_CASES.get((N, C, groups, n_src, C_tail, hw), 0) if seed is None else seed
    rs = rng(N, C, groups, n_src, C_tail, hw, seed)
    n = lambda *s: rs.standard_normal(s).astype(f32)
    C_total = n_src * C + C_tail
    us = [(n(N, C, hw) * (0.5 + rs.rand(1, C, 1)) + n(1, C, 1)).astype(f32) for _ in range(n_src)]
    w, b = (1.0 + 0.5 * n(n_src, C)).astype(f32), (0.5 * n(n_src, C)).astype(f32)
    tail = n(N, C_tail) if C_tail else None
    p = dict(gct_alpha=rs.uniform(0.5, 1.5, C_total).astype(f32), gct_gamma=n(C_total), gct_beta=(0.5 * n(C_total)).astype(f32))
    if planted:
        w[0, 1] = b[0, 1] = 0.0
        gc = C // groups
        if groups > 1:
            us[-1][0, gc:2 * gc] = f32(0.75)
        if C_tail:
            tail[0, 0] = -abs(tail[0, 0]) - f32(0.1)
            tail[-1, 1] = 0.0
        p["gct_gamma"][2] = p["gct_beta"][2] = 0.0
    return dict(us=us, weights=w, biases=b, tail=tail, grad_out=n(N, C_total, hw), groups=groups, gn_eps=1e-5, gct_eps=1e-5, **p)


def back_saved32(s):
    """the float32 tensors the forward would leave (float64 values rounded once): what the host tests feed cat_grad_ref in place of a device run"""
    sv = back_saved64(s["us"], s["groups"], s["weights"], s["biases"], s["gn_eps"], s["tail"], s["gct_alpha"], s["gct_gamma"], s["gct_beta"], s["gct_eps"])
    return {k: v.numpy().astype(f32) for k, v in sv.items()}


def back_ref_args(s, saved):
    return dict(grad_out=s["grad_out"], us=s["us"], stats=saved["stats"], groups=s["groups"], weights=s["weights"], biases=s["biases"], tail=s["tail"],
                plane_sumsq=saved["plane_sumsq"], gate=saved["gate"], gct_alpha=s["gct_alpha"], gct_gamma=s["gct_gamma"], gct_eps=s["gct_eps"])


ASPP_FIXTURES = ("aspp_grad_O3", "aspp_grad_O1")
FIXTURE_SHAPES = {"aspp_grad_O3": (3, 3, 4), "aspp_grad_O1": (1, 2, 3)}          # N, h, w
WEIGHT_SEED = 20240917                                   # the five convolution weights of the fixtures: drawn, not stored
CONV_SHAPES = {"aspp1.atrous_conv.weight": (128, 512, 1, 1), "aspp2.atrous_conv.weight": (128, 512, 3, 3), "aspp3.atrous_conv.weight": (128, 512, 3, 3),
               "aspp4.atrous_conv.weight": (128, 512, 3, 3), "global_avg_pool.1.weight": (128, 512, 1, 1), "conv1.weight": (256, 640, 1, 1)}
# what a fixture keeps of the three large gradients (float64 does not compress): every fourth channel of grad_x, every 32nd row of the two
# recorded weight gradients
X_CHANNELS, W_ROWS = slice(None, None, 4), slice(None, None, 32)


def drawn_weights(seed=WEIGHT_SEED):
    """every convolution weight of ASPP from numpy's seed, He-scaled (fan_in), rounded to float16: shared by the recorder and the tests"""
    rs = np.random.RandomState([int(seed), 79])
    return {k: (rs.standard_normal(s) * np.sqrt(2.0 / (s[1] * s[2] * s[3]))).astype(np.float16).astype(f32) for k, s in CONV_SHAPES.items()}


def load_fixture_parameters(net, fx):
    """the fixture's small parameters (p_*) and the drawn convolution weights into an ASPP of any flavour (reference, mirror, twin), strictly"""
    sd = {k[2:]: torch.from_numpy(np.asarray(v, f32)) for k, v in fx.items() if k.startswith("p_")}
    sd.update({k: torch.from_numpy(v) for k, v in drawn_weights().items()})
    sd = {k: v.reshape(net.state_dict()[k].shape).to(net.state_dict()[k].dtype) for k, v in sd.items()}
    missing, unexpected = net.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return net


def aspp_chain64(x, gy, sd):
    """ASPP forward and backward in float64 with both fused stages differentiated by this module's references (front_chain, cat_grad_ref) and
    the convolutions, the pooled product and bn1 by torch's float64 autograd.  x [N, 512, h, w], gy [N, 256, h, w], sd: a state_dict (any float
    dtype) -> dict 'x' and every parameter name -> float64 gradient."""
    sd = {k: t64(v).clone().requires_grad_(True) for k, v in sd.items()}
    x = t64(x)
    N, C, h, w = x.shape
    hw = h * w
    names = ("aspp1", "aspp2", "aspp3", "aspp4")
    dil = (1, 6, 12, 18)
    gct = lambda pre: [sd[f"{pre}GCT.{k}"].detach().reshape(-1) for k in ("alpha", "gamma", "beta")]
    params = [gct(n + ".") for n in names]
    al, ga, be = ([p[i] for p in params] for i in range(3))
    with torch.no_grad():
        vs, mean = front_forward64(x.reshape(N, C, hw), al, ga, be, 1e-5)
    vs = [v.reshape(N, C, h, w).requires_grad_(True) for v in vs]
    mean = mean.clone().requires_grad_(True)
    us = []
    for n, d, v in zip(names, dil, vs):
        wgt = sd[n + ".atrous_conv.weight"]
        us.append(F.conv2d(v, wgt, None, 1, 0 if wgt.shape[2] == 1 else d, d))
    tail = mean @ sd["global_avg_pool.1.weight"].reshape(128, C).t()
    gw = torch.stack([sd[n + ".bn.weight"].detach() for n in names])
    gb = torch.stack([sd[n + ".bn.bias"].detach() for n in names])
    cal, cga, cbe = gct("")
    ud = [u.detach().reshape(N, 128, hw) for u in us]
    saved = back_saved64(ud, 32, gw, gb, 1e-5, tail.detach(), cal, cga, cbe, 1e-5)
    merged = saved["out"].reshape(N, 640, h, w).clone().requires_grad_(True)
    out = torch.relu(F.group_norm(F.conv2d(merged, sd["conv1.weight"]), 32, sd["bn1.weight"], sd["bn1.bias"], 1e-5))
    out.backward(t64(gy))
    back, _ = cat_grad_ref(merged.grad.reshape(N, 640, hw), ud, saved["stats"], 32, gw, gb, tail.detach(), saved["plane_sumsq"], saved["gate"], cal, cga, 1e-5)
    torch.autograd.backward(us + [tail], [g[0].reshape(N, 128, h, w) for g in back["grad_u"]] + [back["grad_tail"][0]])
    front = front_chain(x.reshape(N, C, hw), [v.grad.reshape(N, C, hw) for v in vs], mean.grad, al, ga, be, 1e-5)
    grads = {k: v.grad for k, v in sd.items() if v.grad is not None}
    grads["x"] = front["grad_x"].reshape(N, C, h, w)
    for k, n in enumerate(names):
        grads[n + ".GCT.alpha"], grads[n + ".GCT.gamma"], grads[n + ".GCT.beta"] = front["grad_alpha"][k], front["grad_gamma"][k], front["grad_beta"][k]
        grads[n + ".bn.weight"], grads[n + ".bn.bias"] = back["grad_gamma"][0][k], back["grad_beta"][0][k]
    grads["GCT.alpha"], grads["GCT.gamma"], grads["GCT.beta"] = back["grad_gct_alpha"][0], back["grad_gct_gamma"][0], back["grad_gct_beta"][0]
    return grads, out.detach()


def recorded_view(name, g):
    """the part of a gradient a fixture keeps"""
    if name == "x":
        return g[:, X_CHANNELS]
    if name in ("aspp1.atrous_conv.weight", "global_avg_pool.1.weight"):
        return g[W_ROWS]
    return g
