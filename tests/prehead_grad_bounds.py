"""References and bounds for the differentiable DynamicPreHead (csrc/prehead_grad.hip, aoc_amd.prehead_train), shared by
tests/test_prehead_grad_host.py, tests/test_gpu_prehead_grad.py, tools/bench_prehead_grad.py and tests/golden/make_golden_prehead_grad.py.

``prehead_grad_ref`` is a pure function of the float32 tensors the backward receives, widened to float64; it returns the six float64
gradients and, for each, an elementwise bound on |kernel - reference|.  The bound is a running error analysis of the kernels' own float32
expressions as include/aoc_hip.h states them, carried by ``gates_grad_bounds.E`` (a value and what a float32 evaluation of it is off by at
most; -ffp-contract=off, so every operation rounds once, U = 2^-24; an fmaf chain rounds once per step).  No constant is fitted to output.

    y                 the forward's fmaf chain of n_in steps: gamma(n_in) (|b| + sum |w x|), as float64_bounds.prehead_ref
    mean, rstd        the forward's saved float32 pair: what prehead_stats_kernel's are off by (its float32 sums over a group's channels per
                      pixel; float64_bounds.prehead_ref) plus their one rounding to float32 each.  A term of every bound below.
    xhat, v, dy       one rounding per operation
    SA, SB            double sums of float32 terms: the terms' own errors only (2^-53 roundings are not counted, as everywhere here)
    grad_beta, grad_gamma, c1, c2     one rounding of the double result to float32
    grad_feat         an fmaf chain of n_out steps from 0.0f
    grad_weight, grad_bias            fmaf chains over the at most 256 pixels of a chunk from 0.0f, the chunks' float32 results added in double,
                                      one rounding to float32
    grad_emb          a float32 sum over the objects from 0.0f: n_obj - 1 roundings

ReLU makes the gradient discontinuous at v = 0.  ``undecided`` marks the elements whose float64 |v| lies within the forward's float32 bound
(float64_bounds.prehead_ref's tol; the backward recomputes v with the forward's instructions, so that bound is the backward's too).  No
element is ever excluded from a comparison and no allowance is made for an undecided one: every case and seed below has none (the host test
asserts it for each), by the choice of the seed -- the first of 0, 1, 2, ... for which the float64 reference alone says so.

Called with float64 tensors that are NOT float32-representable (the host tests do, to compare with float64 autograd) the values are plain
float64 mathematics; the bounds then mean nothing and are ignored."""
import numpy as np
import torch

import float64_bounds as fb
from float64_bounds import U, gamma, eps32, _per_channel, _rstd_err  # noqa: F401
from gates_grad_bounds import E, t64, rng, check  # noqa: F401

f32, f64 = np.float32, np.float64
OUTS = ("grad_feat", "grad_weight", "grad_bias", "grad_gamma", "grad_beta", "grad_emb")
PIX = 256
# slip -> the output it must push out of its bound
SLIPS = {"no_B": "grad_feat", "sample_sums": "grad_feat", "mask_from_y": "grad_beta", "emb_drop_last": "grad_emb", "w_first_chunk": "grad_weight"}


def _mul(a, b):
    """a product that is not rounded on its own (an operand of fmaf, or a double product)"""
    return E(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)


def _conv(feat, w, b):
    """y [O, n_out, hw] as E: the forward's chain"""
    y = torch.einsum("ck,okp->ocp", w, feat) + b.view(1, -1, 1)
    dy = gamma(feat.shape[1]) * (torch.einsum("ck,okp->ocp", w.abs(), feat.abs()) + b.abs().view(1, -1, 1))
    return E(y, dy)


def _saved_stats(y, n_groups, eps, any_order=False):
    """float64 (mean, rstd) of y per channel [O, n_out, 1] as E: prehead_stats_kernel's error (float64_bounds.prehead_ref, the same
    expressions) plus the rounding of each to float32.  any_order: the group's sums wholly in float32, in whatever order."""
    O, n_out, hw = y.v.shape
    gs = n_out // n_groups * (hw if any_order else 1)
    G = lambda t: t.reshape(O, n_groups, -1).mean(2)
    ya, dy = y.v.abs(), y.e
    m = G(y.v)
    var = (G(y.v * y.v) - m * m).clamp_min(0.0)
    dm0 = G(dy) + gamma(gs) * G(ya + dy)
    dq = G(2 * ya * dy + dy * dy) + gamma(gs + 1) * G((ya + dy) ** 2)
    dvar = dq + 2 * m.abs() * dm0 + dm0 * dm0
    r, dr = _rstd_err(var, dvar, eps)
    dm = dm0 + U * (m.abs() + dm0)
    return E(_per_channel(m, n_out), _per_channel(dm, n_out)), E(_per_channel(r, n_out), _per_channel(dr, n_out))


def _group_sum(t, O, n_groups, n_out, depth=0):
    """[O, n_out, 1] -> per channel the sum over its group (depth 0: in double, no rounding)"""
    s = E(t.v.reshape(O, n_groups, -1), t.e.reshape(O, n_groups, -1)).sum(2, depth)
    return E(_per_channel(s.v, n_out), _per_channel(s.e, n_out))


def prehead_grad_ref(grad_out, feat, weight, bias, n_groups, gn_w, gn_b, eps, C=0, slip=None, any_order=False):
    """The backward of out = cat(emb expanded over the objects, relu(GroupNorm(W feat + b) gn_w + gn_b)).  grad_out [O, C + n_out, hw], feat
    [O, n_in, hw], weight [n_out, n_in] -> (dict name -> (want, tol) over OUTS (grad_emb [hw, C], None when C == 0), undecided [O, n_out, hw]
    bool).  The expressions and their order are prehead_grad.hip's.  slip: one of SLIPS.  any_order (tools/bench_prehead_grad.py, for an
    arm whose kernels are not ours): the same expressions with every sum in float32 in whatever order -- a term passes through at most
    (number of terms - 1) additions --, and `undecided` by this analysis' own bound of v."""
    go, x, w, b, gw, gb = (t64(t) for t in (grad_out, feat, weight, bias, gn_w, gn_b))
    w = w.reshape(w.shape[0], -1)
    O, n_in, hw = x.shape
    n_out = w.shape[0]
    gs = n_out // n_groups
    eps = eps32(eps)
    y = _conv(x, w, b)
    mean, rstd = _saved_stats(y, n_groups, eps, any_order)
    gam, bet = E(gw.view(1, -1, 1)), E(gb.view(1, -1, 1))
    xhat = (y - mean) * rstd
    v = xhat * gam + bet
    _, fwd_tol = fb.prehead_ref(x, w, b, n_groups, gw, gb, eps)
    undecided = v.v.abs() <= (v.e if any_order else fwd_tol)
    mask = (y.v > 0) if slip == "mask_from_y" else (v.v > 0)
    gy = go[:, C:]
    dz = E(torch.where(mask, gy, torch.zeros(())))                           # a select: exact
    t = dz * xhat
    d_plane, d_obj, d_group = (hw, O, gs) if any_order else (0, 0, 0)       # ours: double sums, the terms' errors only
    SA, SB = dz.sum(2, d_plane, keepdim=True), t.sum(2, d_plane, keepdim=True)
    grad_beta, grad_gamma = SA.sum(0, d_obj), SB.sum(0, d_obj)
    grad_beta, grad_gamma = E._r(grad_beta.v.reshape(-1), grad_beta.e.reshape(-1)), E._r(grad_gamma.v.reshape(-1), grad_gamma.e.reshape(-1))
    if slip == "sample_sums":
        tot = lambda s: E(s.v.sum(1, keepdim=True).expand(O, n_out, 1) / (n_out * hw), s.e.sum(1, keepdim=True).expand(O, n_out, 1) / (n_out * hw))
        c1, c2 = tot(_mul(gam, SA)), tot(_mul(gam, SB))
    else:
        M = float(gs * hw)
        c1, c2 = _group_sum(_mul(gam, SA), O, n_groups, n_out, d_group), _group_sum(_mul(gam, SB), O, n_groups, n_out, d_group)
        c1, c2 = E(c1.v / M, c1.e / M), E(c2.v / M, c2.e / M)
    c1, c2 = E._r(c1.v, c1.e), E._r(c2.v, c2.e)
    inner = gam * dz - c1
    dy = rstd * (inner if slip == "no_B" else inner - xhat * c2)
    mag = dy.v.abs() + dy.e
    # grad_feat: fmaf chain over c from 0.0f
    gf = E(torch.einsum("ck,ocp->okp", w, dy.v), torch.einsum("ck,ocp->okp", w.abs(), dy.e) + gamma(n_out) * torch.einsum("ck,ocp->okp", w.abs(), mag))
    # grad_weight, grad_bias: fmaf chains over a chunk's pixels, the chunks in double, one rounding
    depth = O * hw if any_order else min(hw, PIX)
    sel = slice(0, PIX) if slip == "w_first_chunk" else slice(None)
    xa = x.abs()
    gwt = E._r(torch.einsum("ocp,okp->ck", dy.v[:, :, sel], x[:, :, sel]),
               torch.einsum("ocp,okp->ck", dy.e, xa) + gamma(depth) * torch.einsum("ocp,okp->ck", mag, xa))
    gbi = E._r(dy.v.sum((0, 2)), dy.e.sum((0, 2)) + gamma(depth) * mag.sum((0, 2)))
    out = {"grad_feat": (gf.v, gf.e), "grad_weight": (gwt.v, gwt.e), "grad_bias": (gbi.v, gbi.e), "grad_gamma": (grad_gamma.v, grad_gamma.e),
           "grad_beta": (grad_beta.v, grad_beta.e), "grad_emb": None}
    if C > 0:
        ge = go[:, :C]
        if slip == "emb_drop_last":
            ge = ge[:-1]
        out["grad_emb"] = (ge.sum(0).t().contiguous(), (gamma(max(O - 1, 0)) * go[:, :C].abs().sum(0)).t().contiguous())
    return out, undecided


def forward64(feat, weight, bias, n_groups, gn_w, gn_b, eps, emb_hwc=None):
    """the forward in float64 torch (for autograd): feat [O, n_in, h, w], emb_hwc [h, w, C] or None -> [O, C + n_out, h, w]"""
    import torch.nn.functional as F
    y = torch.relu(F.group_norm(F.conv2d(feat, weight.reshape(weight.shape[0], -1, 1, 1), bias), n_groups, gn_w, gn_b, eps32(eps)))
    if emb_hwc is None:
        return y
    return torch.cat((emb_hwc.permute(2, 0, 1).unsqueeze(0).expand(feat.shape[0], -1, -1, -1), y), 1)      # aocnet.py:188, 362


# ------------------------------------------------------------------------------------------ inputs shared by the host and the GPU tests
# (n_obj, n_in, n_out, groups, hw, C) -> the seed of the case: the first of 0, 1, 2, ... without an undecided element
# (tests/golden/make_golden_prehead_grad.py --seeds finds them; test_prehead_grad_host asserts the count is zero).
CASES = {(1, 24, 64, 16, 17 * 23, 100): 0, (3, 26, 64, 16, 257, 3): 0, (1, 28, 64, 16, 255, 0): 0, (4, 24, 64, 16, 31 * 33, 100): 13,
         (30, 24, 64, 16, 35, 3): 3, (3, 1, 128, 64, 1, 3): 0, (1, 7, 128, 128, 257, 0): 0, (3, 32, 128, 128, 1, 100): 12, (1, 24, 128, 64, 256, 0): 2,
         (2, 24, 64, 16, 513, 5): 0}
MASK_CASES = {(2, 24, 64, 16, 300, 2): 1, (2, 26, 64, 16, 300, 0): 0, (2, 28, 64, 16, 300, 0): 0, (2, 5, 32, 8, 300, 0): 0}
PLANTED = (2, 24, 64, 16, 300, 3)
PLANTED_SEED = 0
FIXTURES = ("prehead_grad_O1_24", "prehead_grad_O3_26_emb", "prehead_grad_O4_24_emb")


def case(n_obj, n_in, n_out, groups, hw, C, seed):
    """float32 inputs of one backward: feat [O, n_in, hw], grad_out [O, C + n_out, hw], weight [n_out, n_in], bias, gn_w, gn_b [n_out], emb [hw, C]"""
    rs = rng(n_obj, n_in, n_out, groups, hw, C, seed)
    n = lambda *s: rs.standard_normal(s).astype(f32)
    return dict(feat=n(n_obj, n_in, hw), grad_out=n(n_obj, C + n_out, hw), weight=(n(n_out, n_in) * np.sqrt(2.0 / n_in)).astype(f32),
                bias=(0.2 * n(n_out)).astype(f32), gn_w=(1.0 + 0.25 * n(n_out)).astype(f32), gn_b=(0.5 * n(n_out)).astype(f32),
                emb=n(hw, C) if C else None)


def planted_case(*key_and_seed):
    """PLANTED with: object 1's cotangent all zero; the whole group 0 (channels 0 .. 3) and channel 6 alone never active (beta = -100);
    gamma = 0 on channel 9"""
    s = case(*(key_and_seed or PLANTED + (PLANTED_SEED,)))
    C = PLANTED[5]
    s["grad_out"][1, C:] = 0.0
    s["gn_b"][[0, 1, 2, 3, 6]] = -100.0
    s["gn_w"][9] = 0.0
    return s


def ref_args(s, groups, C, eps=1e-5):
    return dict(grad_out=s["grad_out"], feat=s["feat"], weight=s["weight"], bias=s["bias"], n_groups=groups, gn_w=s["gn_w"], gn_b=s["gn_b"], eps=eps, C=C)


def fixture_args(z):
    """a fixture -> (the arguments of prehead_grad_ref, C)"""
    x, wt = z["in_x"], z["in_weight"]
    O, n_in = x.shape[:2]
    C = wt.shape[1] - z["w_conv_w"].shape[0]
    return dict(grad_out=wt.reshape(O, wt.shape[1], -1), feat=x.reshape(O, n_in, -1), weight=z["w_conv_w"], bias=z["w_conv_b"], n_groups=int(z["groups"]),
                gn_w=z["w_gn_w"], gn_b=z["w_gn_b"], eps=float(z["eps"]), C=C), C


def slips_of(n_out, groups, hw, C):
    """the slips that must leave the bound at this shape"""
    out = ["mask_from_y"]
    if n_out // groups * hw > 1:
        out.append("no_B")                       # a group of one element: xhat = 0
    if groups > 1 and n_out // groups * hw > 1:
        out.append("sample_sums")
    if C > 0:
        out.append("emb_drop_last")
    if hw > PIX:
        out.append("w_first_chunk")
    return out


def first_seed(key, build=case, limit=64):
    for seed in range(limit):
        s = build(*key, seed)
        _, und = prehead_grad_ref(**ref_args(s, key[3], key[5]))
        if int(und.sum()) == 0:
            return seed
    raise RuntimeError(f"{key}: no seed below {limit} without an undecided element")
