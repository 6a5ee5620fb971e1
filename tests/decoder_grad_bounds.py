"""References and bounds for the training-time decoder forms (csrc/norm_grad.hip, aoc_amd.decoder_train), shared by
tests/test_decoder_grad_host.py and tests/test_gpu_decoder_grad.py.

Every *_ref is a pure function of the float32 tensors the forward and the backward receive, widened to float64; it returns the float64
gradients and, for each, an elementwise bound on |kernel - reference|.  The bound is a running error analysis of the kernels' own float32
expressions carried by ``gates_grad_bounds.E`` (a value and what a float32 evaluation of it is off by at most; -ffp-contract=off, so every
operation rounds once, U = 2^-24).  The statistics the backward reads are the forward's float32 (mean, rstd): the reference computes them
in float64, and what gn_stats_kernel's are off by (its float32 blocks of 8, tests/float64_bounds.groupnorm_ref) plus their one rounding to
float32 each enters every expression that reads them.  The summation depths are the kernels':

    plane sums       gates_grad_bounds.dot_depth(hw): 4 ceil(ceil(hw / 4) / T) + 2 per thread, 6 butterfly levels, T / 64 wave sums
    s1, s2           serial over the C / groups channels of a group;   grad_gamma, grad_beta   serial over N

No constant is fitted to output.  ReLU makes the gradient discontinuous at z = 0: ``undecided`` marks the elements whose float64 z lies within
the float32 bound of the forward's z (the backward recomputes z with the forward's expression, so that bound is the backward's too).  Either
branch is legitimate there: such an element gets |da| added to its own bound and to the sums it enters.  The random cases below use seeds
for which no element is undecided (the host test asserts it); were a shape not to allow that, MASK_CAP of gates_grad_bounds caps the share.
Every reference has slipped twins (its ``slip`` argument) which the tests demand to leave the bound.

Called with float64 tensors that are NOT float32-representable (the host tests do, to compare with float64 autograd) the values are plain
float64 mathematics; the bounds then mean nothing and are ignored."""
import numpy as np
import torch
import torch.nn.functional as F

from float64_bounds import U, gamma, eps32, _gn_stats, _rstd_err, _per_channel  # noqa: F401
from gates_grad_bounds import E, t64, rng, check, dot_depth, MASK_CAP, film_gain_grad_ref  # noqa: F401

f32, f64 = np.float32, np.float64
GN_OUTS = ("grad_x", "grad_residual", "grad_gamma", "grad_beta", "dgain")
GN_SLIPS = ("s2_no_gamma", "mean_hw", "mask_from_gy", "next_gain")


def _saved_stats(x, groups, eps):
    """float64 (mean, rstd) of x [N, C, hw] per channel [N, C, 1] as E: the error is gn_stats_kernel's (float64_bounds.groupnorm_ref: only the
    blocks of 8 are float32 sums) plus the rounding of each to float32."""
    N, C, hw = x.shape
    xg = x.reshape(N, groups, -1)
    n = xg.shape[2]
    m, var = _gn_stats(x, groups)
    i = torch.arange(n)
    in32 = ((i % 256 + 2048 * (i // 2048) + 7 * 256) < n).double()
    dm0 = gamma(8) * (xg.abs() * in32).mean(2)
    dvar = gamma(9) * (xg * xg * in32).mean(2) + 2 * m.abs() * dm0 + dm0 * dm0
    r, dr = _rstd_err(var, dvar, eps)
    dm = dm0 + U * (m.abs() + dm0)
    return E(_per_channel(m, C), _per_channel(dm, C)), E(_per_channel(r, C), _per_channel(dr, C))


def stats_ref(x, groups, eps):
    """x [N, C, hw] -> (want, tol) [N * groups, 2]: the (mean, rstd) pairs at the start of the forward's workspace"""
    xx = t64(x)
    gc = xx.shape[1] // groups
    mean, rstd = _saved_stats(xx, groups, eps32(eps))
    pick = lambda t: t[:, ::gc, 0].reshape(-1)
    return torch.stack([pick(mean.v), pick(rstd.v)], 1), torch.stack([pick(mean.e), pick(rstd.e)], 1)


def groupnorm_relu_grad_ref(grad_y, x, residual, groups, weight, bias, eps, relu=True, gain=None, slip=None):
    """The backward of y = [gain *] [relu](GroupNorm(x) weight + bias [+ residual]).  grad_y, x, residual [N, C, hw]; weight, bias [C] or None;
    gain [N, C] or None -> (dict name -> (want, tol) over GN_OUTS, undecided [N, C, hw] bool).  The expressions and their order are
    norm_grad.hip's.  slip: 's2_no_gamma' (s2 summed without gamma), 'mean_hw' (the group sums divided by hw, not M), 'mask_from_gy' (the ReLU
    mask taken from grad_y), 'next_gain' (the neighbouring channel's gain)."""
    gy, xx = t64(grad_y), t64(x)
    N, C, hw = xx.shape
    gc = C // groups
    res = t64(residual) if residual is not None else None
    w = t64(weight).reshape(1, C, 1) if weight is not None else torch.ones(1, C, 1, dtype=torch.float64)
    b = t64(bias).reshape(1, C, 1) if bias is not None else torch.zeros(1, C, 1, dtype=torch.float64)
    mean, rstd = _saved_stats(xx, groups, eps32(eps))
    gam = E(w)
    a = rstd * gam                                                           # ng_plane: a = rstd gamma, b = beta - mean a
    bb = E(b) - mean * a
    z = E(xx) * a + bb
    if res is not None:
        z = z + E(res)
    if relu:
        mask = (gy > 0) if slip == "mask_from_gy" else (z.v > 0)
        undecided = (z.v.abs() <= z.e) & (z.e > 0)                          # z.e == 0: the float32 z is the float64 one (a planted exact zero)
        act = E(torch.relu(z.v), z.e)                                       # 1-Lipschitz
    else:
        mask = torch.ones_like(z.v, dtype=torch.bool)
        undecided = torch.zeros_like(mask)
        act = z
    if gain is not None:
        g = t64(gain).reshape(N, C, 1)
        if slip == "next_gain":
            g = torch.roll(g, -1, 1)
        da = E(g) * E(gy)
    else:
        da = E(gy)
    zero = torch.zeros(())
    dz = E(torch.where(mask, da.v, zero), torch.where(mask, da.e, zero) + torch.where(undecided, da.v.abs() + da.e, zero))
    xhat = (E(xx) - mean) * rstd
    depth = dot_depth(hw)
    A, B, DG = dz.sum(2, depth, keepdim=True), (dz * xhat).sum(2, depth, keepdim=True), (E(gy) * act).sum(2, depth, keepdim=True)

    def group_sum(t, with_gamma=True):                                       # [N, C, 1] -> per channel the sum over its group, ascending c
        t = gam * t if with_gamma else t
        s = E(t.v.reshape(N, groups, gc), t.e.reshape(N, groups, gc)).sum(2, gc)
        return E(_per_channel(s.v, C), _per_channel(s.e, C))
    Mf = E._r(torch.full((1, 1, 1), float(hw if slip == "mean_hw" else gc * hw), dtype=torch.float64), torch.zeros(1, 1, 1, dtype=torch.float64))
    c1 = group_sum(A) / Mf
    c2 = group_sum(B, with_gamma=slip != "s2_no_gamma") / Mf
    gx = rstd * ((gam * dz - c1) - xhat * c2)
    gg, gb = B.sum(0, N), A.sum(0, N)
    out = {"grad_x": (gx.v, gx.e), "grad_residual": (dz.v, dz.e), "grad_gamma": (gg.v.reshape(C), gg.e.reshape(C)),
           "grad_beta": (gb.v.reshape(C), gb.e.reshape(C)), "dgain": (DG.v.reshape(N, C), DG.e.reshape(N, C))}
    return out, undecided


def forward64(x, residual, groups, weight, bias, eps, relu=True, gain=None):
    """the forward in float64 torch (for autograd): every argument a float64 tensor or None"""
    y = F.group_norm(x, groups, weight, bias, eps32(eps))
    if residual is not None:
        y = y + residual
    if relu:
        y = torch.relu(y)
    return y * gain.reshape(gain.shape[0], gain.shape[1], *([1] * (x.dim() - 2))) if gain is not None else y


def cat_film_scale_grad_ref(grad_y, x, mem, gain, slip=None):
    """grad_y [O, Cx + Cm, hw], x [O, Cx, hw], mem [O, Cm, hw] or None, gain [O, Cx + Cm] -> dict grad_x, grad_mem (None without mem), dgain ->
    (want, tol).  slip 'next_gain': the neighbouring channel's gain; 'drop_last': the dot without its last element."""
    gy, xx, g = t64(grad_y), t64(x), t64(gain)
    O, Ct, hw = gy.shape
    Cx = xx.shape[1]
    cat = torch.cat([xx, t64(mem)], 1) if mem is not None else xx
    if slip == "next_gain":
        g = torch.roll(g, -1, 1) + (1.0 if Ct == 1 else 0.0)
    full = E(g.reshape(O, Ct, 1)) * E(gy)
    prod = E(gy) * E(cat)
    if slip == "drop_last":
        prod = E(prod.v[:, :, :-1], prod.e[:, :, :-1])
    dg = prod.sum(2, dot_depth(hw))
    return {"grad_x": (full.v[:, :Cx], full.e[:, :Cx]), "grad_mem": (full.v[:, Cx:], full.e[:, Cx:]) if mem is not None else None,
            "dgain": (dg.v, dg.e)}


# ------------------------------------------------------------------------------------------ inputs shared by the host and the GPU tests
# (N, C, groups, hw) -> the seed of the case.  Each seed is the first of 0, 1, 2, ... for which no element of either ReLU variant below is
# undecided (found by tests/golden/make_golden_decoder_grad.py --seeds; test_decoder_grad_host asserts the count is zero).
GN_CASES = {(1, 32, 32, 1): 0, (2, 64, 32, 35): 0, (3, 8, 2, 257): 0, (2, 96, 32, 1023): 0, (2, 96, 32, 1024): 1, (2, 96, 32, 1025): 0,
            (2, 8, 1, 8209): 0, (30, 32, 32, 9): 0, (4, 256, 32, 31 * 33): 2,
            (2, 8, 2, 61 * 107): 0}                  # beyond the issue's list: 256 threads with several float4 each (the unrolled loop runs three times)
# (residual, relu, gain, affine): each on and off, alone and together
GN_VARIANTS = ((True, True, True, True), (False, False, False, False), (False, True, False, True), (True, False, True, False))


def gn_case(N, C, groups, hw, seed=None):
    """float32 inputs of one GroupNorm backward: x, residual, grad_y [N, C, hw], weight, bias [C], gain [N, C]"""
    seed = GN_CASES[(N, C, groups, hw)] if seed is None else seed
    rs = rng(N, C, groups, hw, seed)
    n = lambda *s: rs.standard_normal(s).astype(f32)
    return dict(x=(n(N, C, hw) * (0.5 + rs.rand(1, C, 1)) + n(1, C, 1)).astype(f32), residual=n(N, C, hw), grad_y=n(N, C, hw),
                weight=(1.0 + 0.5 * n(C)).astype(f32), bias=(0.5 * n(C)).astype(f32), gain=(1 + np.tanh(n(N, C))).astype(f32))


def gn_args(s, variant, groups, eps=1e-5):
    """the arguments of groupnorm_relu_grad_ref for one variant of a case"""
    res, relu, gain, affine = variant
    return dict(grad_y=s["grad_y"], x=s["x"], residual=s["residual"] if res else None, groups=groups, weight=s["weight"] if affine else None,
                bias=s["bias"] if affine else None, eps=eps, relu=relu, gain=s["gain"] if gain else None)


def gn_slips(variant, C, groups):
    """the slips that must leave the bound for this variant"""
    res, relu, gain, affine = variant
    out = []
    if affine and C // groups > 1:
        out.append("s2_no_gamma")
    if C // groups > 1:
        out.append("mean_hw")
    if relu:
        out.append("mask_from_gy")
    if gain and C > 1:
        out.append("next_gain")
    return out


CAT_CASES = ((1, 1, 0, 1), (2, 3, 5, 35), (3, 64, 64, 1025), (30, 4, 4, 9),
             (2, 3, 2, 61 * 107))                     # beyond the issue's list: the four-float4 unrolled loop of a 256-thread plane


def cat_case(O, Cx, Cm, hw, seed=1):
    rs = rng(O, Cx, Cm, hw, seed)
    n = lambda *s: rs.standard_normal(s).astype(f32)
    return dict(x=n(O, Cx, hw), mem=n(O, Cm, hw) if Cm else None, grad_y=n(O, Cx + Cm, hw), gain=(1 + np.tanh(n(O, Cx + Cm))).astype(f32))


BOTTLENECK_FIXTURES = ("decoder_grad_bottleneck_down_O2", "decoder_grad_bottleneck_same_O3")


# ------------------------------------------------------------------------------------------ a Bottleneck's parameters, for recorder and tests
def _h16(a):
    return np.asarray(a, f32).astype(np.float16).astype(f64)


def _fill(p, a):
    with torch.no_grad():
        p.copy_(torch.from_numpy(np.asarray(a)).to(p.dtype).reshape(p.shape))


def set_conv_weights(blk, seed):
    """every convolution of a Bottleneck (reference, mirror or twin) from numpy's seed, in named_modules order, He-scaled, rounded to float16"""
    rs = np.random.RandomState([int(seed), 77])
    for _, m in blk.named_modules():
        if isinstance(m, torch.nn.Conv2d):
            fan_out = m.weight.shape[0] * m.weight.shape[2] * m.weight.shape[3]
            _fill(m.weight, _h16(rs.standard_normal(tuple(m.weight.shape)) * np.sqrt(2.0 / fan_out)))


def randomize_small_parameters(blk, gate, rs):
    """GroupNorm weights and biases and the GCT's three vectors away from their constructor values (where half the gradients vanish), the
    gate's linear as constructed; all rounded to float16"""
    for _, m in blk.named_modules():
        if isinstance(m, torch.nn.GroupNorm):
            _fill(m.weight, _h16(1.0 + 0.5 * rs.standard_normal(m.weight.shape)))
            _fill(m.bias, _h16(0.5 * rs.standard_normal(m.bias.shape)))
    _fill(blk.GCT1.alpha, _h16(rs.uniform(0.5, 1.5, blk.GCT1.alpha.shape)))
    _fill(blk.GCT1.gamma, _h16(rs.standard_normal(blk.GCT1.gamma.shape)))
    _fill(blk.GCT1.beta, _h16(0.5 * rs.standard_normal(blk.GCT1.beta.shape)))
    if gate is not None:
        for p in gate.parameters():
            _fill(p, _h16(p.detach().numpy()))


class _RefGN(torch.autograd.Function):
    """float64: forward64 forward, groupnorm_relu_grad_ref backward (its values; gamma / beta / gain may be None)"""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, gain, groups, eps, relu):
        ctx.save_for_backward(x, weight, bias, residual, gain)
        ctx.cfg = (groups, eps, relu)
        return forward64(x, residual, groups, weight, bias, eps, relu, gain)

    @staticmethod
    def backward(ctx, gy):
        x, weight, bias, residual, gain = ctx.saved_tensors
        groups, eps, relu = ctx.cfg
        N, C = x.shape[:2]
        p = lambda t: t.reshape(N, C, -1) if t is not None else None
        ref, _ = groupnorm_relu_grad_ref(p(gy), p(x), p(residual), groups, weight, bias, eps, relu, gain)
        g = {k: v[0] for k, v in ref.items()}
        return (g["grad_x"].reshape(x.shape), g["grad_gamma"], g["grad_beta"], g["grad_residual"].reshape(x.shape) if residual is not None else None,
                g["dgain"] if gain is not None else None, None, None, None)


def bottleneck_chain64(blk, gate, x, head):
    """Bottleneck + IA_gate in float64 with every normalisation (and the gate's a * x) differentiated by groupnorm_relu_grad_ref; the
    convolutions, the GCT and the gate's linear + tanh by torch's float64 autograd.  blk, gate: float64 modules with the reference's names."""
    gn = lambda bn, t, residual=None, relu=True, gain=None: _RefGN.apply(t, bn.weight, bn.bias, residual, gain, bn.num_groups, bn.eps, relu)
    m = blk.GCT1                                                             # gct.py:17-36, mode 'l2', written out: only m's parameters are read
    emb = (x.pow(2).sum((2, 3), keepdim=True) + m.epsilon).pow(0.5) * m.alpha
    norm = m.gamma / (emb.pow(2).mean(dim=1, keepdim=True) + m.epsilon).pow(0.5)
    out = gn(blk.bn1, blk.conv1(x * (1.0 + torch.tanh(emb * norm + m.beta))))
    out = gn(blk.bn2, blk.conv2(out))
    residual = x if blk.downsample is None else gn(blk.downsample[1], blk.downsample[0](x), relu=False)
    gain = 1.0 + torch.tanh(gate.IA(head)) if gate is not None else None
    return gn(blk.bn3, blk.conv3(out), residual, True, gain)
