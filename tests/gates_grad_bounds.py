"""References and bounds for the training-time calibration gates (csrc/gate_grad.hip, aoc_amd.gates_train), shared by
tests/test_gates_grad_host.py and tests/test_gpu_gates_grad.py.

Every *_ref is a pure function of the tensors an entry point receives, widened to float64; it returns the float64 results and, for each, an
elementwise bound on |kernel - reference|.  The bound is a running error analysis of the kernel's own float32 expressions, carried by the
class ``E`` (a value and what a float32 evaluation of it is off by at most): the library is built with -ffp-contract=off, so every product,
sum, difference, quotient and square root rounds once (U = 2^-24 relative), and a sum of terms that each pass through at most k additions is
off by the terms' own errors plus gamma(k) times their magnitudes (tests/float64_bounds.py).  The summation depths are the kernels':

    plane dot        4 ceil(ceil(hw / 4) / T) + 2 additions per thread (float4 body, the front and back scalars), 6 butterfly levels, T / 64
                     wave sums; T = 256 up to 2 048 float4 per plane, else 1 024
    small kernels    serial loops: the summed dimension's length
    GCT sums over c  ceil(C / 256) per thread, 6 butterfly levels, 2 cross-wave levels

No constant is fitted to output.  The backward kernels compute no tanh: they read the saved gate (tanh convention of float64_bounds: n/a).
Every reference has a *_slip twin: the same function with one deliberate mistake (its ``slip`` argument), which the tests demand to leave the bound.

Called with float64 tensors that are NOT float32-representable (the host tests do, to compare with float64 autograd) the values are plain
float64 mathematics; the bounds then mean nothing and are ignored."""
import numpy as np
import torch
import torch.nn.functional as F

from float64_bounds import U, gamma, eps32, _cdiv, _check_bound, cond_scores_ref  # noqa: F401

f32, f64 = np.float32, np.float64


def t64(a):
    return None if a is None else torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a.detach().cpu()).double()


def rng(*seed):
    return np.random.RandomState(list(seed))


class E:
    """value v (float64) and a bound e >= |float32 evaluation - v|"""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def _r(v, e):                                         # one rounding of the computed value
        return E(v, e + U * (v.abs() + e))

    def __mul__(self, o):
        return E._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __add__(self, o):
        return E._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return E._r(self.v - o.v, self.e + o.e)

    def __truediv__(self, o):
        lo = (o.v.abs() - o.e).clamp_min(1e-300)          # the denominator's smallest magnitude
        return E._r(self.v / o.v, (self.e + (self.v / o.v).abs() * o.e) / lo)

    def sqrt(self):
        r = torch.sqrt(self.v)
        return E._r(r, r - torch.sqrt((self.v - self.e).clamp_min(0.0)))      # the side on which the root moves more

    def scale(self, k):                                   # by a power of two, or a sign: exact
        return E(self.v * k, self.e * abs(k))

    def sum(self, dim, depth, keepdim=False):
        """a float32 sum in which every term passes through at most `depth` additions"""
        return E(self.v.sum(dim, keepdim=keepdim), self.e.sum(dim, keepdim=keepdim)
                 + gamma(depth) * (self.v.abs() + self.e).sum(dim, keepdim=keepdim))


def check(got, want, tol, what):
    """max |got - want| / tol over the elements (0 / 0 counts as 0); asserts nothing."""
    got, want, tol = t64(got), t64(want), t64(tol)
    err = (got.reshape(want.shape) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------ 1 aoc_channel_scale_grad
def dot_depth(hw):
    T = 256 if hw // 4 <= 2048 else 1024
    return 4 * _cdiv(_cdiv(hw, 4), T) + 2 + 6 + T // 64


def channel_scale_grad_ref(grad_y, x, gain, slip=None):
    """grad_y, x [P, hw], gain [P] -> ((grad_x, tol), (dgain, tol)).  slip 'drop_last': the dot without its last element; 'prev_gain':
    grad_x with the previous plane's gain."""
    gy, xx, g = E(t64(grad_y)), E(t64(x)), t64(gain)
    if slip == "prev_gain":
        g = torch.roll(g, 1, 0) + (1.0 if g.numel() == 1 else 0.0)
    gx = gy * E(g.reshape(-1, 1))
    prod = gy * xx
    if slip == "drop_last":
        prod = E(prod.v[:, :-1], prod.e[:, :-1])
    dg = prod.sum(1, dot_depth(gy.v.shape[1]))
    return (gx.v, gx.e), (dg.v, dg.e)


# ------------------------------------------------------------------------------------------ 2 aoc_film_gain_grad
def _through_tanh(dgain, gain, slip=None):
    """da = dgain * (1 - t * t), t = gain - 1, as gg_da evaluates it"""
    one = E(torch.ones_like(gain))
    t = E(gain) - one
    s = (one - t) if slip == "one_minus_t" else (one - t * t)
    return E(dgain) * s


def film_gain_grad_ref(dgain, gain, head, weight, slip=None):
    """dgain, gain [O, c], head [O, D], weight [c, D] -> ((grad_head, tol), (grad_weight, tol), (grad_bias, tol)).  slip 'one_minus_t':
    1 - t in place of 1 - t^2; 'drop_last': every sum without its last term."""
    dgain, gain, head, weight = t64(dgain), t64(gain), t64(head), t64(weight)
    da = _through_tanh(dgain, gain, slip)
    O, c = dgain.shape
    cut = (lambda e, dim: E(e.v.narrow(dim, 0, e.v.shape[dim] - 1), e.e.narrow(dim, 0, e.e.shape[dim] - 1))) if slip == "drop_last" else (lambda e, dim: e)
    gh = cut(E(da.v[:, :, None], da.e[:, :, None]) * E(weight[None]), 1).sum(1, c)                   # [O, c, D] over c
    gw = cut(E(da.v[:, :, None], da.e[:, :, None]) * E(head[:, None, :]), 0).sum(0, O)               # [O, c, D] over O
    gb = cut(da, 0).sum(0, O)
    return (gh.v, gh.e), (gw.v, gw.e), (gb.v, gb.e)


# ------------------------------------------------------------------------------------------ 3 aoc_gct_gate_grad
def gct_gate_grad_ref(dgate, gate, s, alpha, gam, eps, l1, slip=None):
    """dgate, gate, s [N, C]; alpha, gam [C] -> ((dsum, tol), (grad_alpha, tol), (grad_gamma, tol), (grad_beta, tol)), gct_gate_grad_kernel's
    expressions in its order.  slip 'no_dM': the dM term dropped; 'one_minus_t'; 'drop_last': the sums over n without the last sample."""
    dgate, gate, s = t64(dgate), t64(gate), t64(s)
    al, ga = E(t64(alpha).reshape(1, -1)), E(t64(gam).reshape(1, -1))
    N, C = s.shape
    eps_e = E(torch.full((1, 1), eps32(eps), dtype=torch.float64))
    Cf = E(torch.full((1, 1), float(C), dtype=torch.float64))
    kc = _cdiv(C, 256) + 8
    root = E(s) if l1 else (E(s) + eps_e).sqrt()
    e = root * al
    du = _through_tanh(dgate, gate, "one_minus_t" if slip == "one_minus_t" else None)
    M = (E(e.v.abs(), e.e) if l1 else e * e).sum(1, kc, keepdim=True) / Cf
    num = ((du * e) * ga).sum(1, kc, keepdim=True)
    q = M + eps_e
    if l1:
        r = q
        dM = (num / (q * q)).scale(-1.0)
        chain = E(torch.sign(e.v) * dM.v, dM.e.expand_as(e.v).clone()) / Cf
    else:
        r = q.sqrt()
        dM = num.scale(-0.5) / (r * q)
        chain = (e.scale(2.0) * dM) / Cf
    if slip == "no_dM":
        chain = E(torch.zeros_like(e.v))
    de = du * (ga / r) + chain
    dsum = de * al if l1 else (de * al) / root.scale(2.0)
    n_sum = (lambda t: E(t.v[:-1], t.e[:-1]).sum(0, N)) if slip == "drop_last" else (lambda t: t.sum(0, N))
    g_al, g_ga, g_be = n_sum(de * root), n_sum((du * e) / r), n_sum(du)
    return (dsum.v, dsum.e), (g_al.v, g_al.e), (g_ga.v, g_ga.e), (g_be.v, g_be.e)


# ------------------------------------------------------------------------------------------ 4 aoc_gct_scale_grad
def gct_scale_grad_ref(grad_y, x, gate, dsum, mode, slip=False):
    """grad_y, x [P, hw]; gate, dsum [P] -> (grad_x, tol).  slip: f' = x for 2x (mode 1), 1 for sign x (mode 2), the dsum term dropped (0)."""
    gy, xx = E(t64(grad_y)), t64(x)
    a, b = E(t64(gate).reshape(-1, 1)), E(t64(dsum).reshape(-1, 1))
    if mode == 1:
        fp = xx if slip else 2.0 * xx
    elif mode == 2:
        fp = torch.ones_like(xx) if slip else torch.sign(xx)
    else:
        fp = torch.zeros_like(xx) if slip else torch.ones_like(xx)
    out = gy * a + b * E(fp)
    return out.v, out.e


# ------------------------------------------------------------------------------------------ 5 aoc_cond_codes_grad
CODE_OUTS = ("dgap", "dpx", "grad_head", "grad_w1", "grad_b1", "grad_w2", "grad_b2", "grad_w3", "grad_b3")


def _outer_sum(a, b, depth, cut=False):
    """sum_n a[n, i] b[n, j] in ascending n -> [i, j]"""
    t = E(a.v[:, :, None], a.e[:, :, None]) * E(b.v[:, None, :], b.e[:, None, :])
    if cut:
        t = E(t.v[:-1], t.e[:-1])
    return t.sum(0, depth)


def _rows_times(a, w, depth):
    """sum_i a[n, i] w[i, j] in ascending i -> [n, j]"""
    return (E(a.v[:, :, None], a.e[:, :, None]) * E(w[None])).sum(1, depth)


def cond_codes_grad_ref(dcode, gap, px, head, w1, w2, w3, slip=None):
    """-> a dict name -> (want, tol) of the nine outputs of aoc_cond_codes_grad.  slip 'no_minus': dpx without the - dd[n] (and grad_w2 with the
    delta without its - px[n]); 'drop_last': the sums over n (parameter gradients) and over i (input gradients) without their last term."""
    dcode, gap, px, head, w1, w2, w3 = (t64(t) for t in (dcode, gap, px, head, w1, w2, w3))
    N, D = head.shape
    C = gap.shape[1]
    d1, d2, d3 = E(dcode[:, :C]), E(dcode[:, C:2 * C]), E(dcode[:, 2 * C:])
    cut = slip == "drop_last"
    ci = (lambda d, w: (E(d.v[:, :-1]), w[:-1])) if cut else (lambda d, w: (d, w))
    out = {}
    out["dgap"] = _rows_times(*ci(d1, w1), C)
    dd = _rows_times(*ci(d2, w2), C)
    tot = dd.sum(0, N, keepdim=True)
    out["dpx"] = E(tot.v.expand_as(dd.v).clone(), tot.e.expand_as(dd.e).clone()) if slip == "no_minus" else E(tot.v.expand_as(dd.v), tot.e.expand_as(dd.e)) - dd
    out["grad_head"] = _rows_times(*ci(d3, w3), D)
    ptot = E(px).sum(0, N, keepdim=True)
    delta = E(ptot.v.expand_as(px).clone(), ptot.e.expand_as(px).clone()) if slip == "no_minus" else E(ptot.v.expand_as(px), ptot.e.expand_as(px)) - E(px)
    for k, (d, inp) in enumerate(((d1, E(gap)), (d2, delta), (d3, E(head))), 1):
        out[f"grad_w{k}"] = _outer_sum(d, inp, N, cut)
        out[f"grad_b{k}"] = (E(d.v[:-1]) if cut else d).sum(0, N)
    return {k: (v.v, v.e) for k, v in out.items()}


# ------------------------------------------------------------------------------------------ 6 aoc_cond_scale_grad
def cond_scale_grad_ref(grad_y, gain, scores, thr, dgap, dpx, slip=False):
    """grad_y [N, C, hw] or None, gain, dgap, dpx [N, C] (the last two or None), scores [N, hw], thr [N] -> (grad_x, tol).  The comparison is
    the float32 one (both operands are the kernel's inputs).  slip: >= in the mask."""
    scores, thr = t64(scores), t64(thr).reshape(-1, 1)
    N, hw = scores.shape
    mask = (scores >= thr) if slip else (scores > thr)
    C = (gain if gain is not None else dgap).shape[1]
    hwf = E(torch.full((1, 1), float(hw), dtype=torch.float64))
    zero = torch.zeros(N, C, dtype=torch.float64)
    b = E(t64(dgap) if dgap is not None else zero) / hwf
    c = E(t64(dpx) if dpx is not None else zero) / hwf
    m = E(torch.where(mask[:, None, :], b.v[:, :, None], torch.zeros(())), b.e[:, :, None].expand(N, C, hw).clone())
    first = (E(t64(grad_y)) * E(t64(gain)[:, :, None]) + m) if grad_y is not None else m
    out = first + E(c.v[:, :, None], c.e[:, :, None])
    return out.v, out.e


# ------------------------------------------------------------------------------------------ the slipped twins, by name
def channel_scale_grad_slip(kind, grad_y, x, gain):
    """'prev_gain' | 'drop_last'"""
    return channel_scale_grad_ref(grad_y, x, gain, kind)


def film_gain_grad_slip(kind, dgain, gain, head, weight):
    """'one_minus_t' | 'drop_last'"""
    return film_gain_grad_ref(dgain, gain, head, weight, kind)


def gct_gate_grad_slip(kind, dgate, gate, s, alpha, gam, eps, l1):
    """'no_dM' | 'one_minus_t' | 'drop_last'"""
    return gct_gate_grad_ref(dgate, gate, s, alpha, gam, eps, l1, kind)


def gct_scale_grad_slip(grad_y, x, gate, dsum, mode):
    return gct_scale_grad_ref(grad_y, x, gate, dsum, mode, True)


def cond_codes_grad_slip(kind, dcode, gap, px, head, w1, w2, w3):
    """'no_minus' | 'drop_last'"""
    return cond_codes_grad_ref(dcode, gap, px, head, w1, w2, w3, kind)


def cond_scale_grad_slip(grad_y, gain, scores, thr, dgap, dpx):
    """>= in the mask"""
    return cond_scale_grad_ref(grad_y, gain, scores, thr, dgap, dpx, True)


# ------------------------------------------------------------------------------------------ the modules in float64, composed of the references
def ia_gate_chain(x, head, weight, bias, grad_y):
    """IA_gate forward and backward (ATT:12-17) in float64 -> dict out, grad_x, grad_head, grad_weight, grad_bias"""
    x, head, weight, bias, grad_y = (t64(t) for t in (x, head, weight, bias, grad_y))
    O, c = x.shape[:2]
    gain = 1.0 + torch.tanh(F.linear(head, weight, bias))
    (gx, _), (dg, _) = channel_scale_grad_ref(grad_y.reshape(O * c, -1), x.reshape(O * c, -1), gain.reshape(-1))
    (gh, _), (gw, _), (gb, _) = film_gain_grad_ref(dg.reshape(O, c), gain, head, weight)
    return dict(out=x * gain.reshape(O, c, *([1] * (x.dim() - 2))), grad_x=gx.reshape(x.shape), grad_head=gh, grad_weight=gw, grad_bias=gb)


def gct_mode(mode, after_relu):
    """-> (aoc_plane_reduce mode, l1)"""
    return (1, False) if mode == "l2" else ((0 if after_relu else 2), True)


def plane_sums64(x, reduce_mode):
    x = t64(x).reshape(x.shape[0], x.shape[1], -1)
    return (x * x if reduce_mode == 1 else (x.abs() if reduce_mode == 2 else x)).sum(2)


def gct_gate64(s, alpha, gam, beta, eps, l1):
    al, ga, be = (t64(t).reshape(1, -1) for t in (alpha, gam, beta))
    eps = eps32(eps)
    e = s * al if l1 else torch.sqrt(s + eps) * al
    norm = ga / (e.abs().mean(1, keepdim=True) + eps) if l1 else ga / torch.sqrt((e * e).mean(1, keepdim=True) + eps)
    return 1.0 + torch.tanh(e * norm + be)


def gct_chain(x, alpha, gam, beta, eps, mode, after_relu, grad_y):
    """GCT forward and backward (gct.py:17-36) in float64 -> dict out, grad_x, grad_alpha, grad_gamma, grad_beta ([C])"""
    reduce_mode, l1 = gct_mode(mode, after_relu)
    x, grad_y = t64(x), t64(grad_y)
    N, C = x.shape[:2]
    s = plane_sums64(x, reduce_mode)
    gate = gct_gate64(s, alpha, gam, beta, eps, l1)
    xp, gp = x.reshape(N * C, -1), grad_y.reshape(N * C, -1)
    _, (dgate, _) = channel_scale_grad_ref(gp, xp, gate.reshape(-1))
    (dsum, _), (g_al, _), (g_ga, _), (g_be, _) = gct_gate_grad_ref(dgate.reshape(N, C), gate, s, alpha, gam, eps, l1)
    gx, _ = gct_scale_grad_ref(gp, xp, gate.reshape(-1), dsum.reshape(-1), reduce_mode)
    return dict(out=x * gate.reshape(N, C, *([1] * (x.dim() - 2))), grad_x=gx.reshape(x.shape), grad_alpha=g_al, grad_gamma=g_ga, grad_beta=g_be)


def cond_forward64(x, phi_w, phi_b, k_rank):
    """CL:27-43 and CLB:68 in float64: x [N, C, hw] -> scores, thr [N], mask, gap, px"""
    x = t64(x)
    scores = torch.einsum("c,ncp->np", t64(phi_w).reshape(-1), x) + t64(phi_b).reshape(())
    thr = torch.topk(scores, k_rank, dim=1).values[:, -1]
    mask = scores > thr[:, None]
    return scores, thr, mask, (x * mask[:, None, :]).mean(2), x.mean(2)


def cond_block_chain(x, head, p, k_rank, grad_y):
    """conditioning_block forward and backward (CLB:66-86 with the vector repair) in float64.  p: phi_w, phi_b, w1, b1, w2, b2, w3, b3, wm, bm.
    -> dict out, grad_x, grad_head, grad_w1 .. grad_b3, grad_wm, grad_bm, and the float64 scores / thr / mask."""
    x, head, grad_y = t64(x), t64(head), t64(grad_y)
    p = {k: t64(v) for k, v in p.items()}
    N, C = x.shape[:2]
    xp, gp = x.reshape(N, C, -1), grad_y.reshape(N, C, -1)
    scores, thr, mask, gap, px = cond_forward64(xp, p["phi_w"], p["phi_b"], k_rank)
    delta = px.sum(0, keepdim=True) - px
    code = torch.cat([F.linear(gap, p["w1"], p["b1"]), F.linear(delta, p["w2"], p["b2"]), F.linear(head, p["w3"], p["b3"])], 1)
    gain = 1.0 + torch.tanh(F.linear(code, p["wm"], p["bm"]))
    _, (dgain, _) = channel_scale_grad_ref(gp.reshape(N * C, -1), xp.reshape(N * C, -1), gain.reshape(-1))
    (dcode, _), (gwm, _), (gbm, _) = film_gain_grad_ref(dgain.reshape(N, C), gain, code, p["wm"])
    g = {k: v[0] for k, v in cond_codes_grad_ref(dcode, gap, px, head, p["w1"], p["w2"], p["w3"]).items()}
    gx, _ = cond_scale_grad_ref(gp, gain, scores, thr, g["dgap"], g["dpx"])
    out = dict(out=x * gain.reshape(N, C, *([1] * (x.dim() - 2))), grad_x=gx.reshape(x.shape), grad_wm=gwm, grad_bm=gbm, scores=scores, thr=thr, mask=mask)
    out.update({k: v for k, v in g.items() if k not in ("dgap", "dpx")})
    return out


def cond_layer_chain(x, p, k_rank, grad_y):
    """conditioning_layer (4-D input, CL:24-48) forward and backward in float64.  p: phi_w, phi_b, w1, b1 -> dict out, grad_x, grad_w1, grad_b1"""
    x, grad_y = t64(x), t64(grad_y)
    p = {k: t64(v) for k, v in p.items()}
    N, C = x.shape[:2]
    scores, thr, mask, gap, _ = cond_forward64(x.reshape(N, C, -1), p["phi_w"], p["phi_b"], k_rank)
    dgap, gw, gb = grad_y @ p["w1"], grad_y.t() @ gap, grad_y.sum(0)
    gx, _ = cond_scale_grad_ref(None, None, scores, thr, dgap, None)
    return dict(out=F.linear(gap, p["w1"], p["b1"]), grad_x=gx.reshape(x.shape), grad_w1=gw, grad_b1=gb, scores=scores, thr=thr, mask=mask)


# ------------------------------------------------------------------------------------------ inputs shared by the host and the GPU tests
def k_rank_of(beta, h, w):
    return int(beta * w * h)                                                # CL:32


def cond_case(N, C, D, h, w, beta, seed, kind="random"):
    """A conditioning block's inputs and parameters as float32 numpy arrays.  kind 'constant': every plane constant (all scores tie: the
    mask is empty); 'tie': per sample the pixel of the (k+1)-th largest float64 score is overwritten with the k-th's (an exact tie in any
    precision: the strict > drops both)."""
    rs = rng(N, C, D, h, w, seed)
    hw = h * w
    x = rs.standard_normal((N, C, hw)).astype(f32)
    p = dict(phi_w=(rs.standard_normal(C) * np.sqrt(2.0)).astype(f32), phi_b=(0.1 * rs.standard_normal(1)).astype(f32),
             w1=(rs.standard_normal((C, C)) / np.sqrt(C)).astype(f32), b1=(0.1 * rs.standard_normal(C)).astype(f32),
             w2=(rs.standard_normal((C, C)) / np.sqrt(C * max(N - 1, 1))).astype(f32), b2=(0.1 * rs.standard_normal(C)).astype(f32),
             w3=(rs.standard_normal((D, D)) / np.sqrt(D)).astype(f32), b3=(0.1 * rs.standard_normal(D)).astype(f32),
             wm=(rs.standard_normal((C, 2 * C + D)) / np.sqrt(2 * C + D)).astype(f32), bm=(0.1 * rs.standard_normal(C)).astype(f32))
    head = rs.standard_normal((N, D)).astype(f32)
    grad_y = rs.standard_normal((N, C, hw)).astype(f32)
    k = k_rank_of(beta, h, w)
    tied = None
    if kind == "constant":
        x[:] = x[:, :, :1]
    elif kind == "tie":
        s = np.einsum("c,ncp->np", p["phi_w"].astype(f64), x.astype(f64))
        order = np.argsort(-s, axis=1, kind="stable")
        for n in range(N):
            x[n, :, order[n, k]] = x[n, :, order[n, k - 1]]
        tied = order[:, k - 1:k + 1].copy()                # per sample the pixels of the k-th and the (k+1)-th largest score
    return dict(x=x.reshape(N, C, h, w), head=head, p=p, grad_y=grad_y.reshape(N, C, h, w), k_rank=k, beta=beta, kind=kind, tied=tied)


# (N, C, D, h, w, beta, seed, kind): N = 1, 3, 30; C in 4, 24, 32 with D smaller and larger; both betas; k = 1 (2 x 3 at 0.3); 9 x 11 and 31 x 33
COND_CASES = ((1, 4, 7, 9, 11, 0.3, 1, "random"), (3, 24, 5, 9, 11, 0.5, 2, "random"), (30, 4, 9, 9, 11, 0.3, 3, "random"),
              (3, 32, 40, 31, 33, 0.3, 4, "random"), (3, 4, 3, 2, 3, 0.3, 5, "random"), (3, 24, 30, 9, 11, 0.3, 6, "constant"),
              (3, 24, 30, 9, 11, 0.5, 7, "tie"), (2, 32, 12, 31, 33, 0.5, 8, "tie"))
MASK_CAP = 0.01                      # share of pixels that may lie within the float32 score bound of the threshold (random cases)


def mask_undecided(x, p, k_rank):
    """float64 scores, threshold and mask of a case, and the pixels whose float64 score lies within the float32 score bound (cond_scores_ref's)
    of the threshold: there a float32 evaluation may decide either way."""
    N, C = x.shape[:2]
    z = t64(x).reshape(N, C, -1)
    scores, thr, mask, _, _ = cond_forward64(z, p["phi_w"], p["phi_b"], k_rank)
    tol = gamma(C + _cdiv(C, 32) + 1) * (torch.einsum("c,ncp->np", t64(p["phi_w"]).abs(), z.abs()) + t64(p["phi_b"]).abs())
    kth = torch.topk(scores, k_rank, dim=1).indices[:, -1]
    near = (scores - thr[:, None]).abs() <= tol + tol.gather(1, kth[:, None])
    near.scatter_(1, kth[:, None], False)                # the threshold pixel itself: equal in any precision, never in the mask
    return scores, thr, mask, near


IA_FIXTURES = ("gates_grad_ia_O3", "gates_grad_ia_O1")
GCT_FIXTURES = ("gates_grad_gct_l2", "gates_grad_gct_l1")
BLOCK_FIXTURES = ("gates_grad_block_N3", "gates_grad_block_N1")
