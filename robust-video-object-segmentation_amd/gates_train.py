"""Differentiable twins of the calibration gates: ``IA_gate`` (networks/layers/attention.py == ATT:7-17), ``GCT`` (networks/layers/gct.py:7-36),
``conditioning_layer`` and ``conditioning_block`` (networks/aoc/conditioning_layer.py == CLB:6-86).  They stand beside the inference mirrors
``attention.IA_gate``, ``gct.GCT`` and ``conditioning_layer.*`` (which raise when a gradient is wanted) the way ``local_train`` stands beside
``matching_train``: the same constructors and parameter names, so a ``state_dict`` of the reference or of a mirror loads.

What PyTorch keeps and moves for the backward of ``y = a * x``: the activation, a full-size ``grad_y * x`` product that is written and read
again by the reduction, and a second read of ``grad_y`` for ``grad_x`` -- about six activation-sized streams.  The kernels of
csrc/gate_grad.hip move three:

    IA_gate             one pass reads grad_y and x, writes grad_x = gain grad_y and the plane dots dgain; then the [O, c] x [c, D] part
    GCT                 the plane dot; the gate's backward on [N, C]; one apply pass  grad_x = grad_y gate + dsum f'(x)
    conditioning_block  the plane dot; the two small backwards; one apply pass  grad_x = grad_y gain + (mask ? dgap : 0) / hw + dpx / hw

Saved for the backward: ``IA_gate`` x, the head and the [O, c] gain; ``GCT`` x, the plane sums and the gate; the conditioning modules x,
the scores [N, hw], the threshold [N], gap, px, the code and the gain.  No mask tensor is kept: the apply pass recomputes
``scores > threshold`` with the forward's strict ``>``.  The small gain comes from ``aoc_film_gain`` (one wave per channel), not from the fused
forward kernel's own dot product: the two differ in summation order only, and the tests' bounds cover it.

``phi_layer`` gets NO gradient: the reference compares the scores (``x > beta_val[..., -1, None]``, CLB:36), so its autograd leaves
``phi_layer.weight.grad`` and ``phi_layer.bias.grad`` at ``None``; so do these twins.

Without a wanted gradient (``ops._wants_grad``) every twin returns the mirror's result through the mirror's own ``ops`` calls;
with one, the forward calls the same entry points, so the output bits are the mirror's.  Frozen parameters and ``ctx.needs_input_grad``
select which optional outputs the kernels are asked for.  All backwards are ``once_differentiable``.  Every sum runs in a fixed order without
float atomics: two runs give the same bits.  The ctypes wrappers of the new entry points live here, not in ``ops`` (whose public names are
a tested table); they keep ``ops``' tensor contract through its helpers: inputs converted by ``_f32c`` / ``_opt`` into names that live until the
call, caller outputs checked by ``_out`` (the named optional ones chosen by ``_wanted``), addresses only through ``_p``.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .ops import _det, _new, _opt, _planes_hw, _wanted, _wants_grad


# ------------------------------------------------------------------------------------------ the C ABI
def channel_scale_backward(grad_y, x=None, gain=None, grad_x=None, dgain=None, want_x=True, want_gain=True):
    """aoc_channel_scale_grad: grad_y, x [N, C, ...], gain [N, C] -> (grad_x = gain * grad_y, dgain [N, C] = plane dots of grad_y and x);
    None where not wanted.  x may be None without want_gain, gain without want_x."""
    grad_y = ops._f32c(grad_y)
    x, gain = _opt(x), _opt(gain)
    ops._need_gpu(grad_y, x, gain, grad_x, dgain)
    planes, hw = _planes_hw("channel_scale_backward", grad_y)
    want_x, want_gain = bool(want_x or grad_x is not None), bool(want_gain or dgain is not None)
    if (want_gain and (x is None or x.shape != grad_y.shape)) or (want_x and (gain is None or gain.numel() != planes)):
        raise ValueError(f"channel_scale_backward: x / gain do not fit grad_y {tuple(grad_y.shape)}")
    if want_x:
        grad_x = torch.empty_like(grad_y) if grad_x is None else ops._out("channel_scale_backward: grad_x", grad_x, grad_y.shape)
    if want_gain:
        dgain = _new(grad_y, grad_y.shape[0], grad_y.shape[1]) if dgain is None else ops._out("channel_scale_backward: dgain", dgain, grad_y.shape[:2])
    _lib.check(_lib.lib().aoc_channel_scale_grad(ops._p(grad_y), ops._p(x), ops._p(gain), planes, hw, ops._p(grad_x), ops._p(dgain), ops._stream()),
               "aoc_channel_scale_grad")
    return grad_x, dgain


def film_gain_backward(dgain, gain, head, weight, grad_head=None, grad_weight=None, grad_bias=None, want=(True, True, True)):
    """aoc_film_gain_grad: dgain, gain [O, c], head [O, D], weight [c, D] -> (grad_head [O, D], grad_weight [c, D], grad_bias [c]); None where
    ``want`` is false and no buffer is given."""
    dgain, gain, head, weight = ops._f32c(dgain), ops._f32c(gain), ops._f32c(head), ops._f32c(weight)
    ops._need_gpu(dgain, gain, head, weight, grad_head, grad_weight, grad_bias)
    if dgain.dim() != 2 or head.dim() != 2 or weight.dim() != 2:
        raise ValueError("film_gain_backward: dgain [O, c], head [O, D] and weight [c, D] must be matrices")
    (n_obj, channels), D = dgain.shape, head.shape[1]
    if gain.shape != dgain.shape or tuple(head.shape) != (n_obj, D) or tuple(weight.shape) != (channels, D):
        raise ValueError(f"film_gain_backward: gain {tuple(gain.shape)}, head {tuple(head.shape)}, weight {tuple(weight.shape)} do not fit dgain "
                         f"{tuple(dgain.shape)}")
    grad_head, grad_weight, grad_bias = _wanted("film_gain_backward", ("grad_head", "grad_weight", "grad_bias"), ((n_obj, D), (channels, D), (channels,)),
                                                want, dict(grad_head=grad_head, grad_weight=grad_weight, grad_bias=grad_bias), dgain)
    _lib.check(_lib.lib().aoc_film_gain_grad(ops._p(dgain), ops._p(gain), ops._p(head), ops._p(weight), n_obj, D, channels, ops._p(grad_head),
                                             ops._p(grad_weight), ops._p(grad_bias), ops._stream()), "aoc_film_gain_grad")
    return grad_head, grad_weight, grad_bias


def gct_gate_backward(dgate, gate, plane_sums, alpha, gamma, beta, eps, l1_mode=False, dsum=None, grad_alpha=None, grad_gamma=None, grad_beta=None,
                      want=(True, True, True, True)):
    """aoc_gct_gate_grad: dgate, gate, plane_sums [N, C]; alpha, gamma, beta [C] (any shape of C elements) -> (dsum [N, C], grad_alpha,
    grad_gamma, grad_beta [C]); None where ``want`` is false and no buffer is given."""
    dgate, gate, plane_sums = ops._f32c(dgate), ops._f32c(gate), ops._f32c(plane_sums)
    al, ga, be = ops._f32c(alpha).reshape(-1), ops._f32c(gamma).reshape(-1), ops._f32c(beta).reshape(-1)      # bound until the launch is enqueued
    ops._need_gpu(dgate, gate, plane_sums, al, ga, be, dsum, grad_alpha, grad_gamma, grad_beta)
    if dgate.dim() != 2 or gate.shape != dgate.shape or plane_sums.shape != dgate.shape or not (al.numel() == ga.numel() == be.numel() == dgate.shape[1]):
        raise ValueError(f"gct_gate_backward: gate, plane_sums must be [N, C] = {tuple(dgate.shape)} and alpha, gamma, beta hold C elements")
    N, C = dgate.shape
    dsum, grad_alpha, grad_gamma, grad_beta = _wanted("gct_gate_backward", ("dsum", "grad_alpha", "grad_gamma", "grad_beta"), ((N, C), (C,), (C,), (C,)), want,
                                                      dict(dsum=dsum, grad_alpha=grad_alpha, grad_gamma=grad_gamma, grad_beta=grad_beta), dgate)
    _lib.check(_lib.lib().aoc_gct_gate_grad(ops._p(dgate), ops._p(gate), ops._p(plane_sums), ops._p(al), ops._p(ga), ops._p(be), N, C, float(eps),
                                            int(bool(l1_mode)), ops._p(dsum), ops._p(grad_alpha), ops._p(grad_gamma), ops._p(grad_beta), ops._stream()),
               "aoc_gct_gate_grad")
    return dsum, grad_alpha, grad_gamma, grad_beta


def gct_scale_backward(grad_y, x, gate, dsum, mode, grad_x=None):
    """aoc_gct_scale_grad: grad_x = grad_y * gate[plane] + dsum[plane] * f'(x); mode as ops.plane_reduce (0: 1, 1: 2x, 2: sign x)."""
    grad_y, x, gate, dsum = ops._f32c(grad_y), ops._f32c(x), ops._f32c(gate), ops._f32c(dsum)
    ops._need_gpu(grad_y, x, gate, dsum, grad_x)
    planes, hw = _planes_hw("gct_scale_backward", x)
    if grad_y.shape != x.shape or gate.numel() != planes or dsum.numel() != planes or int(mode) not in (0, 1, 2):
        raise ValueError(f"gct_scale_backward: grad_y {tuple(grad_y.shape)}, gate {tuple(gate.shape)}, dsum {tuple(dsum.shape)} or mode {mode} do not fit "
                         f"x {tuple(x.shape)}")
    grad_x = torch.empty_like(x) if grad_x is None else ops._out("gct_scale_backward: grad_x", grad_x, x.shape)
    _lib.check(_lib.lib().aoc_gct_scale_grad(ops._p(grad_y), ops._p(x), ops._p(gate), ops._p(dsum), int(mode), planes, hw, ops._p(grad_x), ops._stream()),
               "aoc_gct_scale_grad")
    return grad_x


_CODE_OUTS = ("dgap", "dpx", "grad_head", "grad_w1", "grad_b1", "grad_w2", "grad_b2", "grad_w3", "grad_b3")


def cond_codes_backward(dcode, gap, plane_means, head, w1, w2, w3, want=(True,) * 9, out=None):
    """aoc_cond_codes_grad: dcode [N, 2C + D], gap, plane_means [N, C], head [N, D], w1, w2 [C, C], w3 [D, D] -> the tuple (dgap, dpx, grad_head,
    grad_w1, grad_b1, grad_w2, grad_b2, grad_w3, grad_b3); None where ``want`` is false.  ``out``: a dict of caller buffers by those names.
    With C = 0 (gap, plane_means, w1, w2 = None) the third code alone is the backward of one square ``ops.linear``."""
    dcode, head, w3 = ops._f32c(dcode), ops._f32c(head), ops._f32c(w3)
    gap, plane_means, w1, w2 = _opt(gap), _opt(plane_means), _opt(w1), _opt(w2)
    out = dict(out or {})
    ops._need_gpu(dcode, gap, plane_means, head, w1, w2, w3, *out.values())
    if dcode.dim() != 2 or head.dim() != 2:
        raise ValueError("cond_codes_backward: dcode [N, 2C + D] and head [N, D] must be matrices")
    N, D = head.shape
    C = gap.shape[1] if gap is not None else 0
    have = tuple(tuple(t.shape) if t is not None else None for t in (dcode, gap, plane_means, w1, w2, w3))
    need = ((N, 2 * C + D),) + (((N, C), (N, C), (C, C), (C, C)) if C else (None,) * 4) + ((D, D),)
    if have != need:
        raise ValueError(f"cond_codes_backward: dcode, gap, plane_means, w1, w2, w3 must have shapes {need}, got {have}")
    shapes = ((N, C), (N, C), (N, D), (C, C), (C,), (C, C), (C,), (D, D), (D,))
    bufs = _wanted("cond_codes_backward", _CODE_OUTS, shapes, want, out, dcode)
    dgap, dpx, grad_head, grad_w1, grad_b1, grad_w2, grad_b2, grad_w3, grad_b3 = bufs
    _lib.check(_lib.lib().aoc_cond_codes_grad(ops._p(dcode), ops._p(gap), ops._p(plane_means), ops._p(head), ops._p(w1), ops._p(w2), ops._p(w3), N, C, D,
                                              ops._p(dgap), ops._p(dpx), ops._p(grad_head), ops._p(grad_w1), ops._p(grad_b1), ops._p(grad_w2),
                                              ops._p(grad_b2), ops._p(grad_w3), ops._p(grad_b3), ops._stream()), "aoc_cond_codes_grad")
    return bufs


def cond_scale_backward(grad_y, gain, scores, threshold, dgap, dpx, shape=None, grad_x=None):
    """aoc_cond_scale_grad: grad_x[n, c, p] = grad_y gain[n, c] + (scores[n, p] > threshold[n] ? dgap[n, c] : 0) / hw + dpx[n, c] / hw.  grad_y (with
    gain), dgap and dpx may each be None; ``shape`` = (N, C, ...) of grad_x is needed when grad_y is None."""
    scores, threshold = ops._f32c(scores), ops._f32c(threshold).reshape(-1)
    grad_y, gain, dgap, dpx = _opt(grad_y), _opt(gain), _opt(dgap), _opt(dpx)
    ops._need_gpu(grad_y, gain, scores, threshold, dgap, dpx, grad_x)
    shape = tuple(grad_y.shape if grad_y is not None else shape)
    if len(shape) < 2 or scores.dim() != 2:
        raise ValueError(f"cond_scale_backward: grad_x {shape} must be [N, C, ...] and scores [N, hw]")
    (N, C), hw = shape[:2], scores.shape[1]
    numel = 1
    for s in shape:
        numel *= s
    small = tuple(t.numel() for t in (gain, dgap, dpx) if t is not None)
    if scores.shape[0] != N or numel != N * C * hw or threshold.numel() != N or any(n != N * C for n in small) or (grad_y is not None and gain is None):
        raise ValueError(f"cond_scale_backward: scores {tuple(scores.shape)}, threshold, gain, dgap or dpx do not fit grad_x {shape}")
    grad_x = _new(scores, *shape) if grad_x is None else ops._out("cond_scale_backward: grad_x", grad_x, shape)
    _lib.check(_lib.lib().aoc_cond_scale_grad(ops._p(grad_y), ops._p(gain), ops._p(scores), ops._p(threshold), ops._p(dgap), ops._p(dpx), N, C, hw,
                                              ops._p(grad_x), ops._stream()), "aoc_cond_scale_grad")
    return grad_x


# ------------------------------------------------------------------------------------------ IA_gate
class _FilmScale(torch.autograd.Function):
    """x [O, c, ...], head [O, D], weight [c, D], bias [c] or None -> x * (1 + tanh(head W^T + b)) by aoc_film_scale; saves x, head, the gain."""

    @staticmethod
    def forward(ctx, x, head, weight, bias):
        xd, hd, wd = ops._f32c(x.detach()), ops._f32c(head.detach()), ops._f32c(weight.detach())
        bd = _det(bias)
        gain = ops.film_gain(hd, wd, bd)
        ctx.save_for_backward(xd, hd, wd, gain)
        return ops.film_scale(xd, hd, wd, bd)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        x, head, weight, gain = ctx.saved_tensors
        need_x, need_head, need_w, need_b = ctx.needs_input_grad
        small = need_head or need_w or need_b
        grad_x, dgain = channel_scale_backward(grad_y, x if small else None, gain, want_x=need_x, want_gain=small)
        gh = gw = gb = None
        if small:
            gh, gw, gb = film_gain_backward(dgain, gain, head, weight, want=(need_head, need_w, need_b))
        return grad_x, gh, gw, gb


class IA_gate(nn.Module):
    """ATT:7-17 with a backward for x, the head and ``IA``.  forward(x [O,c,h,w], IA_head [O,D]) -> x * (1 + tanh(IA(IA_head)))[:, :, None, None]"""

    def __init__(self, in_dim, out_dim):
        super(IA_gate, self).__init__()
        self.IA = nn.Linear(in_dim, out_dim)

    def forward(self, x, IA_head):
        if not _wants_grad(x, IA_head, self.IA.weight, self.IA.bias):
            return ops.film_scale(x, IA_head, self.IA.weight.detach(), self.IA.bias.detach())
        ops._need_gpu(x, IA_head, self.IA.weight, self.IA.bias)
        return _FilmScale.apply(x, IA_head, self.IA.weight, self.IA.bias)


# ------------------------------------------------------------------------------------------ GCT
class _Gct(torch.autograd.Function):
    """x [N, C, ...], alpha, gamma, beta [1, C, 1, 1] -> x * gate by aoc_plane_reduce, aoc_gct_gate, aoc_channel_scale; saves x, the plane sums
    and the gate."""

    @staticmethod
    def forward(ctx, x, alpha, gamma, beta, eps, reduce_mode, l1):
        xd = ops._f32c(x.detach())
        al, ga, be = alpha.detach(), gamma.detach(), beta.detach()
        sums = ops.plane_reduce(xd, reduce_mode)
        gate = ops.gct_gate(sums, al, ga, be, eps, l1)
        ctx.save_for_backward(xd, sums, gate, al, ga, be)
        ctx.cfg = (eps, reduce_mode, l1)
        return ops.channel_scale(xd, gate)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        x, sums, gate, al, ga, be = ctx.saved_tensors
        eps, reduce_mode, l1 = ctx.cfg
        need_x, need_al, need_ga, need_be = ctx.needs_input_grad[:4]
        grad_y = ops._f32c(grad_y)
        _, dgate = channel_scale_backward(grad_y, x, None, want_x=False, want_gain=True)
        dsum, g_al, g_ga, g_be = gct_gate_backward(dgate, gate, sums, al, ga, be, eps, l1, want=(need_x, need_al, need_ga, need_be))
        grad_x = gct_scale_backward(grad_y, x, gate, dsum, reduce_mode) if need_x else None
        return (grad_x,) + tuple(g.view(p.shape) if g is not None else None for g, p in ((g_al, al), (g_ga, ga), (g_be, be))) + (None, None, None)


class GCT(nn.Module):
    """Gated channel transformation, gct.py:7-36, with a backward for x, alpha, gamma and beta: y = x * (1 + tanh(embedding * norm + beta))."""

    def __init__(self, num_channels, epsilon=1e-5, mode='l2', after_relu=False):
        super(GCT, self).__init__()
        self.alpha = nn.Parameter(torch.ones(1, num_channels, 1, 1))
        self.gamma = nn.Parameter(torch.zeros(1, num_channels, 1, 1))
        self.beta = nn.Parameter(torch.zeros(1, num_channels, 1, 1))
        self.epsilon = epsilon
        self.mode = mode
        self.after_relu = after_relu

    def forward(self, x):
        if self.mode == 'l2':
            reduce_mode, l1 = 1, False                                     # gct.py:19
        elif self.mode == 'l1':
            reduce_mode, l1 = (0 if self.after_relu else 2), True          # gct.py:23-27
        else:
            raise ValueError("Unknown mode!")                               # gct.py:29-31 prints and exits
        if not _wants_grad(x, self.alpha, self.gamma, self.beta):
            sums = ops.plane_reduce(x, reduce_mode)
            gate = ops.gct_gate(sums, self.alpha.detach(), self.gamma.detach(), self.beta.detach(), self.epsilon, l1)
            return ops.channel_scale(x, gate)
        ops._need_gpu(x, self.alpha, self.gamma, self.beta)
        return _Gct.apply(x, self.alpha, self.gamma, self.beta, self.epsilon, reduce_mode, l1)


# ------------------------------------------------------------------------------------------ conditioning_layer, conditioning_block
def _beta_rank(beta_percentage, x):
    beta_rank = int(beta_percentage * x.size()[-1] * x.size()[-2])          # CL:32
    if beta_rank < 1:
        raise IndexError("conditioning_layer: beta_rank == 0 (the reference fails at beta_val[..., -1])")
    return beta_rank


class _Linear(torch.autograd.Function):
    """v [N, D] -> v W^T + b by aoc_linear for a square W (``mlp_layer`` of a conditioning_layer, CLB:19, 46); the backward is the third
    code of aoc_cond_codes_grad."""

    @staticmethod
    def forward(ctx, v, weight, bias):
        vd, wd, bd = ops._f32c(v.detach()), ops._f32c(weight.detach()), ops._f32c(bias.detach())
        if wd.shape[0] != wd.shape[1]:
            raise ValueError(f"conditioning_layer: mlp_layer must be square, got {tuple(wd.shape)}")
        ctx.save_for_backward(vd, wd)
        return ops.linear(vd, wd, bd)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        v, w = ctx.saved_tensors
        n = ctx.needs_input_grad
        g = cond_codes_backward(grad_y, None, None, v, None, None, w, want=(False, False, n[0], False, False, False, False, n[1], n[2]))
        return g[2], g[7], g[8]


class _GatePool(torch.autograd.Function):
    """z [N, C, h, w] -> gap [N, C] by aoc_cond_gate_pool_ex (CL:27-43); saves the scores and the threshold.  phi gets no gradient (CLB:36)."""

    @staticmethod
    def forward(ctx, z, phi_w, phi_b, k_rank):
        zd = ops._f32c(z.detach())
        gap, scores, thr = ops.cond_gate_pool(zd, phi_w.detach().reshape(-1), phi_b.detach(), k_rank, want_debug=True)
        ctx.save_for_backward(scores, thr)
        ctx.shape = tuple(zd.shape)
        return gap

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, dgap):
        scores, thr = ctx.saved_tensors
        return cond_scale_backward(None, None, scores, thr, dgap, None, shape=ctx.shape), None, None, None


class conditioning_layer(nn.Module):
    """Paper Eq. 7, CL:6-45, with a backward for the input and ``mlp_layer``.  ``phi_layer`` gets no gradient: CLB:36 compares the scores, so the
    reference's own autograd leaves ``phi_layer.weight.grad`` and ``phi_layer.bias.grad`` at None, and so does this twin."""

    def __init__(self, in_dim=256, beta_percentage=0.3):
        super(conditioning_layer, self).__init__()
        self.beta_percentage = beta_percentage
        kernel_size = 1
        self.phi_layer = nn.Conv2d(in_dim, 1, kernel_size=kernel_size, stride=1, padding=int((kernel_size - 1) / 2))
        self.mlp_layer = nn.Linear(in_dim, in_dim)
        nn.init.kaiming_normal_(self.phi_layer.weight, mode='fan_out', nonlinearity='relu')

    def forward(self, z_in):
        w, b = self.mlp_layer.weight, self.mlp_layer.bias
        wants = _wants_grad(z_in, w, b)
        if z_in.dim() == 2:                                   # vector input (conditioning_block repair): one linear
            if not wants:
                return ops.linear(z_in, w.detach(), b.detach())
            ops._need_gpu(z_in, w, b)
            return _Linear.apply(z_in, w, b)
        beta_rank = _beta_rank(self.beta_percentage, z_in)
        phi_w, phi_b = self.phi_layer.weight.detach().reshape(-1), self.phi_layer.bias.detach()
        if not wants:
            return ops.linear(ops.cond_gate_pool(z_in, phi_w, phi_b, beta_rank), w.detach(), b.detach())   # CL:46
        ops._need_gpu(z_in, w, b, phi_w, phi_b)
        return _Linear.apply(_GatePool.apply(z_in, phi_w, phi_b, beta_rank), w, b)


class _CondBlock(torch.autograd.Function):
    """CLB:66-86 by aoc_cond_gate_pool_ex, aoc_cond_codes and aoc_film_scale; saves x, scores, threshold, gap, px, the code, the gain."""

    @staticmethod
    def forward(ctx, x, head, phi_w, phi_b, k_rank, w1, b1, w2, b2, w3, b3, wm, bm):
        xd, hd = ops._f32c(x.detach()), ops._f32c(head.detach())
        w1, b1, w2, b2, w3, b3, wm, bm = (ops._f32c(t.detach()) for t in (w1, b1, w2, b2, w3, b3, wm, bm))
        gap, scores, thr, px = ops.cond_gate_pool(xd, phi_w.detach().reshape(-1), phi_b.detach(), k_rank, want_debug=True, want_plane_mean=True)
        code = ops.cond_codes(gap, px, hd, w1, b1, w2, b2, w3, b3)
        gain = ops.film_gain(code, wm, bm)
        ctx.save_for_backward(xd, hd, scores, thr, gap, px, code, gain, w1, w2, w3, wm)
        return ops.film_scale(xd, code, wm, bm)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        x, head, scores, thr, gap, px, code, gain, w1, w2, w3, wm = ctx.saved_tensors
        n = ctx.needs_input_grad
        need_x, need_head, params = n[0], n[1], n[5:13]                    # w1, b1, w2, b2, w3, b3, wm, bm
        grad_y = ops._f32c(grad_y)
        need_code = need_x or need_head or any(params[:6])
        g = (None,) * 9
        gwm = gbm = None
        if need_code or params[6] or params[7]:
            _, dgain = channel_scale_backward(grad_y, x, None, want_x=False, want_gain=True)
            dcode, gwm, gbm = film_gain_backward(dgain, gain, code, wm, want=(need_code, params[6], params[7]))
            if need_code:
                g = cond_codes_backward(dcode, gap, px, head, w1, w2, w3, want=(need_x, need_x, need_head) + tuple(params[:6]))
        grad_x = cond_scale_backward(grad_y, gain, scores, thr, g[0], g[1]) if need_x else None
        return (grad_x, g[2], None, None, None) + tuple(g[3:9]) + (gwm, gbm)


class conditioning_block(nn.Module):
    """Paper Eq. 5, CLB:50-86, with a backward for x, the proxy head, the three ``mlp_layer`` of CL_1..3 and the block's own.  The three
    ``phi_layer`` get no gradient (see ``conditioning_layer``); CL_2 / CL_3's are never read (the vector repair)."""

    def __init__(self, in_dim=256, proxy_dim=400, beta_percentage=0.3, attention_dim=None):
        super(conditioning_block, self).__init__()
        # decoding_module.py:27-50 constructs the blocks with ``attention_dim=`` (a keyword the reference's own class rejects, CLB:54):
        # accepted here as the width of the IA head, i.e. as ``proxy_dim``
        if attention_dim is not None:
            proxy_dim = attention_dim
        self.CL_1 = conditioning_layer(in_dim, beta_percentage)
        self.CL_2 = conditioning_layer(in_dim, beta_percentage)
        self.CL_3 = conditioning_layer(proxy_dim, 1)
        self.mlp_layer = nn.Linear(in_dim * 2 + proxy_dim, in_dim)

    def forward(self, x, proxy_IA_head):
        beta_rank = _beta_rank(self.CL_1.beta_percentage, x)
        phi_w, phi_b = self.CL_1.phi_layer.weight.detach().reshape(-1), self.CL_1.phi_layer.bias.detach()
        mlps = (self.CL_1.mlp_layer, self.CL_2.mlp_layer, self.CL_3.mlp_layer, self.mlp_layer)
        params = [t for m in mlps for t in (m.weight, m.bias)]
        if not _wants_grad(x, proxy_IA_head, *params):
            # CLB:68 (plane means of x) and CLB:72 / CL:28-45 (gate + masked pooling) from one pass, CLB:69-80 in one launch, CLB:81-84
            gap, px1 = ops.cond_gate_pool(x, phi_w, phi_b, beta_rank, want_plane_mean=True)
            code = ops.cond_codes(gap, px1, proxy_IA_head, *(t.detach() for t in params[:6]))
            return ops.film_scale(x, code, self.mlp_layer.weight.detach(), self.mlp_layer.bias.detach())
        ops._need_gpu(x, proxy_IA_head, phi_w, phi_b, *params)
        return _CondBlock.apply(x, proxy_IA_head, phi_w, phi_b, beta_rank, *params)
