"""Differentiable twin of ``networks/layers/aspp.py`` (``_ASPPModule``, ``ASPP``; decoding_module.py:53, :131).  It stands beside the inference
mirror ``aspp`` (which raises when a gradient is wanted) the way ``decoder_train`` stands beside ``gct.Bottleneck``: the reference's constructor
signatures, attribute and parameter names, so a ``state_dict`` of the reference or of the mirror loads strictly.

``ASPP.forward(x, fused=True)`` keeps the mirror's two fused stages and gives each a hand-written backward (csrc/aspp_grad.hip):

    front   four GCTs and the pooled mean read one x.  Backward: the four plane dots from one read of x (aoc_plane_dot_multi), the four
            gates' backward in one launch (aoc_gct_gate_multi_grad), one apply pass that writes grad_x from the four gradients, the summed
            dsum and the mean's cotangent (aoc_channel_scale_multi_grad_apply): x and the four gradients are read twice, grad_x written once.
    back    four GroupNorm + ReLU into the concatenation, gated in place by GCT(640).  Backward (aoc_groupnorm_cat_relu_grad): a plane pass,
            two small launches, an apply pass.  z, its mask and the concatenation are recomputed with the forward's own float expression;
            neither the ungated concatenation nor a gradient of it is stored.

Saved for the backward: x, the plane sums of squares and the four gates [4, N, C]; the four convolution outputs, the GroupNorm statistics,
the pooled ``tail`` [N, 128], the 640 plane sums and the 640 gate.  The five convolutions are torch's (MIOpen) with torch's own backward; the
pooled 1 x 1 product is ``ops.linear`` with its backward through ``gates_train.film_gain_backward`` at a unit gain (there da = dgain exactly,
so the entry is the backward of a plain product); ``bn1`` goes through ``decoder_train.groupnorm_relu``.  ``fused=False`` is the plain arm:
``gates_train.GCT`` + convolution + ``decoder_train.groupnorm_relu`` per branch, torch's ``cat``, ``gates_train.GCT`` for the 640 gate.

Without a wanted gradient the forward returns the mirror's result through the mirror's own calls; with one it calls the same C entry points,
so the output bits are the mirror's at the same ``fused`` flag.  Frozen parameters and ``ctx.needs_input_grad`` select which optional outputs
the kernels are asked for.  All backwards are ``once_differentiable``; every sum runs in a fixed order without float atomics.  The ctypes
wrappers of the new entry points live here, not in ``ops`` (whose public names are a tested table); they keep ``ops``' tensor contract through its
helpers: inputs converted by ``_f32c`` / ``_opt`` into names that live until the call, caller outputs checked by ``_out`` (the named optional
ones chosen by ``_wanted``), addresses only through ``_p`` / ``_addr``.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, aspp, decoder_train, gates_train, ops
from .ops import _det, _new, _opt, _planes_hw, _wanted, _wants_grad


# ------------------------------------------------------------------------------------------ the C ABI
def _same_shape_list(what, ts, like=None):
    ts = [ops._f32c(t) for t in ts]                              # converted copies stay bound (in the list) until the launch is enqueued
    if not 1 <= len(ts) <= 8:
        raise ValueError(f"{what}: {len(ts)} tensors in a pointer list (1 to 8)")
    shape = tuple(like.shape) if like is not None else tuple(ts[0].shape)
    if any(tuple(t.shape) != shape for t in ts):
        raise ValueError(f"{what}: the listed tensors {[tuple(t.shape) for t in ts]} do not all have shape {shape}")
    return ts


def plane_dot_multi(x, gs, dots=None):
    """aoc_plane_dot_multi: x [N, C, ...] and 1 to 8 tensors g_k of its shape -> dots [n_set, N, C], dots[k] = the plane dots of g_k and x;
    set k is bit-equal to ``gates_train.channel_scale_backward(g_k, x, want_x=False)``."""
    x = ops._f32c(x)
    planes, hw = _planes_hw("plane_dot_multi", x)
    gs = _same_shape_list("plane_dot_multi", gs, x)
    shape = (len(gs), x.shape[0], x.shape[1])
    if dots is not None:
        ops._out("plane_dot_multi: dots", dots, shape)
    ops._need_gpu(x, *gs, dots)
    dots = _new(x, *shape) if dots is None else dots
    _lib.check(_lib.lib().aoc_plane_dot_multi(ops._p(x), ops._ptr_array(gs), len(gs), planes, hw, ops._p(dots), ops._stream()), "aoc_plane_dot_multi")
    return dots


_GATE_OUTS = ("dsum_total", "dsum", "grad_alpha", "grad_gamma", "grad_beta")


def gct_gate_multi_backward(dgate, gate, plane_sums, alpha, gamma, beta, eps, l1_mode=False, want=(True, False, True, True, True), out=None):
    """aoc_gct_gate_multi_grad: dgate, gate [n_set, N, C]; plane_sums [N, C]; alpha, gamma, beta [n_set, C] tensors or lists of n_set per-GCT
    parameters -> the tuple (dsum_total [N, C], dsum [n_set, N, C], grad_alpha, grad_gamma, grad_beta [n_set, C]); None where ``want`` is false
    and ``out`` (a dict of caller buffers by those names) has no buffer.  Set k carries the bits of ``gates_train.gct_gate_backward`` with row k."""
    dgate, gate, plane_sums = ops._f32c(dgate), ops._f32c(gate), ops._f32c(plane_sums)
    if dgate.dim() != 3 or gate.shape != dgate.shape or tuple(plane_sums.shape) != tuple(dgate.shape[1:]):
        raise ValueError(f"gct_gate_multi_backward: dgate, gate must be [n_set, N, C] and plane_sums [N, C], got {tuple(dgate.shape)}, "
                         f"{tuple(gate.shape)}, {tuple(plane_sums.shape)}")
    n_set, N, C = dgate.shape
    al, ga, be = (ops._gct_rows("gct_gate_multi_backward", p, C) for p in (alpha, gamma, beta))      # bound until the launch is enqueued
    if not (al.shape[0] == ga.shape[0] == be.shape[0] == n_set):
        raise ValueError(f"gct_gate_multi_backward: {n_set} sets, parameters for {al.shape[0]}, {ga.shape[0]}, {be.shape[0]}")
    out = dict(out or {})
    ops._need_gpu(dgate, gate, plane_sums, al, ga, be, *out.values())
    bufs = _wanted("gct_gate_multi_backward", _GATE_OUTS, ((N, C), (n_set, N, C), (n_set, C), (n_set, C), (n_set, C)), want, out, dgate)
    L = _lib.lib()
    ws = ops._ws(L.aoc_gct_gate_multi_grad_workspace_bytes(n_set, N, C), dgate.device)
    _lib.check(L.aoc_gct_gate_multi_grad(ops._p(dgate), ops._p(gate), ops._p(plane_sums), ops._p(al), ops._p(ga), ops._p(be), n_set, N, C, float(eps),
                                         int(bool(l1_mode)), *(ops._p(b) for b in bufs), ops._p(ws), ws.numel(), ops._stream()), "aoc_gct_gate_multi_grad")
    return bufs


def channel_scale_multi_backward_apply(gs, gates, x, dsum_total, dmean=None, grad_x=None):
    """aoc_channel_scale_multi_grad_apply: grad_x = ((sum_k g_k * gates[k]) + (2 dsum_total) * x) + dmean / hw per plane, in that order (the
    header states it).  gs: 1 to 8 tensors shaped like x; gates [n_set, N, C]; dsum_total, dmean (or None) [N, C]."""
    x = ops._f32c(x)
    planes, hw = _planes_hw("channel_scale_multi_backward_apply", x)
    gs = _same_shape_list("channel_scale_multi_backward_apply", gs, x)
    gates, dsum_total = ops._f32c(gates), ops._f32c(dsum_total)
    dmean = _opt(dmean)
    if gates.numel() != len(gs) * planes or dsum_total.numel() != planes or (dmean is not None and dmean.numel() != planes):
        raise ValueError(f"channel_scale_multi_backward_apply: gates {tuple(gates.shape)}, dsum_total {tuple(dsum_total.shape)} or dmean do not fit "
                         f"{len(gs)} sets of x {tuple(x.shape)}")
    if grad_x is not None:
        ops._out("channel_scale_multi_backward_apply: grad_x", grad_x, x.shape)
    ops._need_gpu(x, gates, dsum_total, dmean, grad_x, *gs)
    grad_x = torch.empty_like(x) if grad_x is None else grad_x
    _lib.check(_lib.lib().aoc_channel_scale_multi_grad_apply(ops._ptr_array(gs), ops._p(gates), ops._p(x), ops._p(dsum_total), ops._p(dmean), len(gs), planes,
                                                             hw, ops._p(grad_x), ops._stream()), "aoc_channel_scale_multi_grad_apply")
    return grad_x


def _cat_args(what, xs, groups, gamma, beta, tail):
    xs = _same_shape_list(what, xs)
    if xs[0].dim() < 2 or xs[0].numel() == 0:
        raise ValueError(f"{what}: expected non-empty [N, C_src, ...] sources, got {tuple(xs[0].shape)}")
    N, C = xs[0].shape[0], xs[0].shape[1]
    groups = int(groups)
    if groups < 1 or C % groups:
        raise ValueError(f"{what}: {C} channels do not divide into {groups} groups")
    g = ops._gct_rows(what, gamma, C) if gamma is not None else None
    b = ops._gct_rows(what, beta, C) if beta is not None else None
    if any(t is not None and t.shape[0] != len(xs) for t in (g, b)):
        raise ValueError(f"{what}: {len(xs)} sources, affine parameters for {[t.shape[0] for t in (g, b) if t is not None]}")
    C_tail = 0
    if tail is not None:
        if tail.dim() < 2 or tail.shape[0] != N or tail.numel() != N * tail.shape[1]:
            raise ValueError(f"{what}: the tail {tuple(tail.shape)} is not [N = {N}, C_tail] (or [N, C_tail, 1, 1])")
        C_tail = tail.shape[1]
        tail = ops._f32c(tail)
    return xs, N, C, groups, g, b, tail, C_tail, xs[0].numel() // (N * C)


def groupnorm_cat_relu_forward(xs, groups, gamma, beta, eps=1e-5, tail=None):
    """ops.groupnorm_cat_relu(..., relu=True, want_plane_sumsq=True) keeping the statistics: -> (cat, plane_sumsq [N, C_total], stats
    [n_src, N * groups, 2] = (mean, rstd), a view of the call's workspace).  The same C entry as the mirror's wrapper, so cat has its bits."""
    xs, N, C, groups, g, b, tail, C_tail, hw = _cat_args("groupnorm_cat_relu_forward", xs, groups, gamma, beta, tail)
    ops._need_gpu(*xs, g, b, tail)
    n_src = len(xs)
    shape = (N, n_src * C + C_tail) + tuple(xs[0].shape[2:])
    L = _lib.lib()
    y = torch.empty(shape, dtype=torch.float32, device=xs[0].device)
    sq = _new(y, N, shape[1])
    ws = ops._ws(L.aoc_groupnorm_cat_relu_workspace_bytes(n_src, N, groups), y.device)
    _lib.check(L.aoc_groupnorm_cat_relu(ops._ptr_array(xs), n_src, N, C, hw, groups, ops._p(g), ops._p(b), float(eps), ops._p(tail), C_tail, 1, ops._p(y),
                                        ops._p(sq), ops._p(ws), ws.numel(), ops._stream()), "aoc_groupnorm_cat_relu")
    return y, sq, ws[:n_src * N * groups * 8].view(torch.float32).view(n_src, N * groups, 2)


_CAT_OUTS = ("grad_u", "grad_gamma", "grad_beta", "grad_tail", "grad_gct_alpha", "grad_gct_gamma", "grad_gct_beta")


def groupnorm_cat_relu_backward(grad_out, us, stats, groups, gamma, beta, tail, plane_sumsq, gate, gct_alpha, gct_gamma, gct_eps, want=None, out=None):
    """aoc_groupnorm_cat_relu_grad: grad_out [N, C_total, ...]; us: the n_src convolution outputs [N, C_src, ...]; stats as
    groupnorm_cat_relu_forward returns them; gamma, beta [n_src, C_src] (tensors, lists, or None); tail [N, C_tail] or None; plane_sumsq, gate
    [N, C_total]; gct_alpha, gct_gamma of C_total elements -> the tuple (grad_u: a list of n_src tensors or None each, grad_gamma, grad_beta
    [n_src, C_src], grad_tail [N, C_tail], grad_gct_alpha, grad_gct_gamma, grad_gct_beta [C_total]).  ``want``: seven flags, the first a flag
    or one flag per source (default: everything, grad_tail with a tail); ``out``: a dict of caller buffers by those names (grad_u: a list
    with None for a source that is not wanted)."""
    what = "groupnorm_cat_relu_backward"
    us, N, C, groups, g, b, tail, C_tail, hw = _cat_args(what, us, groups, gamma, beta, tail)
    n_src = len(us)
    C_total = n_src * C + C_tail
    grad_out, stats, plane_sumsq, gate = ops._f32c(grad_out), ops._f32c(stats), ops._f32c(plane_sumsq), ops._f32c(gate)
    al, ga = ops._f32c(gct_alpha).reshape(-1), ops._f32c(gct_gamma).reshape(-1)                    # bound until the launch is enqueued
    if tuple(grad_out.shape) != (N, C_total) + tuple(us[0].shape[2:]):
        raise ValueError(f"{what}: grad_out {tuple(grad_out.shape)} is not the concatenation of {n_src} sources {tuple(us[0].shape)} and {C_tail} tail channels")
    if stats.numel() != n_src * N * groups * 2 or plane_sumsq.numel() != N * C_total or gate.numel() != N * C_total or al.numel() != C_total or \
            ga.numel() != C_total:
        raise ValueError(f"{what}: stats must hold {n_src * N * groups} (mean, rstd) pairs, plane_sumsq and gate {N * C_total} and the GCT's alpha, gamma "
                         f"{C_total} elements")
    if want is None:
        want = (True, True, True, C_tail > 0, True, True, True)
    want_u = [bool(want[0])] * n_src if isinstance(want[0], (bool, int)) else [bool(w) for w in want[0]]
    out = dict(out or {})
    if set(out) - set(_CAT_OUTS) or len(want_u) != n_src:
        raise ValueError(f"{what}: unknown outputs {sorted(set(out) - set(_CAT_OUTS))} or {len(want_u)} flags for {n_src} sources")
    if "grad_u" in out:
        if len(out["grad_u"]) != n_src:
            raise ValueError(f"{what}: out['grad_u'] must list {n_src} buffers (None where not wanted)")
        grad_u = [ops._out(f"{what}: grad_u[{k}]", t, us[0].shape) if t is not None else None for k, t in enumerate(out["grad_u"])]
    else:
        grad_u = [torch.empty_like(us[0]) if w else None for w in want_u]
    shapes = ((n_src, C), (n_src, C), (N, C_tail), (C_total,), (C_total,), (C_total,))
    small = _wanted(what, _CAT_OUTS[1:], shapes, want[1:], {k: v for k, v in out.items() if k != "grad_u"}, grad_out)
    ops._need_gpu(grad_out, stats, plane_sumsq, gate, al, ga, g, b, tail, *us, *grad_u, *small)
    L = _lib.lib()
    ws = ops._ws(L.aoc_groupnorm_cat_relu_grad_workspace_bytes(n_src, N, C, C_tail, groups), grad_out.device)
    _lib.check(L.aoc_groupnorm_cat_relu_grad(ops._p(grad_out), ops._ptr_array(us), n_src, N, C, hw, groups, ops._p(stats), ops._p(g), ops._p(b), ops._p(tail),
                                             C_tail, ops._p(plane_sumsq), ops._p(gate), ops._p(al), ops._p(ga), float(gct_eps), ops._ptr_array(grad_u),
                                             *(ops._p(t) for t in small), ops._p(ws), ws.numel(), ops._stream()), "aoc_groupnorm_cat_relu_grad")
    return (grad_u,) + small


# ------------------------------------------------------------------------------------------ the fused stages
class _GateInputs(torch.autograd.Function):
    """x [N, C, ...], then n_set alphas, n_set gammas, n_set betas ([1, C, 1, 1]) -> (GCT_0(x), ..., GCT_{n_set-1}(x), plane means [N, C]) by
    aoc_plane_sum_sumsq, aoc_gct_gate_multi, aoc_channel_scale_multi (``aspp.gate_inputs``' calls); saves x, the plane sums of squares, the gates."""

    @staticmethod
    def forward(ctx, x, eps, n_set, *params):
        xd = _det(x)
        al, ga, be = (torch.stack([p.detach().reshape(-1) for p in params[i * n_set:(i + 1) * n_set]]) for i in range(3))
        _, sumsq, mean = ops.plane_sum_sumsq(xd, want_sum=False)
        gates = ops.gct_gate_multi(sumsq, al, ga, be, eps, False)
        ctx.save_for_backward(xd, sumsq, gates, al, ga, be)
        ctx.cfg = (float(eps), int(n_set), tuple(p.shape for p in params))
        return tuple(ops.channel_scale_multi(xd, gates)) + (mean,)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, *grads):
        x, sumsq, gates, al, ga, be = ctx.saved_tensors
        eps, n_set, shapes = ctx.cfg
        need = ctx.needs_input_grad
        need_x, need_p = need[0], need[3:]
        gs, dmean = [ops._f32c(g) for g in grads[:n_set]], grads[n_set]
        want = (need_x, False) + tuple(any(need_p[i * n_set:(i + 1) * n_set]) for i in range(3))
        grad_x, small = None, (None,) * 5
        if any(want):
            dots = plane_dot_multi(x, gs)
            small = gct_gate_multi_backward(dots, gates, sumsq, al, ga, be, eps, False, want=want)
        if need_x:
            grad_x = channel_scale_multi_backward_apply(gs, gates, x, small[0], dmean)
        gp = []
        for i, rows in enumerate(small[2:]):
            for k in range(n_set):
                j = i * n_set + k
                gp.append(rows[k].view(shapes[j]) if (rows is not None and need_p[j]) else None)
        return (grad_x, None, None) + tuple(gp)


class _Merge(torch.autograd.Function):
    """``aspp.merge`` with a backward: n_src convolution outputs, n_src GroupNorm weights, n_src biases, the pooled tail [N, C_tail] (before its
    ReLU), alpha, gamma, beta of the concatenation's GCT -> GCT(cat) by aoc_groupnorm_cat_relu, aoc_gct_gate, aoc_channel_scale (in place);
    saves the convolution outputs, the statistics, the tail, the plane sums of squares and the gate."""

    @staticmethod
    def forward(ctx, groups, gn_eps, gct_eps, n_src, tail, alpha, gamma, beta, *rest):
        us = [_det(u) for u in rest[:n_src]]
        gn_w = torch.stack([p.detach().reshape(-1) for p in rest[n_src:2 * n_src]])
        gn_b = torch.stack([p.detach().reshape(-1) for p in rest[2 * n_src:3 * n_src]])
        td, al, ga, be = _det(tail), alpha.detach(), gamma.detach(), beta.detach()
        cat, sumsq, stats = groupnorm_cat_relu_forward(us, groups, gn_w, gn_b, gn_eps, td)
        gate = ops.gct_gate(sumsq, al, ga, be, gct_eps, False)
        ctx.save_for_backward(td, sumsq, gate, stats, gn_w, gn_b, al, ga, *us)
        ctx.cfg = (int(groups), float(gct_eps), int(n_src), tuple(p.shape for p in rest[n_src:3 * n_src]), alpha.shape, tail.shape)
        return ops.channel_scale(cat, gate, out=cat)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_out):
        td, sumsq, gate, stats, gn_w, gn_b, al, ga = ctx.saved_tensors[:8]
        us = list(ctx.saved_tensors[8:])
        groups, gct_eps, n_src, shapes, gct_shape, tail_shape = ctx.cfg
        need = ctx.needs_input_grad
        need_tail, need_gct, need_rest = need[4], need[5:8], need[8:]
        need_u, need_w, need_b = need_rest[:n_src], need_rest[n_src:2 * n_src], need_rest[2 * n_src:3 * n_src]
        want = (tuple(need_u), any(need_w), any(need_b), need_tail) + tuple(need_gct)
        gu, gw, gb, gt, g_al, g_ga, g_be = groupnorm_cat_relu_backward(grad_out, us, stats, groups, gn_w, gn_b, td, sumsq, gate, al, ga, gct_eps, want=want)
        rows = lambda t, flags, shp: [t[k].view(shp[k]) if (t is not None and flags[k]) else None for k in range(n_src)]
        gct = tuple(t.view(gct_shape) if t is not None else None for t in (g_al, g_ga, g_be))
        return (None, None, None, None, gt.view(tail_shape) if gt is not None else None) + gct + tuple(gu) + tuple(rows(gw, need_w, shapes[:n_src])) + \
            tuple(rows(gb, need_b, shapes[n_src:]))


class _PooledLinear(torch.autograd.Function):
    """mean [N, C] x weight [O, C] -> mean W^T by aoc_linear (aspp.py:61 without its ReLU: the 1 x 1 convolution of a 1 x 1 map).  The backward is
    aoc_film_gain_grad at a unit gain: there da = dgain * (1 - 0 * 0) = dgain exactly, and the entry returns dgain W and dgain^T mean."""

    @staticmethod
    def forward(ctx, mean, weight):
        md, wd = _det(mean), _det(weight)
        ctx.save_for_backward(md, wd)
        return ops.linear(md, wd, None)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        mean, weight = ctx.saved_tensors
        grad_y = ops._f32c(grad_y)
        gm, gw, _ = gates_train.film_gain_backward(grad_y, torch.ones_like(grad_y), mean, weight, want=(ctx.needs_input_grad[0], ctx.needs_input_grad[1], False))
        return gm, gw


class _PlaneMean(torch.autograd.Function):
    """x [N, C, h, w] -> its plane means [N, C] by aoc_plane_mean (aspp.py:46; the plain arm).  The backward is the broadcast grad / hw, written by
    aoc_cond_scale_grad with nothing but its dpx term (no gated gradient, an empty mask).  That entry reads a score row per sample, so the
    backward allocates and reads a zero [N, hw] tensor (1 / C of the activation) for a mask that is never set: the price of staying on an
    existing entry in the arm that is not the default.  The fused arm adds the mean's share inside aoc_channel_scale_multi_grad_apply."""

    @staticmethod
    def forward(ctx, x):
        xd = _det(x)
        ctx.shape = tuple(xd.shape)
        return ops.plane_mean(xd)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_mean):
        N, C = ctx.shape[:2]
        hw = 1
        for s in ctx.shape[2:]:
            hw *= s
        scores = torch.zeros(N, hw, dtype=torch.float32, device=grad_mean.device)
        thr = torch.zeros(N, dtype=torch.float32, device=grad_mean.device)
        return gates_train.cond_scale_backward(None, None, scores, thr, None, grad_mean, shape=ctx.shape)


def _pooled(mean, conv):
    w = conv.weight
    return _PooledLinear.apply(mean, w.view(w.shape[0], w.shape[1]))


# ------------------------------------------------------------------------------------------ the modules
class _ASPPModule(nn.Module):
    """aspp.py:7-31 with a backward: GCT -> atrous convolution -> GroupNorm(planes / 4) -> ReLU."""

    def __init__(self, inplanes, planes, kernel_size, padding, dilation):
        super(_ASPPModule, self).__init__()
        self.GCT = gates_train.GCT(inplanes)
        self.atrous_conv = nn.Conv2d(inplanes, planes, kernel_size=kernel_size, stride=1, padding=padding, dilation=dilation, bias=False)
        self.bn = nn.GroupNorm(int(planes / 4), planes)
        self.relu = nn.ReLU(inplace=True)
        self._init_weight()

    def forward(self, x):
        x = self.atrous_conv(self.GCT(x))                                                 # aspp.py:19-20
        return decoder_train.groupnorm_relu(x, self.bn.num_groups, self.bn.weight, self.bn.bias, self.bn.eps)      # :21-23

    def _init_weight(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight)


class ASPP(nn.Module):
    """aspp.py:33-78 with a backward for x and every parameter."""

    def __init__(self):
        super(ASPP, self).__init__()
        inplanes = 512
        dilations = [1, 6, 12, 18]
        self.aspp1 = _ASPPModule(inplanes, 128, 1, padding=0, dilation=dilations[0])
        self.aspp2 = _ASPPModule(inplanes, 128, 3, padding=dilations[1], dilation=dilations[1])
        self.aspp3 = _ASPPModule(inplanes, 128, 3, padding=dilations[2], dilation=dilations[2])
        self.aspp4 = _ASPPModule(inplanes, 128, 3, padding=dilations[3], dilation=dilations[3])
        self.global_avg_pool = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)),
                                             nn.Conv2d(inplanes, 128, 1, stride=1, bias=False),
                                             nn.ReLU(inplace=True))
        self.GCT = gates_train.GCT(640)
        self.conv1 = nn.Conv2d(640, 256, 1, bias=False)
        self.bn1 = nn.GroupNorm(32, 256)
        self.relu = nn.ReLU(inplace=True)
        self._init_weight()

    def _mirror(self, x, fused):
        """The mirror's forward on this module's parameters (``aspp.ASPP.forward``'s own calls): the result without a wanted gradient."""
        det = lambda p: p.detach()
        branches = (self.aspp1, self.aspp2, self.aspp3, self.aspp4)
        w = self.global_avg_pool[1].weight.detach()
        pooled = lambda mean: ops.linear(mean, w.view(w.shape[0], w.shape[1]), None)
        if fused:
            gated, mean = aspp.gate_inputs(x, [b.GCT for b in branches])
            convs = [b.atrous_conv(g) for b, g in zip(branches, gated)]
            x = aspp.merge(convs, [b.bn for b in branches], pooled(mean), self.GCT)
        else:
            outs = [ops.groupnorm_relu(b.atrous_conv(b.GCT(x)), b.bn.num_groups, det(b.bn.weight), det(b.bn.bias), b.bn.eps) for b in branches]
            x5 = torch.relu(pooled(ops.plane_mean(x)))
            x5 = x5[:, :, None, None].expand(-1, -1, *outs[0].shape[2:])
            x = self.GCT(torch.cat(outs + [x5], dim=1))
        return ops.groupnorm_relu(self.conv1(x), self.bn1.num_groups, det(self.bn1.weight), det(self.bn1.bias), self.bn1.eps)

    def forward(self, x, fused=True):
        if not _wants_grad(x, *self.parameters()):
            with torch.no_grad():
                return self._mirror(x, fused)
        ops._need_gpu(x, *self.parameters())
        branches = (self.aspp1, self.aspp2, self.aspp3, self.aspp4)
        if fused:
            gcts, bns = [b.GCT for b in branches], [b.bn for b in branches]
            if any(g.mode != 'l2' or g.epsilon != gcts[0].epsilon for g in gcts) or self.GCT.mode != 'l2':
                raise ValueError("aspp_train.ASPP: the fused stages take l2-mode GCTs with one epsilon (aspp.py:10, :50)")
            if any(b.num_groups != bns[0].num_groups or b.eps != bns[0].eps for b in bns):
                raise ValueError("aspp_train.ASPP: the branches' GroupNorms share one group count and one eps (aspp.py:13)")
            params = [getattr(g, k) for k in ("alpha", "gamma", "beta") for g in gcts]
            *gated, mean = _GateInputs.apply(x, gcts[0].epsilon, len(gcts), *params)      # aspp.py:19 x 4, :46
            convs = [b.atrous_conv(g) for b, g in zip(branches, gated)]                   # :20 x 4
            tail = _pooled(mean, self.global_avg_pool[1])                                 # :61 without its ReLU
            x = _Merge.apply(bns[0].num_groups, bns[0].eps, self.GCT.epsilon, len(convs), tail, self.GCT.alpha, self.GCT.gamma, self.GCT.beta, *convs,
                             *(b.weight for b in bns), *(b.bias for b in bns))            # :21-23 x 4, :61-65
        else:
            outs = [b(x) for b in branches]                                               # :57-60
            x5 = torch.relu(_pooled(_PlaneMean.apply(x), self.global_avg_pool[1]))        # :61
            # :62: bilinear interpolation from a 1 x 1 map with align_corners=True repeats the value
            x5 = x5[:, :, None, None].expand(-1, -1, *outs[0].shape[2:])
            x = self.GCT(torch.cat(outs + [x5], dim=1))                                   # :63, :65
        x = self.conv1(x)                                                                 # :66
        return decoder_train.groupnorm_relu(x, self.bn1.num_groups, self.bn1.weight, self.bn1.bias, self.bn1.eps)      # :67-68

    def _init_weight(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight)
