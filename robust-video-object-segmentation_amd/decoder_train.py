"""Differentiable twins of the decoder's fused forms: ``Bottleneck`` (networks/layers/gct.py:38-90) and the memory block of
``CalibrationDecoding`` (networks/aoc/decoding_module.py:133-140, 192-210: ``Modulator_1``, ``Modulator_2``, ``modulate``).  They stand beside the
inference mirrors ``gct.Bottleneck`` and ``decoder_memory.*`` (which raise when a gradient is wanted) the way ``gates_train`` stands beside
``attention`` / ``conditioning_layer``: the same constructors and parameter names, so a ``state_dict`` of the reference or of a mirror loads,
and the same binding onto the reference's decoder class.

What PyTorch keeps and moves for ``gain * relu(F.group_norm(x) + residual)``: the normalised tensor, the sum, the activation and the gated
product, each written forward and read again backward.  The kernels of csrc/norm_grad.hip save x, the residual, the statistics
[N * groups][2] and the [N, C] gain, and move the three streams (grad_y, x, residual) twice backward:

    GroupNorm (+ residual) (+ ReLU) (+ gate)   a plane pass (A = sum dz, B = sum dz xhat, dgain = sum grad_y a), one small launch (group
                                               sums, grad_gamma, grad_beta), one apply pass (grad_x, grad_residual); z and its ReLU mask
                                               are recomputed with the forward's own expression, nothing of activation size is stored
    cat + gate                                 one pass: grad_x = gain grad_y on the x half, the plane dots of grad_y with [x | mem]

and the small [N, C] x [C, D] part of a gate goes through ``gates_train.film_gain_backward``.  The convolutions stay torch's (MIOpen), with
torch's own backward.

Without a wanted gradient every function here returns the mirror's result through the mirror's own ``ops`` calls; with one, the forward
calls the same C entry points, so the output bits are the mirror's.  The gain that is saved comes from ``aoc_film_gain``, not from the fused
forward kernel's own dot product (summation order only; the tests' bounds cover it), as in ``gates_train``.  Frozen parameters and
``ctx.needs_input_grad`` select which optional outputs the kernels are asked for.  All backwards are ``once_differentiable``; every sum runs
in a fixed order without float atomics.  The ctypes wrappers of the two new entry points live here, not in ``ops`` (whose public names are a
tested table); they keep ``ops``' tensor contract through its helpers: inputs converted by ``_f32c`` / ``_opt`` / ``_vec`` into names that live
until the call, caller outputs checked by ``_out`` (the named optional ones chosen by ``_wanted``), addresses only through ``_p``.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, gates_train, ops
from .decoder_memory import select_memory
from .ops import _det, _opt, _planes_hw, _vec, _wanted, _wants_grad


# ------------------------------------------------------------------------------------------ the C ABI
def _gn_shape(what, x, groups):
    _, hw = _planes_hw(what, x)
    N, C = x.shape[0], x.shape[1]
    if int(groups) < 1 or C % int(groups):
        raise ValueError(f"{what}: {C} channels do not divide into {groups} groups")
    return N, C, hw


def groupnorm_relu_forward(x, groups, gamma, beta, eps=1e-5, residual=None, relu=True, gate=None):
    """ops.groupnorm_relu, or with ``gate`` = (head, weight, bias) ops.groupnorm_relu_scale, keeping the statistics: -> (y, stats
    [N * groups, 2] = (mean, rstd), a view of the call's workspace).  The same C entries as the mirror's wrappers, so y has their bits."""
    x, residual = ops._f32c(x), _opt(residual)
    g, b = _vec(gamma), _vec(beta)                                # bound until the launch is enqueued
    head = weight = bias = None
    if gate is not None:
        head, weight = ops._f32c(gate[0]), ops._f32c(gate[1])
        bias = _vec(gate[2])
    N, C, hw = _gn_shape("groupnorm_relu_forward", x, groups)
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"groupnorm_relu_forward: residual {tuple(residual.shape)} does not fit x {tuple(x.shape)}")
    if any(t is not None and t.numel() != C for t in (g, b)):
        raise ValueError(f"groupnorm_relu_forward: gamma / beta must hold {C} elements")
    if gate is not None:
        ops._gate_shapes("groupnorm_relu_forward", N, C, head, weight, bias)
    ops._need_gpu(x, residual, g, b, head, weight, bias)
    L = _lib.lib()
    y = torch.empty_like(x)
    ws = ops._ws(L.aoc_groupnorm_relu_workspace_bytes(N, int(groups)), x.device)
    if gate is None:
        _lib.check(L.aoc_groupnorm_relu(ops._p(x), N, C, hw, int(groups), ops._p(g), ops._p(b), float(eps), ops._p(residual), int(bool(relu)), ops._p(y),
                                        ops._p(ws), ws.numel(), ops._stream()), "aoc_groupnorm_relu")
    else:
        _lib.check(L.aoc_groupnorm_relu_scale(ops._p(x), N, C, hw, int(groups), ops._p(g), ops._p(b), float(eps), ops._p(residual), int(bool(relu)),
                                              ops._p(head), ops._p(weight), ops._p(bias), head.shape[1], ops._p(y), ops._p(ws), ws.numel(), ops._stream()),
                   "aoc_groupnorm_relu_scale")
    return y, ws[:N * int(groups) * 8].view(torch.float32).view(N * int(groups), 2)


_GN_OUTS = ("grad_x", "grad_residual", "grad_gamma", "grad_beta", "dgain")


def groupnorm_relu_backward(grad_y, x, stats, groups, gamma=None, beta=None, residual=None, relu=True, gain=None, want=None, out=None):
    """aoc_groupnorm_relu_grad: grad_y, x, residual [N, C, ...]; stats [N * groups, 2] (mean, rstd) as groupnorm_relu_forward returns them; gamma,
    beta of C elements or None; gain [N, C] or None -> the tuple (grad_x, grad_residual, grad_gamma [C], grad_beta [C], dgain [N, C]); None
    where ``want`` (five flags; default: all, grad_residual with a residual, dgain with a gain) is false.  ``out``: a dict of caller buffers by
    those names."""
    grad_y, x, stats = ops._f32c(grad_y), ops._f32c(x), ops._f32c(stats)
    residual, gain = _opt(residual), _opt(gain)
    g, b = _vec(gamma), _vec(beta)                                # bound until the launch is enqueued
    out = dict(out or {})
    ops._need_gpu(grad_y, x, stats, residual, gain, g, b, *out.values())
    N, C, hw = _gn_shape("groupnorm_relu_backward", x, groups)
    groups = int(groups)
    if grad_y.shape != x.shape or (residual is not None and residual.shape != x.shape):
        raise ValueError(f"groupnorm_relu_backward: grad_y {tuple(grad_y.shape)} or the residual does not fit x {tuple(x.shape)}")
    if stats.numel() != N * groups * 2 or (gain is not None and gain.numel() != N * C) or any(t is not None and t.numel() != C for t in (g, b)):
        raise ValueError(f"groupnorm_relu_backward: stats must hold {N * groups} (mean, rstd) pairs, gain {N * C} and gamma, beta {C} elements")
    if want is None:
        want = (True, residual is not None, True, True, gain is not None)
    bufs = _wanted("groupnorm_relu_backward", _GN_OUTS, (tuple(x.shape), tuple(x.shape), (C,), (C,), (N, C)), want, out, x)
    grad_x, grad_residual, grad_gamma, grad_beta, dgain = bufs
    L = _lib.lib()
    ws = ops._ws(L.aoc_groupnorm_relu_grad_workspace_bytes(N, C, groups), x.device)
    _lib.check(L.aoc_groupnorm_relu_grad(ops._p(grad_y), ops._p(x), ops._p(residual), ops._p(stats), ops._p(g), ops._p(b), ops._p(gain), N, C, hw, groups,
                                         int(bool(relu)), ops._p(grad_x), ops._p(grad_residual), ops._p(grad_gamma), ops._p(grad_beta), ops._p(dgain),
                                         ops._p(ws), ws.numel(), ops._stream()), "aoc_groupnorm_relu_grad")
    return bufs


def cat_film_scale_backward(grad_y, x=None, mem=None, gain=None, grad_x=None, grad_mem=None, dgain=None, want_x=True, want_mem=False, want_gain=True):
    """aoc_cat_film_scale_grad: grad_y [O, Cx + Cm, ...], x [O, Cx, ...], mem [O, Cm, ...] (may be x itself, or None), gain [O, Cx + Cm] ->
    (grad_x = gain[:, :Cx] grad_y[:, :Cx], grad_mem likewise for the memory's channels, dgain = the plane dots of grad_y with [x | mem]);
    None where not wanted.  x and mem are read for dgain only, and only their shapes otherwise."""
    grad_y = ops._f32c(grad_y)
    x, mem, gain = _opt(x), _opt(mem), _opt(gain)
    ops._need_gpu(grad_y, x, mem, gain, grad_x, grad_mem, dgain)
    want_x, want_mem, want_gain = bool(want_x or grad_x is not None), bool(want_mem or grad_mem is not None), bool(want_gain or dgain is not None)
    if grad_y.dim() < 2 or grad_y.numel() == 0 or x is None or x.dim() != grad_y.dim():
        raise ValueError("cat_film_scale_backward: grad_y [O, Cx + Cm, ...] and x [O, Cx, ...] are needed (x for its shape at least)")
    O, Ct = grad_y.shape[0], grad_y.shape[1]
    Cx = x.shape[1]
    Cm = mem.shape[1] if mem is not None else 0
    rest = tuple(grad_y.shape[2:])
    if x.shape[0] != O or tuple(x.shape[2:]) != rest or Cx + Cm != Ct or (mem is not None and (mem.shape[0] != O or tuple(mem.shape[2:]) != rest)):
        raise ValueError(f"cat_film_scale_backward: x {tuple(x.shape)} and the memory {tuple(mem.shape) if mem is not None else None} do not "
                         f"concatenate to grad_y {tuple(grad_y.shape)}")
    if ((want_x or want_mem) and (gain is None or gain.numel() != O * Ct)) or (want_mem and Cm < 1):
        raise ValueError(f"cat_film_scale_backward: gain must hold {O * Ct} elements (and grad_mem needs a memory)")
    hw = grad_y.numel() // (O * Ct)
    if want_x:
        grad_x = torch.empty_like(x) if grad_x is None else ops._out("cat_film_scale_backward: grad_x", grad_x, x.shape)
    if want_mem:
        grad_mem = torch.empty_like(mem) if grad_mem is None else ops._out("cat_film_scale_backward: grad_mem", grad_mem, mem.shape)
    if want_gain:
        dgain = torch.empty(O, Ct, dtype=torch.float32, device=grad_y.device) if dgain is None else ops._out("cat_film_scale_backward: dgain", dgain, (O, Ct))
    _lib.check(_lib.lib().aoc_cat_film_scale_grad(ops._p(grad_y), ops._p(x), ops._p(mem), ops._p(gain), O, Cx, Cm, hw, ops._p(grad_x), ops._p(grad_mem),
                                                  ops._p(dgain), ops._stream()), "aoc_cat_film_scale_grad")
    return grad_x, grad_mem, dgain


# ------------------------------------------------------------------------------------------ the fused forms
class _GroupNormRelu(torch.autograd.Function):
    """x, residual [N, C, ...], gamma, beta [C] -> [relu](GroupNorm(x) gamma + beta [+ residual]) by aoc_groupnorm_relu; saves x, the residual
    and the statistics."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, groups, eps, relu):
        xd, ga, be, rd = _det(x), _det(gamma), _det(beta), _det(residual)
        y, stats = groupnorm_relu_forward(xd, groups, ga, be, eps, rd, relu)
        ctx.save_for_backward(xd, rd, stats, ga, be)
        ctx.cfg = (int(groups), bool(relu))
        return y

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        x, residual, stats, ga, be = ctx.saved_tensors
        groups, relu = ctx.cfg
        need_x, need_ga, need_be, need_r = ctx.needs_input_grad[:4]
        gx, gr, gg, gb, _ = groupnorm_relu_backward(grad_y, x, stats, groups, ga, be, residual, relu, None,
                                                     want=(need_x, need_r and residual is not None, need_ga, need_be, False))
        return gx, gg, gb, gr, None, None, None


class _GroupNormReluScale(torch.autograd.Function):
    """_GroupNormRelu with the IA_gate behind it folded in (aoc_groupnorm_relu_scale): head [N, D], weight [C, D], bias [C] or None; saves x,
    the residual, the statistics, the [N, C] gain (aoc_film_gain), the head and the weight."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, head, weight, bias, groups, eps, relu):
        xd, ga, be, rd = _det(x), _det(gamma), _det(beta), _det(residual)
        hd, wd, bd = _det(head), _det(weight), _det(bias)
        gain = ops.film_gain(hd, wd, bd)
        y, stats = groupnorm_relu_forward(xd, groups, ga, be, eps, rd, relu, gate=(hd, wd, bd))
        ctx.save_for_backward(xd, rd, stats, ga, be, gain, hd, wd)
        ctx.cfg = (int(groups), bool(relu))
        return y

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        x, residual, stats, ga, be, gain, head, weight = ctx.saved_tensors
        groups, relu = ctx.cfg
        need_x, need_ga, need_be, need_r, need_head, need_w, need_b = ctx.needs_input_grad[:7]
        small = need_head or need_w or need_b
        gx, gr, gg, gb, dgain = groupnorm_relu_backward(grad_y, x, stats, groups, ga, be, residual, relu, gain,
                                                         want=(need_x, need_r and residual is not None, need_ga, need_be, small))
        gh = gw = gbias = None
        if small:
            gh, gw, gbias = gates_train.film_gain_backward(dgain, gain, head, weight, want=(need_head, need_w, need_b))
        return gx, gg, gb, gr, gh, gw, gbias, None, None, None


class _CatFilmScale(torch.autograd.Function):
    """x [O, Cx, ...], mem [O, Cm, ...] or None, head [O, D], weight [Cx + Cm, D], bias or None -> cat([x, mem], 1) * (1 + tanh(head W^T + b)) by
    aoc_cat_film_scale; saves x, mem and the gain (and the head and the weight for the gate's own backward)."""

    @staticmethod
    def forward(ctx, x, mem, head, weight, bias):
        xd, md = _det(x), _det(mem)
        hd, wd, bd = _det(head), _det(weight), _det(bias)
        gain = ops.film_gain(hd, wd, bd)
        ctx.has_mem = md is not None
        ctx.save_for_backward(xd, md, gain, hd, wd)
        return ops.cat_film_scale(xd, md, hd, wd, bd)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        x, mem, gain, head, weight = ctx.saved_tensors
        need_x, need_mem, need_head, need_w, need_b = ctx.needs_input_grad
        small = need_head or need_w or need_b
        gx, gm, dgain = cat_film_scale_backward(grad_y, x, mem, gain, want_x=need_x, want_mem=need_mem and ctx.has_mem, want_gain=small)
        gh = gw = gb = None
        if small:
            gh, gw, gb = gates_train.film_gain_backward(dgain, gain, head, weight, want=(need_head, need_w, need_b))
        return gx, gm, gh, gw, gb


def groupnorm_relu(x, groups, gamma, beta, eps=1e-5, residual=None, relu=True, gate=None):
    """[gain *] [relu](GroupNorm(x) gamma + beta [+ residual]) with a backward for x, gamma, beta, the residual and, with ``gate`` = (head,
    weight, bias) of the IA_gate that follows, for those three.  Without a wanted gradient: ops.groupnorm_relu / ops.groupnorm_relu_scale."""
    gate = tuple(gate) if gate is not None else ()
    if not _wants_grad(x, gamma, beta, residual, *gate):
        d = lambda t: t.detach() if t is not None else None
        if not gate:
            return ops.groupnorm_relu(x, groups, d(gamma), d(beta), eps, residual, relu)
        return ops.groupnorm_relu_scale(x, groups, d(gamma), d(beta), eps, residual, relu, gate[0], d(gate[1]), d(gate[2]))
    ops._need_gpu(x, gamma, beta, residual, *gate)
    if not gate:
        return _GroupNormRelu.apply(x, gamma, beta, residual, groups, eps, relu)
    return _GroupNormReluScale.apply(x, gamma, beta, residual, gate[0], gate[1], gate[2], groups, eps, relu)


def cat_film_scale(x, mem, head, weight, bias):
    """torch.cat([x, mem], 1) gated by IA_gate (decoding_module.py:193-194, 203-204) with a backward for x, the head, the gate's weight and
    bias -- and for mem when it wants one (the modulators hand over a detached memory).  Without a wanted gradient: ops.cat_film_scale."""
    if not _wants_grad(x, mem, head, weight, bias):
        return ops.cat_film_scale(x, mem, head, weight.detach(), bias.detach() if bias is not None else None)
    ops._need_gpu(x, mem, head, weight, bias)
    return _CatFilmScale.apply(x, mem, head, weight, bias)


def film_scale(x, head, weight, bias):
    """``gates_train``' IA_gate as a function of the gate's tensors (the fallback behind a block that is not this module's Bottleneck)."""
    if not _wants_grad(x, head, weight, bias):
        return ops.film_scale(x, head, weight.detach(), bias.detach() if bias is not None else None)
    ops._need_gpu(x, head, weight, bias)
    return gates_train._FilmScale.apply(x, head, weight, bias)


# ------------------------------------------------------------------------------------------ Bottleneck
class Bottleneck(nn.Module):
    """networks/layers/gct.py:38-90 with a backward: the mirror's constructor, parameter names (``GCT1``, ``conv1..3``, ``bn1..3``, ``downsample``)
    and ``forward(x, gate=None)``.  ``GCT1`` is ``gates_train.GCT``; the convolutions are torch's; the four normalisations and the folded gate
    go through ``groupnorm_relu``."""

    def __init__(self, inplanes, outplanes, stride=1, dilation=1):
        super(Bottleneck, self).__init__()
        expansion = 4
        planes = int(outplanes / expansion)
        self.GCT1 = gates_train.GCT(inplanes)
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.GroupNorm(32, planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, dilation=dilation, padding=dilation, bias=False)
        self.bn2 = nn.GroupNorm(32, planes)
        self.conv3 = nn.Conv2d(planes, planes * expansion, kernel_size=1, bias=False)
        self.bn3 = nn.GroupNorm(32, planes * expansion)
        if stride != 1 or inplanes != planes * expansion:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * expansion, kernel_size=1, stride=stride, bias=False),
                                            nn.GroupNorm(32, planes * expansion))
        else:
            self.downsample = None
        self.stride = stride
        self.dilation = dilation
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    @staticmethod
    def _gn(bn, x, residual=None, relu=True, gate=None):
        return groupnorm_relu(x, bn.num_groups, bn.weight, bn.bias, bn.eps, residual, relu, gate)

    def forward(self, x, gate=None):
        """gate: None, or ``(IA_head, weight, bias)`` of the ``IA_gate`` that follows this block (decoding_module.py:196,198): the last
        normalisation writes the gated tensor, and its backward returns the gate's gradients with the block's."""
        out = self._gn(self.bn1, self.conv1(self.GCT1(x)))                  # gct.py:69-72
        out = self._gn(self.bn2, self.conv2(out))                           # :74-76
        residual = x
        if self.downsample is not None:
            residual = self._gn(self.downsample[1], self.downsample[0](x), relu=False)     # :81-82
        return self._gn(self.bn3, self.conv3(out), residual=residual, gate=gate)           # :78-79, 84-85 (+ the gate)


# ------------------------------------------------------------------------------------------ the memory modulators
def _gate_params(gate):
    ia = gate.IA                                                       # ATT:10, the reference's parameter name
    return ia.weight, ia.bias


def _modulator(dec, prefix, x, x_memory, IA_head):
    gates = [getattr(dec, f"{prefix}_Reweight_Layer_{i}") for i in (1, 2, 3)]
    blocks = [getattr(dec, f"{prefix}_Bottleneck_{i}") for i in (1, 2, 3)]
    x = cat_film_scale(x, x_memory, IA_head, *_gate_params(gates[0]))  # :193-194 / :203-204 in one launch
    for i, block in enumerate(blocks):
        following = gates[i + 1] if i + 1 < 3 else None
        if following is None:
            x = block(x)                                               # :199 / :209
        elif isinstance(block, Bottleneck):
            x = block(x, gate=(IA_head,) + _gate_params(following))    # :195-196, :197-198: the gate rides on bn3's apply pass
        else:
            x = film_scale(block(x), IA_head, *_gate_params(following))
    return x


def Modulator_1(dec, x, x_memory, IA_head):
    """decoding_module.py:192-200 with a backward.  Reads dec.M1_Reweight_Layer_{1,2,3} and dec.M1_Bottleneck_{1,2,3}."""
    return _modulator(dec, "M1", x, x_memory, IA_head)


def Modulator_2(dec, x, x_memory, IA_head):
    """decoding_module.py:202-210 with a backward.  Reads dec.M2_Reweight_Layer_{1,2,3} and dec.M2_Bottleneck_{1,2,3}."""
    return _modulator(dec, "M2", x, x_memory, IA_head)


def modulate(dec, x, IA_head, memory_list):
    """decoding_module.py:133-140 and :148 as one call, ``decoder_memory.modulate``'s rule with a graph: -> (x after both modulators, the next
    frame's memory_list).  Both memories are detached (:133, :137) and stay on x's device; no gradient flows into a memory."""
    cur_1 = x.detach()                                                 # :133
    mem_1 = select_memory(cur_1, memory_list[0])                       # :134-135
    x = dec.Modulator_1(x, mem_1, IA_head)                             # :136
    cur_2 = x.detach()                                                 # :137
    mem_2 = select_memory(cur_2, memory_list[1])                       # :138-139
    x = dec.Modulator_2(x, mem_2, IA_head)                             # :140
    return x, [cur_1, mem_2]                                           # :148
