"""Differentiable twin of ``DynamicPreHead`` (networks/aoc/decoding_module.py:228-240: 1x1 convolution, GroupNorm(embed_dim / 4), ReLU) with
the concatenation of aocnet.py:360-362 behind it.  It stands beside the inference mirror ``hotpath.DynamicPreHead`` (which raises when a
gradient is wanted) the way ``decoder_train.Bottleneck`` stands beside ``gct.Bottleneck``: the same constructor and parameter names
(``conv``, ``bn``), so a ``state_dict`` of the reference or of the mirror loads strictly, and the same ``forward(x, cur_emb=None)``.

What PyTorch writes and keeps for ``cat(emb.expand(O, ...), relu(GroupNorm(conv(x))))``: the convolution output, the normalised tensor, the
activation and the concatenation, each read again backward, beside the channel-first copy of the embedding expanded over the objects.  The
forward kernel stores none of them (it recomputes y = W x + b from the n_in-channel input in both of its passes), and neither does the
backward of csrc/prehead_grad.hip: it saves the input, the statistics [O * groups][2] and the parameters, recomputes y, the normalised
value and the ReLU mask with the forward's own instructions, and reads the n_out channels of the cotangent and the input twice.  The
embedding's gradient is the cotangent's first C channels summed over the objects, returned channel-last like the operand.

Without a wanted gradient the module returns the mirror's result through ``ops.prehead``; with one, the forward calls the same C entry
(``aoc_prehead``), so the output bits are the mirror's.  Frozen parameters and ``ctx.needs_input_grad`` select which optional outputs the
kernels are asked for.  The backward is ``once_differentiable``; every sum runs in a fixed order without float atomics.  The ctypes wrappers
live here, not in ``ops`` (whose public names are a tested table); they keep ``ops``' tensor contract through its helpers: inputs converted by
``_f32c`` / ``_opt`` / ``_vec`` into names that live until the call, caller outputs checked by ``_out`` (the named optional ones chosen by
``_wanted``), addresses only through ``_p``.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .ops import _det, _opt, _vec, _wanted, _wants_grad

PIX = 256                                   # pixels per chunk of aoc_prehead / aoc_prehead_grad (PH_PIX)
OUTS = ("grad_feat", "grad_weight", "grad_bias", "grad_gamma", "grad_beta", "grad_emb")


# ------------------------------------------------------------------------------------------ the C ABI
def _shapes(what, feat, weight, n_groups):
    if feat.dim() < 3 or feat.numel() == 0:
        raise ValueError(f"{what}: expected a non-empty [O, n_in, ...] tensor, got {tuple(feat.shape)}")
    O, n_in = feat.shape[0], feat.shape[1]
    hw = feat.numel() // (O * n_in)
    n_out = weight.shape[0]
    if weight.numel() != n_out * n_in:
        raise ValueError(f"{what}: DynamicPreHead runs with kernel_size = 1 (weight {tuple(weight.shape)} for {n_in} input channels)")
    if int(n_groups) < 1 or n_out % int(n_groups):
        raise ValueError(f"{what}: {n_out} channels do not divide into {n_groups} groups")
    return O, n_in, n_out, hw


def prehead_forward(feat, weight, bias, n_groups, gamma, beta, eps, emb_hwc=None):
    """ops.prehead keeping the statistics: feat [O, n_in, h, w] -> (out [O, C + n_out, h, w], stats [O * n_groups, 2] = (mean, rstd), a view of
    the call's workspace).  The same C entry as the mirror's wrapper, so out has its bits."""
    feat, weight = ops._f32c(feat), ops._f32c(weight)
    bi, g, b = _vec(bias), _vec(gamma), _vec(beta)                # bound until the launch is enqueued
    emb_hwc = _opt(emb_hwc)
    if feat.dim() != 4:
        raise ValueError(f"prehead_forward: expected feat [O, n_in, h, w], got {tuple(feat.shape)}")
    O, n_in, n_out, hw = _shapes("prehead_forward", feat, weight, n_groups)
    if any(t.numel() != n_out for t in (bi, g, b)):
        raise ValueError(f"prehead_forward: bias, gamma and beta must hold {n_out} elements")
    C = 0
    if emb_hwc is not None:
        C = emb_hwc.shape[-1]
        if emb_hwc.numel() != hw * C:
            raise ValueError(f"prehead_forward: the embedding {tuple(emb_hwc.shape)} does not cover the {feat.shape[2]} x {feat.shape[3]} map")
    ops._need_gpu(feat, weight, bi, g, b, emb_hwc)
    n_groups = int(n_groups)
    L = _lib.lib()
    out = torch.empty(O, C + n_out, feat.shape[2], feat.shape[3], dtype=torch.float32, device=feat.device)
    ws = ops._ws(L.aoc_prehead_workspace_bytes(O, n_out, n_out // n_groups, hw), feat.device)
    _lib.check(L.aoc_prehead(ops._p(feat), O, n_in, hw, ops._p(weight), ops._p(bi), n_out, n_groups, ops._p(g), ops._p(b), float(eps), ops._p(emb_hwc), C,
                             ops._p(out), ops._p(ws), ws.numel(), ops._stream()), "aoc_prehead")
    off = -(-(O * n_groups * (-(-hw // PIX)) * 16) // 256) * 256          # aoc_align_up(n_obj * n_groups * n_chunks * 16, 256)
    return out, ws[off:off + O * n_groups * 8].view(torch.float32).view(O * n_groups, 2)


def prehead_backward(grad_out, feat, stats, weight, bias, n_groups, gamma, beta, C=0, want=None, out=None):
    """aoc_prehead_grad: grad_out [O, C + n_out, ...] (the cotangent of prehead_forward's out), feat [O, n_in, ...], stats [O * n_groups, 2] as
    prehead_forward returns them -> the tuple (grad_feat, grad_weight [n_out, n_in], grad_bias, grad_gamma, grad_beta [n_out], grad_emb
    [..., C] channel-last); None where ``want`` (six flags; default: all, grad_emb with C > 0) is false.  ``out``: a dict of caller buffers by
    those names."""
    grad_out, feat, stats, weight = ops._f32c(grad_out), ops._f32c(feat), ops._f32c(stats), ops._f32c(weight)
    bi, g, b = _vec(bias), _vec(gamma), _vec(beta)                # bound until the launch is enqueued
    out = dict(out or {})
    ops._need_gpu(grad_out, feat, stats, weight, bi, g, b, *out.values())
    O, n_in, n_out, hw = _shapes("prehead_backward", feat, weight, n_groups)
    n_groups, C = int(n_groups), int(C)
    if C < 0 or grad_out.dim() != feat.dim() or grad_out.shape[0] != O or grad_out.shape[1] != C + n_out or tuple(grad_out.shape[2:]) != tuple(feat.shape[2:]):
        raise ValueError(f"prehead_backward: grad_out {tuple(grad_out.shape)} is not [O, C + n_out, ...] = [{O}, {C} + {n_out}, ...] over feat's map")
    if stats.numel() != O * n_groups * 2 or any(t.numel() != n_out for t in (bi, g, b)):
        raise ValueError(f"prehead_backward: stats must hold {O * n_groups} (mean, rstd) pairs and bias, gamma, beta {n_out} elements")
    if want is None:
        want = (True,) * 5 + (C > 0,)
    want = tuple(bool(w) for w in want)
    if len(want) != 6:
        raise ValueError("prehead_backward: want holds six flags")
    if C == 0 and (want[5] or "grad_emb" in out):
        raise ValueError("prehead_backward: the embedding's gradient needs C > 0")
    shapes = (tuple(feat.shape), (n_out, n_in), (n_out,), (n_out,), (n_out,), tuple(feat.shape[2:]) + (C,))
    bufs = _wanted("prehead_backward", OUTS, shapes, want, out, feat)
    L = _lib.lib()
    ws = ops._ws(L.aoc_prehead_grad_workspace_bytes(O, n_in, n_out, n_groups, hw), feat.device)
    _lib.check(L.aoc_prehead_grad(ops._p(grad_out), ops._p(feat), ops._p(stats), ops._p(weight), ops._p(bi), ops._p(g), ops._p(b), O, n_in, n_out, n_groups,
                                  hw, C, *(ops._p(t) for t in bufs), ops._p(ws), ws.numel(), ops._stream()), "aoc_prehead_grad")
    return bufs


# ------------------------------------------------------------------------------------------ autograd
class _PreHead(torch.autograd.Function):
    """feat [O, n_in, h, w], weight, bias, gamma, beta, emb [h, w, C] or None -> [O, C + n_out, h, w] by aoc_prehead; saves feat, the
    statistics and the parameters -- not the output."""

    @staticmethod
    def forward(ctx, feat, weight, bias, gamma, beta, emb, n_groups, eps):
        fd, wd, bd, ga, be, ed = _det(feat), _det(weight), _det(bias), _det(gamma), _det(beta), _det(emb)
        out, stats = prehead_forward(fd, wd, bd, n_groups, ga, be, eps, ed)
        ctx.save_for_backward(fd, stats, wd, bd, ga, be)
        ctx.cfg = (int(n_groups), ed.shape[-1] if ed is not None else 0, tuple(weight.shape), tuple(emb.shape) if emb is not None else None)
        return out

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_out):
        feat, stats, weight, bias, gamma, beta = ctx.saved_tensors
        n_groups, C, w_shape, e_shape = ctx.cfg
        need = ctx.needs_input_grad[:6]
        gf, gw, gb, gg, gbe, ge = prehead_backward(grad_out, feat, stats, weight, bias, n_groups, gamma, beta, C,
                                                    want=tuple(need[:5]) + (bool(need[5]) and C > 0,))
        return (gf, gw.view(w_shape) if gw is not None else None, gb, gg, gbe, ge.view(e_shape) if ge is not None else None, None, None)


class DynamicPreHead(nn.Module):
    """decoding_module.py:228-240 with a backward: the mirror's constructor, parameter names (``conv``, ``bn``), ``kernel_size == 1`` rule and
    ``forward(x, cur_emb=None)``.  ``cur_emb`` is the channel-last [h, w, C] operand of the mirror (aocnet.py:360-362 as one call); its gradient
    comes back in that shape, so a caller's ``cur.permute(1, 2, 0)`` carries it to the [C, h, w] leaf."""

    def __init__(self, in_dim=3, embed_dim=100, kernel_size=1):
        super(DynamicPreHead, self).__init__()
        if kernel_size != 1:
            raise NotImplementedError("aoc_amd.DynamicPreHead: kernel_size 1 only (the reference's configs use the default)")
        self.conv = nn.Conv2d(in_dim, embed_dim, kernel_size=kernel_size, stride=1, padding=int((kernel_size - 1) / 2))
        self.bn = nn.GroupNorm(int(embed_dim / 4), embed_dim)
        nn.init.kaiming_normal_(self.conv.weight, mode='fan_out', nonlinearity='relu')

    def forward(self, x, cur_emb=None):
        conv, bn = self.conv, self.bn
        if not _wants_grad(x, cur_emb, conv.weight, conv.bias, bn.weight, bn.bias):
            return ops.prehead(x, conv.weight.detach(), conv.bias.detach(), bn.num_groups, bn.weight.detach(), bn.bias.detach(), bn.eps, cur_emb)
        ops._need_gpu(x, cur_emb, conv.weight, conv.bias, bn.weight, bn.bias)
        return _PreHead.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, cur_emb, bn.num_groups, bn.eps)
