"""Differentiable twins of the decoder's tail: ``decoder_final`` (networks/aoc/decoding_module.py:162-190), ``predict`` (:144-147 with ``IA_logit``,
:151-160) and ``augment_background_logit`` (:213-225).  They stand beside the inference mirrors of ``decoder_tail`` (which raise when a gradient
is wanted) the way ``decoder_train`` stands beside ``decoder_memory``: the mirrors' signatures and the same binding onto the reference's decoder
class.  With them every non-convolution line of the decoder from ``Modulator_1`` to ``pred`` has a backward on the HIP path.

What PyTorch does for these lines: ``F.interpolate(mode='bicubic')`` scatters its backward with float atomics (other bits every run, refused
under ``torch.use_deterministic_algorithms``), the upsampled tensor, the concatenation and the gated product are written at full resolution
and read back, and ``torch.min(bg_logit, dim=0)`` breaks ties in no stated way.  The kernels of csrc/tail_grad.hip:

    shortcut stage    pass A: t = U^T grad_out at coarse size (gather form, the forward's own tap weights) and the dots <x, t> = <grad_out,
                      bicubic(x)> from ONE read of the fine gradient, the shortcut planes' dots by aoc_channel_scale_grad; the small part
                      (``gates_train.film_gain_backward`` and the delta pull-back, [N, C] sized); pass B: grad_x = gain t + dpx cy cx / HW at
                      coarse size, grad_low = gain grad_out + dpx / HW
    delta gate        ``IA(x, cat([IA_head, delta(mean(x))]))`` (IA11 here, IA9 in front of the ASPP): aoc_channel_scale_grad's dots,
                      film_gain_backward, the pull-back, one apply pass grad_x = gain grad_y + dpx / hw
    logit head        the forward also leaves arg [hw], the object whose bg logit is the minimum (lowest index wins a tie; NaN never wins);
                      the backward reads x once and writes grad_x once, with the rows' gradients in aoc_channel_scale_grad's order

Saved for the backward: the shortcut stage x, low, the head, the plane means and the gain; the delta gate x, the extended head and the gain;
the head x, the two rows [N, C + 1] and arg.  Without a wanted gradient every function here returns the mirror's result through the mirror's
own ``ops`` calls; with one, the forward calls the same C entry points (``aoc_logit_head_argmin`` repeats ``aoc_logit_head``'s sums term by
term), so the output bits are the mirror's.  ``ctx.needs_input_grad`` selects which optional outputs the kernels are asked for.  All backwards
are ``once_differentiable``; every sum runs in a fixed order without float atomics.  The ctypes wrappers of the new entry points live here,
not in ``ops`` (whose public names are a tested table); they keep ``ops``' tensor contract through its helpers: inputs converted by
``_f32c`` / ``_opt`` / ``_i32c`` into names that live until the call, caller outputs checked by ``_out`` (the named optional ones chosen by
``_wanted``), addresses only through ``_p``.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib, decoder_tail, decoder_train, gates_train, gct, ops
from .ops import _det, _new, _opt, _wanted, _wants_grad


# ------------------------------------------------------------------------------------------ the C ABI
def _stage_shapes(what, grad_out, x, low):
    if grad_out.dim() != 4 or x is None or x.dim() != 4 or grad_out.numel() == 0 or x.numel() == 0:
        raise ValueError(f"{what}: grad_out [N, Ce + Cr, H, W] and x [N, Ce, h, w] are needed (x for its shape at least)")
    N, Ct, H, W = grad_out.shape
    Ce, h, w = x.shape[1:]
    Cr = Ct - Ce
    if x.shape[0] != N or Cr < 0 or (low is not None and tuple(low.shape) != (N, Cr, H, W)) or (low is None and Cr > 0):
        raise ValueError(f"{what}: x {tuple(x.shape)} and low {tuple(low.shape) if low is not None else None} do not fit grad_out {tuple(grad_out.shape)}")
    return N, Ce, Cr, h, w, H, W


def shortcut_stage_backward_dots(grad_out, x, low=None, t=None, dgain=None, want_t=True, want_gain=True):
    """aoc_shortcut_stage_grad_dots (pass A): grad_out [N, Ce + Cr, H, W], x [N, Ce, h, w], low [N, Cr, H, W] or None -> (t [N, Ce, h, w] = the
    adjoint of the bicubic upsample applied to grad_out's first Ce channels, dgain [N, Ce + Cr] = the plane dots of grad_out with
    cat(bicubic(x), low)); None where not wanted (t then lives in the call's workspace)."""
    grad_out, x, low = ops._f32c(grad_out), ops._f32c(x), _opt(low)
    ops._need_gpu(grad_out, x, low, t, dgain)
    N, Ce, Cr, h, w, H, W = _stage_shapes("shortcut_stage_backward_dots", grad_out, x, low)
    want_t, want_gain = bool(want_t or t is not None), bool(want_gain or dgain is not None)
    if want_t:
        t = torch.empty_like(x) if t is None else ops._out("shortcut_stage_backward_dots: t", t, x.shape)
    if want_gain:
        dgain = _new(x, N, Ce + Cr) if dgain is None else ops._out("shortcut_stage_backward_dots: dgain", dgain, (N, Ce + Cr))
    L = _lib.lib()
    ws = ops._ws(L.aoc_shortcut_stage_grad_workspace_bytes(N, Ce, h, w, H, W), x.device)
    _lib.check(L.aoc_shortcut_stage_grad_dots(ops._p(grad_out), ops._p(x), ops._p(low), N, Ce, Cr, h, w, H, W, ops._p(t), ops._p(dgain), ops._p(ws), ws.numel(),
                                              ops._stream()), "aoc_shortcut_stage_grad_dots")
    return t, dgain


def shortcut_stage_backward_apply(grad_out, t, gain=None, dpx=None, grad_low=None, want_low=True, channels=None):
    """aoc_shortcut_stage_grad_apply (pass B): grad_out [N, Ce + Cr, H, W]; t [N, Ce, h, w] from pass A, overwritten in place with grad_x (None:
    no grad_x; ``channels`` = Ce is needed then); gain, dpx [N, Ce + Cr] or None (1, 0) -> (grad_x = gain t + cy cx dpx / (H W), which is t itself,
    grad_low [N, Cr, H, W] = gain grad_out + dpx / (H W) or None)."""
    grad_out, gain, dpx = ops._f32c(grad_out), _opt(gain), _opt(dpx)
    ops._need_gpu(grad_out, t, gain, dpx, grad_low)
    if grad_out.dim() != 4 or grad_out.numel() == 0 or (t is None and channels is None) or (t is not None and t.dim() != 4):
        raise ValueError("shortcut_stage_backward_apply: grad_out [N, Ce + Cr, H, W] and t [N, Ce, h, w] (or channels = Ce) are needed")
    N, Ct, H, W = grad_out.shape
    Ce = int(channels) if t is None else t.shape[1]
    Cr = Ct - Ce
    h, w = (1, 1) if t is None else t.shape[2:]
    if t is not None:
        if t.dim() != 4 or t.shape[0] != N or Cr < 0:
            raise ValueError(f"shortcut_stage_backward_apply: t {tuple(t.shape)} does not fit grad_out {tuple(grad_out.shape)}")
        t = ops._out("shortcut_stage_backward_apply: t", t, (N, Ce, h, w))
    if not 1 <= Ce <= Ct or any(v is not None and v.numel() != N * Ct for v in (gain, dpx)):
        raise ValueError(f"shortcut_stage_backward_apply: gain and dpx must hold {N * Ct} elements, Ce = {Ce} of {Ct} channels")
    want_low = bool((want_low or grad_low is not None) and Cr > 0)
    if want_low:
        grad_low = _new(grad_out, N, Cr, H, W) if grad_low is None else ops._out("shortcut_stage_backward_apply: grad_low", grad_low, (N, Cr, H, W))
    _lib.check(_lib.lib().aoc_shortcut_stage_grad_apply(ops._p(grad_out), ops._p(gain), ops._p(dpx), N, Ce, Cr, h, w, H, W, ops._p(t), ops._p(grad_low),
                                                        ops._stream()), "aoc_shortcut_stage_grad_apply")
    return t, grad_low


def delta_gate_backward_apply(grad_y, gain, dpx=None, grad_x=None):
    """aoc_delta_gate_grad_apply: grad_x[n, c] = gain[n, c] grad_y[n, c] + dpx[n, c] / hw (dpx None: no shift)."""
    grad_y, gain, dpx = ops._f32c(grad_y), ops._f32c(gain), _opt(dpx)
    ops._need_gpu(grad_y, gain, dpx, grad_x)
    if grad_y.dim() < 2 or grad_y.numel() == 0:
        raise ValueError(f"delta_gate_backward_apply: expected a non-empty [N, C, ...] tensor, got {tuple(grad_y.shape)}")
    N, C = grad_y.shape[:2]
    if gain.numel() != N * C or (dpx is not None and dpx.numel() != N * C):
        raise ValueError(f"delta_gate_backward_apply: gain and dpx must hold {N * C} elements")
    grad_x = torch.empty_like(grad_y) if grad_x is None else ops._out("delta_gate_backward_apply: grad_x", grad_x, grad_y.shape)
    _lib.check(_lib.lib().aoc_delta_gate_grad_apply(ops._p(grad_y), ops._p(gain), ops._p(dpx), N, C, grad_y.numel() // (N * C), ops._p(grad_x), ops._stream()),
               "aoc_delta_gate_grad_apply")
    return grad_x


def delta_pullback(dd):
    """dpx[n] = sum_m dd[m] - dd[n] (the backward of px1_delta, decoding_module.py:173-174), the objects added in ascending order.  [N, C] sized."""
    total = dd[0]
    for m in range(1, dd.shape[0]):
        total = total + dd[m]
    return (total.unsqueeze(0) - dd).contiguous()


def _head_shapes(what, x, wb_fg, wb_bg):
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"{what}: x must be a non-empty [N, C, H, W] tensor, got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if tuple(wb_fg.shape) != (N, C + 1) or (wb_bg is not None and tuple(wb_bg.shape) != (N, C + 1)) or (wb_bg is None and N > 1):
        raise ValueError(f"{what}: wb_fg and wb_bg must be [{N}, {C + 1}] (weights then bias)")
    return N, C, H, W


def logit_head_forward(x, wb_fg, wb_bg, pred=None, arg=None):
    """aoc_logit_head_argmin: ops.logit_head's pred [1, N, H, W] (the same bits) and arg [H * W] int32, the object n >= 1 with the smallest bg
    logit (the lowest n of a tie; 0 = none); arg is None for N = 1."""
    x, wb_fg, wb_bg = ops._f32c(x), ops._f32c(wb_fg), _opt(wb_bg)
    ops._need_gpu(x, wb_fg, wb_bg, pred, arg)
    N, C, H, W = _head_shapes("logit_head_forward", x, wb_fg, wb_bg)
    pred = _new(x, 1, N, H, W) if pred is None else ops._out("logit_head_forward: pred", pred, (1, N, H, W))
    if N > 1:
        arg = _new(x, H * W, dtype=torch.int32) if arg is None else ops._out("logit_head_forward: arg", arg, (H * W,), torch.int32)
    else:
        arg = None
    _lib.check(_lib.lib().aoc_logit_head_argmin(ops._p(x), ops._p(wb_fg), ops._p(wb_bg), C + 1, N, C, H * W, ops._p(pred), ops._p(arg), ops._stream()),
               "aoc_logit_head_argmin")
    return pred, arg


_HEAD_OUTS = ("grad_x", "grad_wb_fg", "grad_wb_bg")


def logit_head_backward(grad_pred, arg, x, wb_fg, wb_bg, want=(True, True, True), out=None):
    """aoc_logit_head_grad: grad_pred [1, N, H, W] (or [N, H * W]), arg [H * W] int32 (None for N = 1), x [N, C, H, W], wb_fg, wb_bg [N, C + 1] ->
    (grad_x, grad_wb_fg, grad_wb_bg); None where ``want`` is false.  ``out``: a dict of caller buffers by those names."""
    grad_pred, x, wb_fg, wb_bg = ops._f32c(grad_pred), ops._f32c(x), ops._f32c(wb_fg), _opt(wb_bg)
    arg = ops._i32c(arg) if arg is not None else None
    out = dict(out or {})
    ops._need_gpu(grad_pred, arg, x, wb_fg, wb_bg, *out.values())
    N, C, H, W = _head_shapes("logit_head_backward", x, wb_fg, wb_bg)
    if grad_pred.numel() != N * H * W or (N > 1 and (arg is None or arg.numel() != H * W)):
        raise ValueError(f"logit_head_backward: grad_pred must hold {N * H * W} elements and arg {H * W}")
    bufs = _wanted("logit_head_backward", _HEAD_OUTS, (tuple(x.shape), (N, C + 1), (N, C + 1)), want, out, x)
    grad_x, grad_fg, grad_bg = bufs
    _lib.check(_lib.lib().aoc_logit_head_grad(ops._p(grad_pred), ops._p(arg), ops._p(x), ops._p(wb_fg), ops._p(wb_bg), C + 1, N, C, H * W, ops._p(grad_x),
                                              ops._p(grad_fg), ops._p(grad_bg), ops._stream()), "aoc_logit_head_grad")
    return bufs


def background_merge_forward(fg_logit, bg_logit, pred=None, arg=None):
    """aoc_background_merge_argmin: ops.background_merge's pred [1, N, H, W] and arg [H * W] int32 as logit_head_forward leaves it."""
    fg, bg = ops._f32c(fg_logit), ops._f32c(bg_logit)
    ops._need_gpu(fg, bg, pred, arg)
    if fg.dim() != 4 or fg.shape[1] != 1 or bg.shape != fg.shape or fg.numel() == 0:
        raise ValueError(f"background_merge_forward: fg_logit and bg_logit must be [N, 1, H, W], got {tuple(fg.shape)} and {tuple(bg.shape)}")
    N, _, H, W = fg.shape
    pred = _new(fg, 1, N, H, W) if pred is None else ops._out("background_merge_forward: pred", pred, (1, N, H, W))
    if N > 1:
        arg = _new(fg, H * W, dtype=torch.int32) if arg is None else ops._out("background_merge_forward: arg", arg, (H * W,), torch.int32)
    else:
        arg = None
    _lib.check(_lib.lib().aoc_background_merge_argmin(ops._p(fg), ops._p(bg), N, H * W, ops._p(pred), ops._p(arg), ops._stream()), "aoc_background_merge_argmin")
    return pred, arg


def background_merge_backward(grad_pred, arg, grad_fg=None, grad_bg=None, want=(True, True)):
    """aoc_background_merge_grad: grad_pred [1, N, H, W], arg [H * W] int32 (None for N = 1) -> (grad_fg = grad_pred as [N, 1, H, W],
    grad_bg [N, 1, H, W] = grad_pred[0] on the object arg names, 0 elsewhere and on object 0); None where not wanted."""
    grad_pred = ops._f32c(grad_pred)
    arg = ops._i32c(arg) if arg is not None else None
    ops._need_gpu(grad_pred, arg, grad_fg, grad_bg)
    if grad_pred.dim() != 4 or grad_pred.shape[0] != 1 or grad_pred.numel() == 0:
        raise ValueError(f"background_merge_backward: grad_pred must be [1, N, H, W], got {tuple(grad_pred.shape)}")
    _, N, H, W = grad_pred.shape
    if N > 1 and (arg is None or arg.numel() != H * W):
        raise ValueError(f"background_merge_backward: arg must hold {H * W} elements")
    if want[0] or grad_fg is not None:
        grad_fg = _new(grad_pred, N, 1, H, W) if grad_fg is None else ops._out("background_merge_backward: grad_fg", grad_fg, (N, 1, H, W))
    if want[1] or grad_bg is not None:
        grad_bg = _new(grad_pred, N, 1, H, W) if grad_bg is None else ops._out("background_merge_backward: grad_bg", grad_bg, (N, 1, H, W))
    _lib.check(_lib.lib().aoc_background_merge_grad(ops._p(grad_pred), ops._p(arg), N, H * W, ops._p(grad_fg), ops._p(grad_bg), ops._stream()),
               "aoc_background_merge_grad")
    return grad_fg, grad_bg


# ------------------------------------------------------------------------------------------ autograd
class _ShortcutStage(torch.autograd.Function):
    """x [N, Ce, h, w], low [N, Cr, H, W], head [N, D], weight [Ce + Cr, D + Ce + Cr], bias or None -> IA10(cat([bicubic(x), low], 1), cat([head,
    px1_delta], 1)) by aoc_shortcut_stage_enqueue; saves x, low, the head, the weight and the plane means and gain the call emits."""

    @staticmethod
    def forward(ctx, x, low, head, weight, bias):
        xd, ld, hd, wd, bd = _det(x), _det(low), _det(head), _det(weight), _det(bias)
        y, px, gain = ops.shortcut_stage(xd, ld, hd, wd, bd, want_debug=True)
        ctx.save_for_backward(xd, ld, hd, wd, px, gain)
        return y

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_out):
        x, low, head, weight, px, gain = ctx.saved_tensors
        need_x, need_low, need_head, need_w, need_b = ctx.needs_input_grad
        grad_out = ops._f32c(grad_out)
        t, dgain = shortcut_stage_backward_dots(grad_out, x, low, want_t=need_x, want_gain=True)
        head_ext = ops.head_delta(head, px)                                  # the forward's own extended head (the same call, the same bits)
        feedback = need_x or need_low
        ghe, gw, gb = gates_train.film_gain_backward(dgain, gain, head_ext, weight, want=(need_head or feedback, need_w, need_b))
        D = head.shape[1]
        gx = gl = None
        if feedback:
            dpx = delta_pullback(ghe[:, D:])
            gx, gl = shortcut_stage_backward_apply(grad_out, t, gain, dpx, want_low=need_low, channels=x.shape[1])
        return gx, gl, (ghe[:, :D].contiguous() if need_head else None), gw, gb


class _DeltaGate(torch.autograd.Function):
    """x [N, C, ...], head [N, D], weight [C, D + C], bias or None -> x * (1 + tanh([head | delta(mean(x))] W^T + b)) by aoc_plane_mean,
    aoc_head_delta and aoc_film_scale; saves x, the extended head, the weight and the gain (aoc_film_gain)."""

    @staticmethod
    def forward(ctx, x, head, weight, bias):
        xd, hd, wd, bd = _det(x), _det(head), _det(weight), _det(bias)
        head_ext = ops.head_delta(hd, ops.plane_mean(xd))
        gain = ops.film_gain(head_ext, wd, bd)
        ctx.save_for_backward(xd, head_ext, wd, gain)
        ctx.head_dim = hd.shape[1]
        return ops.film_scale(xd, head_ext, wd, bd)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_y):
        x, head_ext, weight, gain = ctx.saved_tensors
        need_x, need_head, need_w, need_b = ctx.needs_input_grad
        grad_y = ops._f32c(grad_y)
        _, dgain = gates_train.channel_scale_backward(grad_y, x, None, want_x=False, want_gain=True)
        ghe, gw, gb = gates_train.film_gain_backward(dgain, gain, head_ext, weight, want=(need_head or need_x, need_w, need_b))
        D = ctx.head_dim
        gx = delta_gate_backward_apply(grad_y, gain, delta_pullback(ghe[:, D:])) if need_x else None
        return gx, (ghe[:, :D].contiguous() if need_head else None), gw, gb


class _HeadLinear(torch.autograd.Function):
    """IA_head [N, D] -> IA_final(IA_head) [N, C + 1] by aoc_linear (decoding_module.py:154); the backward is three torch products of that size."""

    @staticmethod
    def forward(ctx, head, weight, bias):
        hd, wd, bd = _det(head), _det(weight), _det(bias)
        ctx.save_for_backward(hd, wd)
        return ops.linear(hd, wd, bd)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, g):
        head, weight = ctx.saved_tensors
        need_head, need_w, need_b = ctx.needs_input_grad
        return (g @ weight if need_head else None), (g.t() @ head if need_w else None), (g.sum(0) if need_b else None)


class _LogitHead(torch.autograd.Function):
    """x [N, C, H, W], wb_fg, wb_bg [N, C + 1] -> pred [1, N, H, W] by aoc_logit_head_argmin; saves x, the rows and arg."""

    @staticmethod
    def forward(ctx, x, wb_fg, wb_bg):
        xd, fd, bd = _det(x), _det(wb_fg), _det(wb_bg)
        pred, arg = logit_head_forward(xd, fd, bd)
        ctx.save_for_backward(xd, fd, bd, arg)
        return pred

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_pred):
        x, wb_fg, wb_bg, arg = ctx.saved_tensors
        return logit_head_backward(grad_pred, arg, x, wb_fg, wb_bg, want=ctx.needs_input_grad)


class _BackgroundMerge(torch.autograd.Function):
    """fg_logit, bg_logit [N, 1, H, W] -> pred [1, N, H, W] by aoc_background_merge_argmin; saves arg."""

    @staticmethod
    def forward(ctx, fg_logit, bg_logit):
        pred, arg = background_merge_forward(fg_logit.detach(), bg_logit.detach())
        ctx.save_for_backward(arg)
        return pred

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_pred):
        arg, = ctx.saved_tensors
        return background_merge_backward(grad_pred, arg, want=ctx.needs_input_grad)


def _d(t):
    return t.detach() if t is not None else None


def shortcut_stage(x, low, IA_head, weight, bias):
    """decoding_module.py:163, 170-176 (``ops.shortcut_stage``) with a backward for x, low, the head and IA10's weight and bias."""
    if not _wants_grad(x, low, IA_head, weight, bias):
        return ops.shortcut_stage(x, low, IA_head, _d(weight), _d(bias))
    ops._need_gpu(x, low, IA_head, weight, bias)
    return _ShortcutStage.apply(x, low, IA_head, weight, bias)


def delta_gate(x, IA_head, weight, bias):
    """``IA(x, cat([IA_head, delta(mean(x))], 1))`` (decoding_module.py:126-130, :181-185) with a backward for x, the head and the gate's weight and
    bias.  Without a wanted gradient: ops.plane_mean -> ops.head_delta -> ops.film_scale, as ``decoder_tail.decoder_final`` composes them."""
    if not _wants_grad(x, IA_head, weight, bias):
        return ops.film_scale(x, ops.head_delta(IA_head, ops.plane_mean(x)), _d(weight), _d(bias))
    ops._need_gpu(x, IA_head, weight, bias)
    return _DeltaGate.apply(x, IA_head, weight, bias)


def head_linear(IA_head, weight, bias):
    """``IA_final(IA_head)`` (decoding_module.py:154) with a backward for the head, the weight and the bias."""
    if not _wants_grad(IA_head, weight, bias):
        return ops.linear(IA_head, _d(weight), _d(bias))
    ops._need_gpu(IA_head, weight, bias)
    return _HeadLinear.apply(IA_head, weight, bias)


def logit_head(x, wb_fg, wb_bg):
    """``ops.logit_head`` (decoding_module.py:144-147 behind the two linear layers) with a backward for x and both rows."""
    if not _wants_grad(x, wb_fg, wb_bg):
        return ops.logit_head(x, wb_fg, wb_bg)
    ops._need_gpu(x, wb_fg, wb_bg)
    return _LogitHead.apply(x, wb_fg, wb_bg)


# ------------------------------------------------------------------------------------------ the twins
def _gn_relu(bn, x):
    return decoder_train.groupnorm_relu(x, bn.num_groups, bn.weight, bn.bias, bn.eps)


def decoder_final(dec, x, low_level_feat, IA_head):
    """decoding_module.py:162-190 with a backward.  Reads dec.GCT_sc (``gates_train.GCT``), conv_sc, bn_sc, IA10, conv1, bn1, IA11, conv2, bn2; the
    three convolutions are torch's."""
    params = [p for name in ("GCT_sc", "conv_sc", "bn_sc", "IA10", "conv1", "bn1", "IA11", "conv2", "bn2") for p in getattr(dec, name).parameters()]
    if not _wants_grad(x, low_level_feat, IA_head, *params):
        return decoder_tail.decoder_final(dec, x, low_level_feat, IA_head)
    if isinstance(dec.GCT_sc, gct.GCT):
        raise _lib.AocHipError("aoc_amd.tail_train.decoder_final: dec.GCT_sc is the inference mirror aoc_amd.gct.GCT, which builds no autograd graph; "
                               "construct it as aoc_amd.gates_train.GCT (the same parameters, a state_dict loads)")
    low = _gn_relu(dec.bn_sc, dec.conv_sc(dec.GCT_sc(low_level_feat)))                                  # :165-168
    x = shortcut_stage(x, low, IA_head, dec.IA10.IA.weight, dec.IA10.IA.bias)                          # :163, :170-176
    x = _gn_relu(dec.bn1, dec.conv1(x))                                                                # :177-179
    x = delta_gate(x, IA_head, dec.IA11.IA.weight, dec.IA11.IA.bias)                                   # :181-185
    return _gn_relu(dec.bn2, dec.conv2(x))                                                             # :186-188


def augment_background_logit(fg_logit, bg_logit):
    """decoding_module.py:213-225 with a backward: [N, 1, h, w] x 2 -> [1, N, h, w].  The gradient of pred[0] goes to the one object whose bg
    logit is the minimum (the lowest index of a tie)."""
    if not _wants_grad(fg_logit, bg_logit):
        return decoder_tail.augment_background_logit(fg_logit, bg_logit)
    ops._need_gpu(fg_logit, bg_logit)
    return _BackgroundMerge.apply(fg_logit, bg_logit)


def predict(dec, x, IA_head):
    """decoding_module.py:144-147 with a backward for x, the head and both ``IA_final`` layers; x is read once forward and once backward."""
    fg, bg = dec.IA_final_fg, dec.IA_final_bg
    if not _wants_grad(x, IA_head, fg.weight, fg.bias, bg.weight, bg.bias):
        return decoder_tail.predict(dec, x, IA_head)
    return logit_head(x, head_linear(IA_head, fg.weight, fg.bias), head_linear(IA_head, bg.weight, bg.bias))
