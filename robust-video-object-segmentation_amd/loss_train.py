"""The training criterion: ``Concat_CrossEntropyLoss`` (networks/layers/loss.py:52-97) and the lines of ``AOCNet.forward`` in front of it
(aocnet.py:71-82: the bilinear upsample of every sample's logits to the crop, ``argmax`` for ``all_pred``), on csrc/loss_grad.hip.

Per sample the reference interpolates ``[1, C, h, w]`` logits to ``[1, C, H, W]``, takes the per-pixel cross-entropy with ``ignore_index=255``,
keeps the ``k`` hardest pixels by ``torch.topk`` and returns their mean.  Here the upsampled logits are never formed:

    forward    aoc_criterion_forward     the three entries below as ONE call (the same launches and bits; thr, n_gt and the counts in its workspace)
               aoc_upsample_ce_forward   loss, lse [H * W], argmax; a count of valid pixels per 256 pixels
               aoc_topk_mean             thr = the k-th largest loss (radix select), n_gt, mean = (sum_{loss > thr} loss + (k - n_gt) thr) / k
               aoc_topk_select_mask      one byte per pixel: exactly k set, the lowest pixel index wins a tie at thr (torch.topk leaves the
                                         choice among equal losses open; the mean is the same whichever is taken)
    backward   aoc_upsample_ce_grad      grad_pred = U^T[mask * grad_out / k * (softmax - onehot)] in gather form, softmax recomputed from lse

``top_k_percent_pixels=None`` (``reduction='mean'``) runs aoc_valid_mean / aoc_valid_mask instead: the mean over the valid pixels, whose
number is summed on the device.  Saved for the backward: pred, the int32 labels, lse and the mask.  The loss comes back as a 0-d device
tensor and nothing synchronises: ``k`` follows from the shapes and ``step`` in Python, ``grad_out`` and ``n_valid`` are read from device
memory by the gradient kernel.  A label outside ``[0, C)`` other than ``ignore_index`` gets loss 0 and no gradient (torch raises a device
assertion there); ``check_labels=True`` reads the kernel's count of such labels and raises, which synchronises, so it is off by default.

The backward is ``once_differentiable``; every sum runs in a fixed order without float atomics, so a step is bit-reproducible and runs under
``torch.use_deterministic_algorithms``.  The ctypes wrappers live here, not in ``ops`` (whose public names are a tested table); they keep
``ops``' tensor contract and are stricter on inputs: the thin wrappers take contiguous float32 / int32 tensors and raise otherwise (only the
labels are converted from int64), the autograd function and the modules convert what the reference hands over.
``Concat_BCEWithLogitsLoss`` is not built: aocnet.py never imports it, and its top-k branch passes indices as weights.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .ops import _wanted, _wants_grad

IGNORE_INDEX = 255
MAX_CHANNELS = 31


# ------------------------------------------------------------------------------------------ the C ABI
def _in(what, t, dtype=torch.float32):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} tensor")
    return t


def _pred3(what, pred):
    _in(what + ": pred", pred)
    if pred.dim() == 4 and pred.shape[0] == 1:
        pred = pred[0]
    if pred.dim() != 3 or pred.numel() == 0:
        raise ValueError(f"{what}: pred must be [C, h, w] or [1, C, h, w], got {tuple(pred.shape)}")
    if not 1 <= pred.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"{what}: {pred.shape[0]} channels (1 to {MAX_CHANNELS}: the objects of a sample and the background)")
    return pred


def _size(what, size):
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{what}: size {tuple(size)}")
    return H, W


def _labels(what, labels, n):
    """[H * W] int32 labels; an integer tensor of another type is converted (the reference hands over ``.long()`` masks)."""
    if not torch.is_tensor(labels) or labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.numel() != n:
        raise ValueError(f"{what}: labels must be an integer tensor of {n} elements")
    return ops._i32c(labels).reshape(-1)


def _plane(what, t, n, dtype=torch.float32):
    _in(what, t, dtype)
    if t.numel() != n:
        raise ValueError(f"{what} must hold {n} elements, got {t.numel()}")
    return t


def _word(what, t, dtype=torch.float32):
    return _plane(what, t, 1, dtype)


_FWD_OUTS = ("loss", "lse", "argmax", "valid_partial", "bad")


def upsample_ce_forward(pred, labels, size, ignore_index=IGNORE_INDEX, want=(True, True, True, False, False), out=None):
    """aoc_upsample_ce_forward: pred [C, h, w] float32, labels [H * W] integer, size (H, W) -> (loss [H * W], lse [H * W], argmax [H * W]
    int32, valid_partial [ceil(H W / 256)] int32, bad [1] int32); None where ``want`` is false and ``out`` (a dict of caller buffers by those
    names) has no buffer."""
    what = "upsample_ce_forward"
    pred = _pred3(what, pred)
    H, W = _size(what, size)
    n = H * W
    lab = _labels(what, labels, n)                               # bound until the launch is enqueued
    out = dict(out or {})
    L = _lib.lib()
    shapes = ((n,), (n,), (n,), (int(L.aoc_upsample_ce_partials(n)),), (1,))
    ops._need_gpu(pred, lab, *out.values())
    bufs = _wanted(what, _FWD_OUTS, shapes, want, out, pred, (torch.float32, torch.float32, torch.int32, torch.int32, torch.int32))
    C, h, w = pred.shape
    _lib.check(L.aoc_upsample_ce_forward(ops._p(pred), ops._p(lab), C, h, w, H, W, int(ignore_index), *(ops._p(b) for b in bufs), ops._stream()),
               "aoc_upsample_ce_forward")
    return bufs


def _check_k(what, k, n):
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f"{what}: k = {k} of {n} pixels (the reference returns NaN, the mean of nothing, at k = 0; here it is rejected)")
    return k


def topk_mean(loss, k, mean=None, thr=None, n_gt=None, want=(True, True, True)):
    """aoc_topk_mean: loss [n] float32, 1 <= k <= n -> (mean [1], thr [1], n_gt [1] int32) on the device; None where ``want`` is false and no
    buffer is given."""
    loss = _in("topk_mean: loss", loss).reshape(-1)
    n = loss.numel()
    if n < 1:
        raise ValueError("topk_mean: an empty loss")
    k = _check_k("topk_mean", k, n)
    ops._need_gpu(loss, mean, thr, n_gt)
    mean, thr, n_gt = _wanted("topk_mean", ("mean", "thr", "n_gt"), ((1,),) * 3, want, dict(mean=mean, thr=thr, n_gt=n_gt), loss,
                              (torch.float32, torch.float32, torch.int32))
    L = _lib.lib()
    ws = ops._ws(L.aoc_topk_mean_workspace_bytes(n), loss.device)
    _lib.check(L.aoc_topk_mean(ops._p(loss), n, k, ops._p(mean), ops._p(thr), ops._p(n_gt), ops._p(ws), ws.numel(), ops._stream()), "aoc_topk_mean")
    return mean, thr, n_gt


def valid_mean(loss, valid_partial, mean=None, n_valid=None):
    """aoc_valid_mean: loss [n], valid_partial as upsample_ce_forward returns it -> (mean = sum loss / n_valid [1], n_valid [1] int32)."""
    loss = _in("valid_mean: loss", loss).reshape(-1)
    n = loss.numel()
    L = _lib.lib()
    valid_partial = _plane("valid_mean: valid_partial", valid_partial, int(L.aoc_upsample_ce_partials(n)) if n else -1, torch.int32)
    ops._need_gpu(loss, valid_partial, mean, n_valid)
    mean, n_valid = _wanted("valid_mean", ("mean", "n_valid"), ((1,),) * 2, (True, True), dict(mean=mean, n_valid=n_valid), loss, (torch.float32, torch.int32))
    ws = ops._ws(L.aoc_topk_mean_workspace_bytes(n), loss.device)
    _lib.check(L.aoc_valid_mean(ops._p(loss), n, ops._p(valid_partial), valid_partial.numel(), ops._p(mean), ops._p(n_valid), ops._p(ws), ws.numel(),
                                ops._stream()), "aoc_valid_mean")
    return mean, n_valid


def topk_select_mask(loss, k, thr, n_gt, mask=None):
    """aoc_topk_select_mask: loss [n], k, the device words thr and n_gt of topk_mean -> mask [n] uint8 with exactly k bytes set."""
    loss = _in("topk_select_mask: loss", loss).reshape(-1)
    n = loss.numel()
    if n < 1:
        raise ValueError("topk_select_mask: an empty loss")
    k = _check_k("topk_select_mask", k, n)
    thr, n_gt = _word("topk_select_mask: thr", thr), _word("topk_select_mask: n_gt", n_gt, torch.int32)
    ops._need_gpu(loss, thr, n_gt, mask)
    mask, = _wanted("topk_select_mask", ("mask",), ((n,),), (True,), dict(mask=mask), loss, (torch.uint8,))
    L = _lib.lib()
    ws = ops._ws(L.aoc_topk_select_mask_workspace_bytes(n), loss.device)
    _lib.check(L.aoc_topk_select_mask(ops._p(loss), n, k, ops._p(thr), ops._p(n_gt), ops._p(mask), ops._p(ws), ws.numel(), ops._stream()),
               "aoc_topk_select_mask")
    return mask


def valid_mask(labels, channels, ignore_index=IGNORE_INDEX, mask=None):
    """aoc_valid_mask: mask [n] uint8 = the label is not ignore_index and lies in [0, channels)."""
    if not torch.is_tensor(labels) or labels.numel() < 1:
        raise ValueError("valid_mask: labels must be a non-empty integer tensor")
    n = labels.numel()
    lab = _labels("valid_mask", labels, n)
    if not 1 <= int(channels) <= MAX_CHANNELS:
        raise ValueError(f"valid_mask: {channels} channels (1 to {MAX_CHANNELS})")
    ops._need_gpu(lab, mask)
    mask, = _wanted("valid_mask", ("mask",), ((n,),), (True,), dict(mask=mask), lab, (torch.uint8,))
    _lib.check(_lib.lib().aoc_valid_mask(ops._p(lab), n, int(channels), int(ignore_index), ops._p(mask), ops._stream()), "aoc_valid_mask")
    return mask


def upsample_ce_backward(pred, labels, lse, mask, grad_out, size, k=None, n_valid=None, ignore_index=IGNORE_INDEX, grad_pred=None):
    """aoc_upsample_ce_grad: pred [C, h, w], labels, lse [H * W], mask [H * W] uint8, grad_out a device word; the divisor is ``k`` (an int) or
    the device word ``n_valid`` -> grad_pred [C, h, w]."""
    what = "upsample_ce_backward"
    pred = _pred3(what, pred)
    H, W = _size(what, size)
    n = H * W
    lab = _labels(what, labels, n)                               # bound until the launch is enqueued
    lse, mask, grad_out = _plane(what + ": lse", lse, n), _plane(what + ": mask", mask, n, torch.uint8), _word(what + ": grad_out", grad_out)
    if (k is None) == (n_valid is None):
        raise ValueError(f"{what}: give k or n_valid")
    k = _check_k(what, k, n) if k is not None else 0
    if n_valid is not None:
        _word(what + ": n_valid", n_valid, torch.int32)
    if grad_pred is not None:
        ops._out(what + ": grad_pred", grad_pred, pred.shape)
    ops._need_gpu(pred, lab, lse, mask, grad_out, n_valid, grad_pred)
    grad_pred = torch.empty_like(pred) if grad_pred is None else grad_pred
    C, h, w = pred.shape
    _lib.check(_lib.lib().aoc_upsample_ce_grad(ops._p(pred), ops._p(lab), ops._p(lse), ops._p(mask), ops._p(grad_out), k, ops._p(n_valid), C, h, w, H, W,
                                               int(ignore_index), ops._p(grad_pred), ops._stream()), "aoc_upsample_ce_grad")
    return grad_pred


def criterion_forward(pred, labels, size, k=None, ignore_index=IGNORE_INDEX, want_backward=True, want_bad=False):
    """aoc_criterion_forward: the forward of one sample as one call (the launches of upsample_ce_forward, then topk_mean + topk_select_mask,
    or with ``k=None`` valid_mean + valid_mask; the same bits) -> (mean [1], lse [H * W], argmax [H * W] int32, mask [H * W] uint8, n_valid [1]
    int32, bad [1] int32); lse and mask are None without ``want_backward``, n_valid with a ``k``, bad without ``want_bad``.  The per-pixel
    losses, thr and n_gt live in the call's workspace and are not returned."""
    what = "criterion_forward"
    pred = _pred3(what, pred)
    H, W = _size(what, size)
    n = H * W
    lab = _labels(what, labels, n)                               # bound until the launch is enqueued
    k = _check_k(what, k, n) if k is not None else 0
    ops._need_gpu(pred, lab)
    dev = pred.device
    L = _lib.lib()
    loss, arg, mean = torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, device=dev)
    lse = torch.empty(n, device=dev) if want_backward else None
    mask = torch.empty(n, dtype=torch.uint8, device=dev) if want_backward else None
    n_valid = torch.empty(1, dtype=torch.int32, device=dev) if k == 0 else None
    bad = torch.empty(1, dtype=torch.int32, device=dev) if want_bad else None
    ws = ops._ws(L.aoc_criterion_forward_workspace_bytes(n), dev)
    C, h, w = pred.shape
    _lib.check(L.aoc_criterion_forward(ops._p(pred), ops._p(lab), C, h, w, H, W, int(ignore_index), k, ops._p(loss), ops._p(lse), ops._p(arg), ops._p(mask),
                                       ops._p(mean), ops._p(n_valid), ops._p(bad), ops._p(ws), ws.numel(), ops._stream()), "aoc_criterion_forward")
    return mean, lse, arg, mask, n_valid, bad


# ------------------------------------------------------------------------------------------ autograd
class _UpsampleTopkCE(torch.autograd.Function):
    """pred [C, h, w] or [1, C, h, w], labels of H * W integers, (H, W), k (None: the mean over the valid pixels) -> (loss, a 0-d tensor;
    argmax [H * W] int32, not differentiable).  Saves pred, the int32 labels, lse and the mask, and only when pred wants a gradient."""

    @staticmethod
    def forward(ctx, pred, labels, size, k, ignore_index, check_labels):
        p3 = _pred3("_UpsampleTopkCE", ops._f32c(pred.detach()))
        H, W = _size("_UpsampleTopkCE", size)
        lab = _labels("_UpsampleTopkCE", labels, H * W)          # converted once: the int32 plane is what the backward reads
        need = ctx.needs_input_grad[0]
        mean, lse, arg, mask, n_valid, bad = criterion_forward(p3, lab, (H, W), k, ignore_index, want_backward=need, want_bad=bool(check_labels))
        if check_labels and int(bad):                            # reads a device word: synchronises
            raise ValueError(f"{int(bad)} labels lie outside [0, {p3.shape[0]}) and are not ignore_index = {ignore_index}")
        if need:
            ctx.save_for_backward(p3, lab, lse, mask, n_valid)
            ctx.cfg = ((H, W), k, int(ignore_index), tuple(pred.shape))
        ctx.mark_non_differentiable(arg)
        return mean.view(()), arg

    @staticmethod
    @once_differentiable                       # the gradient kernel builds no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_loss, _grad_arg):
        p3, lab, lse, mask, n_valid = ctx.saved_tensors
        size, k, ignore_index, shape = ctx.cfg
        grad_out = ops._f32c(grad_loss).reshape(1)
        grad = upsample_ce_backward(p3, lab, lse, mask, grad_out, size, k=k, n_valid=n_valid if k is None else None, ignore_index=ignore_index)
        return grad.view(shape), None, None, None, None, None


def top_k_pixels(top_k_percent_pixels, hard_example_mining_step, step, num_pixels):
    """loss.py:83-89 in its own double arithmetic; ``num_pixels`` an int."""
    num_pixels = float(num_pixels)
    if hard_example_mining_step == 0:
        return int(top_k_percent_pixels * num_pixels)
    ratio = min(1.0, step / float(hard_example_mining_step))
    return int((ratio * top_k_percent_pixels + (1.0 - ratio)) * num_pixels)


class Concat_CrossEntropyLoss(nn.Module):
    """loss.py:52-97 with the reference's constructor, so it drops into ``AOCNet.criterion``.  ``forward(dic_tmp, y, step)`` takes
    full-resolution logits ``[1, C, H, W]`` per sample (the identity geometry: the kernels read the logits through bit for bit);
    ``sample(pred, labels, step, size)`` is one sample at any geometry and returns ``(loss, argmax [1, H, W] int64)``."""

    def __init__(self, top_k_percent_pixels=None, hard_example_mining_step=100000, check_labels=False):
        super(Concat_CrossEntropyLoss, self).__init__()
        self.top_k_percent_pixels = top_k_percent_pixels
        if top_k_percent_pixels is not None:
            assert (top_k_percent_pixels > 0 and top_k_percent_pixels < 1)
        self.hard_example_mining_step = hard_example_mining_step
        self.ignore_index = IGNORE_INDEX
        self.check_labels = check_labels

    def sample(self, pred, labels, step, size=None):
        if pred.dim() != 4 or pred.shape[0] != 1:
            raise ValueError(f"Concat_CrossEntropyLoss: the logits of one sample are [1, C, h, w], got {tuple(pred.shape)}")
        H, W = (pred.shape[2], pred.shape[3]) if size is None else _size("Concat_CrossEntropyLoss", size)
        k = None
        if self.top_k_percent_pixels is not None:
            k = _check_k("Concat_CrossEntropyLoss", top_k_pixels(self.top_k_percent_pixels, self.hard_example_mining_step, step, H * W), H * W)
        ops._need_gpu(pred, labels)
        if not _wants_grad(pred):
            pred = pred.detach()                                 # under no_grad an input still says it wants a gradient: build no mask, save nothing
        loss, arg = _UpsampleTopkCE.apply(pred, labels, (H, W), k, self.ignore_index, self.check_labels)
        return loss, arg.view(1, H, W).long()

    def forward(self, dic_tmp, y, step):
        return torch.stack([self.sample(dic_tmp[i], y[i], step)[0] for i in range(len(dic_tmp))])


def upsampled_criterion(criterion, tmp_dic, current_frame_mask, step, size):
    """The fused form of aocnet.py:71-82 with the criterion behind it: the coarse logits ``tmp_dic[i]`` [1, C_i, h, w] of every sample, the
    label maps ``current_frame_mask[i]`` ([1, H, W] or [H, W], any integer type, or the reference's float maps of integers) and ``size``
    (H, W) -> (losses [bs], all_pred [bs, H, W] int64).  One set of launches per sample (the samples have different C_i), and the upsampled
    logits are never formed."""
    losses, preds = [], []
    for i in range(len(tmp_dic)):
        lab = current_frame_mask[i]
        if lab.dtype.is_floating_point:
            lab = lab.to(torch.int32)                            # aocnet.py:76 `.long()`
        loss, arg = criterion.sample(tmp_dic[i], lab, step, size)
        losses.append(loss)
        preds.append(arg)
    return torch.stack(losses), torch.cat(preds, dim=0)
