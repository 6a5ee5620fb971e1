"""Differentiable twins of the reference's local matching (networks/layers/matching.py == AEM): ``local_matching`` (AEM:968-1060,
aocnet.py:255) and ``local_matching_proxy`` (AEM:1064-1156, a verbatim copy; aocnet.py:328), same positional order and defaults.

The reference unfolds the previous frame into [HW, C, (2R+1)^2] (AEM:955-961) and autograd keeps that tensor, the masked distance volume
[H, W, (2R+1)^2, O] and one more copy per nested window.  Here the forward is the fused HIP kernel that also reports the winning
previous-frame pixel of every window (aoc_local_window_match_argmin) and the backward needs only that pixel, the saved output T and the
two maps (csrc/local_grad.hip):

    g = grad_out (1 - T^2) / 2,   grad_query[i] = sum 2 g (q_i - p*),   grad_prev[p*] += 2 g (p* - q_i),   grad_bias = sum g

``torch.min`` sends the gradient of a tie to one position; so does the kernel (the first in row-major window order).  The three sums run in
a fixed order without float atomics: the two entries give the same bits on the same buffers.  The bilinear resizes around them
(AEM:938-941, 1054-1058) are torch's own ``F.interpolate``, which torch differentiates (its backward adds atomically).

When autograd is off, or no input wants a gradient, ``aoc_amd.matching.local_matching``'s result is returned unchanged.  Labels are never
differentiated and never written into.  ``allow_parallel`` is accepted and ignored: the parallel path's semantics are the contract (the
reference's for-loop path, AEM:875-919, shadows both embeddings with its loop variables; under autograd its query gets no gradient).
``use_float16=True`` has no backward (the model trains with MODEL_FLOAT16_MATCHING = False).  ``matmul(labels, prev_head_pos)`` of
aocnet.py:325 stays the caller's torch op: its result is the ``prev_frame_embedding`` of ``local_matching_proxy``.

This is a module of its own because ``aoc_amd.matching_train.local_matching`` is pinned as a raising stub; see STATUS.md.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import matching, ops
from .matching_train import _bias_arg, _guard
from .ops import _wants_grad


class _LocalMatch(torch.autograd.Function):
    """planes [O, n_radii, H, W] = T of the nearest right pixel per object and nested window (AEM:1032-1049); saves T, the winning pixels
    and the two maps."""

    @staticmethod
    def forward(ctx, query, prev, bias, right_bits, radii, atrous_rate):
        q, p, b = ops._f32c(query.detach()), ops._f32c(prev.detach()), ops._f32c(bias.detach())
        planes, arg = ops.local_window_match_argmin(q, p, right_bits, radii, b, b.numel(), True, atrous_rate=atrous_rate)
        ctx.save_for_backward(q, p, planes, arg)
        ctx.window = atrous_rate * (radii[-1] // atrous_rate)          # AEM:949 pad_max_distance
        return planes

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_planes):
        q, p, T, arg = ctx.saved_tensors
        want_q, want_p, want_b = ctx.needs_input_grad[:3]
        gq, gp, gb = ops.local_match_backward(ops._f32c(grad_planes), T, arg, q, p, ctx.window, want_q, want_p, want_b)
        return gq, gp, gb, None, None, None


def _down(x, H, W):
    """AEM:936-941: [h, w, C] -> [H, W, C] through torch's bilinear interpolate (align_corners=True), kept in the graph."""
    y = F.interpolate(x.float().permute(2, 0, 1).unsqueeze(0), size=(H, W), mode="bilinear", align_corners=True)
    return y.squeeze(0).permute(1, 2, 0).contiguous()


def local_matching(prev_frame_embedding, query_embedding, prev_frame_labels, dis_bias=0., multi_local_distance=[15],
                   ori_size=None, atrous_rate=1, use_float16=True, allow_downsample=True, allow_parallel=True):
    """AEM:968-1060 with a backward for prev_frame_embedding, query_embedding and a tensor dis_bias.
    -> [1, H, W, O, len(multi_local_distance)], channel order [max, d_0, d_1, ...]."""
    if not _wants_grad(prev_frame_embedding, query_embedding, dis_bias):
        return matching.local_matching(prev_frame_embedding, query_embedding, prev_frame_labels, dis_bias, multi_local_distance, ori_size,
                                       atrous_rate, use_float16, allow_downsample, allow_parallel)
    _guard("local_matching", use_float16, prev_frame_embedding, query_embedding, prev_frame_labels, dis_bias, module="local_train")
    h, w, _ = prev_frame_embedding.size()
    ori_size = (h, w) if ori_size is None else (int(ori_size[0]), int(ori_size[1]))
    obj_num = prev_frame_labels.size(2)
    dev = query_embedding.device
    radii = [int(r) for r in multi_local_distance]
    rate = int(atrous_rate)
    right, _ = ops.label_bits(prev_frame_labels.detach().reshape(-1, obj_num), want_wrong=False)
    if allow_downsample:
        H, W = int(h / 2) + 1, int(w / 2) + 1                              # AEM:939
        q, p = _down(query_embedding, H, W), _down(prev_frame_embedding, H, W)
    else:
        H, W = h, w
        q, p = query_embedding, prev_frame_embedding
    if (H, W) != ori_size:
        right = ops.resize_nearest_bits(right, h, w, H, W)                 # AEM:1017-1018: 'nearest' from the labels' own size
    elif (H, W) != (h, w):
        raise ValueError("local_matching: label map and distance map sizes differ")   # the reference would fail in unfold too
    planes = _LocalMatch.apply(q, p, _bias_arg(dis_bias, obj_num, dev), right, radii, rate)       # [O, nr, H, W]
    if (H, W) != ori_size:
        planes = F.interpolate(planes, size=ori_size, mode="bilinear", align_corners=True)     # AEM:1054-1056
    return planes.permute(2, 3, 0, 1).reshape(1, ori_size[0], ori_size[1], obj_num, len(radii))   # AEM:1057-1058


local_matching_proxy = local_matching   # AEM:1064-1156 is a verbatim copy of AEM:968-1060
