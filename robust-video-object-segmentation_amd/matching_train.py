"""Differentiable twins of the reference's training-time global matching (networks/layers/matching.py == AEM): ``global_matching``
(AEM:616-685, aocnet.py:170) and ``global_matching_proxy`` (AEM:336-402, aocnet.py:216), same positional order and defaults.

The reference materialises the [m, O, n] distance tensor per chunk and autograd keeps it for the backward.  Here the forward is the fused
HIP kernel that also reports the winning pool row (aoc_dense_match_argmin; for the k = 1 proxies aoc_proxy_corr_min, there is no min) and
the backward needs only that row, the saved output T and the operands (csrc/match_grad.hip):

    g = grad_out (1 - T^2) / 2,   grad_query = sum_o 2 g (q - r*),   grad_ref[r*] += 2 g (r* - q),   grad_bias = sum_i g

``torch.min`` sends the gradient of a tie to one row; so does the kernel (the lowest row).  grad_ref and grad_bias are summed in a fixed
order without float atomics: two runs give the same bits.

When autograd is off, or no input wants a gradient, every function here returns ``aoc_amd.matching``'s result unchanged.  Labels are never
differentiated and never written into (the reference writes its atrous mask into the caller's tensor).  ``n_chunks`` is accepted and
ignored.  ``use_float16=True`` has no backward (the model trains with MODEL_FLOAT16_MATCHING = False).  ``global_matching_cluster2`` and
``local_matching`` are here so that an aliased import fails loudly: they are differentiable in ``aoc_amd.cluster_train`` and
``aoc_amd.local_train`` (modules of their own until the stubs below may go; their error texts point there).
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, matching, ops
from .ops import _wants_grad


def _guard(what, use_float16, *tensors, module="matching_train", why="the `.half()` matching mode is inference-only"):
    """The float16 refusal and the device check of a differentiable matching; ``module`` and ``why`` fill local_train's and cluster_train's texts."""
    if use_float16:
        raise _lib.AocHipError(f"aoc_amd.{module}.{what}: use_float16=True has no backward ({why}); "
                               "pass use_float16=False, as the model does with MODEL_FLOAT16_MATCHING = False")
    ops._need_gpu(*[t for t in tensors if torch.is_tensor(t)])


def _bias_arg(dis_bias, obj_nums, device):
    """matching._bias_vec's shapes, kept in the graph: [O, 1, 1, 1] (aocnet.py:144) or one element expanded to O objects (autograd then sums
    the expanded gradient back into the one element); a float becomes a constant."""
    if torch.is_tensor(dis_bias):
        b = dis_bias.to(device=device, dtype=torch.float32).reshape(-1)
        if b.numel() == 1 and obj_nums > 1:
            b = b.expand(obj_nums)
        return b
    return torch.full((obj_nums,), float(dis_bias), dtype=torch.float32, device=device)


def _emit(planes, h, w, obj_nums, ori_size):
    """planes [O, h * w] -> [1, H, W, O, 1] (AEM:675-681); a real resize goes through torch's own interpolate, which torch differentiates."""
    x = planes.view(obj_nums, 1, h, w)
    if ori_size is not None and (int(ori_size[0]), int(ori_size[1])) != (h, w):
        x = F.interpolate(x, size=(int(ori_size[0]), int(ori_size[1])), mode="bilinear", align_corners=True)
    return x.permute(2, 3, 0, 1).reshape(1, x.shape[2], x.shape[3], obj_nums, 1)


class _DenseMatch(torch.autograd.Function):
    """planes [O, m] = T of the nearest kept reference row per object (AEM:671-676); saves T, the winning rows and the operands."""

    @staticmethod
    def forward(ctx, query_flat, pool, bias, prep):
        q, p, b = ops._f32c(query_flat.detach()), ops._f32c(pool.detach()), ops._f32c(bias.detach())
        m = q.shape[0]
        planes = torch.empty(prep.n_obj, m, dtype=torch.float32, device=q.device)
        arg = torch.empty(prep.n_obj, m, dtype=torch.int32, device=q.device)
        ops.dense_match_argmin(q, p, prep, b, planes, arg, 1, m, True)
        ctx.save_for_backward(q, p, planes, arg)
        return planes

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_planes):
        q, p, T, arg = ctx.saved_tensors
        n_obj, m = T.shape
        want_q, want_p, want_b = ctx.needs_input_grad[:3]
        gq, gp, gb = ops.dense_match_backward(ops._f32c(grad_planes), T, arg, 1, m, q, p, n_obj, want_q, want_p, want_b)
        return gq, gp, gb, None


class _ProxyMatch(torch.autograd.Function):
    """planes [O, m] = T of the distance to each object's single proxy (AEM:388-393)."""

    @staticmethod
    def forward(ctx, query_flat, proxies, bias):
        q, p, b = ops._f32c(query_flat.detach()), ops._f32c(proxies.detach()), ops._f32c(bias.detach())
        m, n_obj = q.shape[0], p.shape[0]
        planes = torch.empty(n_obj, m, dtype=torch.float32, device=q.device)
        ops.proxy_corr_min(q, p, None, list(range(n_obj)), [1] * n_obj, [o * m for o in range(n_obj)], b, planes, 1, True)
        ctx.save_for_backward(q, p, planes)
        return planes

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_planes):
        q, p, T = ctx.saved_tensors
        want_q, want_p, want_b = ctx.needs_input_grad[:3]
        return ops.proxy_match_backward(ops._f32c(grad_planes), T, 1, T.shape[1], q, p, want_q, want_p, want_b)


def global_matching(reference_embeddings, query_embeddings, reference_labels,
                    n_chunks=100, dis_bias=0., ori_size=None, atrous_rate=1, use_float16=True, atrous_obj_pixel_num=0):
    """AEM:616-685 with a backward for reference_embeddings, query_embeddings and a tensor dis_bias.  -> [1, H, W, O, 1]."""
    if not _wants_grad(reference_embeddings, query_embeddings, dis_bias):
        return matching.global_matching(reference_embeddings, query_embeddings, reference_labels, n_chunks, dis_bias, ori_size, atrous_rate,
                                        use_float16, atrous_obj_pixel_num)
    _guard("global_matching", use_float16, reference_embeddings, query_embeddings, reference_labels, dis_bias)
    assert reference_embeddings.size()[:2] == reference_labels.size()[:2]     # AEM:641
    h, w, embedding_dim = query_embeddings.size()
    obj_nums = reference_labels.size(2)
    dev = query_embeddings.device
    labels = matching._train_twin_labels(reference_labels.detach(), h, w, atrous_rate, atrous_obj_pixel_num)      # AEM:648-657
    pool, labels_flat = matching._flatten_pool([reference_embeddings], [labels], h, w, 1, 0)
    prep = ops.label_prep(labels_flat)
    if int(prep.counts[obj_nums]) == 0:
        return torch.ones(1, h, w, obj_nums, 1, device=dev)                   # AEM:666-667
    planes = _DenseMatch.apply(query_embeddings.reshape(-1, embedding_dim), pool, _bias_arg(dis_bias, obj_nums, dev), prep)
    return _emit(planes, h, w, obj_nums, ori_size)


def global_matching_proxy(reference_embeddings, query_embeddings, reference_labels,
                          n_chunks=100, dis_bias=0., ori_size=None, atrous_rate=1, use_float16=True, atrous_obj_pixel_num=0):
    """AEM:336-402 with a backward: ``reference_embeddings`` is the [O, C] tensor of mean-pooled proxies (aocnet.py:314-315)."""
    if not _wants_grad(reference_embeddings, query_embeddings, dis_bias):
        return matching.global_matching_proxy(reference_embeddings, query_embeddings, reference_labels, n_chunks, dis_bias, ori_size,
                                              atrous_rate, use_float16, atrous_obj_pixel_num)
    _guard("global_matching_proxy", use_float16, reference_embeddings, query_embeddings, reference_labels, dis_bias)
    h, w, embedding_dim = query_embeddings.size()
    obj_nums = reference_labels.size(2)
    dev = query_embeddings.device
    labels = matching._train_twin_labels(reference_labels.detach(), h, w, atrous_rate, atrous_obj_pixel_num)      # AEM:368-377
    right, _ = ops.label_bits(labels.reshape(-1, obj_nums), want_wrong=False)
    if not bool((right < 0).any()):
        return torch.ones(1, h, w, obj_nums, 1, device=dev)                   # AEM:385-386
    planes = _ProxyMatch.apply(query_embeddings.reshape(-1, embedding_dim), reference_embeddings.float(), _bias_arg(dis_bias, obj_nums, dev))
    return _emit(planes, h, w, obj_nums, ori_size)


def _not_yet(name, fn, elsewhere=None):
    def wrapper(*args, **kwargs):
        if _wants_grad(*args, *kwargs.values()):
            tail = f"; aoc_amd.{elsewhere} is the differentiable form" if elsewhere else ""
            raise _lib.AocHipError(f"aoc_amd.matching_train.{name} is not yet differentiable (only global_matching and global_matching_proxy "
                                   "have a backward): keep the reference's own function for it in a training run" + tail)
        return fn(*args, **kwargs)
    wrapper.__name__ = name
    wrapper.__doc__ = f"aoc_amd.matching.{name} when no gradient is wanted; raises under autograd (not yet differentiable)."
    return wrapper


global_matching_cluster2 = _not_yet("global_matching_cluster2", matching.global_matching_cluster2, "cluster_train.global_matching_cluster2")
local_matching = _not_yet("local_matching", matching.local_matching, "local_train.local_matching")
