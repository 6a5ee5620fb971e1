"""Differentiable twin of the reference's adaptive-proxy matching (networks/layers/matching.py == AEM): ``global_matching_cluster2``
(AEM:405-478 over AEM:231-332; matching.py:1324-1404 over 506-640, aocnet.py:305), same positional order and defaults, plus the trailing
keywords ``init_rows`` and ``cluster_num`` of ``aoc_amd.matching.global_matching_for_eval_cluster``.

What autograd sees in the reference: set 0 of an object, the k-means code book, is ``torch.from_numpy(centroid)`` (AEM:279), a constant --
only the query and the bias get a gradient through it; set 1, ``centroid_avg`` (AEM:280), is a mean of reference rows, so the gradient
reaches ``reference_embeddings`` -- through the reference's own indexing (segment-local positions into the global kept-row array), which
``aoc_build_proxies`` reproduces and ``aoc_centroid_avg_grad`` pulls back through.  Labels, the k-means assignment and the drawn rows carry
no gradient: the device k-means chain (bit-identical to scipy's kmeans2) runs without a graph.  The forward is the set minimum that also
reports the winning slot (aoc_proxy_set_match_argmin); the backward needs only that slot, the saved output T, the operands and the
cluster state (csrc/cluster_grad.hip):

    g = grad_out (1 - T^2) / 2,   grad_query = sum_s 2 g (q - p*),   grad_proxy[p*] += 2 g (p* - q),   grad_bias[o] = sum g,
    grad_ref[fg[p]] = sum_s grad_proxy[s, 1, label_s[p]] / count_s(label_s[p])

No float atomics, every sum in a fixed order: two runs give the same bits.  When autograd is off, or no input wants a gradient,
``aoc_amd.matching.global_matching_cluster2``'s result is returned unchanged.  Labels are never written into.  ``n_chunks`` is accepted and
ignored.  ``use_float16=True`` has no backward (and no clustering either: scipy rejects float16, AEM:275-286).

This is a module of its own because ``aoc_amd.matching_train.global_matching_cluster2`` is pinned as a raising stub; see STATUS.md.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import matching, ops
from .matching import DEFAULT_CLUSTER_NUM
from .matching_train import _bias_arg, _guard
from .ops import _wants_grad


def _plane_sets(levels, n_obj, kmax, m):
    """The sets of matching.global_matching_for_eval_cluster, in its order: (level l, object o, centroid | centroid_avg f) is proxy rows
    ((l O + o) 2 + f) kmax .. + K_l and lands in plane o 2L + 2l + f (AEM:599-612 per level).  -> begin, size, offset, object."""
    L = len(levels)
    begin, size, off, obj = [], [], [], []
    for l, k in enumerate(levels):
        for o in range(n_obj):
            for f in range(2):
                begin.append(((l * n_obj + o) * 2 + f) * kmax)
                size.append(min(k, kmax))
                off.append((o * 2 * L + 2 * l + f) * m)
                obj.append(o)
    return begin, size, off, obj


class _ClusterMatch(torch.autograd.Function):
    """planes [O * 2L, m] = T of the nearest proxy of every (object, level, set) (AEM:316-319, 467-468); saves T, the winning slots, the
    operands and the cluster state (proxies, packed labels, segment offsets)."""

    @staticmethod
    def forward(ctx, query_flat, pool, bias, cp):
        q, p, b = ops._f32c(query_flat.detach()), ops._f32c(pool.detach()), ops._f32c(bias.detach())
        m, C = q.shape
        prep, levels = cp["prep"], cp["levels"]
        n_obj, kmax = prep.n_obj, cp["proxies"].shape[2]
        begin, size, off, obj = _plane_sets(levels, n_obj, kmax, m)
        planes = torch.empty(len(begin), m, dtype=torch.float32, device=q.device)
        arg = torch.empty(len(begin), m, dtype=torch.int32, device=q.device)
        proxies = cp["proxies"].reshape(-1, C)
        ops.proxy_set_match_argmin(q, proxies, cp["proxy_sqnorm"].reshape(-1), begin, size, off, b[torch.tensor(obj, device=q.device)], planes, arg, 1, True)
        seg_k = [k for lv in (cp["seg_k"] if isinstance(cp["seg_k"][0], (list, tuple)) else [cp["seg_k"]]) for k in lv]
        ctx.save_for_backward(q, p, planes, arg, proxies, cp["labels"], cp["seg_offsets"], prep.fg_rows, prep.counts,
                              torch.tensor(seg_k, dtype=torch.int32, device=q.device))
        ctx.sets = (begin, size, off, obj)
        ctx.shape = (n_obj, len(levels), kmax)
        return planes

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_planes):
        q, p, T, arg, proxies, labels, seg_offsets, fg_rows, counts, seg_k = ctx.saved_tensors
        begin, size, off, obj = ctx.sets
        n_obj, L, kmax = ctx.shape
        want_q, want_p, want_b = ctx.needs_input_grad[:3]
        gq, gpx, gb = ops.proxy_set_match_backward(ops._f32c(grad_planes), T, arg, 1, q, proxies, begin, size, off, obj, n_obj, want_q, want_p, want_b)
        gp = None
        if want_p:
            gp = ops.centroid_avg_backward(gpx.view(L * n_obj, 2, kmax, -1), fg_rows, counts[n_obj:n_obj + 1], seg_offsets, seg_k, labels, p.shape[0])
        return gq, gp, gb, None


def global_matching_cluster2(reference_embeddings, query_embeddings, reference_labels,
                             n_chunks=100, dis_bias=0., ori_size=None, atrous_rate=1, use_float16=True, atrous_obj_pixel_num=0,
                             init_rows=None, cluster_num=DEFAULT_CLUSTER_NUM):
    """AEM:405-478 with a backward for reference_embeddings, query_embeddings and a tensor dis_bias.  -> [1, H, W, O, 2]; a sequence of
    levels as ``cluster_num`` gives [1, H, W, O, 2 * levels].  ``init_rows``: the rows k-means starts from (matching.cluster_proxies'
    ``init_rows``); None draws them from numpy's global RandomState as scipy's kmeans2 does."""
    if not _wants_grad(reference_embeddings, query_embeddings, dis_bias):
        if init_rows is None and cluster_num == DEFAULT_CLUSTER_NUM:
            return matching.global_matching_cluster2(reference_embeddings, query_embeddings, reference_labels, n_chunks, dis_bias, ori_size,
                                                     atrous_rate, use_float16, atrous_obj_pixel_num)
        assert reference_embeddings.size()[:2] == reference_labels.size()[:2]     # AEM:430
        h, w, _ = query_embeddings.size()
        labels = matching._train_twin_labels(reference_labels, h, w, atrous_rate, atrous_obj_pixel_num)
        out = matching.global_matching_for_eval_cluster([reference_embeddings], query_embeddings, [labels], n_chunks, dis_bias, ori_size, 1,
                                                        use_float16, 0, init_rows, cluster_num)
        return torch.ones(1, h, w, reference_labels.size(2), 2, device=query_embeddings.device) if out.shape[-1] == 1 else out
    _guard("global_matching_cluster2", use_float16, reference_embeddings, query_embeddings, reference_labels, dis_bias, module="cluster_train",
           why="scipy's kmeans2 rejects float16 and the reference degrades to a constant, AEM:275-286")
    assert reference_embeddings.size()[:2] == reference_labels.size()[:2]         # AEM:430
    h, w, embedding_dim = query_embeddings.size()
    obj_nums = reference_labels.size(2)
    dev = query_embeddings.device
    levels, _ = matching._level_list(cluster_num)
    labels = matching._train_twin_labels(reference_labels.detach(), h, w, atrous_rate, atrous_obj_pixel_num)      # AEM:437-446
    pool, labels_flat = matching._flatten_pool([reference_embeddings], [labels], h, w, 1, 0)
    with torch.no_grad():                                                         # labels, assignment and drawn rows carry no gradient
        cp = matching.cluster_proxies(pool.detach(), labels_flat, cluster_num, init_rows)
    if cp is None:
        return torch.ones(1, h, w, obj_nums, 2, device=dev)                       # AEM:455-456
    planes = _ClusterMatch.apply(query_embeddings.reshape(-1, embedding_dim), pool, _bias_arg(dis_bias, obj_nums, dev), cp)
    n_planes = 2 * len(levels)
    x = planes.view(obj_nums * n_planes, 1, h, w)
    if ori_size is not None and (int(ori_size[0]), int(ori_size[1])) != (h, w):
        x = F.interpolate(x, size=(int(ori_size[0]), int(ori_size[1])), mode="bilinear", align_corners=True)     # AEM:604-607
    return x.permute(2, 3, 0, 1).reshape(1, x.shape[2], x.shape[3], obj_nums, n_planes)


global_matching_cluster = global_matching_cluster2   # aocnet.py:6 imports the ...2 name; AEM:405 defines the other
