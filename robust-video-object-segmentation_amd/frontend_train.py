"""Differentiable front end of ``before_seghead_process`` for one training sample (networks/aoc/aocnet.py:141-358): the glue between the
five differentiable matchers (``matching_train``, ``local_train``, ``cluster_train``) -- the mean-pooled attention heads
(networks/layers/attention.py == ATT:79-153), ``foreground2background`` (networks/layers/matching.py == AEM:9-23) and the concatenation
of aocnet.py:341-358 -- and ``proto_mask_features``, which wires all of it from the three embeddings to the proto-mask tensor.

What the reference keeps for its backward here: ``emb * label`` at [O, C, h, w] per frame (ATT:136, 144), and per object one
concatenation of the other objects' maps plus the index tensor of its ``torch.min`` (AEM:13-20), for the global map and for every local
radius.  The kernels of csrc/frontend_grad.hip keep none of them:

    pooling      grad_emb[c,p] = sum_o ( gpos[o,c] l[o,p] / (Np_o + eps) + gneg[o,c] (1 - l[o,p]) / (Nn_o + eps) )     saves the labels
    fg2bg        grad_dis[winner(o,x)] += grad_out[o,x]; the winners are recomputed from the saved dis                   saves dis
    aggregate    grad_fg[o'] = g_fg[o'] + sum_{o: winner(o) = o'} g_bg[o]; the winners are read off the saved feat       saves feat

Every sum runs in ascending object order without float atomics: two runs give the same bits.  Among equal minima the lowest (object,
channel) of the reference's concatenation order wins -- ``torch.min`` also sends the gradient of a tie to one entry; which one it picks
is not specified, and where the matchers saturate (T == 1.0f where nothing is labelled) the choice meets a factor 1 - T^2 = 0.

When autograd is off, or no input wants a gradient, the heads and ``foreground2background`` return the inference mirror's result
unchanged.  Labels and ``epsilon`` are never differentiated.  ``use_float16=True`` has no backward.  All backwards are
``once_differentiable``.  The ctypes wrappers of the new entry points live here, not in ``ops`` (whose public names are a tested table);
they keep ``ops``' tensor contract: inputs converted by ``_f32c`` into names that live until the call, caller outputs checked by ``_out``,
addresses only through ``_p``.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib, attention, cluster_train, local_train, matching, matching_train, ops
from .matching import DEFAULT_CLUSTER_NUM
from .ops import _wants_grad


# ------------------------------------------------------------------------------------------ the C ABI
def masked_mean_pool_backward(grad_pos, grad_neg, labels, epsilon, pixel_major=False, grad_emb=None):
    """aoc_masked_mean_pool_grad: grad_pos [O, C], grad_neg [O, C] or None, labels [O, hw] (or [hw, O] with pixel_major)
    -> grad_emb [C, hw]."""
    grad_pos, labels = ops._f32c(grad_pos), ops._f32c(labels)
    if grad_neg is not None:
        grad_neg = ops._f32c(grad_neg)
    ops._need_gpu(grad_pos, grad_neg, labels, grad_emb)
    n_obj, C = grad_pos.shape
    hw = labels.shape[0] if pixel_major else labels.shape[1]
    if tuple(labels.shape) != ((hw, n_obj) if pixel_major else (n_obj, hw)) or (grad_neg is not None and grad_neg.shape != grad_pos.shape):
        raise ValueError(f"masked_mean_pool_backward: labels {tuple(labels.shape)} / grad_neg do not fit grad_pos {tuple(grad_pos.shape)}")
    if grad_emb is None:
        grad_emb = torch.empty(C, hw, dtype=torch.float32, device=grad_pos.device)
    ops._out("masked_mean_pool_backward: grad_emb", grad_emb, (C, hw))
    L = _lib.lib()
    ws = ops._ws(L.aoc_masked_mean_pool_grad_workspace_bytes(n_obj), grad_pos.device)
    _lib.check(L.aoc_masked_mean_pool_grad(ops._p(grad_pos), ops._p(grad_neg), ops._p(labels), hw, C, n_obj, int(bool(pixel_major)), float(epsilon),
                                           ops._p(grad_emb), ops._p(ws), ws.numel(), ops._stream()), "aoc_masked_mean_pool_grad")
    return grad_emb


def fg2bg_backward(grad_out, dis, n_obj, grad_dis=None):
    """aoc_fg2bg_grad: grad_out [O, 1, ...], the forward's dis [O, c, ...] -> grad_dis [O, c, ...]."""
    grad_out, dis = ops._f32c(grad_out), ops._f32c(dis)
    ops._need_gpu(grad_out, dis, grad_dis)
    if dis.dim() < 2 or dis.numel() == 0 or n_obj < 2:
        raise ValueError(f"fg2bg_backward: dis must be a non-empty [O, c, ...] tensor of at least two objects, got {tuple(dis.shape)} for {n_obj} objects")
    n_ch = dis.shape[1]
    inner = dis.numel() // (n_obj * n_ch)
    if dis.shape[0] != n_obj or grad_out.numel() != n_obj * inner:
        raise ValueError(f"fg2bg_backward: grad_out {tuple(grad_out.shape)} does not fit dis {tuple(dis.shape)} for {n_obj} objects")
    if grad_dis is None:
        grad_dis = torch.empty_like(dis)
    ops._out("fg2bg_backward: grad_dis", grad_dis, dis.shape)
    _lib.check(_lib.lib().aoc_fg2bg_grad(ops._p(grad_out), inner, ops._p(dis), n_obj, n_ch, inner, n_ch * inner, ops._p(grad_dis), n_ch * inner,
                                         ops._stream()), "aoc_fg2bg_grad")
    return grad_dis


def aggregate_channels(n_cluster, n_local, matching_background=True):
    """Channels of the proto-mask tensor, aocnet.py:355-358."""
    return 1 + int(n_cluster) + 1 + 2 * int(n_local) + 1 + ((int(n_local) + 1) if matching_background else 0)


def _aggregate_shapes(what, global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg):
    n_obj, hw = global_fg.shape[0], global_fg.shape[-1]
    n_cluster, n_local = cluster_fg.shape[1], local_fg.shape[1]
    for name, t, k in (("global_fg", global_fg, 1), ("cluster_fg", cluster_fg, n_cluster), ("proxy_fg", proxy_fg, 1), ("local_fg", local_fg, n_local),
                       ("local_proxy_fg", local_proxy_fg, n_local)):
        if tuple(t.shape) != (n_obj, k, hw):
            raise ValueError(f"{what}: {name} must be [O, k, hw] = {(n_obj, k, hw)}, got {tuple(t.shape)}")
    return n_obj, hw, n_cluster, n_local


def proto_aggregate(global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg, prev_label, matching_background=True, feat=None):
    """aoc_proto_aggregate: the five matching outputs as planes [O, k_i, hw] and the previous-frame label [O, hw] -> feat [O, n_ch, hw]."""
    global_fg, cluster_fg, proxy_fg = ops._f32c(global_fg), ops._f32c(cluster_fg), ops._f32c(proxy_fg)
    local_fg, local_proxy_fg, prev_label = ops._f32c(local_fg), ops._f32c(local_proxy_fg), ops._f32c(prev_label)
    ops._need_gpu(global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg, prev_label, feat)
    n_obj, hw, n_cluster, n_local = _aggregate_shapes("proto_aggregate", global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg)
    if tuple(prev_label.shape) != (n_obj, hw):
        raise ValueError(f"proto_aggregate: prev_label must be [O, hw] = {(n_obj, hw)}, got {tuple(prev_label.shape)}")
    n_ch = aggregate_channels(n_cluster, n_local, matching_background)
    if feat is None:
        feat = torch.empty(n_obj, n_ch, hw, dtype=torch.float32, device=global_fg.device)
    ops._out("proto_aggregate: feat", feat, (n_obj, n_ch, hw))
    _lib.check(_lib.lib().aoc_proto_aggregate(ops._p(global_fg), ops._p(cluster_fg), ops._p(proxy_fg), ops._p(local_fg), ops._p(local_proxy_fg),
                                              ops._p(prev_label), n_obj, hw, n_cluster, n_local, int(bool(matching_background)), ops._p(feat),
                                              ops._stream()), "aoc_proto_aggregate")
    return feat


def proto_aggregate_backward(grad_feat, feat, n_cluster, n_local, matching_background=True, want=(True,) * 5):
    """aoc_proto_aggregate_grad: grad_feat and the saved feat [O, n_ch, hw] -> the gradients of (global, cluster, proxy, local, local proxy) as
    planes [O, k_i, hw]; None where ``want`` is false."""
    grad_feat, feat = ops._f32c(grad_feat), ops._f32c(feat)
    ops._need_gpu(grad_feat, feat)
    n_obj, n_ch, hw = feat.shape
    if n_ch != aggregate_channels(n_cluster, n_local, matching_background) or grad_feat.shape != feat.shape:
        raise ValueError(f"proto_aggregate_backward: feat {tuple(feat.shape)} / grad_feat {tuple(grad_feat.shape)} do not fit "
                         f"{n_cluster} cluster and {n_local} local channels")
    g_global, g_cluster, g_proxy, g_local, g_local_proxy = (
        torch.empty(n_obj, k, hw, dtype=torch.float32, device=feat.device) if w else None
        for k, w in zip((1, n_cluster, 1, n_local, n_local), want))
    _lib.check(_lib.lib().aoc_proto_aggregate_grad(ops._p(grad_feat), ops._p(feat), n_obj, hw, int(n_cluster), int(n_local), int(bool(matching_background)),
                                                   ops._p(g_global), ops._p(g_cluster), ops._p(g_proxy), ops._p(g_local), ops._p(g_local_proxy),
                                                   ops._stream()), "aoc_proto_aggregate_grad")
    return g_global, g_cluster, g_proxy, g_local, g_local_proxy


# ------------------------------------------------------------------------------------------ foreground2background
class _Fg2Bg(torch.autograd.Function):
    """[O, c, ...] -> [O, 1, ...] by aoc_fg2bg_min; saves dis, no index tensor."""

    @staticmethod
    def forward(ctx, dis, obj_num):
        d = ops._f32c(dis.detach())
        ctx.save_for_backward(d)
        ctx.obj_num = obj_num
        return ops.fg2bg_min(d, obj_num)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_out):
        d, = ctx.saved_tensors
        return fg2bg_backward(grad_out, d, ctx.obj_num), None


def foreground2background(dis, obj_num):
    """AEM:9-23 with a backward for dis.  dis [O, c, ...] -> [O, 1, ...]; one object is the identity (AEM:10-11)."""
    if obj_num == 1:
        return dis
    if not _wants_grad(dis):
        return matching.foreground2background(dis, obj_num)
    ops._need_gpu(dis)
    return _Fg2Bg.apply(dis, int(obj_num))


# ------------------------------------------------------------------------------------------ attention heads
class _Pool(torch.autograd.Function):
    """One frame's embedding [C, h, w] and labels [O, hw] -> (pos, neg) [O, C] by aoc_masked_mean_pool; saves the labels only.  The
    channel-last copy the forward kernel reads is made here, outside the graph."""

    @staticmethod
    def forward(ctx, emb, labels, epsilon):
        e = ops._f32c(emb.detach())
        channel_last = e.reshape(e.shape[0], -1).t().contiguous().unsqueeze(0)
        ctx.save_for_backward(labels)
        ctx.epsilon, ctx.emb_shape = epsilon, emb.shape
        ctx.set_materialize_grads(False)       # an unused half of the pair arrives as None, and aoc_masked_mean_pool_grad leaves its term out
        return ops.masked_mean_pool(channel_last, labels.unsqueeze(0), epsilon)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_pos, grad_neg):
        labels, = ctx.saved_tensors
        if grad_pos is None:
            if grad_neg is None:
                return None, None, None
            grad_pos = torch.zeros_like(grad_neg)
        return masked_mean_pool_backward(grad_pos, grad_neg, labels, ctx.epsilon).view(ctx.emb_shape), None, None


def _pool_frame(embedding, label, epsilon):
    """attention._pool_inputs for one frame under autograd: row 0 of the broadcast embedding stays in the graph, so the gradient goes back
    through the caller's ``expand``."""
    if embedding.dim() != 4 or label.dim() != 4:
        raise ValueError("expected [N,C,h,w] embeddings and [O,1,h,w] labels")
    if embedding.size(0) != 1 and embedding.stride(0) != 0:
        # per-object embeddings are not produced anywhere in the reference (aocnet.py:273-275 pass one map broadcast over objects); a
        # materialised copy of the broadcast has one gradient per row, which row 0 alone cannot carry
        raise NotImplementedError("aoc_amd: per-object embeddings in attention pooling (pass the [1,C,h,w] map or its expand())")
    labels = ops._f32c(label.detach().reshape(label.size(0), -1))
    return _Pool.apply(embedding[0], labels, float(epsilon))


def calculate_attention_head_p_m(ref_embedding, ref_label, prev_embedding, prev_label, epsilon=1e-5):
    """ATT:134-153 with a backward for both embeddings -> (total_head [O,4C], ref_head_pos, ref_head_neg, prev_head_pos, prev_head_neg)."""
    if not _wants_grad(ref_embedding, prev_embedding):
        return attention.calculate_attention_head_p_m(ref_embedding, ref_label, prev_embedding, prev_label, epsilon)
    ops._need_gpu(ref_embedding, ref_label, prev_embedding, prev_label)
    ref_pos, ref_neg = _pool_frame(ref_embedding, ref_label, epsilon)
    prev_pos, prev_neg = _pool_frame(prev_embedding, prev_label, epsilon)
    total_head = torch.cat([ref_pos, ref_neg, prev_pos, prev_neg], dim=1)     # ATT:152
    return total_head, ref_pos, ref_neg, prev_pos, prev_neg


def calculate_attention_head(ref_embedding, ref_label, prev_embedding, prev_label, epsilon=1e-5):
    """ATT:79-100 with a backward for both embeddings: the head only."""
    if not _wants_grad(ref_embedding, prev_embedding):
        return attention.calculate_attention_head(ref_embedding, ref_label, prev_embedding, prev_label, epsilon)
    return calculate_attention_head_p_m(ref_embedding, ref_label, prev_embedding, prev_label, epsilon)[0]


# ------------------------------------------------------------------------------------------ aggregation
class _Aggregate(torch.autograd.Function):
    """Five plane tensors [O, k_i, h, w] and the previous-frame label [O, hw] -> feat [O, n_ch, h, w]; saves feat."""

    @staticmethod
    def forward(ctx, global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg, prev_label, matching_background):
        O, _, h, w = global_fg.shape
        g, c, p, l, lp = (ops._f32c(t.detach()).view(O, t.shape[1], h * w) for t in (global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg))
        feat = proto_aggregate(g, c, p, l, lp, prev_label, matching_background)
        ctx.save_for_backward(feat)
        ctx.cfg = (c.shape[1], l.shape[1], matching_background, h, w)
        return feat.view(O, -1, h, w)

    @staticmethod
    @once_differentiable                       # the gradient kernels build no graph: a double backward (create_graph=True) raises
    def backward(ctx, grad_feat):
        feat, = ctx.saved_tensors
        n_cluster, n_local, background, h, w = ctx.cfg
        grads = proto_aggregate_backward(grad_feat.reshape(feat.shape), feat, n_cluster, n_local, background, ctx.needs_input_grad[:5])
        return tuple(g.view(g.shape[0], g.shape[1], h, w) if g is not None else None for g in grads) + (None, None)


def _planes(t, what):
    """[1, h, w, O, k] as the matchers return it -> [O, k, h, w]: a contiguous view of the planes their ``_emit`` built (aocnet.py:341-345)."""
    if t.dim() != 5 or t.size(0) != 1:
        raise ValueError(f"aggregate: {what} must be [1, h, w, O, k], got {tuple(t.shape)}")
    return t.squeeze(0).permute(2, 3, 0, 1)


def aggregate(global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg, prev_label, matching_background=True):
    """aocnet.py:341-358: the five matching outputs [1, h, w, O, k_i] and the previous-frame label ([O, 1, h, w], aocnet.py:155, or
    [h, w, O]) -> pre_to_cat [O, n_ch, h, w], with a backward for the five."""
    g, c, p, l, lp = (_planes(t, n) for t, n in ((global_fg, "global_fg"), (cluster_fg, "cluster_fg"), (proxy_fg, "proxy_fg"), (local_fg, "local_fg"),
                                                 (local_proxy_fg, "local_proxy_fg")))
    O, _, h, w = g.shape
    ops._need_gpu(g, c, p, l, lp, prev_label)
    lab = prev_label.detach()
    lab = lab.reshape(O, h * w) if lab.dim() == 4 else lab.permute(2, 0, 1).reshape(O, h * w)
    lab = ops._f32c(lab)
    if not _wants_grad(g, c, p, l, lp):
        return proto_aggregate(*(ops._f32c(t).view(O, t.shape[1], h * w) for t in (g, c, p, l, lp)), lab, matching_background).view(O, -1, h, w)
    return _Aggregate.apply(g, c, p, l, lp, lab, bool(matching_background))


# ------------------------------------------------------------------------------------------ one training sample
def proto_mask_features(ref_emb, prev_emb, cur_emb, ref_label, prev_label, gt_id, bg_bias, fg_bias, multi_local_distance=(2, 4, 6, 8, 10, 12),
                        global_chunks=1, global_atrous_rate=1, local_atrous_rate=1, local_downsample=True, local_parallel=True, use_float16=False,
                        matching_background=True, epsilon=1e-5, init_rows=None, cluster_num=DEFAULT_CLUSTER_NUM):
    """aocnet.py:141-358 for sample n in training mode.  ref_emb, prev_emb, cur_emb: [C, h, w] (``..._frame_embedding[n]``); ref_label,
    prev_label: the id maps at the embeddings' size ([h, w] or [1, h, w], ``scale_..._label[n]``); gt_id = ``gt_ids[n]``; bg_bias, fg_bias
    [1, 1, 1, 1].  The keywords are the cfg entries the lines read (MODEL_MULTI_LOCAL_DISTANCE, TRAIN_GLOBAL_CHUNKS, TRAIN_GLOBAL_ATROUS_RATE,
    TRAIN_LOCAL_ATROUS_RATE, MODEL_LOCAL_DOWNSAMPLE, TRAIN_LOCAL_PARALLEL, MODEL_FLOAT16_MATCHING, MODEL_MATCHING_BACKGROUND, MODEL_EPSILON);
    ``init_rows`` / ``cluster_num`` go to ``cluster_train.global_matching_cluster2``.  -> (pre_to_cat [O, n_ch, h, w], attention_head [O, 4C])."""
    wants = _wants_grad(ref_emb, prev_emb, cur_emb, bg_bias, fg_bias)
    if use_float16 and wants:
        raise _lib.AocHipError("aoc_amd.frontend_train.proto_mask_features: use_float16=True has no backward (the `.half()` matching mode is "
                               "inference-only); pass use_float16=False, as the model does with MODEL_FLOAT16_MATCHING = False")
    ops._need_gpu(*[t for t in (ref_emb, prev_emb, cur_emb, ref_label, prev_label, bg_bias, fg_bias) if torch.is_tensor(t)])
    gt_id = int(gt_id)
    obj_num = gt_id + 1
    C, h, w = cur_emb.shape
    dev = cur_emb.device
    ref_obj_ids = torch.arange(0, obj_num, device=dev).int().view(-1, 1, 1, 1)                       # aocnet.py:141
    dis_bias = torch.cat([bg_bias, fg_bias.expand(gt_id, -1, -1, -1)], dim=0) if gt_id > 0 else bg_bias    # aocnet.py:143-146
    cur, prev, ref = cur_emb.permute(1, 2, 0), prev_emb.permute(1, 2, 0), ref_emb.permute(1, 2, 0)  # aocnet.py:149, 153, 164
    to_cat_prev = (prev_label.reshape(1, h, w).int() == ref_obj_ids).float()                        # aocnet.py:154
    seq_prev_label = to_cat_prev.squeeze(1).permute(1, 2, 0)
    to_cat_ref = (ref_label.reshape(1, h, w).int() == ref_obj_ids).float()                          # aocnet.py:166
    seq_ref_label = to_cat_ref.squeeze(1).permute(1, 2, 0)
    radii = list(multi_local_distance)

    global_fg = matching_train.global_matching(ref, cur, seq_ref_label, global_chunks, dis_bias, None, global_atrous_rate, use_float16)
    cluster_fg = cluster_train.global_matching_cluster2(ref, cur, seq_ref_label, global_chunks, dis_bias, None, global_atrous_rate, use_float16, 0,
                                                        init_rows=init_rows, cluster_num=cluster_num)
    local_fg = local_train.local_matching(prev, cur, seq_prev_label, dis_bias, radii, None, local_atrous_rate, use_float16, local_downsample,
                                          local_parallel)
    attention_head, ref_head_pos, _, prev_head_pos, _ = calculate_attention_head_p_m(                # aocnet.py:290-295
        ref_emb.unsqueeze(0).expand(obj_num, -1, -1, -1), to_cat_ref, prev_emb.unsqueeze(0).expand(obj_num, -1, -1, -1), to_cat_prev, epsilon)
    proxy_fg = matching_train.global_matching_proxy(ref_head_pos, cur, seq_ref_label, global_chunks, dis_bias, None, global_atrous_rate, use_float16)
    prev_inst = torch.matmul(seq_prev_label, prev_head_pos)                                         # aocnet.py:325, torch's own
    local_proxy_fg = local_train.local_matching_proxy(prev_inst, cur, seq_prev_label, dis_bias, radii, None, local_atrous_rate, use_float16,
                                                      local_downsample, local_parallel)
    pre_to_cat = aggregate(global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg, to_cat_prev, matching_background)
    return pre_to_cat, attention_head
