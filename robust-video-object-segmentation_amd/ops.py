"""Tensor-level front-end of the C ABI: allocates outputs / workspaces as torch device tensors
and passes raw pointers + the current HIP stream to libaoc_hip.so.  PyTorch is plumbing here
(device memory and streams); every computation happens in the HIP library.

All functions require CUDA(HIP) tensors and raise otherwise -- there is no CPU path.

The tensor contract (the library reads bare pointers; tests/ops_contract_cases.py holds every public callable to it):
  * INPUTS are converted: a float input of another dtype or a non-contiguous view becomes a contiguous float32 copy (_f32c), an integer
    list (rows, offsets, counts, label bits, label maps) a contiguous int32 copy (_i32c; no range check, see there).  The copies are bound
    to names that live until the library call has been made.  Inputs the library addresses with the CALLER's strides (grad_out / T / arg of
    the dense and proxy backward calls, `dis` of fg2bg_min with explicit strides) cannot be converted and are checked like outputs.
  * Caller-provided OUTPUTS (out=, arg=, grad_*=, outs=, the tables of cluster_chain, the SplitRows of split_rows(out=...)) are never
    converted behind the caller's back: contiguous, the exact dtype and the exact shape (_out) -- or, for a destination addressed with
    explicit strides from its data pointer, contiguous, the exact dtype and at least the elements the strides reach (_span).  Anything else
    raises ValueError (AssertionError in the per-frame calls FrameCall / GateBatch, which assert instead of converting) BEFORE anything is
    enqueued, so the buffer is untouched.
  * Every address leaves through _p (ctypes arguments) or _addr (structure fields, pointer arrays), given a NAME, never a call expression.
  * ALIGNMENT (include/aoc_hip.h, "Pointer alignment"; tests/alignment_cases.py has the class of every pointer): a pointer the kernels reach
    through 16-byte accesses (class 16: embedding rows, proxy tables, split records) must sit on the 16-byte grid; the library refuses it
    otherwise.  A slice such as buf.view(-1)[1:1 + n * C].view(n, C) is contiguous float32 and still off that grid.  _a16 copies such an
    INPUT into a fresh tensor (bound to a name like every converted copy) and raises ValueError for such a caller-provided OUTPUT; every
    other pointer (class 4: labels, bit masks, row lists, norms, biases, the strided destinations) may sit at any float boundary.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

PAD_DISTANCE = 5e4
MAX_OBJECTS = 30


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.AocHipError("aoc_amd operators run only on an MI355X device tensor (no CPU fallback); "
                                   f"got a tensor on {t.device}")


# mirrors whose training twin has a backward (keyed by the name the guard is called with) -> module.function of the differentiable form
_TRAINABLE = {"global_matching_for_eval": "matching_train.global_matching", "global_matching_for_eval_proxy": "matching_train.global_matching_proxy",
              "local_matching": "local_train.local_matching", "local_matching_proxy": "local_train.local_matching_proxy",
              "global_matching_for_eval_cluster": "cluster_train.global_matching_cluster2",
              "foreground2background": "frontend_train.foreground2background",
              "calculate_attention_head_for_eval_p_m": "frontend_train.calculate_attention_head_p_m",
              "IA_gate": "gates_train.IA_gate", "GCT": "gates_train.GCT", "conditioning_layer": "gates_train.conditioning_layer",
              "conditioning_block": "gates_train.conditioning_block",
              "Bottleneck": "decoder_train.Bottleneck", "M1": "decoder_train.Modulator_1", "M2": "decoder_train.Modulator_2",
              "decoder_final": "tail_train.decoder_final", "predict": "tail_train.predict",
              "augment_background_logit": "tail_train.augment_background_logit",
              "ASPP": "aspp_train.ASPP", "_ASPPModule": "aspp_train._ASPPModule",
              "DynamicPreHead": "prehead_train.DynamicPreHead"}


def inference_only(what, *tensors):
    """The HIP kernels of the mirrors have no backward: every mirror returns tensors WITHOUT an autograd graph.  Dropping the reference's
    training-time names (IA_gate, conditioning_block, GCT, global_matching, ...) into a training run would therefore train
    nothing, silently.  Raise instead when autograd is recording and an input or parameter wants a gradient.  The functions that do
    have a backward live in aoc_amd.matching_train (global_matching, global_matching_proxy), aoc_amd.local_train (local_matching,
    local_matching_proxy), aoc_amd.cluster_train (global_matching_cluster2), aoc_amd.frontend_train (foreground2background, the attention
    heads, the aggregation), aoc_amd.gates_train (IA_gate, GCT, conditioning_layer, conditioning_block), aoc_amd.decoder_train (Bottleneck,
    Modulator_1, Modulator_2), aoc_amd.tail_train (decoder_final, predict, augment_background_logit), aoc_amd.aspp_train (ASPP, _ASPPModule) and aoc_amd.prehead_train (DynamicPreHead);
    the error text says so for them."""
    if torch.is_grad_enabled():
        for t in tensors:
            if torch.is_tensor(t) and t.requires_grad:
                hint = ("; aoc_amd." + _TRAINABLE[what] + " is the differentiable form") if what in _TRAINABLE else ""
                raise _lib.AocHipError(f"aoc_amd.{what} is inference-only (no autograd graph is built): call it under torch.no_grad() "
                                       "or detach its inputs; training must use the reference's PyTorch modules" + hint)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _addr(t):
    """_p's sibling for the fields of ctypes structures and for pointer arrays: the integer address (None stays None).  _p and _addr are the
    only two places where a tensor's address leaves for the library; the tensor they are given must be bound to a name that lives until
    the library call has been made (never a temporary: a copy freed right after its address is taken can be handed out again)."""
    return t.data_ptr() if t is not None else None


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    # raw hipStream_t of torch's current stream (the private getters skip ~8 us of Stream-object construction per call;
    # the public API is the fallback when a torch build does not have them)
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return ctypes.c_void_p(_RAW_STREAM(_RAW_DEVICE()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    """float32 + contiguous (the reference hands over permuted views, aocnet.py:149,153,188)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _i32c(t):
    """int32 + contiguous: the integer lists of the C ABI (rows, offsets, counts, label bits) are int32, torch's default integer is int64.
    The conversion does NOT check the range: row indices and counts are below 2^31 by construction (a pool of 2^31 rows does not fit the
    device), label bits are 32-bit patterns, and a check would need a device synchronisation."""
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    return t.contiguous()


def _out(what, t, shape, dtype=torch.float32):
    """A caller-provided output is written in place through its bare pointer and is never converted behind the caller's back: ValueError
    unless it is contiguous and has exactly this dtype and shape."""
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {tuple(shape)}, got "
                         f"{'a' if t.is_contiguous() else 'a non-contiguous'} {str(t.dtype).replace('torch.', '')} tensor of shape {tuple(t.shape)}")
    return t


def _a16(what, t, output=False):
    """A class-16 pointer of the alignment contract (include/aoc_hip.h; a kernel reaches it through float4 / uint4 or an LDS-direct load): an
    INPUT whose address is off the 16-byte grid becomes a fresh copy (the allocator's grid), a caller-provided OUTPUT raises ValueError --
    outputs are never converted.  On the grid: one integer test, the tensor itself."""
    if t is not None and (t.data_ptr() & 15) != 0:
        if output:
            raise ValueError(f"{what} does not start on the 16-byte grid: the kernels write it with 16-byte accesses "
                             "(a caller-provided output is never copied behind the caller's back)")
        t = t.clone()
    return t


def _span(what, t, need, dtype=torch.float32):
    """A buffer the library addresses with explicit strides from its data pointer (a channel slice of a larger tensor, the tail of a table):
    ValueError unless it is contiguous, has this dtype and holds at least `need` elements counted from its first."""
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < int(need):
        raise ValueError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} tensor of at least {int(need)} elements, got "
                         f"{'a' if t.is_contiguous() else 'a non-contiguous'} {str(t.dtype).replace('torch.', '')} tensor of {t.numel()}")
    return t


def _prep_lists(prep):
    """The six int32 lists of a LabelPrep, converted where a caller built them in another integer type
    -> (right_bits, wrong_bits, fg_rows, obj_rows, counts, obj_offsets); None for a list the caller left out (the exact-fp32 dense calls read
    three of the six)."""
    return tuple(_i32c(t) if t is not None else None
                 for t in (getattr(prep, f, None) for f in ("right_bits", "wrong_bits", "fg_rows", "obj_rows", "counts", "obj_offsets")))


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# The helpers of the ctypes wrappers that live in the *_train modules (their entry points are not in this module's tested table of public
# names); one copy, here, beside the contract they keep.
def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def _opt(t):
    """_f32c of an optional input (None stays None)."""
    return _f32c(t) if t is not None else None


def _vec(t):
    """An optional parameter of any shape as a flat float32 vector."""
    return _f32c(t).reshape(-1) if t is not None else None


def _det(t):
    """What an autograd Function hands to the wrappers and saves: the optional input detached, float32, contiguous."""
    return _f32c(t.detach()) if t is not None else None


def _new(like, *shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=like.device)


def _planes_hw(what, x):
    """x [N, C, ...] -> (N * C planes, elements per plane)."""
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"{what}: expected a non-empty [N, C, ...] tensor, got {tuple(x.shape)}")
    planes = x.shape[0] * x.shape[1]
    return planes, x.numel() // planes


def _wanted(what, names, shapes, want, out, like, dtypes=None):
    """The named optional outputs of a backward entry -> a tuple in the order of ``names``.  For each name, in this order: the caller's
    buffer ``out[name]`` checked by _out (a caller buffer is always written, whatever its ``want`` flag says); a fresh tensor on ``like``'s
    device if wanted and every extent is positive; else None (the library skips an output whose pointer is null).  ``out``: a dict by those
    names, None entries count as absent; a name outside ``names`` raises ValueError."""
    out = out or {}
    if set(out) - set(names):
        raise ValueError(f"{what}: unknown outputs {sorted(set(out) - set(names))}")
    bufs = []
    for k, (name, shape, w) in enumerate(zip(names, shapes, want)):
        dtype = dtypes[k] if dtypes else torch.float32
        if out.get(name) is not None:
            bufs.append(_out(f"{what}: {name}", out[name], shape, dtype))
        else:
            bufs.append(_new(like, *shape, dtype=dtype) if w and all(s > 0 for s in shape) else None)
    return tuple(bufs)


# ------------------------------------------------------------------------------------------ labels
def label_bits(labels_flat, want_wrong=True):
    """labels [n, O] float -> (right_bits, wrong_bits) uint32-as-int32 tensors [n]."""
    labels_flat = _f32c(labels_flat)
    _need_gpu(labels_flat)
    n, n_obj = labels_flat.shape
    right = torch.empty(n, dtype=torch.int32, device=labels_flat.device)
    wrong = torch.empty(n, dtype=torch.int32, device=labels_flat.device) if want_wrong else None
    _lib.check(_lib.lib().aoc_label_bits(_p(labels_flat), n, n_obj, _p(right), _p(wrong), _stream()), "aoc_label_bits")
    return right, wrong


class LabelPrep:
    """Result of aoc_label_prep (all device tensors)."""
    __slots__ = ("n", "n_obj", "right_bits", "wrong_bits", "fg_rows", "obj_rows", "counts", "obj_offsets")

    def tensors(self):
        """The six lists, in the order of _prep_lists."""
        return self.right_bits, self.wrong_bits, self.fg_rows, self.obj_rows, self.counts, self.obj_offsets


def label_prep(labels_flat):
    labels_flat = _f32c(labels_flat)
    _need_gpu(labels_flat)
    n, n_obj = labels_flat.shape
    dev = labels_flat.device
    L = _lib.lib()
    r = LabelPrep()
    r.n, r.n_obj = n, n_obj
    r.right_bits = torch.empty(n, dtype=torch.int32, device=dev)
    r.wrong_bits = torch.empty(n, dtype=torch.int32, device=dev)
    r.fg_rows = torch.empty(n, dtype=torch.int32, device=dev)
    r.obj_rows = torch.empty(n * n_obj, dtype=torch.int32, device=dev)
    r.counts = torch.empty(n_obj + 1, dtype=torch.int32, device=dev)
    r.obj_offsets = torch.empty(n_obj + 1, dtype=torch.int32, device=dev)
    ws = _ws(L.aoc_label_prep_workspace_bytes(n, n_obj), dev)
    _lib.check(L.aoc_label_prep(_p(labels_flat), n, n_obj, _p(r.right_bits), _p(r.wrong_bits), _p(r.fg_rows), _p(r.obj_rows),
                                _p(r.counts), _p(r.obj_offsets), _p(ws), ws.numel(), _stream()), "aoc_label_prep")
    return r


def kmeans_plan(counts, n_seg, cluster_num):
    _need_gpu(counts)
    counts = _i32c(counts)
    seg_k = torch.empty(n_seg, dtype=torch.int32, device=counts.device)
    _lib.check(_lib.lib().aoc_kmeans_plan(_p(counts), n_seg, int(cluster_num), _p(seg_k), _stream()), "aoc_kmeans_plan")
    return seg_k


# ------------------------------------------------------------------------------------------ k-means
def kmeans_init_rows_draw(rng, counts, levels, n_frames, kmax=None):
    """Initial rows of the k-means calls of `n_frames` frames that see one pool state, drawn from `rng` (a numpy.random.RandomState, advanced
    in place) exactly as the reference's per-frame kmeans2(minit='points') calls would draw them (aoc_kmeans_init_rows_draw; HOST function).
    counts: rows per object.  Returns (rows int32 [n_frames, len(levels) * n_obj, kmax], states): states[f] = the generator state in front of
    frame f's draws (for rng.set_state when the frames from f on are not used after all)."""
    import numpy as np
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.int32).reshape(-1))
    lv = np.ascontiguousarray(np.asarray(list(levels), dtype=np.int32))
    kmax = int(max(levels) if kmax is None else kmax)
    st = rng.get_state()
    assert st[0] == "MT19937"
    key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
    pos = ctypes.c_int32(int(st[2]))
    rows = np.empty((int(n_frames), len(lv) * len(counts), kmax), dtype=np.int32)
    snaps = np.empty((int(n_frames), 625), dtype=np.uint32)
    _lib.check(_lib.lib().aoc_kmeans_init_rows_draw(key.ctypes.data, ctypes.byref(pos), counts.ctypes.data, len(counts), lv.ctypes.data, len(lv),
                                                    int(n_frames), kmax, rows.ctypes.data, snaps.ctypes.data), "aoc_kmeans_init_rows_draw")
    rng.set_state((st[0], key, int(pos.value), st[3], st[4]))
    states = [(st[0], snaps[f, :624].copy(), int(snaps[f, 624]), st[3], st[4]) for f in range(int(n_frames))]
    return rows, states


def kmeans_segmented(pool, rows, seg_offsets, seg_k, init_rows, kmax, iters=20, rows_capacity=None, n_rep=1):
    """Segmented k-means, bit-identical to scipy kmeans2 (see include/aoc_hip.h).
    n_rep > 1: the segment lists are n_rep replicas of n_seg / n_rep base segments (kmeans_replicate[_levels]).
    Returns (centroids [S,kmax,C], labels [rows_capacity], cluster_counts [S,kmax])."""
    pool = _a16("kmeans_segmented: pool", _f32c(pool))
    _need_gpu(pool, rows, seg_offsets, seg_k, init_rows)
    n_seg = seg_k.numel()
    C = pool.shape[1]
    cap = int(rows.numel() if rows_capacity is None else rows_capacity)
    dev = pool.device
    L = _lib.lib()
    centroids = torch.empty(n_seg, kmax, C, dtype=torch.float32, device=dev)
    labels = torch.empty(cap, dtype=torch.int32, device=dev)
    ccounts = torch.empty(n_seg, kmax, dtype=torch.int32, device=dev)
    ws = _ws(L.aoc_kmeans_workspace_bytes(cap, n_seg, kmax, C), dev)
    rows, seg_offsets, seg_k, init_rows = _i32c(rows), _i32c(seg_offsets), _i32c(seg_k), _i32c(init_rows)
    _lib.check(L.aoc_kmeans_segmented_rep(_p(pool), pool.shape[0], C, _p(rows), _p(seg_offsets), _p(seg_k), _p(init_rows), n_seg, int(n_rep), kmax,
                                          int(iters), cap, _p(centroids), _p(labels), _p(ccounts), _p(ws), ws.numel(), _stream()),
               "aoc_kmeans_segmented_rep")
    return centroids, labels, ccounts


def kmeans_replicate(rows, seg_offsets, seg_k, n_rep, rows_capacity=None):
    """Segment lists replicated n_rep times (aoc_kmeans_replicate) -> (rows [n_rep*cap], seg_offsets [n_rep*S+1], seg_k [n_rep*S])."""
    _need_gpu(rows, seg_offsets, seg_k)
    rows, seg_offsets, seg_k = _i32c(rows), _i32c(seg_offsets), _i32c(seg_k)
    n_seg = seg_k.numel()
    cap = int(rows.numel() if rows_capacity is None else rows_capacity)
    dev = rows.device
    rows_out = torch.empty(n_rep * cap, dtype=torch.int32, device=dev)
    off_out = torch.empty(n_rep * n_seg + 1, dtype=torch.int32, device=dev)
    k_out = torch.empty(n_rep * n_seg, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().aoc_kmeans_replicate(_p(rows), _p(seg_offsets), _p(seg_k), n_seg, int(n_rep), cap, _p(rows_out), _p(off_out), _p(k_out),
                                               _stream()), "aoc_kmeans_replicate")
    return rows_out, off_out, k_out


def kmeans_replicate_levels(rows, seg_offsets, n_seg, n_rep, levels, rows_capacity=None):
    """aoc_kmeans_replicate_levels: n_rep replicas of the segment lists, replica f clustering at K = levels[f % len(levels)] with the
    sticky rule of AEM:268 applied on the device -> (rows [n_rep*cap], seg_offsets [n_rep*S+1], seg_k [n_rep*S])."""
    _need_gpu(rows, seg_offsets)
    rows, seg_offsets = _i32c(rows), _i32c(seg_offsets)
    cap = int(rows.numel() if rows_capacity is None else rows_capacity)
    dev = rows.device
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.int32))
    rows_out = rows if n_rep == 1 else torch.empty(n_rep * cap, dtype=torch.int32, device=dev)
    off_out = torch.empty(n_rep * n_seg + 1, dtype=torch.int32, device=dev)
    k_out = torch.empty(n_rep * n_seg, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().aoc_kmeans_replicate_levels(_p(rows), _p(seg_offsets), int(n_seg), int(n_rep), lv.ctypes.data_as(ctypes.c_void_p), int(lv.size),
                                                      cap, _p(rows_out), _p(off_out), _p(k_out), _stream()), "aoc_kmeans_replicate_levels")
    return rows_out, off_out, k_out


def build_proxies(pool, fg_rows, seg_offsets, seg_k, labels, centroids):
    """AEM:280-282 -> (proxies [S,2,kmax,C], proxy_sqnorm [S,2,kmax]); +inf norm = absent proxy."""
    pool = _a16("build_proxies: pool", _f32c(pool))
    _need_gpu(pool, fg_rows, seg_offsets, seg_k, labels, centroids)
    fg_rows, seg_offsets, seg_k, labels, centroids = _i32c(fg_rows), _i32c(seg_offsets), _i32c(seg_k), _i32c(labels), _f32c(centroids)
    n_seg, kmax, C = centroids.shape
    L = _lib.lib()
    proxies = torch.empty(n_seg, 2, kmax, C, dtype=torch.float32, device=pool.device)
    sqnorm = torch.empty(n_seg, 2, kmax, dtype=torch.float32, device=pool.device)
    cap = int(labels.numel())
    ws = _ws(L.aoc_build_proxies_workspace_bytes(cap, n_seg, kmax), pool.device)
    _lib.check(L.aoc_build_proxies(_p(pool), pool.shape[0], C, _p(fg_rows), _p(seg_offsets), _p(seg_k), _p(labels), _p(centroids), n_seg, kmax,
                                   cap, _p(proxies), _p(sqnorm), _p(ws), ws.numel(), _stream()), "aoc_build_proxies")
    return proxies, sqnorm


# ------------------------------------------------------------------------------------------ correlation
def proxy_corr_min(query_flat, proxies, proxy_sqnorm, set_begin, set_size, set_out_offset, set_bias, out, out_pixel_stride,
                   transform=True, float16=False):
    """For every pixel i and set s writes f(min over proxies[set_begin[s] : +set_size[s]] of d(q_i, p)) at
    out.data_ptr()[i*out_pixel_stride + set_out_offset[s]]  (see include/aoc_hip.h).  float16: the reference's `.half()` mode
    (aoc_proxy_corr_min_f16)."""
    query_flat = _f32c(query_flat)
    proxies = _a16("proxy_corr_min: proxies", _f32c(proxies))
    proxy_sqnorm = _opt(proxy_sqnorm)
    _need_gpu(query_flat, proxies, proxy_sqnorm, out, set_bias)
    m, C = query_flat.shape
    sb = np.ascontiguousarray(np.asarray(set_begin, dtype=np.int32))
    ss = np.ascontiguousarray(np.asarray(set_size, dtype=np.int32))
    so = np.ascontiguousarray(np.asarray(set_out_offset, dtype=np.int64))
    n_set = sb.size
    assert ss.size == n_set and so.size == n_set
    if set_bias is not None:
        set_bias = _f32c(set_bias)
        assert set_bias.numel() == n_set
    _span("proxy_corr_min: out", out, (m - 1) * int(out_pixel_stride) + int(so.max()) + 1 if n_set and m else 0)
    vp = ctypes.c_void_p
    fn = _lib.lib().aoc_proxy_corr_min_f16 if float16 else _lib.lib().aoc_proxy_corr_min
    _lib.check(fn(_p(query_flat), m, C, _p(proxies), _p(proxy_sqnorm), proxies.shape[0], n_set,
                  sb.ctypes.data_as(vp), ss.ctypes.data_as(vp), so.ctypes.data_as(vp), _p(set_bias), _p(out),
                  int(out_pixel_stride), int(bool(transform)), _stream()), "aoc_proxy_corr_min_f16" if float16 else "aoc_proxy_corr_min")
    return out


class _CorrFrame(ctypes.Structure):
    """aoc_corr_frame of include/aoc_hip.h."""
    _fields_ = [("query", ctypes.c_void_p), ("proxies", ctypes.c_void_p), ("proxy_sqnorm", ctypes.c_void_p), ("set_bias", ctypes.c_void_p),
                ("out", ctypes.c_void_p)]


class _CorrFrameRec(ctypes.Structure):
    """aoc_corr_frame_rec of include/aoc_hip.h."""
    _fields_ = [("query", ctypes.c_void_p), ("query_rec", ctypes.c_void_p), ("query_sqnorm", ctypes.c_void_p), ("proxies", ctypes.c_void_p),
                ("proxy_sqnorm", ctypes.c_void_p), ("set_bias", ctypes.c_void_p), ("out", ctypes.c_void_p)]


CORR_PRECISION = {"split": 0, "fp32": 1}
_corr_ws = {}


def _corr_workspace(dev):
    # the 256-byte flag workspace is only touched by kernels of one call, which are ordered on the call's stream: one per (device, stream)
    key = (dev.index, _stream().value)
    ws = _corr_ws.get(key)
    if ws is None:
        ws = _corr_ws[key] = torch.zeros(int(_lib.lib().aoc_proxy_corr_min_batched_workspace_bytes()), dtype=torch.uint8, device=dev)
    return ws


def proxy_corr_min_batched(frames, set_begin, set_size, set_out_offset, transform=True, precision="split"):
    """aoc_proxy_corr_min_batched: the correlation of several frames (of one or of several sequences) in ONE launch.
    frames: sequence of (query_flat [m, C], proxies [n_proxy, C], proxy_sqnorm [n_proxy] or None, set_bias [n_set] or None, out) with the same m, C,
    n_proxy; element (pixel i, set s) of a frame is written at out.data_ptr()[set_out_offset[s] + i] (pixel-contiguous planes)."""
    q0, p0 = frames[0][0], frames[0][1]
    m, C = q0.shape
    n_proxy = p0.shape[0]
    sb = np.ascontiguousarray(np.asarray(set_begin, dtype=np.int32))
    ss = np.ascontiguousarray(np.asarray(set_size, dtype=np.int32))
    so = np.ascontiguousarray(np.asarray(set_out_offset, dtype=np.int64))
    n_set = sb.size
    assert ss.size == n_set and so.size == n_set
    arr = (_CorrFrame * len(frames))()
    keep = []
    for i, (q, p, sq, b, out) in enumerate(frames):
        q, p = _a16("proxy_corr_min_batched: query", _f32c(q)), _a16("proxy_corr_min_batched: proxies", _f32c(p))
        sq = _opt(sq)
        b = _opt(b)
        _need_gpu(q, p, sq, b, out)
        assert q.shape == (m, C) and p.shape == (n_proxy, C) and (b is None or b.numel() == n_set)
        _span("proxy_corr_min_batched: out", out, int(so.max()) + m if n_set else 0)
        keep.append((q, p, sq, b, out))
        arr[i] = _CorrFrame(_addr(q), _addr(p), _addr(sq), _addr(b), _addr(out))
    L = _lib.lib()
    ws = _corr_workspace(q0.device)
    vp = ctypes.c_void_p
    _lib.check(L.aoc_proxy_corr_min_batched(ctypes.cast(arr, vp), len(frames), m, C, n_proxy, n_set, sb.ctypes.data_as(vp), ss.ctypes.data_as(vp),
                                            so.ctypes.data_as(vp), int(bool(transform)), CORR_PRECISION[precision], _p(ws), ws.numel(), _stream()),
               "aoc_proxy_corr_min_batched")
    return [f[4] for f in frames]


class CorrTableCache:
    """Workspace + host key of aoc_proxy_corr_min_records_cached: the tile tables of a frame's correlation passes stay in the workspace, so
    every call is ONE launch whatever the number of proxy tiles.  One per stream / sequence (the calls that share it are stream-ordered)."""

    def __init__(self, device):
        self.ws = torch.zeros(int(_lib.lib().aoc_proxy_corr_min_records_cached_workspace_bytes()), dtype=torch.uint8, device=device)
        self.key = ctypes.c_int64(0)


def proxy_corr_min_records(frames, set_begin, set_size, set_out_offset, transform=True, prepare_only=False, cache=None):
    """aoc_proxy_corr_min_records: proxy_corr_min_batched with every frame's query handed over as the tile-major split records the dense
    kernel consumes for the same frame.  frames: sequence of (query_flat [m, C], query_split (SplitRows, tiled), proxies, proxy_sqnorm or
    None, set_bias or None, out).  cache: a CorrTableCache -> aoc_proxy_corr_min_records_cached (all passes in one launch; same results)."""
    q0, p0 = frames[0][0], frames[0][2]
    m, C = q0.shape
    n_proxy = p0.shape[0]
    sb = np.ascontiguousarray(np.asarray(set_begin, dtype=np.int32))
    ss = np.ascontiguousarray(np.asarray(set_size, dtype=np.int32))
    so = np.ascontiguousarray(np.asarray(set_out_offset, dtype=np.int64))
    n_set = sb.size
    assert ss.size == n_set and so.size == n_set
    arr = (_CorrFrameRec * len(frames))()
    keep = []
    for i, (q, qs, p, sq, b, out) in enumerate(frames):
        q, p = _f32c(q), _a16("proxy_corr_min_records: proxies", _f32c(p))
        sq = _opt(sq)
        b = _opt(b)
        _need_gpu(q, p, sq, b, out, qs.records, qs.sqnorm)
        assert qs.tiled and qs.n == m, "the records kernel reads aoc_split_rows_tiled records of the whole query"
        assert q.shape == (m, C) and p.shape == (n_proxy, C) and (b is None or b.numel() == n_set)
        _span("proxy_corr_min_records: out", out, int(so.max()) + m if n_set else 0)
        rec, rsq = _a16("proxy_corr_min_records: query records", qs.records), qs.sqnorm
        keep.append((q, p, sq, b, out, rec, rsq))
        arr[i] = _CorrFrameRec(_addr(q), _addr(rec), _addr(rsq), _addr(p), _addr(sq), _addr(b), _addr(out))
    vp = ctypes.c_void_p
    fn = _lib.lib().aoc_proxy_corr_min_records
    dev = q0.device
    n_frames = len(frames)
    outs = [f[5] for f in frames]

    def launch():
        if cache is not None:
            _lib.check(_lib.lib().aoc_proxy_corr_min_records_cached(ctypes.cast(arr, vp), n_frames, m, C, n_proxy, n_set, sb.ctypes.data_as(vp),
                                                                    ss.ctypes.data_as(vp), so.ctypes.data_as(vp), int(bool(transform)), _p(cache.ws),
                                                                    cache.ws.numel(), ctypes.byref(cache.key), _stream()), "aoc_proxy_corr_min_records_cached")
            return outs
        ws = _corr_workspace(dev)
        _lib.check(fn(ctypes.cast(arr, vp), n_frames, m, C, n_proxy, n_set, sb.ctypes.data_as(vp), ss.ctypes.data_as(vp), so.ctypes.data_as(vp),
                      int(bool(transform)), _p(ws), ws.numel(), _stream()), "aoc_proxy_corr_min_records")
        return outs

    launch.keep = (keep, frames)          # the tensors behind the raw pointers
    if prepare_only:
        return launch                     # bench.py: the argument marshalling stays outside the timed bracket
    return launch()


def _dense_span(m, n_obj, pixel_stride, obj_stride):
    """Elements from the data pointer that [i * pixel_stride + o * obj_stride], i < m, o < n_obj, reaches."""
    return (m - 1) * int(pixel_stride) + (n_obj - 1) * int(obj_stride) + 1 if m > 0 and n_obj > 0 else 0


def dense_match_min(query_flat, pool, prep, obj_bias, out, out_pixel_stride, out_obj_stride, transform=True, float16=False):
    query_flat = _f32c(query_flat)
    pool = _a16("dense_match_min: pool", _f32c(pool))
    _need_gpu(query_flat, pool, out)
    m, C = query_flat.shape
    n_obj = prep.n_obj
    L = _lib.lib()
    ws = _ws(L.aoc_dense_match_workspace_bytes(m, prep.n, n_obj), pool.device)
    if obj_bias is not None:
        obj_bias = _f32c(obj_bias)
    _span("dense_match_min: out", out, _dense_span(m, n_obj, out_pixel_stride, out_obj_stride))
    _, wrong_bits, fg_rows, _, counts, _ = _prep_lists(prep)
    n_fg = counts[n_obj:n_obj + 1]
    fn = L.aoc_dense_match_min_f16 if float16 else L.aoc_dense_match_min
    _lib.check(fn(_p(query_flat), m, C, _p(pool), _p(fg_rows), _p(n_fg), prep.n, _p(wrong_bits),
                  _p(obj_bias), n_obj, _p(out), int(out_pixel_stride), int(out_obj_stride), int(bool(transform)),
                  _p(ws), ws.numel(), _stream()), "aoc_dense_match_min_f16" if float16 else "aoc_dense_match_min")
    return out


def dense_match_argmin(query_flat, pool, prep, obj_bias, out, arg, out_pixel_stride, out_obj_stride, transform=True):
    """aoc_dense_match_argmin: dense_match_min's values (bit for bit) and, in ``arg`` (int32, addressed like ``out``), the pool row of every
    minimum; -1 where the winner is a padded distance or nothing is labelled."""
    query_flat = _f32c(query_flat)
    pool = _a16("dense_match_argmin: pool", _f32c(pool))
    _need_gpu(query_flat, pool, out, arg)
    assert arg.dtype == torch.int32
    m, C = query_flat.shape
    n_obj = prep.n_obj
    L = _lib.lib()
    ws = _ws(L.aoc_dense_match_argmin_workspace_bytes(m, prep.n, n_obj), pool.device)
    if obj_bias is not None:
        obj_bias = _f32c(obj_bias)
    _span("dense_match_argmin: out", out, _dense_span(m, n_obj, out_pixel_stride, out_obj_stride))
    _span("dense_match_argmin: arg", arg, _dense_span(m, n_obj, out_pixel_stride, out_obj_stride), torch.int32)
    _, wrong_bits, fg_rows, _, counts, _ = _prep_lists(prep)
    n_fg = counts[n_obj:n_obj + 1]
    _lib.check(L.aoc_dense_match_argmin(_p(query_flat), m, C, _p(pool), _p(fg_rows), _p(n_fg), prep.n, _p(wrong_bits),
                                        _p(obj_bias), n_obj, _p(out), _p(arg), int(out_pixel_stride), int(out_obj_stride), int(bool(transform)),
                                        _p(ws), ws.numel(), _stream()), "aoc_dense_match_argmin")
    return out, arg


def dense_match_backward(grad_out, T, arg, pixel_stride, obj_stride, query_flat, pool, n_obj, want_query=True, want_pool=True, want_bias=True,
                         grad_query=None, grad_pool=None, grad_bias=None):
    """aoc_dense_match_grad.  grad_out, T and arg are addressed as [i * pixel_stride + o * obj_stride] from their data pointers.
    -> (grad_query [m, C], grad_pool [n, C], grad_bias [n_obj]); None for an output that is not wanted (nothing is written for it).  The
    keyword buffers, when given, are written in place."""
    query_flat = _f32c(query_flat)
    pool = _f32c(pool)
    _need_gpu(grad_out, T, arg, query_flat, pool, grad_query, grad_pool, grad_bias)
    m, C = query_flat.shape
    n = pool.shape[0]
    dev = pool.device
    # grad_out, T and arg are addressed with the caller's strides from their data pointers: they cannot be converted, only checked
    need = _dense_span(m, n_obj, pixel_stride, obj_stride)
    _span("dense_match_backward: grad_out", grad_out, need)
    _span("dense_match_backward: T", T, need)
    _span("dense_match_backward: arg", arg, need, torch.int32)
    if want_query and grad_query is None:
        grad_query = torch.empty(m, C, dtype=torch.float32, device=dev)
    if want_pool and grad_pool is None:
        grad_pool = torch.empty(n, C, dtype=torch.float32, device=dev)
    if want_bias and grad_bias is None:
        grad_bias = torch.empty(n_obj, dtype=torch.float32, device=dev)
    gq, gp, gb = (grad_query if want_query else None), (grad_pool if want_pool else None), (grad_bias if want_bias else None)
    for what, t, shape in (("grad_query", gq, (m, C)), ("grad_pool", gp, (n, C)), ("grad_bias", gb, (n_obj,))):
        if t is not None:
            _out("dense_match_backward: " + what, t, shape)
    L = _lib.lib()
    ws = _ws(L.aoc_dense_match_grad_workspace_bytes(m, n, C, n_obj), dev)
    _lib.check(L.aoc_dense_match_grad(_p(grad_out), _p(T), _p(arg), int(pixel_stride), int(obj_stride), _p(query_flat), m, C, _p(pool), n, n_obj,
                                      _p(gq), _p(gp), _p(gb), _p(ws), ws.numel(), _stream()), "aoc_dense_match_grad")
    return gq, gp, gb


def proxy_match_backward(grad_out, T, pixel_stride, obj_stride, query_flat, proxies, want_query=True, want_proxies=True, want_bias=True,
                         grad_query=None, grad_proxies=None, grad_bias=None):
    """aoc_proxy_match_grad (k = 1 proxies [n_obj, C]).  -> (grad_query, grad_proxies, grad_bias), None where not wanted."""
    query_flat = _f32c(query_flat)
    proxies = _f32c(proxies)
    _need_gpu(grad_out, T, query_flat, proxies, grad_query, grad_proxies, grad_bias)
    m, C = query_flat.shape
    n_obj = proxies.shape[0]
    dev = query_flat.device
    need = _dense_span(m, n_obj, pixel_stride, obj_stride)
    _span("proxy_match_backward: grad_out", grad_out, need)
    _span("proxy_match_backward: T", T, need)
    if want_query and grad_query is None:
        grad_query = torch.empty(m, C, dtype=torch.float32, device=dev)
    if want_proxies and grad_proxies is None:
        grad_proxies = torch.empty(n_obj, C, dtype=torch.float32, device=dev)
    if want_bias and grad_bias is None:
        grad_bias = torch.empty(n_obj, dtype=torch.float32, device=dev)
    gq, gp, gb = (grad_query if want_query else None), (grad_proxies if want_proxies else None), (grad_bias if want_bias else None)
    for what, t, shape in (("grad_query", gq, (m, C)), ("grad_proxies", gp, (n_obj, C)), ("grad_bias", gb, (n_obj,))):
        if t is not None:
            _out("proxy_match_backward: " + what, t, shape)
    L = _lib.lib()
    ws = _ws(L.aoc_proxy_match_grad_workspace_bytes(m, C, n_obj), dev)
    _lib.check(L.aoc_proxy_match_grad(_p(grad_out), _p(T), int(pixel_stride), int(obj_stride), _p(query_flat), m, C, _p(proxies), n_obj,
                                      _p(gq), _p(gp), _p(gb), _p(ws), ws.numel(), _stream()), "aoc_proxy_match_grad")
    return gq, gp, gb


def _set_arrays(set_begin, set_size, set_out_offset):
    sb = np.ascontiguousarray(np.asarray(set_begin, dtype=np.int32))
    ss = np.ascontiguousarray(np.asarray(set_size, dtype=np.int32))
    so = np.ascontiguousarray(np.asarray(set_out_offset, dtype=np.int64))
    assert ss.size == sb.size and so.size == sb.size
    return sb, ss, so


def proxy_set_match_argmin(query_flat, proxies, proxy_sqnorm, set_begin, set_size, set_out_offset, set_bias, out, arg, out_pixel_stride,
                           transform=True):
    """aoc_proxy_set_match_argmin: proxy_corr_min's values (bit for bit) and, in ``arg`` (int32, addressed like ``out``), the slot within the
    set of every minimum (ties: the lowest); -1 where the set is empty or all-ignored."""
    query_flat = _f32c(query_flat)
    proxies = _f32c(proxies)
    proxy_sqnorm = _opt(proxy_sqnorm)
    _need_gpu(query_flat, proxies, proxy_sqnorm, out, arg, set_bias)
    m, C = query_flat.shape
    sb, ss, so = _set_arrays(set_begin, set_size, set_out_offset)
    if set_bias is not None:
        set_bias = _f32c(set_bias)
        assert set_bias.numel() == sb.size
    need = (m - 1) * int(out_pixel_stride) + int(so.max()) + 1 if sb.size and m else 0
    _span("proxy_set_match_argmin: out", out, need)
    _span("proxy_set_match_argmin: arg", arg, need, torch.int32)
    vp = ctypes.c_void_p
    _lib.check(_lib.lib().aoc_proxy_set_match_argmin(_p(query_flat), m, C, _p(proxies), _p(proxy_sqnorm), proxies.shape[0], sb.size,
                                                     sb.ctypes.data_as(vp), ss.ctypes.data_as(vp), so.ctypes.data_as(vp), _p(set_bias), _p(out), _p(arg),
                                                     int(out_pixel_stride), int(bool(transform)), _stream()), "aoc_proxy_set_match_argmin")
    return out, arg


def proxy_set_match_backward(grad_out, T, arg, pixel_stride, query_flat, proxies, set_begin, set_size, set_out_offset, set_bias_index, n_bias,
                             want_query=True, want_proxies=True, want_bias=True, grad_query=None, grad_proxies=None, grad_bias=None):
    """aoc_proxy_set_match_grad.  grad_out, T and arg are addressed as [i * pixel_stride + set_out_offset[s]] from their data pointers;
    set_bias_index[s] = the element of grad_bias set s belongs to.  -> (grad_query [m, C], grad_proxies [n_proxy, C], grad_bias [n_bias]);
    None for an output that is not wanted.  The keyword buffers, when given, are written in place."""
    query_flat = _f32c(query_flat)
    proxies = _f32c(proxies)
    _need_gpu(grad_out, T, arg, query_flat, proxies, grad_query, grad_proxies, grad_bias)
    m, C = query_flat.shape
    dev = query_flat.device
    sb, ss, so = _set_arrays(set_begin, set_size, set_out_offset)
    si = np.ascontiguousarray(np.asarray(set_bias_index, dtype=np.int32))
    assert si.size == sb.size
    need = (m - 1) * int(pixel_stride) + int(so.max()) + 1 if sb.size and m else 0
    _span("proxy_set_match_backward: grad_out", grad_out, need)
    _span("proxy_set_match_backward: T", T, need)
    _span("proxy_set_match_backward: arg", arg, need, torch.int32)
    if want_query and grad_query is None:
        grad_query = torch.empty(m, C, dtype=torch.float32, device=dev)
    if want_proxies and grad_proxies is None:
        grad_proxies = torch.empty(proxies.shape[0], C, dtype=torch.float32, device=dev)
    if want_bias and grad_bias is None:
        grad_bias = torch.empty(int(n_bias), dtype=torch.float32, device=dev)
    gq, gp, gb = (grad_query if want_query else None), (grad_proxies if want_proxies else None), (grad_bias if want_bias else None)
    for what, t, shape in (("grad_query", gq, (m, C)), ("grad_proxies", gp, (proxies.shape[0], C)), ("grad_bias", gb, (int(n_bias),))):
        if t is not None:
            _out("proxy_set_match_backward: " + what, t, shape)
    L = _lib.lib()
    ws = _ws(L.aoc_proxy_set_match_grad_workspace_bytes(m, C, int(ss.sum())) if (want_proxies or want_bias) else 0, dev)
    vp = ctypes.c_void_p
    _lib.check(L.aoc_proxy_set_match_grad(_p(grad_out), _p(T), _p(arg), int(pixel_stride), _p(query_flat), m, C, _p(proxies), proxies.shape[0], sb.size,
                                          sb.ctypes.data_as(vp), ss.ctypes.data_as(vp), so.ctypes.data_as(vp), si.ctypes.data_as(vp), int(n_bias),
                                          _p(gq), _p(gp), _p(gb), _p(ws), ws.numel(), _stream()), "aoc_proxy_set_match_grad")
    return gq, gp, gb


def centroid_avg_backward(grad_proxies, fg_rows, n_fg, seg_offsets, seg_k, labels, pool_rows, grad_pool=None):
    """aoc_centroid_avg_grad: grad_proxies [n_seg, 2, kmax, C] (only [:, 1] is read) pulled back through build_proxies' means
    -> grad_pool [pool_rows, C]; n_fg is the device element that holds the number of kept rows (LabelPrep.counts[n_obj:])."""
    grad_proxies = _f32c(grad_proxies)
    _need_gpu(grad_proxies, fg_rows, n_fg, seg_offsets, seg_k, labels, grad_pool)
    fg_rows, n_fg, seg_offsets, seg_k, labels = _i32c(fg_rows), _i32c(n_fg), _i32c(seg_offsets), _i32c(seg_k), _i32c(labels)
    n_seg, two, kmax, C = grad_proxies.shape
    assert two == 2 and seg_k.numel() == n_seg and seg_offsets.numel() == n_seg + 1
    if grad_pool is None:
        grad_pool = torch.empty(int(pool_rows), C, dtype=torch.float32, device=grad_proxies.device)
    _out("centroid_avg_backward: grad_pool", grad_pool, (int(pool_rows), C))
    L = _lib.lib()
    ws = _ws(L.aoc_centroid_avg_grad_workspace_bytes(n_seg, kmax), grad_proxies.device)
    _lib.check(L.aoc_centroid_avg_grad(_p(grad_proxies), C, _p(fg_rows), _p(n_fg), _p(seg_offsets), _p(seg_k), _p(labels), n_seg, kmax,
                                       int(labels.numel()), _p(grad_pool), int(pool_rows), _p(ws), ws.numel(), _stream()), "aoc_centroid_avg_grad")
    return grad_pool


class SplitRows:
    """fp16 split records of embedding rows (aoc_split_rows): records [n, 448] uint8, sqnorm [n], overflow flag [1].  tiled: the records
    in tile-major order (aoc_split_rows_tiled; [ceil(n / 32) * 32, 448] uint8) -- the query side of the dense and correlation kernels."""
    __slots__ = ("records", "sqnorm", "overflow", "n", "tiled")

    def __init__(self):
        self.tiled = False


def split_record_bytes(C):
    return int(_lib.lib().aoc_split_record_bytes(int(C)))


def split_rows(x_flat, out=None, row0=0, overflow=None, tiled=False):
    """x [n, C] fp32 -> SplitRows.  With `out` (a SplitRows with capacity) the records are written at row `row0` of it
    (the reference pool grows in place: only the appended frame is converted).  tiled: tile-major records of the whole x (a query)."""
    x_flat = _a16("split_rows: x", _f32c(x_flat))
    _need_gpu(x_flat)
    n, C = x_flat.shape
    rb = split_record_bytes(C)
    if rb == 0:
        raise _lib.AocHipError(f"split records need C % 4 == 0 and C <= 100 (got {C})")
    dev = x_flat.device
    if overflow is not None:
        _span("split_rows: overflow", overflow, 1, torch.int32)
    if tiled:
        assert out is None and row0 == 0
        out = SplitRows()
        out.tiled = True
        out.records = torch.empty((n + 31) // 32 * 32, rb, dtype=torch.uint8, device=dev)
        out.sqnorm = torch.empty(n, dtype=torch.float32, device=dev)
        out.overflow = overflow if overflow is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        out.n = n
        rec, sq, flag = out.records, out.sqnorm, out.overflow
        _lib.check(_lib.lib().aoc_split_rows_tiled(_p(x_flat), n, C, _p(rec), _p(sq), _p(flag), _stream()), "aoc_split_rows_tiled")
        return out
    if out is None:
        out = SplitRows()
        out.records = torch.empty(n, rb, dtype=torch.uint8, device=dev)
        out.sqnorm = torch.empty(n, dtype=torch.float32, device=dev)
        out.overflow = overflow if overflow is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        out.n = n
        row0 = 0
    rec = out.records[row0:row0 + n]
    sq = out.sqnorm[row0:row0 + n]
    flag = out.overflow
    _out("split_rows: out.records[row0 : row0 + n]", rec, (n, rb), torch.uint8)
    _a16("split_rows: out.records[row0 : row0 + n]", rec, output=True)
    _out("split_rows: out.sqnorm[row0 : row0 + n]", sq, (n,))
    _span("split_rows: out.overflow", flag, 1, torch.int32)
    _lib.check(_lib.lib().aoc_split_rows(_p(x_flat), n, C, _p(rec), _p(sq), _p(flag), _stream()), "aoc_split_rows")
    return out


def dense_prune_stats(reset=True):
    """Developer counters of the coarse-then-rescore dense kernel (aoc_dense_prune_stats_ex): dict(tested, rescored, tiles_rescored, tiles).
    The keys `stopped` and `dev_cycles` are kept so that no caller breaks; they belonged to the removed checkpoint and core-clock stamps and are
    always zero (out8[4..7] are reserved)."""
    import ctypes
    v = (ctypes.c_uint64 * 8)()
    _lib.check(_lib.lib().aoc_dense_prune_stats_ex(v, 1 if reset else 0), "aoc_dense_prune_stats_ex")
    return dict(tested=int(v[0]), rescored=int(v[1]), tiles_rescored=int(v[2]), tiles=int(v[3]), stopped=int(v[4]),
                dev_cycles=[int(v[5]), int(v[6]), int(v[7])])


def dense_match_min_split(query_flat, query_split, pool, pool_split, prep, obj_bias, out, out_pixel_stride, out_obj_stride, transform=True):
    """aoc_dense_match_min_split: fp16-split matrix pipe with the exact-fp32 kernels as device-side take-over."""
    query_flat = _a16("dense_match_min_split: query", _f32c(query_flat))
    pool = _a16("dense_match_min_split: pool", _f32c(pool))
    _need_gpu(query_flat, pool, out, query_split.records, pool_split.records)
    m, C = query_flat.shape
    n_obj = prep.n_obj
    n = prep.n
    assert pool.shape[0] >= n and pool_split.records.shape[0] >= n and query_split.records.shape[0] >= m
    L = _lib.lib()
    ws = _ws(L.aoc_dense_match_split_workspace_bytes(m, n, n_obj), pool.device)
    if obj_bias is not None:
        obj_bias = _f32c(obj_bias)
    # one sticky flag covers both operands
    flag = pool_split.overflow
    if query_split.overflow.data_ptr() != flag.data_ptr():
        flag = torch.maximum(flag, query_split.overflow)
    assert not pool_split.tiled
    _span("dense_match_min_split: out", out, _dense_span(m, n_obj, out_pixel_stride, out_obj_stride))
    right_bits, wrong_bits, fg_rows, obj_rows, counts, obj_offsets = _prep_lists(prep)
    q_rec, q_sq = _a16("dense_match_min_split: query records", query_split.records), query_split.sqnorm
    p_rec = _a16("dense_match_min_split: pool records", pool_split.records)
    _lib.check(L.aoc_dense_match_min_split(_p(query_flat), _p(q_rec), _p(q_sq), int(query_split.tiled), m, C, _p(pool),
                                           _p(p_rec),
                                           _p(flag), n, _p(right_bits), _p(wrong_bits), _p(fg_rows), _p(obj_rows),
                                           _p(counts), _p(obj_offsets), _p(obj_bias), n_obj, _p(out), int(out_pixel_stride),
                                           int(out_obj_stride), int(bool(transform)), _p(ws), ws.numel(), _stream()),
               "aoc_dense_match_min_split")
    return out


# "split" = fp16-split matrix pipe with fp32-equivalent products (default); "fp32" = exact-fp32 MFMA everywhere.
DENSE_PRECISION = os.environ.get("AOC_DENSE_PRECISION", "split")


def set_stream_cus(n_cus=None, dense_share=None):
    """aoc_set_stream_cus: how many CUs the streams that launch the matrix kernels may use (a caller that runs them under a HIP CU mask
    says so; 0 = every CU of the device).  dense_share (aoc_set_dense_share): the share of those CUs, in 256ths (1 .. 256), that the dense
    matching kernel's resident workgroups take; the rest stays free for other streams.  None leaves a value as it is.
    -> the dense share now in force (aoc_dense_share)."""
    L = _lib.lib()
    if n_cus is not None:
        _lib.check(L.aoc_set_stream_cus(int(n_cus)), "aoc_set_stream_cus")
    if dense_share is not None:
        _lib.check(L.aoc_set_dense_share(int(dense_share)), "aoc_set_dense_share")
    return int(L.aoc_dense_share())


def dense_match(query_flat, pool, prep, obj_bias, out, out_pixel_stride, out_obj_stride, transform=True, precision=None,
                query_split=None, pool_split=None):
    """Dense matching front door: picks the split-fp16 entry point when the shape supports it (C % 4 == 0, C <= 100,
    <= 16 objects) and the precision mode allows, else the exact-fp32 one.  `query_split` / `pool_split` are optional
    cached SplitRows (otherwise the rows are converted here)."""
    precision = precision or DENSE_PRECISION
    if precision not in ("split", "fp32", "f16"):
        raise ValueError(f"unknown dense precision {precision!r}")
    C = query_flat.shape[1]
    # (checked here too: the split path converts the operands first, and a refused output must be refused before anything is enqueued)
    _span("dense_match: out", out, _dense_span(query_flat.shape[0], prep.n_obj, out_pixel_stride, out_obj_stride))
    if precision == "f16":          # the reference's use_float16=True arithmetic (AEM:801-803)
        return dense_match_min(query_flat, pool, prep, obj_bias, out, out_pixel_stride, out_obj_stride, transform, float16=True)
    if precision == "fp32" or split_record_bytes(C) == 0 or prep.n_obj > 16:
        return dense_match_min(query_flat, pool, prep, obj_bias, out, out_pixel_stride, out_obj_stride, transform)
    if pool_split is None:
        pool_split = split_rows(pool[:prep.n])
    if query_split is None:
        query_split = split_rows(query_flat, overflow=pool_split.overflow, tiled=True)
    return dense_match_min_split(query_flat, query_split, pool, pool_split, prep, obj_bias, out, out_pixel_stride, out_obj_stride, transform)


# ------------------------------------------------------------------------------------------ local matching + resize
def resize_bilinear_hwc(x, H, W, float16=False):
    x = _f32c(x)
    _need_gpu(x)
    h, w, C = x.shape
    out = torch.empty(H, W, C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().aoc_resize_bilinear_hwc_ex(_p(x), h, w, C, _p(out), H, W, int(bool(float16)), _stream()), "aoc_resize_bilinear_hwc_ex")
    return out


def resize_bilinear_planes(x, H, W, out, out_plane_stride, out_pixel_stride, inner_count=None, out_outer_stride=0):
    """x [P,h,w] -> strided destination (see include/aoc_hip.h); ``out`` may be a view: its data_ptr is the base."""
    x = _f32c(x)
    _need_gpu(x, out)
    P, h, w = x.shape
    inner = P if inner_count is None else int(inner_count)
    last = ((P - 1) // inner) * int(out_outer_stride) + min(inner - 1, P - 1) * int(out_plane_stride) if P else 0
    _span("resize_bilinear_planes: out", out, last + (H * W - 1) * int(out_pixel_stride) + 1 if P and H * W else 0)
    _lib.check(_lib.lib().aoc_resize_bilinear_planes(_p(x), P, h, w, _p(out), H, W, inner, int(out_outer_stride), int(out_plane_stride),
                                                     int(out_pixel_stride), _stream()), "aoc_resize_bilinear_planes")
    return out


def atrous_subsample(x, rate):
    """aoc_atrous_subsample: [h, w, X] -> [ceil(h / rate), ceil(w / rate), X] = x[::rate, ::rate] (AEM:533-579, the atrous grid of the reference pool)."""
    x = _a16("atrous_subsample: x", _f32c(x))
    _need_gpu(x)
    h, w, X = x.shape
    rate = int(rate)
    out = torch.empty((h + rate - 1) // rate, (w + rate - 1) // rate, X, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().aoc_atrous_subsample(_p(x), h, w, X, rate, _p(out), _stream()), "aoc_atrous_subsample")
    return out


def resize_nearest_bits(bits, h, w, H, W):
    _need_gpu(bits)
    bits = _i32c(bits)
    out = torch.empty(H * W, dtype=torch.int32, device=bits.device)
    _lib.check(_lib.lib().aoc_resize_nearest_bits(_p(bits), h, w, _p(out), H, W, _stream()), "aoc_resize_nearest_bits")
    return out


def local_window_match(query, prev, right_bits, radii, obj_bias, n_obj, transform=True, atrous_rate=1, float16=False):
    """query, prev [H,W,C] -> [n_obj, len(radii), H, W] (channel order [max, r_0, ...]); atrous_rate / float16 as in the reference call."""
    query, prev = _a16("local_window_match: query", _f32c(query)), _a16("local_window_match: prev", _f32c(prev))
    _need_gpu(query, prev, right_bits)
    right_bits = _i32c(right_bits)
    H, W, C = query.shape
    radii = np.ascontiguousarray(np.asarray(radii, dtype=np.int32))
    out = torch.empty(n_obj, radii.size, H, W, dtype=torch.float32, device=query.device)
    if obj_bias is not None:
        obj_bias = _f32c(obj_bias)
    _lib.check(_lib.lib().aoc_local_window_match_ex(_p(query), _p(prev), _p(right_bits), H, W, C, radii.ctypes.data_as(ctypes.c_void_p),
                                                    int(radii.size), _p(obj_bias), n_obj, _p(out), int(bool(transform)), int(atrous_rate),
                                                    int(bool(float16)), _stream()), "aoc_local_window_match_ex")
    return out


def local_window_match_argmin(query, prev, right_bits, radii, obj_bias, n_obj, transform=True, atrous_rate=1, out=None, arg=None):
    """aoc_local_window_match_argmin: local_window_match's values (float16=False; bit for bit at C = 100 / 128) and, in ``arg`` (int32, shaped
    like ``out``), the previous-frame pixel cy * W + cx of every minimum; -1 where the value is the padding.  -> (out, arg)
    [n_obj, len(radii), H, W].  The keyword buffers, when given, are written in place."""
    query, prev = _a16("local_window_match_argmin: query", _f32c(query)), _a16("local_window_match_argmin: prev", _f32c(prev))
    _need_gpu(query, prev, right_bits, out, arg)
    right_bits = _i32c(right_bits)
    H, W, C = query.shape
    radii = np.ascontiguousarray(np.asarray(radii, dtype=np.int32))
    if out is None:
        out = torch.empty(n_obj, radii.size, H, W, dtype=torch.float32, device=query.device)
    if arg is None:
        arg = torch.empty(n_obj, radii.size, H, W, dtype=torch.int32, device=query.device)
    _out("local_window_match_argmin: out", out, (n_obj, radii.size, H, W))
    _out("local_window_match_argmin: arg", arg, (n_obj, radii.size, H, W), torch.int32)
    if obj_bias is not None:
        obj_bias = _f32c(obj_bias)
    _lib.check(_lib.lib().aoc_local_window_match_argmin(_p(query), _p(prev), _p(right_bits), H, W, C, radii.ctypes.data_as(ctypes.c_void_p),
                                                        int(radii.size), _p(obj_bias), n_obj, _p(out), _p(arg), int(bool(transform)),
                                                        int(atrous_rate), _stream()), "aoc_local_window_match_argmin")
    return out, arg


def local_match_backward(grad_out, T, arg, query, prev, window, want_query=True, want_prev=True, want_bias=True,
                         grad_query=None, grad_prev=None, grad_bias=None):
    """aoc_local_match_grad.  grad_out, T, arg [n_obj, n_radii, H, W] contiguous; query, prev [H, W, C]; window = the largest window's
    half-size in pixels.  -> (grad_query [H, W, C], grad_prev [H, W, C], grad_bias [n_obj]); None for an output that is not wanted (nothing
    is written for it).  The keyword buffers, when given, are written in place."""
    query, prev = _f32c(query), _f32c(prev)
    _need_gpu(grad_out, T, arg, query, prev, grad_query, grad_prev, grad_bias)
    grad_out, T, arg = _f32c(grad_out), _f32c(T), _i32c(arg)
    n_obj, n_radii, H, W = T.shape
    if tuple(grad_out.shape) != tuple(T.shape) or tuple(arg.shape) != tuple(T.shape) or tuple(query.shape[:2]) != (H, W) or query.shape != prev.shape:
        raise ValueError(f"local_match_backward: grad_out {tuple(grad_out.shape)}, T {tuple(T.shape)}, arg {tuple(arg.shape)}, query {tuple(query.shape)} "
                         f"and prev {tuple(prev.shape)} do not fit")
    C = query.shape[2]
    dev = query.device
    if want_query and grad_query is None:
        grad_query = torch.empty(H, W, C, dtype=torch.float32, device=dev)
    if want_prev and grad_prev is None:
        grad_prev = torch.empty(H, W, C, dtype=torch.float32, device=dev)
    if want_bias and grad_bias is None:
        grad_bias = torch.empty(n_obj, dtype=torch.float32, device=dev)
    gq, gp, gb = (grad_query if want_query else None), (grad_prev if want_prev else None), (grad_bias if want_bias else None)
    for what, t, shape in (("grad_query", gq, (H, W, C)), ("grad_prev", gp, (H, W, C)), ("grad_bias", gb, (n_obj,))):
        if t is not None:
            _out("local_match_backward: " + what, t, shape)
    L = _lib.lib()
    ws = _ws(L.aoc_local_match_grad_workspace_bytes(H, W, C, n_radii, n_obj), dev)
    _lib.check(L.aoc_local_match_grad(_p(grad_out), _p(T), _p(arg), _p(query), _p(prev), H, W, C, n_radii, n_obj, int(window),
                                      _p(gq), _p(gp), _p(gb), _p(ws), ws.numel(), _stream()), "aoc_local_match_grad")
    return gq, gp, gb


def local_prep(cur_emb, prev_emb, prev_labels_flat, prev_pos, H2, W2, obj_bias=None, n_pair_sets=0, set_bias_out=None, copies=()):
    """aoc_local_prep: the half-resolution operands of both local matchings in one launch -> (q2, p2, pm2 [H2, W2, C], bits2 [H2 * W2]).
    copies: up to two (src, dst) float tensor pairs copied by the same launch; set_bias_out [n_pair_sets + O] is filled from obj_bias."""
    cur_emb, prev_emb, prev_labels_flat, prev_pos = _f32c(cur_emb), _f32c(prev_emb), _f32c(prev_labels_flat), _f32c(prev_pos)
    _need_gpu(cur_emb, prev_emb, prev_labels_flat, prev_pos, obj_bias, set_bias_out)
    h, w, C = cur_emb.shape
    n_obj = prev_labels_flat.shape[-1]
    dev = cur_emb.device
    q2 = torch.empty(H2, W2, C, dtype=torch.float32, device=dev)
    p2, pm2 = torch.empty_like(q2), torch.empty_like(q2)
    bits2 = torch.empty(H2 * W2, dtype=torch.int32, device=dev)
    cp = [(None, None, 0), (None, None, 0)]
    for i, (src, dst) in enumerate(copies):
        assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype == torch.float32 and src.numel() == dst.numel()
        cp[i] = (src, dst, src.numel())
    if obj_bias is not None:
        obj_bias = _f32c(obj_bias)
    if set_bias_out is not None:
        _out("local_prep: set_bias_out", set_bias_out, (int(n_pair_sets) + n_obj,))
    (src_a, dst_a, n_a), (src_b, dst_b, n_b) = cp
    _lib.check(_lib.lib().aoc_local_prep(_p(cur_emb), _p(prev_emb), _p(prev_labels_flat), _p(prev_pos), h, w, C, n_obj, _p(q2), _p(p2), _p(pm2), _p(bits2),
                                         int(H2), int(W2), _p(obj_bias), int(n_pair_sets), _p(set_bias_out), _p(src_a), _p(dst_a), n_a,
                                         _p(src_b), _p(dst_b), n_b, _stream()), "aoc_local_prep")
    return q2, p2, pm2, bits2


def local_window_match_pair(query, prev_a, prev_b, right_bits, radii, obj_bias, n_obj, transform=True):
    """aoc_local_window_match_pair -> [2, n_obj, len(radii), H, W]: local matching against prev_a and prev_b in one launch."""
    query, prev_a, prev_b = (_a16("local_window_match_pair: " + w, _f32c(t)) for w, t in (("query", query), ("prev_a", prev_a), ("prev_b", prev_b)))
    _need_gpu(query, prev_a, prev_b, right_bits)
    right_bits = _i32c(right_bits)
    H, W, C = query.shape
    radii = np.ascontiguousarray(np.asarray(radii, dtype=np.int32))
    out = torch.empty(2, n_obj, radii.size, H, W, dtype=torch.float32, device=query.device)
    out_a, out_b = out[0], out[1]
    if obj_bias is not None:
        obj_bias = _f32c(obj_bias)
    _lib.check(_lib.lib().aoc_local_window_match_pair(_p(query), _p(prev_a), _p(prev_b), _p(right_bits), H, W, C, radii.ctypes.data_as(ctypes.c_void_p),
                                                      int(radii.size), _p(obj_bias), n_obj, _p(out_a), _p(out_b), int(bool(transform)), _stream()),
               "aoc_local_window_match_pair")
    return out


def resize_bilinear_planes_grouped(x, H, W, out, inner_count, outer_count, group_stride, outer_stride, plane_stride, pixel_stride=1):
    """aoc_resize_bilinear_planes_grouped: x [P, h, w], plane p = (group, outer, inner) -> strided destination."""
    x = _f32c(x)
    _need_gpu(x, out)
    P, h, w = x.shape
    ic, oc = int(inner_count), int(outer_count)
    if P and P % (ic * oc) == 0:
        last = (P // (ic * oc) - 1) * int(group_stride) + (oc - 1) * int(outer_stride) + (ic - 1) * int(plane_stride)
    else:
        last = max(((p // (ic * oc)) * int(group_stride) + (p // ic % oc) * int(outer_stride) + (p % ic) * int(plane_stride) for p in range(P)), default=0)
    _span("resize_bilinear_planes_grouped: out", out, last + (H * W - 1) * int(pixel_stride) + 1 if P and H * W else 0)
    _lib.check(_lib.lib().aoc_resize_bilinear_planes_grouped(_p(x), P, h, w, _p(out), H, W, int(inner_count), int(outer_count), int(group_stride),
                                                             int(outer_stride), int(plane_stride), int(pixel_stride), _stream()),
               "aoc_resize_bilinear_planes_grouped")
    return out


def proto_finish(feat, hw, obj_stride, ch_local, n_local, ch_local_bg, ch_global, ch_global_bg, ch_prev_mask, prev_labels_flat,
                 ref_pos=None, ref_neg=None, prev_pos=None, prev_neg=None):
    """aoc_proto_finish: background channels, previous-mask channel and (when the four pooled heads are given) the attention head
    [O, 4C] of one frame in one launch.  Returns the head (or None)."""
    _need_gpu(feat, prev_labels_flat, ref_pos, ref_neg, prev_pos, prev_neg)
    n_obj = feat.shape[0]
    head, C = None, 0
    if ref_pos is not None:
        C = ref_pos.shape[1]
        head = torch.empty(n_obj, 4 * C, dtype=torch.float32, device=feat.device)
        ref_pos, ref_neg, prev_pos, prev_neg = _f32c(ref_pos), _f32c(ref_neg), _f32c(prev_pos), _f32c(prev_neg)
        for t in (ref_pos, ref_neg, prev_pos, prev_neg):
            assert t.shape == (n_obj, C)
    if prev_labels_flat is not None:
        prev_labels_flat = _f32c(prev_labels_flat)
    # feat is read and written in place, channel by channel: the highest channel any switched-on part touches bounds what it must hold
    top = max(max(int(ch_local), int(ch_local_bg)) + int(n_local) if int(ch_local_bg) >= 0 else 0,
              max(int(ch_global), int(ch_global_bg)) + 1 if int(ch_global_bg) >= 0 else 0, int(ch_prev_mask) + 1, 0)
    _span("proto_finish: feat", feat, (n_obj - 1) * int(obj_stride) + top * int(hw) if n_obj else 0)
    _lib.check(_lib.lib().aoc_proto_finish(_p(feat), n_obj, int(hw), int(obj_stride), int(ch_local), int(n_local), int(ch_local_bg), int(ch_global),
                                           int(ch_global_bg), int(ch_prev_mask), _p(prev_labels_flat), _p(ref_pos), _p(ref_neg), _p(prev_pos), _p(prev_neg),
                                           int(C), _p(head), _stream()), "aoc_proto_finish")
    return head


class _FrameDesc(ctypes.Structure):
    """aoc_frame_desc of include/aoc_hip.h."""
    _fields_ = [("h", ctypes.c_int32), ("w", ctypes.c_int32), ("C", ctypes.c_int32), ("n_obj", ctypes.c_int32),
                ("R", ctypes.c_int32), ("R_capacity", ctypes.c_int32),
                ("n_radii", ctypes.c_int32), ("radii", ctypes.c_int32 * 8),
                ("n_levels", ctypes.c_int32), ("levels", ctypes.c_int32 * 8),
                ("kmax", ctypes.c_int32), ("matching_background", ctypes.c_int32), ("n_adaptive", ctypes.c_int32), ("epsilon", ctypes.c_float),
                ("pool_prefix_frames", ctypes.c_int32), ("stream_cus", ctypes.c_int32),
                ("float16_matching", ctypes.c_int32), ("local_downsample", ctypes.c_int32), ("local_atrous_rate", ctypes.c_int32), ("match_hw", ctypes.c_int32),
                ("pool_key", ctypes.c_int64),
                ("ref_emb", ctypes.c_void_p), ("ref_labels", ctypes.c_void_p), ("match_emb", ctypes.c_void_p), ("prev_emb", ctypes.c_void_p), ("prev_labels", ctypes.c_void_p),
                ("cur_emb", ctypes.c_void_p), ("dis_bias", ctypes.c_void_p),
                ("right_bits", ctypes.c_void_p), ("wrong_bits", ctypes.c_void_p), ("fg_rows", ctypes.c_void_p), ("obj_rows", ctypes.c_void_p),
                ("counts", ctypes.c_void_p), ("obj_offsets", ctypes.c_void_p),
                ("proxy_table", ctypes.c_void_p), ("proxy_sqnorm", ctypes.c_void_p), ("prep_ready", ctypes.c_void_p), ("proxies_ready", ctypes.c_void_p),
                ("feat", ctypes.c_void_p), ("head", ctypes.c_void_p), ("probe", ctypes.c_void_p * 6)]


class _ChainDesc(ctypes.Structure):
    """aoc_chain_desc of include/aoc_hip.h."""
    _fields_ = [("C", ctypes.c_int32), ("n_obj", ctypes.c_int32), ("n_frames", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("levels", ctypes.c_int32 * 8),
                ("kmax", ctypes.c_int32), ("iters", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("pool_rows", ctypes.c_int64), ("rows_capacity", ctypes.c_int64),
                ("pool", ctypes.c_void_p), ("fg_rows", ctypes.c_void_p), ("obj_rows", ctypes.c_void_p), ("obj_offsets", ctypes.c_void_p),
                ("init_rows", ctypes.c_void_p), ("tables", ctypes.c_void_p * 8), ("sqnorms", ctypes.c_void_p * 8)]


CHAIN_MAX_FRAMES = 8      # frames one aoc_chain_desc names (tables[8] / sqnorms[8])


def _adaptive_rows(levels, n_obj):
    """Rows of the adaptive part of a proxy table: levels x objects x (centroid | centroid_avg) x kmax."""
    return len(levels) * n_obj * 2 * int(max(levels))


def cluster_chain(pool, prep, levels, init_rows, tables, sqnorms, iters=20):
    """aoc_cluster_chain_enqueue: the k-means chain of len(tables) frames that see one pool state -- replicated lists with sticky K, 20 Lloyd
    iterations, proxy construction, every frame's proxies scattered into ITS table -- as ONE C call out of one workspace (on the current stream,
    no host synchronisation).  pool [rows, C]; prep = LabelPrep of the pool's labels; init_rows int32 [F * L * O, kmax]; tables[f] [L*O*2*kmax + O, C],
    sqnorms[f] [L*O*2*kmax + O].  Returns a dict of views into the workspace (centroids, labels, cluster_counts, proxies, proxy_sqnorm, seg_k,
    seg_offsets), valid until the workspace is reused."""
    pool = _a16("cluster_chain: pool", _f32c(pool))
    _need_gpu(pool, init_rows, *tables, *sqnorms)
    F, L, O, C = len(tables), len(levels), prep.n_obj, pool.shape[1]
    kmax, n_ad = int(max(levels)), _adaptive_rows(levels, O)
    init_rows = _i32c(init_rows)
    _, _, fg_rows, obj_rows, _, obj_offsets = _prep_lists(prep)
    if not (1 <= F <= CHAIN_MAX_FRAMES and 1 <= L <= 8 and len(sqnorms) == F and init_rows.numel() == F * L * O * kmax):
        raise _lib.AocHipError("cluster_chain: 1..8 frames, 1..8 levels, one squared-norm array per table, init_rows [F * L * O, kmax]")
    d = _ChainDesc()
    d.C, d.n_obj, d.n_frames, d.n_levels, d.kmax, d.iters = C, O, F, L, kmax, int(iters)
    for i, k in enumerate(levels):
        d.levels[i] = int(k)
    d.pool_rows, d.rows_capacity = pool.shape[0], obj_rows.numel()
    d.pool, d.fg_rows, d.obj_rows, d.obj_offsets, d.init_rows = _addr(pool), _addr(fg_rows), _addr(obj_rows), _addr(obj_offsets), _addr(init_rows)
    for f in range(F):
        table, sqn = tables[f], sqnorms[f]
        if table.dim() != 2 or table.shape[0] < n_ad:
            raise ValueError(f"cluster_chain: tables[{f}] {tuple(table.shape)} has fewer than {n_ad} rows")
        _out(f"cluster_chain: tables[{f}]", table, (table.shape[0], C))
        _a16(f"cluster_chain: tables[{f}]", table, output=True)
        _span(f"cluster_chain: sqnorms[{f}]", sqn, n_ad)
        d.tables[f], d.sqnorms[f] = _addr(table), _addr(sqn)
    lib = _lib.lib()
    ws = _ws(lib.aoc_cluster_chain_workspace_bytes(ctypes.byref(d)), pool.device)
    _lib.check(lib.aoc_cluster_chain_enqueue(ctypes.byref(d), _p(ws), ws.numel(), _stream()), "aoc_cluster_chain_enqueue")
    off = (ctypes.c_int64 * 7)()
    _lib.check(lib.aoc_cluster_chain_layout(ctypes.byref(d), off), "aoc_cluster_chain_layout")
    S, cap = F * L * O, F * L * prep.obj_rows.numel()

    def view(i, n, dtype, shape):
        return ws[off[i]:off[i] + n * 4].view(dtype).view(shape)
    return dict(workspace=ws, keep=(pool, init_rows, fg_rows, obj_rows, obj_offsets), centroids=view(0, S * kmax * C, torch.float32, (S, kmax, C)), labels=view(1, cap, torch.int32, (cap,)),
                cluster_counts=view(2, S * kmax, torch.int32, (S, kmax)), proxies=view(3, S * 2 * kmax * C, torch.float32, (S, 2, kmax, C)),
                proxy_sqnorm=view(4, S * 2 * kmax, torch.float32, (S, 2, kmax)), seg_k=view(5, S, torch.int32, (S,)),
                seg_offsets=view(6, S + 1, torch.int32, (S + 1,)))


class _GateDesc(ctypes.Structure):
    """aoc_gate_desc of include/aoc_hip.h."""
    _fields_ = [("kind", ctypes.c_int32), ("channels", ctypes.c_int32), ("k_rank", ctypes.c_int32), ("reserved", ctypes.c_int32), ("hw", ctypes.c_int64),
                ("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("w", ctypes.c_void_p), ("b", ctypes.c_void_p),
                ("phi_w", ctypes.c_void_p), ("phi_b", ctypes.c_void_p), ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p),
                ("b2", ctypes.c_void_p), ("w3", ctypes.c_void_p), ("b3", ctypes.c_void_p), ("probe", ctypes.c_void_p * 4)]


class GateBatch:
    """aoc_gates_enqueue: a fixed list of gates (modules + the activations they modulate + persistent outputs) applied by ONE C call per frame.
    entries: (kind, x, params) with params = (w, b) for kinds 0 / 1 and (w, b, phi_w, phi_b, w1, b1, w2, b2, w3, b3, k_rank) for kind 2."""

    def __init__(self, entries, n_obj, head_dim):
        self.n, self.n_obj, self.D = len(entries), int(n_obj), int(head_dim)
        self.arr = (_GateDesc * self.n)()
        self.keep, self.outs = [], []
        self.converted = False
        for i, (kind, x, prm) in enumerate(entries):
            _need_gpu(x, *prm[:10])
            assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] == n_obj
            y = torch.empty_like(x)
            ts = [_f32c(t.detach()) for t in prm[:10]]
            # a parameter that had to be converted is read from a COPY kept here: an in-place update of the original is not seen through it
            # (hotpath.CalibrationGates watches the parameters' versions then)
            self.converted = self.converted or any(t.dtype != torch.float32 or not t.is_contiguous() for t in prm[:10])
            self.keep.append((x, ts))
            self.outs.append(y)
            d = self.arr[i]
            d.kind, d.channels, d.hw = int(kind), int(x.shape[1]), int(x.numel() // (x.shape[0] * x.shape[1]))
            d.x, d.y, d.w, d.b = _addr(x), _addr(y), _addr(ts[0]), _addr(ts[1])
            if kind == 2:
                d.phi_w, d.phi_b, d.w1, d.b1, d.w2, d.b2, d.w3, d.b3 = [_addr(t) for t in ts[2:10]]
                d.k_rank = int(prm[10])
        L = _lib.lib()
        self.ws = torch.empty(max(16, int(L.aoc_gates_workspace_bytes(ctypes.cast(self.arr, ctypes.c_void_p), self.n, self.n_obj, self.D))),
                              dtype=torch.uint8, device=entries[0][1].device)

    def __call__(self, head, probes=None):
        """probes (measurement only): per gate a list of four raw hipEvent_t handles or None (aoc_gate_desc.probe)."""
        head = _f32c(head)
        _need_gpu(head)
        assert tuple(head.shape) == (self.n_obj, self.D)
        for i in range(self.n):
            for k in range(4):
                self.arr[i].probe[k] = probes[i][k] if probes is not None else None
        _lib.check(_lib.lib().aoc_gates_enqueue(ctypes.cast(self.arr, ctypes.c_void_p), self.n, _p(head), self.n_obj, self.D, _p(self.ws), self.ws.numel(),
                                                _stream()), "aoc_gates_enqueue")
        return self.outs


class _SeqState(ctypes.Structure):
    """aoc_seq_state of include/aoc_hip.h."""
    _fields_ = [("initialised", ctypes.c_int64), ("records_frames", ctypes.c_int64), ("ref_pool_key", ctypes.c_int64), ("plan_key", ctypes.c_int64),
                ("plan_rows", ctypes.c_int64), ("corr_tables_key", ctypes.c_int64)]


class FrameCall:
    """aoc_frame_enqueue for the frames of ONE sequence: owns the sequence's device workspace and host state record.
    supported(...) says whether the one-call path covers a configuration (otherwise hotpath.proto_mask_features drives the individual calls)."""

    @staticmethod
    def supported(C, n_obj, local_downsample, float16_matching, n_radii, n_levels):
        """Round 5: every switch of the reference's evaluation CLI / config is covered (float16 matching, local matching with or without the
        down-sample, the atrous rates, up to 30 objects); what remains outside is another embedding width and the developer's exact-fp32 mode."""
        return C == 100 and n_obj <= MAX_OBJECTS and n_radii <= 8 and n_levels <= 8 and DENSE_PRECISION == "split"

    def __init__(self, h, w, C, n_obj, capacity_frames, radii, levels, matching_background, epsilon, device, float16_matching=False, local_downsample=True,
                 local_atrous_rate=1, global_atrous_rate=1):
        L = _lib.lib()
        self.h, self.w, self.C, self.n_obj, self.cap = int(h), int(w), int(C), int(n_obj), int(capacity_frames)
        self.n_ch = int(L.aoc_frame_channels(len(radii), len(levels), int(bool(matching_background))))
        nbytes = int(L.aoc_frame_workspace_bytes(self.h, self.w, self.C, self.n_obj, self.cap, len(radii), len(levels)))
        if nbytes == 0:
            raise _lib.AocHipError("aoc_frame_workspace_bytes: unsupported configuration")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.state = _SeqState()
        d = self.desc = _FrameDesc()
        d.h, d.w, d.C, d.n_obj, d.R_capacity = self.h, self.w, self.C, self.n_obj, self.cap
        d.n_radii, d.n_levels, d.kmax = len(radii), len(levels), max(levels)
        for i, r in enumerate(radii):
            d.radii[i] = int(r)
        for i, k in enumerate(levels):
            d.levels[i] = int(k)
        d.matching_background = int(bool(matching_background))
        d.n_adaptive = _adaptive_rows(levels, self.n_obj)
        d.epsilon = float(epsilon)
        d.float16_matching, d.local_downsample, d.local_atrous_rate = int(bool(float16_matching)), int(bool(local_downsample)), int(local_atrous_rate)
        # TEST_GLOBAL_ATROUS_RATE > 1: the dense and cluster matchings see every pool frame on the atrous grid (AEM:533-579); the sub-sampled pool is
        # kept here, one aoc_atrous_subsample per frame that joins (append-only), and handed over as match_emb
        self.grate = int(global_atrous_rate)
        self.match_hw = ((self.h + self.grate - 1) // self.grate) * ((self.w + self.grate - 1) // self.grate) if self.grate > 1 else 0
        self.match_emb = torch.empty(self.cap, self.match_hw, self.C, dtype=torch.float32, device=device) if self.grate > 1 else None
        self.match_frames = 0
        self.device = device

    def reset(self):
        """A new sequence starts in this workspace (eval_manager_mm.py:376-382)."""
        ctypes.memset(ctypes.byref(self.state), 0, ctypes.sizeof(self.state))
        self.match_frames = 0

    def match_pool(self, ref_emb, ref_labels, pool_prefix_frames=None):
        """TEST_GLOBAL_ATROUS_RATE > 1: (embeddings [R, h', w', C], labels [R, h', w', O]) of the pool on the atrous grid -- what the label prep and the
        k-means chain of the frame have to be computed from.  The embeddings are kept per sequence (only frames that joined are sub-sampled);
        rate 1: the arguments themselves."""
        if self.grate <= 1:
            return ref_emb, ref_labels
        R = ref_emb.shape[0]
        done = min(self.match_frames, R if pool_prefix_frames is None else int(pool_prefix_frames))
        hh, ww = (self.h + self.grate - 1) // self.grate, (self.w + self.grate - 1) // self.grate
        assert ref_emb.dtype == torch.float32 and ref_emb.is_contiguous() and tuple(ref_emb.shape[1:]) == (self.h, self.w, self.C) and R <= self.cap, \
            "match_pool takes the contiguous float32 pool [R <= capacity, h, w, C]"
        _need_gpu(ref_emb)
        for r in range(done, R):
            src, dst = _a16("FrameCall.match_pool: ref_emb[r]", ref_emb[r]), self.match_emb[r]
            _lib.check(_lib.lib().aoc_atrous_subsample(_p(src), self.h, self.w, self.C, self.grate, _p(dst), _stream()), "aoc_atrous_subsample")
        self.match_frames = R
        labs = torch.stack([atrous_subsample(ref_labels[r], self.grate) for r in range(R)])
        return self.match_emb[:R].view(R, hh, ww, self.C), labs

    def __call__(self, ref_emb, ref_labels, prev_emb, prev_labels, cur_emb, dis_bias, prep, table, sqn, prep_event=None, done_event=None, pool_key=None,
                 probes=None, pool_prefix_frames=None, stream_cus=0):
        """ref_emb [R, h, w, C] / ref_labels [R, h, w, O] contiguous fp32 views of the resident pool; prep = LabelPrep of ref_labels; table / sqn = this
        frame's proxy table (adaptive rows written by the k-means chain).  Returns (feat [O, n_ch, h, w], head [O, 4C]).
        pool_key (REQUIRED, != 0): identifies the pool's content -- it keys the pooled reference heads and the dense kernel's plan; an append-only pool
        may pass its frame count.  pool_prefix_frames: leading pool frames unchanged since the previous call (their split records are kept); None =
        the pool is append-only (everything converted so far stays valid); a caller that REPLACES pool frames passes the first replaced index."""
        if pool_key is None or int(pool_key) == 0:
            raise _lib.AocHipError("FrameCall: pool_key is required (a non-zero value that changes whenever the pool's content changes)")
        _need_gpu(ref_emb, ref_labels, prev_emb, prev_labels, cur_emb, dis_bias, table, sqn)
        for t in (ref_emb, ref_labels, prev_emb, prev_labels, cur_emb, dis_bias, table, sqn):
            assert t.dtype == torch.float32 and t.is_contiguous(), "aoc_frame_enqueue takes contiguous float32 tensors"
        right_bits, wrong_bits, fg_rows, obj_rows, counts, obj_offsets = prep.tensors()
        for t in (right_bits, wrong_bits, fg_rows, obj_rows, counts, obj_offsets):
            assert t.dtype == torch.int32 and t.is_contiguous(), "aoc_frame_enqueue takes the contiguous int32 lists of ops.label_prep"
        # class-16 pointers of aoc_frame_desc: the three embeddings are inputs (copied when off the grid), the proxy table is also written
        ref_emb, prev_emb, cur_emb = _a16("FrameCall: ref_emb", ref_emb), _a16("FrameCall: prev_emb", prev_emb), _a16("FrameCall: cur_emb", cur_emb)
        _a16("FrameCall: table", table, output=True)
        R = ref_emb.shape[0]
        d = self.desc
        assert R <= self.cap and tuple(cur_emb.shape) == (self.h, self.w, self.C) and ref_labels.shape[-1] == self.n_obj and dis_bias.numel() == self.n_obj
        hw = self.h * self.w
        assert ref_emb.numel() == R * hw * self.C and ref_labels.numel() == R * hw * self.n_obj and prev_emb.numel() == hw * self.C \
            and prev_labels.numel() == hw * self.n_obj and table.numel() == table.shape[0] * self.C and sqn.numel() == table.shape[0], \
            "aoc_frame_enqueue reads whole maps and tables through bare pointers: a smaller tensor would be read past its end"
        assert table.shape[0] == d.n_adaptive + self.n_obj and prep.n ==R * (self.match_hw if self.grate > 1 else self.h * self.w), \
            "prep = the label prep of the pool the matchings see (match_pool(...) with a global atrous rate)"
        if self.grate > 1:
            assert self.match_frames >= R, "call match_pool(ref_emb, ref_labels) first: it keeps the sub-sampled pool the matchings read"
            d.match_hw, d.match_emb = self.match_hw, _addr(self.match_emb)
        else:
            d.match_hw, d.match_emb = 0, None
        feat = torch.empty(self.n_obj, self.n_ch, self.h, self.w, dtype=torch.float32, device=self.device)
        head = torch.empty(self.n_obj, 4 * self.C, dtype=torch.float32, device=self.device)
        d.R = R
        d.pool_key = int(pool_key)
        d.pool_prefix_frames = int(R if pool_prefix_frames is None else pool_prefix_frames)
        d.stream_cus = int(stream_cus)              # > 0: this call's stream runs under a CU mask of that many CUs (else: aoc_set_stream_cus)
        d.ref_emb, d.ref_labels, d.prev_emb, d.prev_labels, d.cur_emb = _addr(ref_emb), _addr(ref_labels), _addr(prev_emb), _addr(prev_labels), _addr(cur_emb)
        d.dis_bias = _addr(dis_bias)
        d.right_bits, d.wrong_bits, d.fg_rows, d.obj_rows = _addr(right_bits), _addr(wrong_bits), _addr(fg_rows), _addr(obj_rows)
        d.counts, d.obj_offsets = _addr(counts), _addr(obj_offsets)
        d.proxy_table, d.proxy_sqnorm = _addr(table), _addr(sqn)
        d.prep_ready = prep_event.cuda_event if prep_event is not None else None
        d.proxies_ready = done_event.cuda_event if done_event is not None else None
        d.feat, d.head = _addr(feat), _addr(head)
        for i in range(6):                      # measurement only: raw hipEvent_t handles (bench.py)
            d.probe[i] = probes[i] if probes is not None else None
        _lib.check(_lib.lib().aoc_frame_enqueue(ctypes.byref(d), ctypes.byref(self.state), _p(self.ws), self.ws.numel(), _stream()), "aoc_frame_enqueue")
        return feat, head


# ------------------------------------------------------------------------------------------ calibration side
def fg2bg_min(dis, n_obj, out=None, dis_obj_stride=None, out_obj_stride=None, n_ch=None, inner=None):
    """dis [O, c, ...] -> [O, 1, ...]: min over the other objects and over dim 1 (AEM:18-20).
    With explicit strides / sizes it reads and writes channel slices of a larger buffer in place."""
    _need_gpu(dis)
    if out is None:
        dis = _f32c(dis)
        n_ch = dis.shape[1]
        inner = dis.numel() // (n_obj * n_ch)
        out = torch.empty((n_obj, 1) + tuple(dis.shape[2:]), dtype=torch.float32, device=dis.device)
        dis_obj_stride, out_obj_stride = n_ch * inner, inner
    else:
        # channel slices of larger buffers, addressed with the caller's strides: neither can be converted, both are checked
        _need_gpu(out)
        _span("fg2bg_min: dis", dis, (n_obj - 1) * int(dis_obj_stride) + int(n_ch) * int(inner) if n_obj else 0)
        _span("fg2bg_min: out", out, (n_obj - 1) * int(out_obj_stride) + int(inner) if n_obj else 0)
    _lib.check(_lib.lib().aoc_fg2bg_min(_p(dis), n_obj, int(n_ch), int(inner), int(dis_obj_stride), _p(out), int(out_obj_stride), _stream()),
               "aoc_fg2bg_min")
    return out


def label_mix(labels_flat, rows):
    """out[p,:] = sum_o labels[p,o] * rows[o,:]   (aocnet.py:325)."""
    labels_flat, rows = _f32c(labels_flat), _f32c(rows)
    _need_gpu(labels_flat, rows)
    n, n_obj = labels_flat.shape
    C = rows.shape[1]
    out = torch.empty(n, C, dtype=torch.float32, device=rows.device)
    _lib.check(_lib.lib().aoc_label_mix(_p(labels_flat), _p(rows), n, n_obj, C, _p(out), _stream()), "aoc_label_mix")
    return out


def masked_mean_pool(emb, labels, epsilon, pixel_major=False, out_pos=None, out_neg=None, out_pos_sqnorm=None):
    """emb [F, hw, C]; labels [F, O, hw] (or [F, hw, O] with pixel_major) -> (pos [O,C], neg [O,C])   (ATT:155-189)."""
    emb, labels = _f32c(emb), _f32c(labels)
    _need_gpu(emb, labels)
    F_, hw, C = emb.shape
    n_obj = labels.shape[2] if pixel_major else labels.shape[1]
    L = _lib.lib()
    pos = torch.empty(n_obj, C, dtype=torch.float32, device=emb.device) if out_pos is None else out_pos
    neg = torch.empty(n_obj, C, dtype=torch.float32, device=emb.device) if out_neg is None else out_neg
    _need_gpu(out_pos, out_neg, out_pos_sqnorm)
    _out("masked_mean_pool: out_pos", pos, (n_obj, C))
    _out("masked_mean_pool: out_neg", neg, (n_obj, C))
    if out_pos_sqnorm is not None:
        _out("masked_mean_pool: out_pos_sqnorm", out_pos_sqnorm, (n_obj,))
    ws = _ws(L.aoc_masked_mean_pool_workspace_bytes(F_, hw, n_obj, C), emb.device)
    _lib.check(L.aoc_masked_mean_pool(_p(emb), _p(labels), F_, hw, C, n_obj, int(bool(pixel_major)), float(epsilon), _p(pos), _p(neg),
                                      _p(out_pos_sqnorm), _p(ws), ws.numel(), _stream()), "aoc_masked_mean_pool")
    return pos, neg


def film_gain(head, weight, bias):
    head, weight = _f32c(head), _f32c(weight)
    bias = _opt(bias)
    _need_gpu(head, weight, bias)
    n_obj, D = head.shape
    channels = weight.shape[0]
    gain = torch.empty(n_obj, channels, dtype=torch.float32, device=head.device)
    _lib.check(_lib.lib().aoc_film_gain(_p(head), _p(weight), _p(bias), n_obj, D, channels, _p(gain), _stream()), "aoc_film_gain")
    return gain


def channel_scale(x, gain, out=None):
    """y[n,c,:,:] = gain[n,c] * x[n,c,:,:]."""
    x, gain = _f32c(x), _f32c(gain)
    _need_gpu(x, gain)
    planes = x.shape[0] * x.shape[1]
    hw = x.numel() // planes
    assert gain.numel() == planes
    y = torch.empty_like(x) if out is None else _out("channel_scale: out", out, x.shape)
    _need_gpu(out)
    _lib.check(_lib.lib().aoc_channel_scale(_p(x), _p(gain), planes, hw, _p(y), _stream()), "aoc_channel_scale")
    return y


def film_scale(x, head, weight, bias, out=None):
    """y[o,c,:,:] = (1 + tanh(head[o,:] . weight[c,:] + bias[c])) * x[o,c,:,:] in one launch (ATT:12-17, CLB:81-84)."""
    x, head, weight = _f32c(x), _f32c(head), _f32c(weight)
    bias = _opt(bias)
    _need_gpu(x, head, weight, bias)
    n_obj, channels = x.shape[0], x.shape[1]
    assert head.shape[0] == n_obj and weight.shape[0] == channels and weight.shape[1] == head.shape[1]
    hw = x.numel() // (n_obj * channels)
    y = torch.empty_like(x) if out is None else _out("film_scale: out", out, x.shape)
    _need_gpu(out)
    _lib.check(_lib.lib().aoc_film_scale(_p(x), _p(head), _p(weight), _p(bias), n_obj, head.shape[1], channels, hw, _p(y), _stream()), "aoc_film_scale")
    return y


def _gate_shapes(what, n_obj, channels, head, weight, bias):
    """A gate's head [n_obj, D], weight [channels, D] and bias [channels]: ValueError on a mismatch (no device is needed for it)."""
    if head.dim() != 2 or weight.dim() != 2 or head.shape[0] != n_obj or weight.shape[1] != head.shape[1]:
        raise ValueError(f"{what}: head {tuple(head.shape)} and weight {tuple(weight.shape)} do not fit {n_obj} objects")
    if weight.shape[0] != channels or (bias is not None and bias.numel() != channels):
        raise ValueError(f"{what}: the gate has {weight.shape[0]} rows, the tensor {channels} channels")


def cat_film_scale(x, mem, head, weight, bias, out=None):
    """torch.cat([x, mem], 1) gated by IA_gate in one launch (decoding_module.py:193-194, 203-204): bit-equal to
    ``film_scale(torch.cat([x, mem], 1), head, weight, bias)``.  mem may be x itself (first frame) or None (plain film_scale)."""
    x, head, weight = _f32c(x), _f32c(head), _f32c(weight)
    mem = _opt(mem)
    bias = _opt(bias)
    n_obj, Cx = x.shape[0], x.shape[1]
    Cm = mem.shape[1] if mem is not None else 0
    if mem is not None and (mem.shape[0] != n_obj or mem.shape[2:] != x.shape[2:]):
        raise ValueError(f"cat_film_scale: x {tuple(x.shape)} and the memory {tuple(mem.shape)} differ outside dim 1")
    _gate_shapes("cat_film_scale", n_obj, Cx + Cm, head, weight, bias)
    _need_gpu(x, mem, head, weight, bias)
    hw = x.numel() // (n_obj * Cx)
    shape = (n_obj, Cx + Cm) + tuple(x.shape[2:])
    y = torch.empty(shape, dtype=torch.float32, device=x.device) if out is None else out
    assert y.is_contiguous() and tuple(y.shape) == shape and y.dtype == torch.float32
    _lib.check(_lib.lib().aoc_cat_film_scale(_p(x), _p(mem), _p(head), _p(weight), _p(bias), n_obj, head.shape[1], Cx, Cm, hw, _p(y), _stream()),
               "aoc_cat_film_scale")
    return y


def cond_gate_pool(z, phi_w, phi_b, k_rank, want_debug=False, want_plane_mean=False):
    """CL:23-43 -> gap [N, C] (optionally also scores [N,HW] and threshold [N]; with want_plane_mean also the plane means [N, C] of z,
    CLB:68, from the same pass that computes the scores)."""
    z, phi_w, phi_b = _f32c(z), _f32c(phi_w).reshape(-1), _f32c(phi_b).reshape(-1)
    _need_gpu(z, phi_w, phi_b)
    N, C = z.shape[0], z.shape[1]
    hw = z.numel() // (N * C)
    L = _lib.lib()
    gap = torch.empty(N, C, dtype=torch.float32, device=z.device)
    pm = torch.empty(N, C, dtype=torch.float32, device=z.device) if want_plane_mean else None
    scores = torch.empty(N, hw, dtype=torch.float32, device=z.device) if want_debug else None
    thr = torch.empty(N, dtype=torch.float32, device=z.device) if want_debug else None
    ws = _ws(L.aoc_cond_gate_pool_workspace_bytes(N, C, hw), z.device)
    _lib.check(L.aoc_cond_gate_pool_ex(_p(z), N, C, hw, _p(phi_w), _p(phi_b), int(k_rank), _p(gap), _p(pm), _p(scores), _p(thr), _p(ws), ws.numel(),
                                       _stream()), "aoc_cond_gate_pool_ex")
    out = (gap, scores, thr) if want_debug else gap
    if want_plane_mean:
        return (out + (pm,)) if want_debug else (gap, pm)
    return out


def linear(x, weight, bias):
    x, weight = _f32c(x), _f32c(weight)
    bias = _opt(bias)
    _need_gpu(x, weight, bias)
    N, in_dim = x.shape
    out_dim = weight.shape[0]
    y = torch.empty(N, out_dim, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().aoc_linear(_p(x), _p(weight), _p(bias), N, in_dim, out_dim, _p(y), _stream()), "aoc_linear")
    return y


def plane_mean(x):
    """[N, C, H, W] -> [N, C] (CLB:68 avg_pool2d over the whole map)."""
    x = _f32c(x)
    _need_gpu(x)
    planes = x.shape[0] * x.shape[1]
    hw = x.numel() // planes
    out = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().aoc_plane_mean(_p(x), planes, hw, _p(out), _stream()), "aoc_plane_mean")
    return out


def head_delta(head, plane_means):
    """torch.cat([head, plane_means.sum(0, keepdim=True) - plane_means], 1) in one launch (aoc_head_delta; decoding_module.py:126-130)."""
    head, plane_means = _f32c(head), _f32c(plane_means)
    _need_gpu(head, plane_means)
    n_obj, D = head.shape
    C = plane_means.shape[1]
    out = torch.empty(n_obj, D + C, dtype=torch.float32, device=head.device)
    _lib.check(_lib.lib().aoc_head_delta(_p(head), D, _p(plane_means), n_obj, C, _p(out), _stream()), "aoc_head_delta")
    return out


# ------------------------------------------------------------------------------------------ eval-loop memory policy
def confident_labels(probs_flat, exist_bits, join_label=None, unc_ratio=1.0):
    """aoc_confident_labels: probs [n_ch, n] -> (labels [n], confident [n] with 125 = uncertain, entropy [n])."""
    probs_flat = _f32c(probs_flat)
    _need_gpu(probs_flat, join_label)
    n_ch, n = probs_flat.shape
    dev = probs_flat.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    confident = torch.empty(n, dtype=torch.int32, device=dev)
    entropy = torch.empty(n, dtype=torch.float32, device=dev)
    if join_label is not None:
        join_label = _i32c(join_label).reshape(-1)
        assert join_label.numel() == n
    _lib.check(_lib.lib().aoc_confident_labels(_p(probs_flat), n_ch, n, int(exist_bits) & 0xFFFFFFFF, _p(join_label), float(unc_ratio), _p(labels),
                                               _p(confident), _p(entropy), _stream()), "aoc_confident_labels")
    return labels, confident, entropy


def label_onehot_nearest(label_hw, h, w, n_obj):
    """aoc_label_onehot_nearest: int label map [H, W] -> float one-hot [h, w, n_obj] at matching resolution."""
    _need_gpu(label_hw)
    label_hw = _i32c(label_hw)
    H, W = label_hw.shape
    out = torch.empty(h, w, n_obj, dtype=torch.float32, device=label_hw.device)
    _lib.check(_lib.lib().aoc_label_onehot_nearest(_p(label_hw), H, W, int(h), int(w), int(n_obj), _p(out), _stream()), "aoc_label_onehot_nearest")
    return out


MAX_TTA_AUGS = 16


class _TtaDesc(ctypes.Structure):
    """aoc_tta_desc of include/aoc_hip.h."""
    _fields_ = [("n_aug", ctypes.c_int32), ("n_ch", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("unc_ratio", ctypes.c_float),
                ("h", ctypes.c_int32 * MAX_TTA_AUGS), ("w", ctypes.c_int32 * MAX_TTA_AUGS), ("flip", ctypes.c_int32 * MAX_TTA_AUGS),
                ("exist_bits", ctypes.c_uint32 * MAX_TTA_AUGS), ("scale_h", ctypes.c_float * MAX_TTA_AUGS), ("scale_w", ctypes.c_float * MAX_TTA_AUGS),
                ("plane_stride", ctypes.c_int64 * MAX_TTA_AUGS), ("logits", ctypes.c_void_p * MAX_TTA_AUGS),
                ("join_label", ctypes.c_void_p),
                ("label", ctypes.c_void_p), ("confident", ctypes.c_void_p), ("label_flipped", ctypes.c_void_p), ("confident_flipped", ctypes.c_void_p),
                ("entropy", ctypes.c_void_p), ("mean_probs", ctypes.c_void_p)]


TTA_MODES = {"reference": 0, "consistent": 1}


def tta_merge(logits_list, flips, H, W, exist_bits, join_label=None, unc_ratio=1.0, mode="reference", want_mean=False):
    """aoc_tta_merge: the per-augmentation decoder logits of one frame ([n_ch, h_a, w_a] each, those of flipped augmentations in the
    mirrored image's orientation) -> dict(label, confident, label_flipped, entropy [H, W]; + confident_flipped in mode "consistent";
    + mean_probs [n_ch, H, W] with want_mean) in ONE launch.  exist_bits: an int, or one int per augmentation (see include/aoc_hip.h)."""
    logits_list = [_f32c(l) for l in logits_list]
    _need_gpu(*logits_list, join_label)
    A = len(logits_list)
    if not 1 <= A <= MAX_TTA_AUGS:
        raise ValueError(f"tta_merge: 1 .. {MAX_TTA_AUGS} augmentations, got {A}")
    if len(flips) != A:
        raise ValueError("tta_merge: one flip flag per augmentation")
    bits = [exist_bits] * A if isinstance(exist_bits, int) else list(exist_bits)
    if len(bits) != A:
        raise ValueError("tta_merge: exist_bits is one value, or one per augmentation")
    n_ch = logits_list[0].shape[0]
    dev = logits_list[0].device
    H, W = int(H), int(W)
    d = _TtaDesc()
    d.n_aug, d.n_ch, d.H, d.W, d.mode, d.unc_ratio = A, n_ch, H, W, TTA_MODES[mode], float(unc_ratio)
    for a, l in enumerate(logits_list):
        if l.dim() != 3 or l.shape[0] != n_ch:
            raise ValueError("tta_merge: every augmentation is [n_ch, h, w] with the same n_ch")
        d.h[a], d.w[a], d.flip[a], d.exist_bits[a] = l.shape[1], l.shape[2], int(bool(flips[a])), int(bits[a]) & 0xFFFFFFFF
        d.plane_stride[a], d.logits[a] = l.shape[1] * l.shape[2], _addr(l)
    if join_label is not None:
        join_label = _i32c(join_label)
        assert join_label.shape == (H, W)
        d.join_label = _addr(join_label)
    out = {k: torch.empty(H, W, dtype=torch.int32, device=dev) for k in ("label", "confident", "label_flipped")}
    if d.mode == 1:
        out["confident_flipped"] = torch.empty(H, W, dtype=torch.int32, device=dev)
    out["entropy"] = torch.empty(H, W, dtype=torch.float32, device=dev)
    if want_mean:
        out["mean_probs"] = torch.empty(n_ch, H, W, dtype=torch.float32, device=dev)
    for k, t in out.items():
        setattr(d, k, _addr(t))
    _lib.check(_lib.lib().aoc_tta_merge(ctypes.byref(d), _stream()), "aoc_tta_merge")
    return out


class MaskJF:
    """Device-side accumulator of the DAVIS region similarity J and boundary measure F (aoc_mask_jf_accumulate): add(pred, gt) enqueues
    three small kernels and never synchronises; totals() reads the four float64 accumulators back once."""

    def __init__(self, device):
        self.accum = torch.zeros(4, dtype=torch.float64, device=device)
        self.ws = None
        self.shape = None

    def add(self, pred, gt, n_obj):
        _need_gpu(pred, gt)
        pred, gt = _i32c(pred), _i32c(gt)
        H, W = pred.shape
        assert gt.shape == (H, W)
        L = _lib.lib()
        clean = 1
        if self.shape != (H, W):
            self.ws = torch.zeros(int(L.aoc_mask_jf_workspace_bytes(H, W)), dtype=torch.uint8, device=pred.device)
            self.shape = (H, W)
        bound_pix = int(np.ceil(0.008 * np.hypot(H, W)))
        _lib.check(L.aoc_mask_jf_accumulate(_p(pred), _p(gt), H, W, int(n_obj), bound_pix, _p(self.ws), self.ws.numel(), clean, _p(self.accum), _stream()),
                   "aoc_mask_jf_accumulate")

    def totals(self):
        sj, sf, n, frames = self.accum.tolist()
        return dict(sum_j=sj, sum_f=sf, objects=n, frames=frames)


# ------------------------------------------------------------------------------------------ decoder-side streams (8f-4)
def plane_reduce(x, mode):
    """x [N, C, H, W] -> [N, C] plane sums of x (mode 0), x^2 (1) or |x| (2)."""
    x = _f32c(x)
    _need_gpu(x)
    N, C = x.shape[0], x.shape[1]
    hw = x.numel() // (N * C)
    out = torch.empty(N, C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().aoc_plane_reduce(_p(x), N * C, hw, int(mode), _p(out), _stream()), "aoc_plane_reduce")
    return out


def groupnorm_relu(x, groups, gamma, beta, eps=1e-5, residual=None, relu=True, out=None):
    """aoc_groupnorm_relu: [relu](GroupNorm(x) [+ residual]) in two streams over x (gct.py:69-90)."""
    x = _f32c(x)
    residual = _opt(residual)
    _need_gpu(x, gamma, beta, residual)
    N, C = x.shape[0], x.shape[1]
    hw = x.numel() // (N * C)
    L = _lib.lib()
    y = torch.empty_like(x) if out is None else _out("groupnorm_relu: out", out, x.shape)
    _need_gpu(out)
    ws = _ws(L.aoc_groupnorm_relu_workspace_bytes(N, int(groups)), x.device)
    # converted copies stay bound until the launch is enqueued: a temporary freed right after data_ptr() can be handed out again by the allocator
    g = _opt(gamma)
    b = _opt(beta)
    _lib.check(L.aoc_groupnorm_relu(_p(x), N, C, hw, int(groups), _p(g), _p(b),
                                    float(eps), _p(residual), int(bool(relu)), _p(y), _p(ws), ws.numel(), _stream()), "aoc_groupnorm_relu")
    return y


def groupnorm_relu_scale(x, groups, gamma, beta, eps, residual, relu, head, weight, gate_bias, out=None):
    """aoc_groupnorm_relu_scale: groupnorm_relu with the IA_gate that follows folded into its apply pass; bit-equal to
    ``film_scale(groupnorm_relu(x, groups, gamma, beta, eps, residual, relu), head, weight, gate_bias)``."""
    x, head, weight = _f32c(x), _f32c(head), _f32c(weight)
    residual = _opt(residual)
    gate_bias = _opt(gate_bias)
    N, C = x.shape[0], x.shape[1]
    if int(groups) < 1 or C % int(groups):
        raise ValueError(f"groupnorm_relu_scale: {C} channels do not divide into {groups} groups")
    _gate_shapes("groupnorm_relu_scale", N, C, head, weight, gate_bias)
    _need_gpu(x, gamma, beta, residual, head, weight, gate_bias)
    hw = x.numel() // (N * C)
    L = _lib.lib()
    y = torch.empty_like(x) if out is None else _out("groupnorm_relu_scale: out", out, x.shape)
    _need_gpu(out)
    ws = _ws(L.aoc_groupnorm_relu_workspace_bytes(N, int(groups)), x.device)
    g = _opt(gamma)              # bound until the launch is enqueued (see groupnorm_relu)
    b = _opt(beta)
    _lib.check(L.aoc_groupnorm_relu_scale(_p(x), N, C, hw, int(groups), _p(g), _p(b), float(eps), _p(residual), int(bool(relu)), _p(head), _p(weight),
                                          _p(gate_bias), head.shape[1], _p(y), _p(ws), ws.numel(), _stream()), "aoc_groupnorm_relu_scale")
    return y


def gct_gate(plane_sums, alpha, gamma, beta, eps, l1_mode=False):
    plane_sums = _f32c(plane_sums)
    _need_gpu(plane_sums, alpha, gamma, beta)
    N, C = plane_sums.shape
    gate = torch.empty(N, C, dtype=torch.float32, device=plane_sums.device)
    al, ga, be = _f32c(alpha).reshape(-1), _f32c(gamma).reshape(-1), _f32c(beta).reshape(-1)      # kept alive across the launch
    _lib.check(_lib.lib().aoc_gct_gate(_p(plane_sums), _p(al), _p(ga), _p(be), N, C,
                                       float(eps), int(bool(l1_mode)), _p(gate), _stream()), "aoc_gct_gate")
    return gate


# ------------------------------------------------------------------------------------------ ASPP (networks/layers/aspp.py)
def plane_sum_sumsq(x, want_sum=True, want_sumsq=True, want_mean=True):
    """x [N, C, H, W] -> (sum, sumsq, mean), each [N, C] or None where not wanted, from ONE pass over x (aspp.py:19 via gct.py:19, and :46)."""
    if x.dim() < 2:
        raise ValueError(f"plane_sum_sumsq: x {tuple(x.shape)} has no [N, C] planes")
    if not (want_sum or want_sumsq or want_mean):
        raise ValueError("plane_sum_sumsq: no output wanted")
    x = _f32c(x)
    _need_gpu(x)
    N, C = x.shape[0], x.shape[1]
    hw = x.numel() // (N * C)
    new = lambda want: torch.empty(N, C, dtype=torch.float32, device=x.device) if want else None
    s, q, m = new(want_sum), new(want_sumsq), new(want_mean)
    _lib.check(_lib.lib().aoc_plane_sum_sumsq(_p(x), N * C, hw, _p(s), _p(q), _p(m), _stream()), "aoc_plane_sum_sumsq")
    return s, q, m


def _gct_rows(what, params, C):
    """A list of per-set parameters ([1, C, 1, 1] or [C]) or one [n_sets, C] tensor -> a contiguous float32 [n_sets, C]."""
    rows = params if torch.is_tensor(params) else torch.stack([p.reshape(-1) for p in params])
    if rows.dim() != 2 or rows.shape[1] != C:
        raise ValueError(f"{what}: parameters {tuple(rows.shape)} do not fit {C} channels")
    return _f32c(rows)


def gct_gate_multi(plane_sums, alpha, gamma, beta, eps, l1_mode=False):
    """aoc_gct_gate_multi: the gates of several GCTs that read the same tensor.  alpha, gamma, beta: [n_sets, C] tensors or lists of n_sets
    per-GCT parameters; returns gate [n_sets, N, C], set k bit-equal to ``gct_gate(plane_sums, alpha[k], gamma[k], beta[k], eps, l1_mode)``."""
    if plane_sums.dim() != 2:
        raise ValueError(f"gct_gate_multi: plane sums {tuple(plane_sums.shape)} are not [N, C]")
    N, C = plane_sums.shape
    al, ga, be = (_gct_rows("gct_gate_multi", p, C) for p in (alpha, gamma, beta))          # bound until the launch is enqueued
    if not (al.shape[0] == ga.shape[0] == be.shape[0]) or al.shape[0] < 1:
        raise ValueError(f"gct_gate_multi: {al.shape[0]} alpha, {ga.shape[0]} gamma and {be.shape[0]} beta sets")
    plane_sums = _f32c(plane_sums)
    _need_gpu(plane_sums, al, ga, be)
    n_sets = al.shape[0]
    gate = torch.empty(n_sets, N, C, dtype=torch.float32, device=plane_sums.device)
    _lib.check(_lib.lib().aoc_gct_gate_multi(_p(plane_sums), _p(al), _p(ga), _p(be), n_sets, N, C, float(eps), int(bool(l1_mode)), _p(gate), _stream()),
               "aoc_gct_gate_multi")
    return gate


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[_addr(t) for t in tensors])


def channel_scale_multi(x, gains, outs=None):
    """aoc_channel_scale_multi: [gains[k][:, :, None, None] * x for k] with x read once.  gains [n_out, N, C] (n_out <= 8); outs: optional list
    of n_out contiguous float32 tensors shaped like x (outs[0] may be x itself when n_out == 1).  Each result is bit-equal to channel_scale."""
    if x.dim() < 2 or gains.dim() != 3 or tuple(gains.shape[1:]) != tuple(x.shape[:2]):
        raise ValueError(f"channel_scale_multi: gains {tuple(gains.shape)} do not fit x {tuple(x.shape)}")
    n_out = gains.shape[0]
    if not 1 <= n_out <= 8:
        raise ValueError(f"channel_scale_multi: {n_out} outputs (1 to 8)")
    if outs is not None and (len(outs) != n_out or any(tuple(o.shape) != tuple(x.shape) or o.dtype != torch.float32 or not o.is_contiguous() for o in outs)):
        raise ValueError(f"channel_scale_multi: outs must be {n_out} contiguous float32 tensors of shape {tuple(x.shape)}")
    x, gains = _f32c(x), _f32c(gains)
    _need_gpu(x, gains, *(outs or ()))
    planes = x.shape[0] * x.shape[1]
    hw = x.numel() // planes
    ys = [torch.empty_like(x) for _ in range(n_out)] if outs is None else list(outs)
    _lib.check(_lib.lib().aoc_channel_scale_multi(_p(x), _p(gains), n_out, planes, hw, _ptr_array(ys), _stream()), "aoc_channel_scale_multi")
    return ys


def groupnorm_cat_relu(xs, groups, gamma, beta, eps=1e-5, tail=None, relu=True, want_plane_sumsq=False, out=None):
    """aoc_groupnorm_cat_relu: ``torch.cat([groupnorm_relu(x_k, groups, gamma[k], beta[k], eps, None, relu) for k] + [tail expanded], 1)`` (bit-equal)
    in a statistics launch and an apply launch (aspp.py:21-23 x 4, :62-63).  xs: 1 to 8 tensors [N, C_src, H, W]; gamma, beta: [n_src, C_src],
    lists of n_src [C_src] tensors, or None; tail [N, C_tail] or [N, C_tail, 1, 1] (relu applies to it too) or None.  With want_plane_sumsq
    also returns the plane sums of squares [N, C_total] of the result (what GCT's l2 mode reads it for)."""
    xs = list(xs)
    n_src = len(xs)
    if not 1 <= n_src <= 8:
        raise ValueError(f"groupnorm_cat_relu: {n_src} sources (1 to 8)")
    if any(x.dim() < 2 or tuple(x.shape) != tuple(xs[0].shape) for x in xs):
        raise ValueError(f"groupnorm_cat_relu: the sources differ in shape: {[tuple(x.shape) for x in xs]}")
    N, C = xs[0].shape[0], xs[0].shape[1]
    if int(groups) < 1 or C % int(groups):
        raise ValueError(f"groupnorm_cat_relu: {C} channels do not divide into {groups} groups")
    g = b = None
    if gamma is not None:
        g = _gct_rows("groupnorm_cat_relu", gamma, C)                   # converted copies stay bound until the launch is enqueued
    if beta is not None:
        b = _gct_rows("groupnorm_cat_relu", beta, C)
    if any(t is not None and t.shape[0] != n_src for t in (g, b)):
        raise ValueError(f"groupnorm_cat_relu: {n_src} sources, affine parameters for {[t.shape[0] for t in (g, b) if t is not None]}")
    C_tail = 0
    if tail is not None:
        if tail.dim() < 2 or tail.shape[0] != N or tail.numel() != N * tail.shape[1]:
            raise ValueError(f"groupnorm_cat_relu: the tail {tuple(tail.shape)} is not [N = {N}, C_tail] (or [N, C_tail, 1, 1])")
        C_tail = tail.shape[1]
        tail = _f32c(tail)
    xs = [_f32c(x) for x in xs]
    shape = (N, n_src * C + C_tail) + tuple(xs[0].shape[2:])
    if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError(f"groupnorm_cat_relu: out must be a contiguous float32 tensor of shape {shape}")
    _need_gpu(*xs, g, b, tail, out)
    hw = xs[0].numel() // (N * C)
    L = _lib.lib()
    y = torch.empty(shape, dtype=torch.float32, device=xs[0].device) if out is None else out
    sq = torch.empty(N, shape[1], dtype=torch.float32, device=y.device) if want_plane_sumsq else None
    ws = _ws(L.aoc_groupnorm_cat_relu_workspace_bytes(n_src, N, int(groups)), y.device)
    _lib.check(L.aoc_groupnorm_cat_relu(_ptr_array(xs), n_src, N, C, hw, int(groups), _p(g), _p(b), float(eps), _p(tail), C_tail, int(bool(relu)),
                                        _p(y), _p(sq), _p(ws), ws.numel(), _stream()), "aoc_groupnorm_cat_relu")
    return (y, sq) if want_plane_sumsq else y


def object_logit(x, weight_bias):
    """x [N, C, H, W], weight_bias [N, C + 1] (weights then bias, decoding_module.py:154-156) -> [N, 1, H, W]."""
    x = _f32c(x)
    weight_bias = _f32c(weight_bias)
    _need_gpu(x, weight_bias)
    N, C, H, W = x.shape
    assert weight_bias.shape == (N, C + 1)
    out = torch.empty(N, 1, H, W, dtype=torch.float32, device=x.device)
    base = _addr(weight_bias)
    _lib.check(_lib.lib().aoc_object_logit(_p(x), N, C, H * W, ctypes.c_void_p(base), C + 1, ctypes.c_void_p(base + 4 * C), C + 1, _p(out), _stream()),
               "aoc_object_logit")
    return out


# ------------------------------------------------------------------------------------------ the decoder's tail (csrc/decoder_tail.hip)
def bicubic_plane_mean(x, size):
    """x [N, C, h, w] -> [N, C]: the mean over the map of F.interpolate(x, size, mode='bicubic', align_corners=True), from x alone."""
    x = _f32c(x)
    _need_gpu(x)
    N, C, h, w = x.shape
    H, W = (int(v) for v in size)
    out = torch.empty(N, C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().aoc_bicubic_plane_mean(_p(x), N * C, h, w, H, W, _p(out), _stream()), "aoc_bicubic_plane_mean")
    return out


def bicubic_cat_scale(x, low=None, gain=None, size=None, out=None):
    """gain[:, :, None, None] * torch.cat([F.interpolate(x, size, mode='bicubic', align_corners=True), low], 1) in one call
    (decoding_module.py:163, :170 and the scaling of ATT:15-16).  x [N, Ce, h, w]; low [N, Cr, H, W] or None (size gives H, W then);
    gain [N, Ce + Cr] or None (= 1)."""
    x = _f32c(x)
    low = _opt(low)
    gain = _opt(gain)
    _need_gpu(x, low, gain)
    N, Ce, h, w = x.shape
    Cr = low.shape[1] if low is not None else 0
    H, W = (int(v) for v in (low.shape[2:] if size is None else size))
    if low is not None and tuple(low.shape) != (N, Cr, H, W):
        raise _lib.AocHipError(f"aoc_bicubic_cat_scale: low must be [{N}, Cr, {H}, {W}], got {tuple(low.shape)}")
    if gain is not None and tuple(gain.shape) != (N, Ce + Cr):
        raise _lib.AocHipError(f"aoc_bicubic_cat_scale: gain must be [{N}, {Ce + Cr}], got {tuple(gain.shape)}")
    y = torch.empty(N, Ce + Cr, H, W, dtype=torch.float32, device=x.device) if out is None else _out("bicubic_cat_scale: out", out, (N, Ce + Cr, H, W))
    _need_gpu(out)
    _lib.check(_lib.lib().aoc_bicubic_cat_scale(_p(x), _p(low), _p(gain), N, Ce, Cr, h, w, H, W, _p(y), _stream()), "aoc_bicubic_cat_scale")
    return y


def shortcut_stage(x, low, IA_head, weight, bias, want_debug=False, out=None):
    """decoding_module.py:163 and :170-176 in one C call: IA10(cat([bicubic(x), low], 1), cat([IA_head, px1_delta], 1)) with IA10's
    Linear given as weight [Ce + Cr, D + Ce + Cr], bias.  x [N, Ce, h, w], low [N, Cr, H, W] (the shortcut branch after its ReLU),
    IA_head [N, D].  want_debug: also the plane means and the gain, both [N, Ce + Cr]."""
    x, low, IA_head, weight = _f32c(x), _f32c(low), _f32c(IA_head), _f32c(weight)
    bias = _opt(bias)
    _need_gpu(x, low, IA_head, weight, bias)
    N, Ce, h, w = x.shape
    Cr, H, W = low.shape[1:]
    D = IA_head.shape[1]
    want = ((N, Cr, H, W), (N, D), (Ce + Cr, D + Ce + Cr))
    have = tuple(tuple(t.shape) for t in (low, IA_head, weight))
    if have != want or (bias is not None and tuple(bias.shape) != (Ce + Cr,)):
        raise _lib.AocHipError(f"aoc_shortcut_stage_enqueue: low, IA_head, weight must have shapes {want} and bias [{Ce + Cr}], got {have}")
    L = _lib.lib()
    y = torch.empty(N, Ce + Cr, H, W, dtype=torch.float32, device=x.device) if out is None else _out("shortcut_stage: out", out, (N, Ce + Cr, H, W))
    _need_gpu(out)
    pm = torch.empty(N, Ce + Cr, dtype=torch.float32, device=x.device) if want_debug else None
    gain = torch.empty(N, Ce + Cr, dtype=torch.float32, device=x.device) if want_debug else None
    ws = _ws(L.aoc_shortcut_stage_workspace_bytes(N, Ce, Cr, D), x.device)
    _lib.check(L.aoc_shortcut_stage_enqueue(_p(x), _p(low), _p(IA_head), _p(weight), _p(bias), N, Ce, Cr, D, h, w, H, W, _p(y), _p(pm), _p(gain),
                                            _p(ws), ws.numel(), _stream()), "aoc_shortcut_stage_enqueue")
    return (y, pm, gain) if want_debug else y


def logit_head(x, wb_fg, wb_bg):
    """decoding_module.py:144-147 in one launch.  x [N, C, H, W]; wb_fg, wb_bg [N, C + 1] (the two IA_final outputs: weights then bias)
    -> pred [1, N, H, W] = fg logits, object 0's plus the min over the other objects' bg logits."""
    x, wb_fg, wb_bg = _f32c(x), _f32c(wb_fg), _f32c(wb_bg)
    _need_gpu(x, wb_fg, wb_bg)
    N, C, H, W = x.shape
    assert wb_fg.shape == (N, C + 1) and wb_bg.shape == (N, C + 1)
    pred = torch.empty(1, N, H, W, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().aoc_logit_head(_p(x), _p(wb_fg), _p(wb_bg), C + 1, N, C, H * W, _p(pred), _stream()), "aoc_logit_head")
    return pred


def background_merge(fg_logit, bg_logit):
    """augment_background_logit (decoding_module.py:213-225): fg_logit, bg_logit [N, 1, H, W] -> pred [1, N, H, W]."""
    fg, bg = _f32c(fg_logit), _f32c(bg_logit)
    _need_gpu(fg, bg)
    N, _, H, W = fg.shape
    assert fg.shape[1] == 1 and bg.shape == fg.shape
    pred = torch.empty(1, N, H, W, dtype=torch.float32, device=fg.device)
    _lib.check(_lib.lib().aoc_background_merge(_p(fg), _p(bg), N, H * W, _p(pred), _stream()), "aoc_background_merge")
    return pred


def cond_codes(gap, plane_means, head, w1, b1, w2, b2, w3, b3):
    """aoc_cond_codes: the three conditioning codes of CLB:68-80 concatenated -> [N, 2C + D]."""
    gap, plane_means, head = _f32c(gap), _f32c(plane_means), _f32c(head)
    _need_gpu(gap, plane_means, head, w1, w2, w3)
    N, C = gap.shape
    D = head.shape[1]
    # the library reads W1, W2 as [C, C] and W3 as [D, D] from bare pointers: a smaller tensor would be read past its end
    want = ((N, C), (N, D), (C, C), (C,), (C, C), (C,), (D, D), (D,))
    have = tuple(tuple(t.shape) for t in (plane_means, head, w1, b1, w2, b2, w3, b3))
    if have != want:
        raise _lib.AocHipError(f"aoc_cond_codes: plane_means, head, w1, b1, w2, b2, w3, b3 must have shapes {want}, got {have}")
    code = torch.empty(N, 2 * C + D, dtype=torch.float32, device=gap.device)
    # converted copies stay bound until the launch is enqueued (see groupnorm_relu): taken inline, each copy died as soon as its address was
    # read and the next conversion was handed the same block
    w1, b1, w2, b2, w3, b3 = _f32c(w1), _f32c(b1), _f32c(w2), _f32c(b2), _f32c(w3), _f32c(b3)
    _lib.check(_lib.lib().aoc_cond_codes(_p(gap), _p(plane_means), _p(head), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3),
                                         _p(b3), N, C, D, _p(code), _stream()), "aoc_cond_codes")
    return code


def prehead(feat, weight, bias, n_groups, gamma, beta, eps, emb_hwc=None):
    """aoc_prehead: feat [O, n_in, h, w] -> [O, C + n_out, h, w] = (embedding expanded over the objects || ReLU(GN(conv1x1(feat))))."""
    feat = _f32c(feat)
    _need_gpu(feat, weight, bias, gamma, beta, emb_hwc)
    O, n_in, h, w = feat.shape
    weight = _f32c(weight).reshape(weight.shape[0], -1)
    n_out = weight.shape[0]
    assert weight.shape[1] == n_in, "DynamicPreHead runs with kernel_size = 1"
    C = 0
    if emb_hwc is not None:
        emb_hwc = _f32c(emb_hwc)
        C = emb_hwc.shape[-1]
    L = _lib.lib()
    out = torch.empty(O, C + n_out, h, w, dtype=torch.float32, device=feat.device)
    ws = _ws(L.aoc_prehead_workspace_bytes(O, n_out, n_out // n_groups, h * w), feat.device)
    bi, g, b = _f32c(bias), _f32c(gamma), _f32c(beta)            # kept alive across the launch (see groupnorm_relu)
    _lib.check(L.aoc_prehead(_p(feat), O, n_in, h * w, _p(weight), _p(bi), n_out, int(n_groups), _p(g), _p(b), float(eps),
                             _p(emb_hwc), C, _p(out), _p(ws), ws.numel(), _stream()), "aoc_prehead")
    return out
