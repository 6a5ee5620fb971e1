"""The pointer-alignment contract of the matching and k-means entries of libaoc_hip.so, as data (include/aoc_hip.h, "Pointer alignment").

CLASS[entry][parameter] is 16 or 4:
  16  some device or host access through the pointer uses a type wider than 4 bytes that is not declared aligned(4) (float4 / uint4 / a
      16-byte buffer load), or an inline-asm / LDS-direct load; the opaque records of aoc_split_rows count too.  The entry returns
      AOC_ERR_INVALID_ARG for such a pointer off the 16-byte grid before it enqueues or writes anything; aoc_amd.ops copies such an input
      and raises ValueError for such a caller-provided output.
   4  everything else: 4-byte accesses only.  May sit at any float boundary (channel slices at odd hw, out_step destinations, counts[n_obj:]).
WHY[(entry, parameter)] names, for every class-16 pointer, the source line that decides it (csrc/<file>:<line> of the tree this table was
read from; the line moves with the file, the access it names does not).

HOST lists the parameters that are HOST pointers (arrays and descriptors the entry reads before it returns).  They are class 4 in the
table: the contract is about device addresses; a host array is read by compiled C with the natural alignment of its element type (8 bytes
for int64_t and for structures that hold pointers), which every C caller, numpy and ctypes give.

DESCRIPTORS maps a descriptor parameter to the structure whose pointer fields it carries; the fields are classed under the structure's name.

Shared by tests/test_alignment_host.py (CPU: the prototypes of the header against this table, aoc_amd.ops under a stub library) and
tests/test_gpu_alignment.py."""
import re

_KM = {"pool": 16, "rows": 4, "seg_offsets": 4, "seg_k": 4, "init_rows": 4, "centroids": 16, "labels": 4, "cluster_counts": 4, "workspace": 16}
_CORR = {"query": 4, "proxies": 16, "proxy_sqnorm": 4, "set_begin_host": 4, "set_size_host": 4, "set_out_offset_host": 4, "set_bias": 4, "out": 4}
_CORR_B = {"frames_host": 4, "set_begin_host": 4, "set_size_host": 4, "set_out_offset_host": 4, "workspace": 4}
_DENSE = {"query": 4, "pool": 16, "fg_rows": 4, "n_fg": 4, "wrong_bits": 4, "obj_bias": 4, "out": 4, "workspace": 4}
_SPLIT_ROWS = {"x": 16, "records": 16, "sqnorm": 4, "overflow_flag": 4}
_DENSE_SPLIT = {"query": 16, "query_rec": 16, "query_sqnorm": 4, "pool": 16, "pool_rec": 16, "overflow_flag": 4, "right_bits": 4, "wrong_bits": 4,
                "fg_rows": 4, "obj_rows": 4, "counts": 4, "obj_offsets": 4, "obj_bias": 4, "out": 4, "workspace": 16}
_LOCAL = {"query": 16, "prev": 16, "right_bits": 4, "radii_host": 4, "obj_bias": 4, "out": 4}
_RESIZE = {"in": 4, "out": 4}

CLASS = {
    "aoc_label_prep": {"labels": 4, "right_bits": 4, "wrong_bits": 4, "fg_rows": 4, "obj_rows": 4, "counts": 4, "obj_offsets": 4, "workspace": 4},
    "aoc_label_bits": {"labels": 4, "right_bits": 4, "wrong_bits": 4},
    "aoc_kmeans_segmented": _KM, "aoc_kmeans_segmented_ex": _KM, "aoc_kmeans_segmented_rep": _KM,
    "aoc_kmeans_replicate": {"rows": 4, "seg_offsets": 4, "seg_k": 4, "rows_out": 4, "seg_offsets_out": 4, "seg_k_out": 4},
    "aoc_kmeans_replicate_levels": {"rows": 4, "seg_offsets": 4, "levels_host": 4, "rows_out": 4, "seg_offsets_out": 4, "seg_k_out": 4},
    "aoc_build_proxies": {"pool": 16, "fg_rows": 4, "seg_offsets": 4, "seg_k": 4, "labels": 4, "centroids": 4, "proxies": 4, "proxy_sqnorm": 4, "workspace": 16},
    "aoc_proxy_corr_min": _CORR, "aoc_proxy_corr_min_f16": _CORR,
    "aoc_proxy_corr_min_batched": _CORR_B,
    "aoc_corr_frame": {"query": 16, "proxies": 16, "proxy_sqnorm": 4, "set_bias": 4, "out": 4},
    "aoc_proxy_corr_min_records": _CORR_B,
    "aoc_proxy_corr_min_records_cached": dict(_CORR_B, workspace=16, tables_key=4),
    "aoc_corr_frame_rec": {"query": 4, "query_rec": 16, "query_sqnorm": 4, "proxies": 16, "proxy_sqnorm": 4, "set_bias": 4, "out": 4},
    "aoc_dense_match_min": _DENSE, "aoc_dense_match_min_f16": _DENSE, "aoc_dense_match_argmin": dict(_DENSE, arg=4),
    "aoc_split_rows": _SPLIT_ROWS, "aoc_split_rows_tiled": _SPLIT_ROWS,
    "aoc_dense_match_min_split": _DENSE_SPLIT, "aoc_dense_match_min_split_cached": _DENSE_SPLIT,
    "aoc_dense_match_grad": {"grad_out": 4, "T": 4, "arg": 4, "query": 4, "pool": 4, "grad_query": 4, "grad_pool": 4, "grad_bias": 4, "workspace": 4},
    "aoc_proxy_match_grad": {"grad_out": 4, "T": 4, "query": 4, "proxies": 4, "grad_query": 4, "grad_proxies": 4, "grad_bias": 4, "workspace": 4},
    "aoc_local_window_match": _LOCAL, "aoc_local_window_match_ex": _LOCAL,
    "aoc_local_window_match_pair": {"query": 16, "prev_a": 16, "prev_b": 16, "right_bits": 4, "radii_host": 4, "obj_bias": 4, "out_a": 4, "out_b": 4},
    "aoc_local_window_match_argmin": dict(_LOCAL, arg=4),
    "aoc_local_match_grad": {"grad_out": 4, "T": 4, "arg": 4, "query": 4, "prev": 4, "grad_query": 4, "grad_prev": 4, "grad_bias": 4, "workspace": 4},
    "aoc_local_prep": {"cur_emb": 4, "prev_emb": 4, "prev_labels": 4, "prev_pos": 4, "q2": 4, "p2": 4, "pm2": 4, "bits2": 4, "obj_bias": 4,
                       "set_bias_out": 4, "copy_src_a": 4, "copy_dst_a": 4, "copy_src_b": 4, "copy_dst_b": 4},
    "aoc_resize_bilinear_hwc": _RESIZE, "aoc_resize_bilinear_hwc_ex": _RESIZE, "aoc_resize_nearest_bits": _RESIZE,
    "aoc_atrous_subsample": {"in": 16, "out": 16},
    "aoc_proxy_set_match_argmin": dict(_CORR, proxies=4, arg=4),
    "aoc_proxy_set_match_grad": {"grad_out": 4, "T": 4, "arg": 4, "query": 4, "proxies": 4, "set_begin_host": 4, "set_size_host": 4,
                                 "set_out_offset_host": 4, "set_bias_index_host": 4, "grad_query": 4, "grad_proxies": 4, "grad_bias": 4, "workspace": 4},
    "aoc_centroid_avg_grad": {"grad_proxies": 4, "fg_rows": 4, "n_fg": 4, "seg_offsets": 4, "seg_k": 4, "labels": 4, "grad_pool": 4, "workspace": 4},
    "aoc_proto_finish": {"feat": 4, "prev_labels": 4, "ref_pos": 4, "ref_neg": 4, "prev_pos": 4, "prev_neg": 4, "head": 4},
    "aoc_fg2bg_min": {"dis": 4, "out": 4},
    "aoc_frame_enqueue": {"desc": 4, "state": 4, "workspace": 16},
    "aoc_frame_desc": {"ref_emb": 16, "ref_labels": 4, "match_emb": 16, "prev_emb": 16, "prev_labels": 4, "cur_emb": 16, "dis_bias": 4, "right_bits": 4,
                       "wrong_bits": 4, "fg_rows": 4, "obj_rows": 4, "counts": 4, "obj_offsets": 4, "proxy_table": 16, "proxy_sqnorm": 4, "feat": 4, "head": 4},
    "aoc_cluster_chain_enqueue": {"desc": 4, "workspace": 16},
    "aoc_chain_desc": {"pool": 16, "fg_rows": 4, "obj_rows": 4, "obj_offsets": 4, "init_rows": 4, "tables": 16, "sqnorms": 4},
}

# entries whose class-16 check is conditional, with the condition (the library enforces the class only then)
CONDITIONAL = {"aoc_atrous_subsample": "X % 4 == 0: the kernel moves 16 bytes per thread then, 4 bytes for every other X",
               "aoc_proxy_corr_min_records_cached": "workspace: tables_key != NULL (only then does the workspace hold the tile tables; with a NULL key the "
                                                    "call is aoc_proxy_corr_min_records, whose workspace is class 4)"}

HOST = {"set_begin_host", "set_size_host", "set_out_offset_host", "set_bias_index_host", "levels_host", "radii_host", "frames_host", "tables_key",
        "desc", "state"}
DESCRIPTORS = {("aoc_proxy_corr_min_batched", "frames_host"): "aoc_corr_frame", ("aoc_proxy_corr_min_records", "frames_host"): "aoc_corr_frame_rec",
               ("aoc_proxy_corr_min_records_cached", "frames_host"): "aoc_corr_frame_rec", ("aoc_frame_enqueue", "desc"): "aoc_frame_desc",
               ("aoc_cluster_chain_enqueue", "desc"): "aoc_chain_desc"}
STRUCTS = ("aoc_corr_frame", "aoc_corr_frame_rec", "aoc_frame_desc", "aoc_chain_desc")
# members of the descriptors that are no data pointers: HIP event handles
NOT_DATA = {"aoc_frame_desc": {"prep_ready", "proxies_ready", "probe"}}

_KMW = "the entry's workspace holds float4 chunk sums (labels_kmeans.hip:1380) and the member lists its LDS-direct loads read (labels_kmeans.hip:2270)"
_POOL_KM = ("float4 row loads labels_kmeans.hip:212, 581, 650, 761, 979, 1365, 1587, 1697; 16-byte buffer loads :1891; the LDS-direct "
            "global_load_lds_dwordx4 of the sum tail and the ordered mean :2158 / :2279")
_PROXIES = "correlation.hip:55 (stage_tile_rows: float4 loads of every proxy row)"
_POOL_DENSE = "correlation.hip:440 (dense_match_partial_kernel issue_rows: float4 loads of the pool rows)"
WHY = {}
for _e in ("aoc_kmeans_segmented", "aoc_kmeans_segmented_ex", "aoc_kmeans_segmented_rep"):
    WHY[(_e, "pool")] = _POOL_KM
    WHY[(_e, "centroids")] = "labels_kmeans.hip:787, 1009 (the matrix-pipe assignment kernels stage the code book with float4 loads)"
    WHY[(_e, "workspace")] = _KMW
WHY[("aoc_build_proxies", "pool")] = _POOL_KM
WHY[("aoc_build_proxies", "workspace")] = _KMW
for _e in ("aoc_proxy_corr_min", "aoc_proxy_corr_min_f16"):
    WHY[(_e, "proxies")] = _PROXIES
WHY[("aoc_corr_frame", "query")] = "correlation_batched.hip:481, 487 (u32x4 view of the fp32 query streamed by LDS-direct global_load_lds_dwordx4, :141)"
WHY[("aoc_corr_frame", "proxies")] = "correlation_batched.hip:190, 237 (float4 loads in cb_stage_frame) and, in the exact-fp32 take-over, " + _PROXIES
WHY[("aoc_corr_frame_rec", "query_rec")] = "correlation_batched.hip:633 (u32x4 loads of the tile-major records); opaque records of aoc_split_rows_tiled"
WHY[("aoc_corr_frame_rec", "proxies")] = WHY[("aoc_corr_frame", "proxies")]
WHY[("aoc_proxy_corr_min_records_cached", "workspace")] = ("correlation_batched.hip:733 (AocCorrTiles tables with int64_t members at workspace + 256, read as "
                                                           "structures by proxy_corr_records_multi_kernel)")
for _e in ("aoc_dense_match_min", "aoc_dense_match_min_f16", "aoc_dense_match_argmin"):
    WHY[(_e, "pool")] = _POOL_DENSE
for _e in ("aoc_split_rows", "aoc_split_rows_tiled"):
    WHY[(_e, "x")] = "dense_split.hip:76, 97 (float4 loads of the row)"
    WHY[(_e, "records")] = "dense_split.hip:132-142 (uint4 stores); the opaque records themselves"
for _e in ("aoc_dense_match_min_split", "aoc_dense_match_min_split_cached"):
    WHY[(_e, "query")] = "dense_split.hip:639 (dense_seed_kernel: float4 loads of the query row)"
    WHY[(_e, "query_rec")] = "dense_split.hip:366-370 (uint4 loads); opaque records"
    WHY[(_e, "pool")] = "dense_split.hip:647 (dense_seed_kernel) and, in the take-over, " + _POOL_DENSE
    WHY[(_e, "pool_rec")] = "dense_split.hip:165-166 (uint4 load in split_plan_kernel), :426 (LDS-direct global_load_lds_dwordx4, :239); opaque records"
    WHY[(_e, "workspace")] = "dense_split.hip:414 (LDS-direct 16-byte loads of the tile row lists the plan leaves in the workspace)"
for _e in ("aoc_local_window_match", "aoc_local_window_match_ex"):
    WHY[(_e, "query")] = "local_match.hip:219 via :249 (register-operand kernel, C = 100 / 128: float4 pieces of the query row)"
    WHY[(_e, "prev")] = "local_match.hip:81 (LDS-image kernel) and :219 via :275 (register-operand kernel): float4 loads of the candidate rows"
WHY[("aoc_local_window_match_pair", "query")] = WHY[("aoc_local_window_match", "query")]
WHY[("aoc_local_window_match_pair", "prev_a")] = WHY[("aoc_local_window_match", "prev")]
WHY[("aoc_local_window_match_pair", "prev_b")] = WHY[("aoc_local_window_match", "prev")]
WHY[("aoc_local_window_match_argmin", "query")] = "local_grad.hip:92 via :119 (float4 pieces of the query row, C = 100 / 128)"
WHY[("aoc_local_window_match_argmin", "prev")] = "local_grad.hip:92 via :141 and :229 (float4 loads of the candidate rows in both kernels)"
WHY[("aoc_atrous_subsample", "in")] = "local_match.hip:435 (float4 moves when X % 4 == 0)"
WHY[("aoc_atrous_subsample", "out")] = "local_match.hip:435 (float4 moves when X % 4 == 0)"
WHY[("aoc_frame_enqueue", "workspace")] = "frame.hip:128 (frame_carve: the records, the dense and correlation workspaces and the half-resolution maps handed to the entries below)"
WHY[("aoc_frame_desc", "ref_emb")] = "frame.hip:184, 195 (aoc_split_rows x, aoc_dense_match_min_split_cached pool when match_hw == 0)"
WHY[("aoc_frame_desc", "match_emb")] = "frame.hip:184, 195 (aoc_split_rows x, aoc_dense_match_min_split_cached pool when match_hw > 0)"
WHY[("aoc_frame_desc", "prev_emb")] = "frame.hip:240 (aoc_local_window_match_ex prev without the down-sample)"
WHY[("aoc_frame_desc", "cur_emb")] = "frame.hip:187, 195, 240 (aoc_split_rows_tiled x, dense query, local query)"
WHY[("aoc_frame_desc", "proxy_table")] = "frame.hip:273 (proxies of aoc_proxy_corr_min_f16), :280 / :290 (fr.proxies of the records and batched calls)"
WHY[("aoc_cluster_chain_enqueue", "workspace")] = "frame.hip:379 (chain_carve: code book, k-means and proxy-build workspaces; :357 float4 reads of the proxies it holds)"
WHY[("aoc_chain_desc", "pool")] = "frame.hip:387, 390 (pool of aoc_kmeans_segmented_rep and aoc_build_proxies)"
WHY[("aoc_chain_desc", "tables")] = "frame.hip:357 (chain_scatter_kernel: float4 stores)"


def covered_entries():
    return sorted(e for e in CLASS if e not in STRUCTS)


# ------------------------------------------------------------------------------------------ the header's side
def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def prototype_pointers(header_text):
    """{entry: [pointer parameter names, in order]} for every `int aoc_*(...)` prototype of the header."""
    text = _strip_comments(header_text)
    out = {}
    for m in re.finditer(r"\bint\s+(aoc_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        names = []
        for prm in m.group(2).split(","):
            prm = " ".join(prm.split())
            if "*" in prm:
                names.append(re.search(r"(\w+)\s*(\[\d*\])?$", prm).group(1))
        out[m.group(1)] = names
    return out


def prototype_params(header_text):
    """{entry: [(parameter name, is_pointer), in order]} -- the position of every argument of a call."""
    text = _strip_comments(header_text)
    out = {}
    for m in re.finditer(r"\bint\s+(aoc_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        prms = []
        for prm in m.group(2).split(","):
            prm = " ".join(prm.split())
            if prm in ("", "void"):
                continue
            prms.append((re.search(r"(\w+)\s*(\[\d*\])?$", prm).group(1), "*" in prm or prm.startswith("aoc_stream_t")))
        out[m.group(1)] = prms
    return out


def struct_pointers(header_text, name):
    """Pointer members of `typedef struct <name> { ... } <name>;` (arrays of pointers included), in order."""
    text = _strip_comments(header_text)
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        if "*" not in decl:
            continue
        for piece in decl.split(","):
            m = re.search(r"\*\s*(\w+)\s*(\[\d+\])?\s*$", piece.strip())
            if m:
                names.append(m.group(1))
    return names


# ------------------------------------------------------------------------------------------ tensors off the 16-byte grid
OFFSETS = (4, 8, 12)


def off_grid(t, k, fill=None):
    """Equal values `k` bytes off the 16-byte grid: buf[lo : lo + n].view(shape) inside a buffer whose own base is asserted to be on the grid,
    with at least 16 bytes of margin on either side (filled with `fill` when given: NaN / a sentinel the device tests look for afterwards).
    -> (view, buf, lo)."""
    import torch
    isz = t.element_size()
    assert k % isz == 0 and 0 < k < 16
    pad = 16 // isz
    lo = pad + k // isz
    buf = torch.empty(t.numel() + 3 * pad, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0, "the allocator's grid: the base of a fresh buffer is 16-byte aligned"
    if fill is not None:
        buf.fill_(fill)
    v = buf[lo:lo + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == k
    return v, buf, lo


def margins_intact(buf, lo, n, fill):
    """The bytes around an off_grid view still hold `fill` (NaN compares through isnan)."""
    import torch
    edge = torch.cat([buf[:lo], buf[lo + n:]])
    if isinstance(fill, float) and fill != fill:
        return bool(torch.isnan(edge).all())
    return bool((edge == fill).all())


# ------------------------------------------------------------------------------------------ aoc_amd.ops against the table (shared by both test modules)
import ctypes
import functools
import os

import pytest
import torch

import ops_contract_cases as occ
from aoc_amd import _lib, ops

ERRORS = occ.ERRORS + (_lib.AocHipError,)
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aoc_hip.h")).read()
PARAMS = prototype_params(HEADER)
# a registry role that the alignment rule reads differently, with the reason
ROLE = {("FrameCall", "table"): occ.OUT}        # aoc_frame_enqueue WRITES the k = 1 rows into the proxy table it also reads: never copied


def _address(x):
    if x is None or isinstance(x, int):
        return x
    if isinstance(x, ctypes.c_void_p):
        return x.value
    if hasattr(x, "_obj"):                          # ctypes.byref(...)
        return ctypes.addressof(x._obj)
    try:
        return ctypes.addressof(x)
    except TypeError:
        return None


_STRUCT_OF = {"aoc_corr_frame": "_CorrFrame", "aoc_corr_frame_rec": "_CorrFrameRec", "aoc_frame_desc": "_FrameDesc", "aoc_chain_desc": "_ChainDesc"}


class DecodingStub(occ.StubLib):
    """occ.StubLib that also notes, for every covered entry it is called with, (entry or descriptor, parameter, address) of every pointer
    argument in prototype order, the descriptors' members behind their own."""

    def __init__(self, recorder):
        super().__init__(recorder)
        self.seen = []

    def __getattr__(self, name):
        inner = super().__getattr__(name)
        if name not in CLASS:
            return inner

        def call(*a):
            prms = [(p, is_ptr) for p, is_ptr in PARAMS[name]]
            assert len(a) == len(prms), f"{name}: {len(a)} arguments for {len(prms)} parameters"
            for i, (p, is_ptr) in enumerate(prms):
                if not is_ptr or p == "stream":
                    continue
                addr = _address(a[i])
                self.seen.append((name, p, addr))
                struct = DESCRIPTORS.get((name, p))
                if struct and addr:
                    cls = getattr(ops, _STRUCT_OF[struct])
                    count = a[1] if p == "frames_host" else 1
                    arr = ctypes.cast(addr, ctypes.POINTER(cls))
                    for f in range(count):
                        for member in CLASS[struct]:
                            v = getattr(arr[f], member)
                            if isinstance(v, ctypes.Array):         # tables[8] / sqnorms[8]: the first n_frames are set
                                for k in range(arr[f].n_frames):
                                    self.seen.append((struct, member, v[k]))
                            else:
                                self.seen.append((struct, member, v))
            return inner(*a)
        return call


def run(case, a):
    """One call of `case` with the arguments `a` under the recorder and the decoding stub -> (error or None, recorder, stub)."""
    with pytest.MonkeyPatch.context() as mp:
        rec = occ.install(mp, ops)
        stub = DecodingStub(rec)
        mp.setattr(ops._lib, "lib", lambda: stub)
        err, _ = occ.run_recorded(ops, case, a, ERRORS)
    return err, rec, stub


def tensors(case, a):
    return [n for n in case.roles if torch.is_tensor(a.get(n)) and a[n].numel() > 0]


def role(case, n):
    return ROLE.get((case.name, n), case.roles[n])


def check_variant(case, canon_a, canon_stub, canon_rec, a, moved, err, rec, stub, device="cpu"):
    """The rule for one variant: `moved` = the names of the tensors that sit off the grid in `a`.  -> complaints."""
    bad = []
    cls_of = lambda e, p: CLASS[e][p]
    where = {n: [k for k, (e, p, addr) in enumerate(canon_stub.seen) if addr is not None and addr == canon_a[n].data_ptr()] for n in moved}
    must_raise = [n for n in moved if role(case, n) == occ.OUT and any(cls_of(*canon_stub.seen[k][:2]) == 16 for k in where[n])]
    if err is not None:
        if rec.calls:
            bad.append(f"raised {type(err).__name__} AFTER the library had been called ({rec.calls})")
        if not must_raise:
            bad.append(f"raised {type(err).__name__}: {err} -- but no moved tensor is a class-16 output")
        return bad
    if must_raise:
        return [f"{must_raise}: a caller-provided class-16 output off the grid was accepted (outputs are never copied: it must raise)"]
    if [s[:2] for s in stub.seen] != [s[:2] for s in canon_stub.seen]:
        return ["the library calls or their pointer parameters differ from the canonical run's"]
    for k, (e, p, addr) in enumerate(stub.seen):
        if cls_of(e, p) == 16 and addr is not None and addr % 16:
            bad.append(f"{e}.{p} (class 16) received an address {addr % 16} bytes off the grid")
    for n in moved:
        for k in where[n]:
            e, p, addr = stub.seen[k]
            if cls_of(e, p) == 4 and addr != a[n].data_ptr():
                bad.append(f"{e}.{p} (class 4) did not receive the caller's own `{n}` (a silent copy)")
            if cls_of(e, p) == 16 and addr == a[n].data_ptr():
                bad.append(f"{e}.{p} (class 16) received the caller's off-grid `{n}` itself")
    # the recorder notes the address modulo 16 where _p / _addr read it: what left ops off the grid is exactly what the library was handed
    # off the grid (device pointers only: host arrays and descriptors do not pass through _p / _addr), and none of it at a class-16 position
    if all(c in CLASS for c in rec.calls):
        off_rec = sorted(r.mod16 for r in rec.records if r.shape is not None and r.mod16)
        off_seen = sorted(addr % 16 for e, p, addr in stub.seen if p not in HOST and addr and addr % 16)
        if off_rec != off_seen:
            bad.append(f"_p / _addr took addresses {off_rec} bytes off the grid, the library received {off_seen}")
        if any(cls_of(e, p) == 16 for e, p, addr in stub.seen if p not in HOST and addr and addr % 16):
            bad.append("an address the recorder saw off the grid reached a class-16 position")
    # dtype, contiguity, size and lifetime of whatever was handed over instead (the tensor contract's own rule)
    bad += occ.check_rule(canon_rec.records, rec, None, occ.F, device)
    return bad


def variants(case, a):
    """-> [(label, names moved, offset)]: each tensor one at a time at 4 / 8 / 12 bytes, then all inputs at once."""
    names = tensors(case, a)
    inputs = [n for n in names if role(case, n) != occ.OUT]
    out = [(f"{n}+{k}", [n], k) for n in names for k in OFFSETS]
    if len(inputs) > 1:
        out += [(f"all inputs+{k}", inputs, k) for k in OFFSETS]
    return out


def canonical(name, device="cpu"):
    case = occ.CASES[name]
    a = case.build(ops, device)
    err, rec, stub = run(case, a)
    assert err is None, f"{name}: the canonical call raised {err!r}"
    return case, a, rec, stub


@functools.lru_cache(maxsize=None)
def covering():
    """The registry cases whose canonical call reaches a covered entry (run once, under the stub)."""
    return tuple(sorted(n for n in occ.CASES if canonical(n)[3].seen))


def class16_inputs(name):
    """The tensors of a case that reach a class-16 position as inputs (the cases the helper is there for)."""
    case, a, _, stub = canonical(name)
    return [n for n in tensors(case, a) if role(case, n) != occ.OUT
            and any(addr == a[n].data_ptr() and CLASS[e][p] == 16 for e, p, addr in stub.seen)]
