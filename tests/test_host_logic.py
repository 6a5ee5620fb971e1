"""CPU-side tests: the C-ABI library loads and exports every symbol include/aoc_hip.h declares, the
Python mirrors keep the reference's signatures, operators refuse CPU tensors (no fallback), the
synthetic generator is deterministic, and the N > 1 sharding path works over gloo (world_size 2)."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import aoc_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "aoc_hip.h")).read()
    declared = set(re.findall(r"\b(aoc_[a-z0-9_]+)\s*\(", header))
    declared -= {"aoc_status"}
    assert len(declared) >= 25
    lib = aoc_amd._lib.lib()                       # loads csrc/libaoc_hip.so (no GPU needed to load)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} is declared in aoc_hip.h but not exported"
    assert declared == set(aoc_amd._lib.SIGNATURES), "ctypes table and header differ"
    assert b"gfx950" in lib.aoc_version()


DEV_SWITCH = re.compile(rb"AOC_[A-Z][A-Z0-9_]{2,}")


def _dynamic_imports(path):
    out = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}


def test_release_library_never_reads_the_environment():
    """Release hygiene: libaoc_hip.so has no developer switch -- it does not import getenv and none of the switch names
    (AOC_*_DEBUG, AOC_KM_*, ...) is in the binary, so a stray environment variable cannot change a result or a kernel choice.
    There is no other build: no source under csrc/ calls getenv or knows an AOC_DEV conditional."""
    rel = aoc_amd._lib.RELEASE_SO
    blob = open(rel, "rb").read()
    names = {m.group(0).decode() for m in DEV_SWITCH.finditer(blob)} - {"AOC_OK"}
    names = {n for n in names if not n.startswith(("AOC_ERR", "AOC_MAX", "AOC_RETURN"))}
    assert not names, f"environment switch names in the release library: {sorted(names)}"
    assert "getenv" not in _dynamic_imports(rel) and "secure_getenv" not in _dynamic_imports(rel)
    srcs = os.path.join(ROOT, "robust-video-object-segmentation_amd", "csrc")
    checked = 0
    for f in os.listdir(srcs):
        if f.endswith((".hip", ".h")) or f == "Makefile":
            text = open(os.path.join(srcs, f)).read()
            assert "getenv" not in text and "AOC_DEV" not in text, f"{f}: the library has one build and does not read the environment"
            checked += 1
    assert checked >= 17                                    # fourteen translation units, two headers, the Makefile


def test_frame_call_structs_match_the_header(tmp_path):
    """aoc_frame_desc / aoc_seq_state as ctypes lays them out (ops._FrameDesc, ops._SeqState) against the C compiler's view of include/aoc_hip.h."""
    import ctypes
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(aoc_frame_desc), '
                   'sizeof(aoc_seq_state), offsetof(aoc_frame_desc, pool_key), offsetof(aoc_frame_desc, ref_emb), offsetof(aoc_frame_desc, feat), '
                   'offsetof(aoc_frame_desc, probe), sizeof(aoc_gate_desc), offsetof(aoc_gate_desc, x), offsetof(aoc_gate_desc, probe));return 0;}\n' % os.path.join(ROOT, "include", "aoc_hip.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, S, G = aoc_amd.ops._FrameDesc, aoc_amd.ops._SeqState, aoc_amd.ops._GateDesc
    assert got == [ctypes.sizeof(D), ctypes.sizeof(S), D.pool_key.offset, D.ref_emb.offset, D.feat.offset, D.probe.offset, ctypes.sizeof(G), G.x.offset, G.probe.offset]
    L = aoc_amd._lib.lib()
    assert L.aoc_frame_channels(6, 1, 1) == 24 and L.aoc_frame_channels(6, 3, 1) == 28 and L.aoc_frame_channels(6, 1, 0) == 17      # aocnet.py:43-46
    assert L.aoc_frame_workspace_bytes(121, 213, 100, 4, 12, 6, 1) > 0 and L.aoc_frame_workspace_bytes(121, 213, 64, 4, 12, 6, 1) > 0
    assert L.aoc_frame_workspace_bytes(121, 213, 130, 4, 12, 6, 1) == 0          # no split records beyond C = 100


def test_reference_signatures_are_kept():
    """Positional order and defaults of the reference API."""
    m = aoc_amd.matching
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    glob = [("n_chunks", 20), ("dis_bias", 0.), ("ori_size", None), ("atrous_rate", 1), ("use_float16", True), ("atrous_obj_pixel_num", 0)]
    for f in (m.global_matching_for_eval, m.global_matching_for_eval_proxy):
        assert sig(f)[:3] == [("all_reference_embeddings", inspect._empty), ("query_embeddings", inspect._empty),
                              ("all_reference_labels", inspect._empty)]
        assert sig(f)[3:9] == glob
    assert sig(m.global_matching_for_eval_cluster)[3:9] == glob
    train = [("n_chunks", 100)] + glob[1:]
    for f in (m.global_matching, m.global_matching_proxy, m.global_matching_cluster):
        assert [n for n, _ in sig(f)[:3]] == ["reference_embeddings", "query_embeddings", "reference_labels"]
        assert sig(f)[3:9] == train
    for f in (m.local_matching, m.local_matching_proxy):
        assert [n for n, _ in sig(f)] == ["prev_frame_embedding", "query_embedding", "prev_frame_labels", "dis_bias", "multi_local_distance",
                                          "ori_size", "atrous_rate", "use_float16", "allow_downsample", "allow_parallel"]
        assert dict(sig(f))["multi_local_distance"] == [15] and dict(sig(f))["allow_downsample"] is True
    assert [n for n, _ in sig(m.foreground2background)] == ["dis", "obj_num"]
    a = aoc_amd.attention
    assert [n for n, _ in sig(a.calculate_attention_head_for_eval_p_m)] == ["ref_embeddings", "ref_labels", "prev_embedding", "prev_label", "epsilon"]
    gate = a.IA_gate(8, 4)
    assert set(gate.state_dict()) == {"IA.weight", "IA.bias"}
    blk = aoc_amd.conditioning_layer.conditioning_block(8, 6, 0.3)
    names = set(blk.state_dict())
    for n in ("CL_1.phi_layer.weight", "CL_1.mlp_layer.weight", "CL_2.mlp_layer.bias", "CL_3.mlp_layer.weight", "mlp_layer.weight"):
        assert n in names
    assert blk.CL_3.mlp_layer.in_features == 6 and blk.mlp_layer.in_features == 2 * 8 + 6      # CLB:62-64


def test_no_cpu_fallback():
    with pytest.raises(aoc_amd._lib.AocHipError):
        aoc_amd.matching.foreground2background(torch.zeros(3, 1, 4, 4), 3)
    with pytest.raises(aoc_amd._lib.AocHipError):
        aoc_amd.attention.IA_gate(4, 2)(torch.zeros(1, 2, 3, 3), torch.zeros(1, 4))
    with pytest.raises(aoc_amd._lib.AocHipError, match="no CPU fallback"):      # float16 mode is implemented (round 2): only the missing GPU is reported
        aoc_amd.matching.local_matching(torch.zeros(4, 4, 8), torch.zeros(4, 4, 8), torch.zeros(4, 4, 2), use_float16=True)


def test_synthetic_clip_is_deterministic_and_shaped():
    syn = aoc_amd.synthetic
    cfg = syn.CONFIGS["tiny"]
    a, b = syn.make_clip(cfg, 3), syn.make_clip(cfg, 3)
    assert np.array_equal(a["emb"], b["emb"]) and np.array_equal(a["lab"], b["lab"])
    assert a["emb"].shape == (cfg.frames, cfg.h, cfg.w, cfg.c) and a["emb"].min() >= 0
    assert set(np.unique(a["lab"])) <= set(range(cfg.n_obj))
    rows = syn.kmeans_init_rows(1, [100, 5, 0, 50], 16)
    assert len(rows[0]) == 16 and len(rows[1]) == 5 and rows[2] is None and rows[3] is None     # sticky K (AEM:268)
    assert syn.CONFIGS["cfg2"].h == 121 and syn.CONFIGS["cfg2"].w == 213 and syn.CONFIGS["cfg2"].n_obj == 4


def test_lpt_partition():
    sh = aoc_amd.sharding
    costs = [60 * 4, 30 * 2, 100 * 3, 10, 80 * 6, 45, 45]
    parts = sh.lpt_partition(costs, 3)
    assert sorted(i for p in parts for i in p) == list(range(len(costs)))
    loads = [sum(costs[i] for i in p) for p in parts]
    assert max(loads) <= sum(costs) / 3 + max(costs)
    assert sh.lpt_partition(costs, 3) == parts                        # deterministic
    assert sh.lpt_partition([5.0], 4) == [[0], [], [], []]


_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
import aoc_amd
from aoc_amd import sharding
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
costs = [60 * 4, 30 * 2, 100 * 3, 10, 80 * 6, 45, 45]
mine = sharding.lpt_partition(costs, world)[rank]
local = dict(frames=sum(costs[i] for i in mine), objects=len(mine), gpu_seconds=0.5 + rank, sum_iou=0.25 * len(mine), iou_count=len(mine))
tot = sharding.allreduce_metrics(local)
if rank == 0:
    assert tot["frames"] == sum(costs) and tot["objects"] == len(costs), tot
    assert abs(tot["gpu_seconds"] - sum(0.5 + r for r in range(world))) < 1e-12
    assert abs(tot["sum_iou"] - 0.25 * len(costs)) < 1e-12
    print("SHARD_OK", tot["frames"])
dist.destroy_process_group()
'''


def test_sharding_allreduce_gloo_world2(tmp_path):
    """The multi-GPU path (sequence sharding + one metric all-reduce) on CPU: gloo, world_size 2."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29533", str(script), ROOT], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "SHARD_OK 1180" in out.stdout      # 1180 = total cost of the seven sequences


def test_mask_iou_sums():
    sh = aoc_amd.sharding
    a = torch.tensor([[0, 1, 1], [2, 2, 0]])
    b = torch.tensor([[0, 1, 2], [2, 2, 0]])
    s, n = sh.mask_iou_sums(a, b, 3)
    assert n == 3 and abs(s - (1.0 + 0.5 + 2 / 3)) < 1e-9
    s, n = sh.mask_iou_sums(a, a, 4)                                   # absent object: empty vs empty counts as 1
    assert s == 4.0


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """Status codes of the C ABI (include/aoc_hip.h: aoc_status) for calls that fail validation before any launch:
    these run on the CPU-only container as well (no kernel is launched)."""
    import ctypes
    L = aoc_amd._lib.lib()
    vp = ctypes.c_void_p
    dummy = (ctypes.c_float * 16)()
    p = ctypes.cast(dummy, vp)
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    # null pointers / negative sizes
    assert L.aoc_fg2bg_min(None, 3, 1, 10, 10, p, 10, None) == INVALID
    assert L.aoc_plane_mean(p, 0, 10, p, None) == INVALID
    assert L.aoc_linear(p, p, p, 1, 0, 4, p, None) == INVALID
    assert L.aoc_confident_labels(p, 40, 8, 0, None, 0.5, p, p, p, None) == UNSUPPORTED          # more than 32 channels
    assert L.aoc_proxy_corr_min(p, 16, 6, p, p, 4, 1, p, p, p, p, p, 1, 1, None) == UNSUPPORTED   # C not a multiple of 4
    # workspace too small is reported, not overrun
    assert L.aoc_dense_match_workspace_bytes(100, 50, 3) > 0
    i32 = (ctypes.c_int32 * 4)()
    ip = ctypes.cast(i32, vp)
    assert L.aoc_dense_match_min(p, 100, 100, p, ip, ip, 50, ip, p, 3, p, 1, 100, 1, p, 16, None) == WORKSPACE
    assert L.aoc_split_record_bytes(100) == 448 and L.aoc_split_record_bytes(104) == 0 and L.aoc_split_record_bytes(98) == 0
    assert L.aoc_dense_match_workspace_bytes(0, 5, 3) == 0
    # tile-major records: whole 32-row tiles; the records correlation entry validates its frame table before anything is enqueued
    assert L.aoc_split_rows_tiled_bytes(33, 100) == 64 * 448 and L.aoc_split_rows_tiled_bytes(32, 100) == 32 * 448
    assert L.aoc_split_rows_tiled_bytes(10, 98) == 0
    assert L.aoc_split_rows_tiled(None, 10, 100, p, p, ip, None) == INVALID
    assert L.aoc_split_rows_tiled(p, 10, 98, p, p, ip, None) == UNSUPPORTED

    # replicated segment lists: the replica count has to divide the segment count
    assert L.aoc_kmeans_segmented_rep(p, 10, 100, ip, ip, ip, ip, 6, 4, 16, 20, 100, p, ip, ip, p, 16, None) == INVALID
    assert L.aoc_kmeans_segmented_rep(p, 10, 100, ip, ip, ip, ip, 6, 0, 16, 20, 100, p, ip, ip, p, 16, None) == INVALID
    assert L.aoc_kmeans_segmented_rep(p, 10, 100, ip, ip, ip, ip, 6, 3, 16, 20, 100, p, ip, ip, p, 16, None) == WORKSPACE

    class Frame(ctypes.Structure):
        _fields_ = [(n, vp) for n in ("query", "query_rec", "query_sqnorm", "proxies", "proxy_sqnorm", "set_bias", "out")]
    fr = (Frame * 1)(Frame(ctypes.addressof(dummy), ctypes.addressof(dummy), ctypes.addressof(dummy), ctypes.addressof(dummy), None, None,
                           ctypes.addressof(dummy)))
    fp = ctypes.cast(fr, vp)
    i64 = (ctypes.c_int64 * 4)()
    lp = ctypes.cast(i64, vp)
    ws = (ctypes.c_char * 256)()
    wp = ctypes.cast(ws, vp)
    assert L.aoc_proxy_corr_min_records(fp, 1, 64, 96, 4, 1, ip, ip, lp, 1, wp, 256, None) == UNSUPPORTED      # records exist for C = 100 only
    assert L.aoc_proxy_corr_min_records(fp, 1, 64, 100, 4, 1, ip, ip, lp, 1, None, 0, None) == WORKSPACE
    assert L.aoc_proxy_corr_min_records(fp, 0, 64, 100, 4, 1, ip, ip, lp, 1, wp, 256, None) == INVALID
    fr[0].query_rec = None
    assert L.aoc_proxy_corr_min_records(fp, 1, 64, 100, 4, 1, ip, ip, lp, 1, wp, 256, None) == INVALID         # a frame without records

    # the host-side draw of the k-means initial rows: generator position outside 0..624, a level above kmax, a negative count
    key = (ctypes.c_uint32 * 624)()
    pos = ctypes.c_int32(700)
    counts = (ctypes.c_int32 * 2)(5, 3)
    lv = (ctypes.c_int32 * 1)(4)
    rows = (ctypes.c_int32 * 8)()
    kp, cp, lvp, rp = (ctypes.cast(x, vp) for x in (key, counts, lv, rows))
    assert L.aoc_kmeans_init_rows_draw(kp, ctypes.byref(pos), cp, 2, lvp, 1, 1, 4, rp, None) == INVALID
    pos.value = 624
    lv[0] = 5
    assert L.aoc_kmeans_init_rows_draw(kp, ctypes.byref(pos), cp, 2, lvp, 1, 1, 4, rp, None) == INVALID
    lv[0], counts[1] = 4, -1
    assert L.aoc_kmeans_init_rows_draw(kp, ctypes.byref(pos), cp, 2, lvp, 1, 1, 4, rp, None) == INVALID
    counts[1] = 3
    assert L.aoc_kmeans_init_rows_draw(kp, ctypes.byref(pos), cp, 2, lvp, 1, 1, 4, rp, None) == 0 and pos.value != 624


def test_frame_call_validates_everything_before_it_touches_the_state():
    """aoc_frame_enqueue rejects a bad cluster level / window radius / prefix count up front -- nothing is launched (this runs without a
    GPU) and the caller's aoc_seq_state is untouched -- instead of failing in the correlation or local-matching stage of a half-enqueued frame."""
    import ctypes
    L = aoc_amd._lib.lib()
    D, S = aoc_amd.ops._FrameDesc, aoc_amd.ops._SeqState
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)

    def desc():
        d = D()
        d.h, d.w, d.C, d.n_obj, d.R, d.R_capacity = 24, 40, 100, 3, 1, 2
        d.n_radii, d.n_levels, d.kmax, d.matching_background, d.epsilon = 2, 2, 16, 1, 1e-5
        d.radii[0], d.radii[1] = 4, 8
        d.levels[0], d.levels[1] = 8, 16
        d.n_adaptive = 2 * 3 * 2 * 16
        d.pool_key, d.pool_prefix_frames = 1, 1
        for name in ("ref_emb", "ref_labels", "prev_emb", "prev_labels", "cur_emb", "dis_bias", "right_bits", "wrong_bits", "fg_rows", "obj_rows", "counts",
                     "obj_offsets", "proxy_table", "proxy_sqnorm", "feat", "head"):
            setattr(d, name, ptr)
        return d
    need = L.aoc_frame_workspace_bytes(24, 40, 100, 3, 2, 2, 2)
    assert need > 0
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4

    def call(d, nbytes=need):
        st = S()
        rc = L.aoc_frame_enqueue(ctypes.byref(d), ctypes.byref(st), ctypes.c_void_p(ptr), nbytes, None)
        assert (st.initialised, st.records_frames, st.ref_pool_key, st.plan_key, st.plan_rows) == (0, 0, 0, 0, 0), "the state record was touched"
        return rc
    d = desc(); d.levels[1] = 17                      # a level above kmax
    assert call(d) == INVALID
    d = desc(); d.levels[0] = 0
    assert call(d) == INVALID
    d = desc(); d.radii[1] = 4                        # radii not ascending
    assert call(d) == INVALID
    d = desc(); d.radii[1] = 40                       # window beyond the kernel's reach
    assert call(d) == UNSUPPORTED
    d = desc(); d.pool_prefix_frames = -1
    assert call(d) == INVALID
    d = desc(); d.stream_cus = -3
    assert call(d) == INVALID
    d = desc(); d.pool_key = 0                        # a key is required
    assert call(d) == INVALID
    d = desc(); d.n_adaptive = 5
    assert call(d) == INVALID
    assert call(desc(), nbytes=1024) == WORKSPACE     # a complete descriptor: the next check is the workspace size


def test_chain_desc_matches_the_header(tmp_path):
    """aoc_chain_desc as ctypes lays it out (ops._ChainDesc) against the C compiler's view of include/aoc_hip.h; validation without a GPU."""
    import ctypes
    src = tmp_path / "cz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(aoc_chain_desc), '
                   'offsetof(aoc_chain_desc, pool_rows), offsetof(aoc_chain_desc, pool), offsetof(aoc_chain_desc, init_rows), offsetof(aoc_chain_desc, sqnorms));return 0;}\n'
                   % os.path.join(ROOT, "include", "aoc_hip.h"))
    exe = tmp_path / "cz"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = aoc_amd.ops._ChainDesc
    assert got == [ctypes.sizeof(D), D.pool_rows.offset, D.pool.offset, D.init_rows.offset, D.sqnorms.offset]
    L = aoc_amd._lib.lib()
    d = D()
    assert L.aoc_cluster_chain_workspace_bytes(ctypes.byref(d)) == 0                 # an empty descriptor
    d.C, d.n_obj, d.n_frames, d.n_levels, d.kmax, d.iters, d.pool_rows, d.rows_capacity = 100, 3, 2, 2, 16, 20, 960, 2880
    d.levels[0], d.levels[1] = 8, 16
    need = L.aoc_cluster_chain_workspace_bytes(ctypes.byref(d))
    off = (ctypes.c_int64 * 7)()
    assert need > 0 and L.aoc_cluster_chain_layout(ctypes.byref(d), off) == 0 and list(off) == sorted(off) and off[0] == 0 and off[6] < need
    buf = (ctypes.c_float * 16)()
    assert L.aoc_cluster_chain_enqueue(ctypes.byref(d), ctypes.cast(buf, ctypes.c_void_p), need, None) == -1          # null pool / lists
    d.levels[1] = 17
    assert L.aoc_cluster_chain_workspace_bytes(ctypes.byref(d)) == 0                 # a level above kmax


def test_round5_entry_points_reject_bad_arguments_without_a_gpu():
    """aoc_atrous_subsample and aoc_proxy_corr_min_records_cached validate before any launch."""
    import ctypes
    L = aoc_amd._lib.lib()
    vp = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, vp)
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    assert L.aoc_atrous_subsample(None, 4, 4, 4, 2, p, None) == INVALID
    assert L.aoc_atrous_subsample(p, 4, 4, 4, 0, p, None) == INVALID              # rate >= 1
    assert L.aoc_atrous_subsample(p, 0, 4, 4, 2, p, None) == INVALID
    need = L.aoc_proxy_corr_min_records_cached_workspace_bytes()
    assert need > L.aoc_proxy_corr_min_batched_workspace_bytes() >= 256 and need % 256 == 0

    class Frame(ctypes.Structure):
        _fields_ = [(n, vp) for n in ("query", "query_rec", "query_sqnorm", "proxies", "proxy_sqnorm", "set_bias", "out")]
    fr = (Frame * 1)(Frame(*([ctypes.addressof(buf)] * 4), None, None, ctypes.addressof(buf)))
    fp = ctypes.cast(fr, vp)
    i32 = (ctypes.c_int32 * 4)()
    i64 = (ctypes.c_int64 * 4)()
    ip, lp = ctypes.cast(i32, vp), ctypes.cast(i64, vp)
    key = ctypes.c_int64(0)
    small = (ctypes.c_char * 256)()
    # with a key the workspace has to hold the pass tables; without one the 256-byte flag workspace is enough to get past the size check
    assert L.aoc_proxy_corr_min_records_cached(fp, 1, 64, 100, 4, 1, ip, ip, lp, 1, ctypes.cast(small, vp), 256, ctypes.byref(key), None) == WORKSPACE
    assert L.aoc_proxy_corr_min_records_cached(fp, 1, 64, 96, 4, 1, ip, ip, lp, 1, ctypes.cast(small, vp), 256, ctypes.byref(key), None) == UNSUPPORTED
    assert L.aoc_proxy_corr_min_records_cached(fp, 0, 64, 100, 4, 1, ip, ip, lp, 1, ctypes.cast(small, vp), 256, None, None) == INVALID
    assert key.value == 0


def test_mirrors_refuse_to_run_under_autograd():
    """the drop-in names include the reference's training-time ones; they build no autograd graph, so they must raise
    (instead of silently training nothing) when a gradient is wanted."""
    import aoc_amd
    gate = aoc_amd.attention.IA_gate(8, 4)
    x, head = torch.randn(2, 4, 3, 3), torch.randn(2, 8)
    with pytest.raises(aoc_amd._lib.AocHipError, match="inference-only"):
        gate(x, head)                                         # parameters require grad and autograd is on
    blk = aoc_amd.conditioning_layer.conditioning_block(4, 8, 0.3)
    with pytest.raises(aoc_amd._lib.AocHipError, match="inference-only"):
        blk(x, head)
    q = torch.randn(5, 6, 4, requires_grad=True)
    with pytest.raises(aoc_amd._lib.AocHipError, match="inference-only"):
        aoc_amd.matching.global_matching(torch.randn(5, 6, 4), q, torch.ones(5, 6, 2), 1, 0., None, 1, False, 0)
    with torch.no_grad():                                     # under no_grad the guard passes and the missing GPU is what is reported
        with pytest.raises(aoc_amd._lib.AocHipError, match="no CPU fallback"):
            gate(x, head)


_RUNNER_WORKER = r'''
import json, os, sys
sys.path.insert(0, sys.argv[1])
import torch
import torch.distributed as dist
import aoc_amd
from aoc_amd import eval_runner as er

class StubBackend:
    """CPU stand-in for the HIP hot path: a deterministic label map from the embedding (the loop, the partition, the metric and the
    reduction are the product's own)."""
    def start(self, spec): self.spec = spec
    def first_frame(self, emb, gt): pass
    def frame(self, emb):
        lab = (emb[..., :3].sum(-1) * 40.0).long() % self.spec.n_obj
        return lab.repeat_interleave(4, 0).repeat_interleave(4, 1).to(torch.int32)

rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
if world > 1:
    dist.init_process_group("gloo", rank=rank, world_size=world)
specs = er.make_sequence_set("cfg5", scale=0.012, seed=3)          # 1 DAVIS-like + 6 YTB-like sequences
tot = er.eval_sharded(specs, rank, world, torch.device("cpu"), backend=StubBackend(), max_frames=4)
if rank == 0:
    print("RUNNER " + json.dumps({k: tot[k] for k in ("frames", "objects", "sum_iou", "iou_count", "sequences", "ranks", "planned_imbalance")}))
if world > 1:
    dist.destroy_process_group()
'''


@pytest.mark.parametrize("world", [2, 8])
def test_eval_runner_sharded_gloo_equals_single_process(tmp_path, world):
    """BASELINE.json configs[4] path on CPU: the real runner (sequence set, LPT partition, per-sequence loop, metric accumulators,
    all-reduce) with a stub backend, world_size 2 and 8 over gloo (8 ranks for 7 sequences: one rank stays empty), must give the totals
    of the single-process run."""
    script = tmp_path / "runner_worker.py"
    script.write_text(_RUNNER_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    one = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert one.returncode == 0, one.stderr[-2000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                          "--master-port", str(29541 + world), str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert two.returncode == 0, two.stderr[-2000:]
    import json
    a = json.loads([l for l in one.stdout.splitlines() if l.startswith("RUNNER ")][0][7:])
    b = json.loads([l for l in two.stdout.splitlines() if l.startswith("RUNNER ")][0][7:])
    assert a["ranks"] == 1 and b["ranks"] == world and a["sequences"] == b["sequences"] == 7
    for k in ("frames", "objects", "iou_count"):
        assert a[k] == b[k]
    assert abs(a["sum_iou"] - b["sum_iou"]) < 1e-9 and a["sum_iou"] > 0
    assert 1.0 <= b["planned_imbalance"] < (1.5 if world == 2 else 4.0)


def test_sequence_set_mirrors_the_evaluation_sets():
    from aoc_amd import eval_runner as er
    s = er.make_sequence_set("cfg5")
    assert len(s) == 537 and sum(x.name.startswith("davis") for x in s) == 30
    assert all(x.levels == (8, 16, 32) and (x.h, x.w) == (145, 261) and 2 <= x.n_obj <= 6 for x in s if x.name.startswith("ytb"))
    assert all(x.levels == (16,) and (x.h, x.w) == (121, 213) and 2 <= x.n_obj <= 4 for x in s if x.name.startswith("davis"))
    parts = aoc_amd.sharding.lpt_partition([x.cost for x in s], 8)
    loads = [sum(s[i].cost for i in p) for p in parts]
    assert max(loads) / (sum(loads) / 8) < 1.01                      # LPT balances 537 sequences over 8 ranks to within 1 %


def test_oracle_davis_metrics_known_answers():
    """oracle/metrics.py (restated DAVIS J / F): hand-checkable cases."""
    from oracle import metrics as om
    a = np.zeros((20, 30), bool)
    a[5:15, 5:20] = True
    assert om.db_eval_iou(a, a) == 1.0 and om.db_eval_boundary(a, a) == 1.0
    assert om.db_eval_iou(np.zeros_like(a), np.zeros_like(a)) == 1.0 and om.db_eval_boundary(np.zeros_like(a), np.zeros_like(a)) == 1.0
    b = np.zeros_like(a)
    b[5:15, 10:25] = True
    assert abs(om.db_eval_iou(a, b) - (10 * 10) / (10 * 20)) < 1e-12
    assert om.db_eval_boundary(a, np.zeros_like(a)) == 0.0
    bm = om.seg2bmap(a)
    assert bm[4, 10] and bm[14, 10] and not bm[8, 10] and bm[8, 4] and bm[8, 19]


def _numpy_init_rows(rng, counts, levels, n_frames, kmax):
    """What eval_runner drew before aoc_kmeans_init_rows_draw existed: scipy kmeans2(minit='points') = RandomState.permutation(n)[:k]
    per frame, level and object, with the sticky cluster count of AEM:268."""
    rows = np.zeros((n_frames, len(levels) * len(counts), kmax), np.int32)
    states = []
    for f in range(n_frames):
        states.append(rng.get_state())
        for li, k in enumerate(levels):
            for i in range(len(counts)):
                k = min(k, int(counts[i]))
                if k > 0:
                    rows[f, li * len(counts) + i, :k] = rng.permutation(int(counts[i]))[:k]
    return rows, states


def test_init_rows_draw_is_numpys_legacy_stream():
    """aoc_kmeans_init_rows_draw (host function of the library) against numpy itself: same rows, same generator state afterwards (key,
    position, cached gaussian untouched), same per-frame snapshots -- over object sizes 0 / 1 / 2 / powers of two +- 1, generator positions
    in the middle and at the end of a 624-word block, one to three levels."""
    r = np.random.RandomState(11)
    sizes = [0, 1, 2, 3, 4, 5, 17, 31, 32, 33, 255, 256, 257, 1000, 4097, 30000]
    for trial in range(120):
        counts = [int(x) for x in r.choice(sizes, r.randint(1, 7))]
        levels = [[16], [8, 16, 32], [4], [64, 2]][r.randint(4)]
        n = int(r.randint(1, 6))
        seed = int(r.randint(1 << 30))
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        skip = int(r.choice([0, 1, 623, 624, 625, 1247, 1500]))
        a.randint(0, 10, skip)
        b.randint(0, 10, skip)
        if r.rand() < 0.3:
            a.randn(1), b.randn(1)                          # a cached gaussian in the state: must survive
        want, want_states = _numpy_init_rows(a, counts, levels, n, max(levels))
        got, got_states = aoc_amd.ops.kmeans_init_rows_draw(b, counts, levels, n)
        assert np.array_equal(want, got), (trial, counts, levels, n)
        sa, sb = a.get_state(), b.get_state()
        assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
        for x, y in zip(want_states, got_states):
            assert np.array_equal(x[1], y[1]) and x[2:] == y[2:]
        assert a.randint(0, 1 << 30) == b.randint(0, 1 << 30)
    # a handed-back frame: restoring a snapshot replays the same draws
    a = np.random.RandomState(3)
    rows, states = aoc_amd.ops.kmeans_init_rows_draw(a, [500, 20, 0, 7], [8, 16], 4)
    a.set_state(states[2])
    again, _ = aoc_amd.ops.kmeans_init_rows_draw(a, [500, 20, 0, 7], [8, 16], 2)
    assert np.array_equal(again, rows[2:])


def test_reference_model_files_import_against_the_mirrors():
    """INTEGRATION.md section 1 applied to the reference's OWN networks/aoc/aocnet.py and networks/aoc/decoding_module.py, as recorded with the sys.modules
    aliases in place by tests/golden/make_golden_integration.py (tests/golden/integration_decoder.json): every name the two files import from the aliased
    modules is an object of that mirror; every constructor call the reference's decoder constructor makes of a mirror class (decoding_module.py:10-93,
    arguments of aocnet.py:37-42, incl. the ``attention_dim=`` keyword it passes to conditioning_block) builds on the mirror's class with the parameter
    shapes it built then; the gates hotpath.CalibrationGates holds are the decoder's, name by name and shape by shape (a reference state_dict loads into
    either), and so is DynamicPreHead's state_dict.  CPU only: constructors, no forward."""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "integration_decoder.json")))
    A = aoc_amd
    mirrors = {n: getattr(A, n) for n in ("matching", "attention", "conditioning_layer", "gct")}
    for fname, names in rec["imports"].items():
        for name, mod in names.items():
            assert inspect.isfunction(getattr(mirrors[mod], name, None)) or inspect.isclass(getattr(mirrors[mod], name, None)), (fname, name)
    an, dm = rec["imports"]["aocnet"], rec["imports"]["decoding_module"]
    for name in ("global_matching", "global_matching_for_eval", "local_matching", "foreground2background", "global_matching_proxy", "local_matching_proxy",
                 "global_matching_cluster2", "global_matching_cluster", "global_matching_for_eval_cluster", "global_matching_for_eval_proxy"):
        assert an[name] == "matching", name
    for name in ("calculate_attention_head", "calculate_attention_head_for_eval", "calculate_attention_head_p_m", "calculate_attention_head_for_eval_p_m"):
        assert an[name] == "attention", name
    assert dm["IA_gate"] == "attention" and dm["Bottleneck"] == dm["GCT"] == "gct" and dm["conditioning_block"] == dm["conditioning_layer"] == "conditioning_layer"
    assert rec["decoder_class"] == "CalibrationDecoding" and rec["prehead_is_reference_class"]
    shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}
    built = {}
    for c in rec["calls"]:
        m = getattr(mirrors[c["module"]], c["cls"])(*c["args"], **c["kwargs"])
        assert shapes(m) == c["state_dict"], c["attr"]
        built[c["attr"]] = m
    assert isinstance(built["IA1"], A.attention.IA_gate) and built["IA1"].IA.weight.shape == (164, 400)
    assert isinstance(built["CLB2"], A.conditioning_layer.conditioning_block) and built["CLB2"].CL_3.mlp_layer.weight.shape == (400, 400)
    assert built["CLB4"].mlp_layer.weight.shape == (512, 2 * 512 + 400) and built["CLB2"].CL_1.beta_percentage == 0.3
    assert isinstance(built["layer2"], A.gct.Bottleneck) and isinstance(built["GCT_sc"], A.gct.GCT) and built["GCT_sc"].alpha.shape == (1, 512, 1, 1)
    assert built["IA9"].IA.weight.shape == (512, 400 + 512) and built["IA10"].IA.weight.shape == (320, 400 + 320) and built["IA11"].IA.weight.shape == (128, 400 + 128)
    sd = rec["state_dict"]["decoder"]
    for c in rec["calls"]:                                  # the recorded calls are the decoder's own sub-modules
        assert all(sd[c["attr"] + "." + k] == v for k, v in c["state_dict"].items()), c["attr"]
    gates = A.hotpath.CalibrationGates(A.hotpath.MatchingConfig())
    for k, v in gates.state_dict().items():
        assert k in sd and sd[k] == list(v.shape), k
    assert shapes(A.hotpath.DynamicPreHead(in_dim=24, embed_dim=64)) == rec["state_dict"]["DynamicPreHead"]


def test_package_import_asks_for_enough_hardware_queues_unless_the_caller_chose():
    """The evaluation runner keeps 8 streams busy (4 lanes + their chain streams): the package asks the HIP runtime for 16 hardware queues on
    import (profiles/r05_closed_loop_hw_queues.txt) and leaves a caller's own setting alone."""
    code = "import os, sys; sys.path.insert(0, %r); import aoc_amd; print(os.environ['GPU_MAX_HW_QUEUES'])" % ROOT
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.strip() == "16"
    env["GPU_MAX_HW_QUEUES"] = "6"
    assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.strip() == "6"


def test_bench_help_prints():
    """argparse expands '%' in help strings: an unescaped one made `python bench.py --help` raise."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--gpus" in r.stdout and "--steps" in r.stdout and "--warmup" in r.stdout


def test_every_profile_a_document_cites_is_committed():
    """The current-state documents point at files under profiles/ for every figure: each such path has to exist (round-4 verdict: docs follow the files)."""
    import re
    missing = []
    for doc in ("DESIGN.md", "STATUS.md", "README.md", "INTEGRATION.md", "HISTORY.md", "tools/README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for m in re.finditer(r"(profiles/[A-Za-z0-9_./\-]+)", text):
            path = m.group(1).rstrip(".,;:)")
            if "*" in path or path.endswith(("_", "/")):
                continue                                    # a family of files (r05_pmc_*), or the directory
            if not os.path.exists(os.path.join(ROOT, path)):
                missing.append((doc, path))
    text = open(os.path.join(ROOT, "profiles", "README.md")).read()
    for m in re.finditer(r"`(r0\d_[A-Za-z0-9_.\-]+)`", text):
        if "*" not in m.group(1) and not os.path.exists(os.path.join(ROOT, "profiles", m.group(1))):
            missing.append(("profiles/README.md", m.group(1)))
    assert not missing, missing


def test_headline_figures_in_the_documents_are_the_committed_line():
    """STATUS.md / README.md quote the driver-style line of the final code: the figures they print are the ones in profiles/r06_bench_line_driver_style.json (and, for the
    optional legs, r06_bench_line_all_legs.json); both committed lines are compact records with the keys the driver needs."""
    line = json.loads([l for l in open(os.path.join(ROOT, "profiles", "r06_bench_line_driver_style.json")) if l.startswith("{")][-1])
    legs = json.loads([l for l in open(os.path.join(ROOT, "profiles", "r06_bench_line_all_legs.json")) if l.startswith("{")][-1])
    status, readme = open(os.path.join(ROOT, "STATUS.md")).read(), open(os.path.join(ROOT, "README.md")).read()
    for doc in (status, readme):
        assert "%.1f frames/s" % line["value"] in doc
        assert "cfg3 %.1f" % line["cfg3_value"] in doc and "cfg4 %.1f" % line["cfg4_value"] in doc
        assert "%.1f" % legs["closed_loop_value"] in doc
    for rec in (line, legs):
        assert len(json.dumps(rec)) < 4096 and rec["schema"] == 6 and rec["roofline"]["bound"] == "mfma" and rec["roofline_correlation"]["bound"] == "hbm"
        assert rec["cpu_baseline"]["kind"] == "port" and rec["cpu_baseline"]["runs"] == 5 and rec["config"]["workload"].startswith("cfg2")
        assert os.path.exists(os.path.join(ROOT, "profiles", "r06_" + os.path.basename(rec["details_file"])))


def _canned_full_record():
    """A full bench record shaped like bench.py's, with numbers made up and every free-text field as long as round 5's."""
    prose = "x" * 900
    roof = dict(kernel="dense_prune_kernel (aoc_dense_match_min_split), " + prose, bound="mfma", achieved=652.123, peak=2500.0, unit="TFLOP/s", frac=0.2608,
                traffic=400123456.0, traffic_source=prose, avg_launch_ms=1.3229, algorithmic_flops_per_launch=8.56e11, executed_tflops=870.1, pipe_frac=0.348,
                note=prose, op_avg_ms=1.598)
    corr = dict(kernel="proxy_corr_records_kernel (" + prose + ")", bound="hbm", achieved=573.1, peak=8000.0, unit="GB/s", frac=0.0716, traffic=None,
                avg_launch_ms=0.0202, frames_per_launch=1, in_run_frac=0.0079, best_frac=0.4225, best_frames_per_launch=16,
                isolated=[dict(frames_per_launch=b, note=prose) for b in (1, 4, 16, 32)])
    hbm = dict(kernel="k (" + prose + ")", bound="hbm", achieved=213.07, peak=8000.0, unit="GB/s", frac=0.0266, traffic=None, avg_launch_ms=6.81, note=prose, offline={"a": prose})
    return {"metric": "frames/sec, AOC-Net matching + calibration hot path (480p, 3 objects)", "value": 422.321, "unit": "frames/s", "n_gpus": 8, "steps": 20, "warmup": 5,
            "ms_per_step": 4.7357, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "dtype_detail": prose,
            "timed_regions": 11, "region_ms": [94.7] * 15, "ranks_seen": 8, "frames_per_rank": [40] * 8, "imbalance": 1.0123,
            "config": {"workload": "cfg2: 121x213 stride-4 maps (480p), O=4 (3 objects + background), K=16 proxies, C=100, 60-frame clips, MEM_EVERY=5 (pool R=1..12), "
                                   "20 Lloyd iterations, local windows 2..12, 10 IA gates + 4 conditioning blocks", "R_mean": 6.4, "R_timed": {"histogram": {str(r): 10 for r in range(1, 13)}},
                       "sequences_per_gpu": 2, "proxy_mode": "reference", "proxy_mode_detail": prose, "frame_call": prose, "dense_precision": prose},
            "host_enqueue_ms_per_step": 4.1, "host_enqueue_cpu_ms_per_step": 0.95, "probe_sampling": prose,
            "exact_fp32_dense_run": dict(value=109.6, note=prose), "exact_fp32_value": 109.6, "cfg3_value": 239.917, "cfg4_value": 202.7, "closed_loop_value": 364.4,
            "roofline": roof, "roofline_correlation": corr, "roofline_kmeans_chain": hbm, "roofline_film_scale": dict(hbm), "roofline_cond_gate_pool": dict(hbm),
            "strong_scaling": dict(note=prose, workload=prose), "other_configs": {"cfg3": dict(workload=prose), "cfg4": dict(workload=prose)},
            "image_level_end_to_end": dict(note=prose),
            "cpu_baseline": dict(value=0.04185, unit="frames/s", cores=32, kind="port", runs=5, sample="median of 5 runs after 1 warm-up: " + prose, detail=prose,
                                 frame_seconds=[23.9] * 5),
            "parity": dict(max_abs_feature_diff=1.43e-6, per_branch={k: 1e-6 for k in ("dense", "cluster", "proxy", "local", "local_proxy")}, surrogate_mask_mean_iou=1.0),
            "kernels": {f"op{i}": dict(calls=100, avg_ms=1.0, note=prose) for i in range(12)}, "skipped": ["cfg4:budget"], "phases_s": {"a": 1.0}, "wall_s": 93.2}


def test_bench_line_is_compact():
    """Round 5's headline went unmeasured because the ONE line bench.py prints had grown to 23 KB and the driver (which keeps an 8 KB tail of stdout) could
    not parse it.  The printed line is a pure function of the full record: whatever prose the record carries, the line stays one line under 4 KB, parses,
    and holds every key the contract and the verdict ask for; everything else lives in the details file the line points at."""
    import bench
    full = _canned_full_record()
    assert len(json.dumps(full)) > 20000                   # the canned record is as verbose as round 5's line
    line = bench.compact_line(full, "gpurun_out/bench_details.json")
    text = json.dumps(line)
    assert len(text) < 4096 and "\n" not in text, len(text)
    back = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "parity", "exact_fp32_value", "cfg3_value", "cfg4_value", "details_file", "ranks_seen", "imbalance", "schema"):
        assert k in back, k
    assert back["config"]["workload"].startswith("cfg2") and "model" not in back["config"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in back["roofline"], k
    assert back["roofline"]["bound"] == "mfma" and back["roofline_correlation"]["bound"] == "hbm" and back["roofline_correlation"]["traffic"] is None
    assert abs(back["roofline"]["frac"] - back["roofline"]["achieved"] / back["roofline"]["peak"]) < 1e-3
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in back["cpu_baseline"], k
    assert back["parity"]["max_abs_feature_diff"] == 1.43e-6
    # a record whose optional objects are absent (N > 1: no CPU baseline, no other configs) still makes a valid line
    for k in ("cpu_baseline", "parity", "exact_fp32_value", "cfg3_value", "cfg4_value", "roofline_film_scale", "skipped"):
        full[k] = None
    back = json.loads(json.dumps(bench.compact_line(full, "d.json")))
    assert back["cpu_baseline"] is None and back["value"] == 422.321 and "cfg3_value" not in back


def test_bench_reads_pmc_traffic_from_the_committed_file():
    """`roofline.traffic` is read from the committed rocprofv3 --pmc summary at bench time (FETCH x 2 + WRITE, KB -> bytes), not copied into bench.py."""
    import bench
    import re
    text = open(os.path.join(ROOT, "profiles", "r06_pmc_dense_R6.txt")).read()
    fetch = float(re.search(r"^FETCH_SIZE .*avg=([0-9.e+]+)", text, re.M).group(1))
    write = float(re.search(r"^WRITE_SIZE .*avg=([0-9.e+]+)", text, re.M).group(1))
    t = bench.pmc_traffic_bytes("profiles/r06_pmc_dense_R6.txt")
    assert t is not None and abs(t - (2 * fetch + write) * 1024) < 1.0 and 2.0e8 < t < 6.0e8
    assert bench.pmc_traffic_bytes("profiles/does_not_exist.txt") is None


def test_bench_dump_outputs_stay_within_the_limit_and_repeat(tmp_path, monkeypatch):
    """--dump-outputs: small outputs are written whole, large ones as a fixed, seeded sample of their flat elements; all files together stay
    under the limit, and the same outputs give the same files."""
    import bench
    import torch
    # the cfg2 plan: two sequences x (features, attention head, 14 gate outputs) stay under 64 MB
    numels = [4 * 24 * 121 * 213, 4 * 400] + [4 * c * 121 * 213 for c in (164, 256, 256, 320, 128)] + [4 * c * 61 * 107 for c in (512,) * 7 + (256,) * 2]
    keep = bench.dump_sample_sizes([4 * n for n in numels * 2], bench.DUMP_LIMIT_BYTES)
    assert sum(keep) <= bench.DUMP_LIMIT_BYTES < 64 * 10 ** 6 and keep[1] == 4 * 4 * 400 and min(keep) > 0
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    g = torch.Generator().manual_seed(0)
    named = [("small", torch.randn(3, 5, generator=g)), ("wide", torch.randn(4, 300, 1000, generator=g)), ("f64", torch.randn(7, dtype=torch.float64, generator=g))]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), named)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["f64.npy", "small.npy", "wide.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 20
    small, wide, f64 = (np.load(tmp_path / "a" / f) for f in ("small.npy", "wide.npy", "f64.npy"))
    assert small.dtype == np.float32 and np.array_equal(small, named[0][1].numpy()) and f64.dtype == np.float64 and np.array_equal(f64, named[2][1].numpy())
    idx = bench.dump_sample_index("wide", 4 * 300 * 1000, wide.size)
    assert wide.ndim == 1 and 0 < wide.size < 4 * 300 * 1000 and np.all(np.diff(idx) > 0) and np.array_equal(wide, named[1][1].numpy().reshape(-1)[idx])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dense_seed_margin_covers_the_worst_case():
    """dense_seed_kernel (csrc/dense_split.hip) publishes  seed = fp32[2^20 (q.r - |r|^2 / 2)] - margin  and relies on  seed <= the value the matrix kernel computes for
    the same pair  -- whatever the roundings.  Replay in numpy: the matrix kernel's value is the EXACT sum of the fp16 split products qh.rh + qh.rl + ql.rh and the
    three fp16 norm pieces (float64 holds every such product and sum exactly at these sizes) perturbed by at most 336 half-ulps of the largest partial sum; the seed
    is computed in float32 with sequential adds as the kernel does.  Random rows, rows at the fp16-split range limits, anti-correlated and tiny rows."""
    rng = np.random.RandomState(0)
    f32, f64 = np.float32, np.float64

    def split(x):                                           # x' = 2^10 x = hi + lo, both fp16 (dense_split.hip: split_rows_kernel)
        v = (x.astype(f32) * f32(1024.0)).astype(f32)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(f32)).astype(np.float16)
        return hi.astype(f64), lo.astype(f64)

    worst = 1e30
    for case in range(400):
        C = 100
        scale = [0.3, 0.3, 1.0, 6.0, 0.01][case % 5]
        q = (np.maximum(rng.randn(C), 0) * scale).astype(f32)
        r = (np.maximum(rng.randn(C), 0) * scale).astype(f32) if case % 7 else q.copy()          # every 7th: the pair at distance 0
        if case % 11 == 0:
            r = (-q).astype(f32)                            # anti-correlated: large negative value
        if float((r.astype(f64) ** 2).sum()) > 4000.0 or np.abs(q).max() * 1024 > 65000 or np.abs(r).max() * 1024 > 65000:
            continue                                        # outside the split kernels' preconditions: the exact-fp32 kernels take over
        qh, ql = split(q)
        rh, rl = split(r)
        r2_32 = f32(0.0)
        for t in range(C):                                  # |r|^2 as split_rows_kernel sums it (sequential fp32)
            r2_32 = f32(r2_32 + f32(r[t] * r[t]))
        p = f32(-16.0) * r2_32                              # three fp16 pieces of -16 |r|^2, times the query side's 2^15
        p1 = np.float16(p); p2 = np.float16(f32(p - f32(p1))); p3 = np.float16(f32(f32(p - f32(p1)) - f32(p2)))
        norm_term = (f64(p1) + f64(p2) + f64(p3)) * 32768.0
        exact3 = float((qh * rh).sum() + (qh * rl).sum() + (ql * rh).sum() + norm_term)          # what the 21 MFMAs add up, before their roundings
        qn, rn = float(np.sqrt((q.astype(f64) ** 2).sum())), float(np.sqrt((r.astype(f64) ** 2).sum()))
        M = 2.0 ** 20 * (qn * rn + 0.5 * rn * rn)
        kernel_lowest = exact3 - 336 * 2.0 ** -24 * M       # the matrix kernel's value can be this low, not lower
        # the seed, as dense_seed_kernel computes it
        dot, r2 = f32(0.0), f32(0.0)
        for t in range(C):
            dot = f32(dot + f32(q[t] * r[t]))
            r2 = f32(r2 + f32(r[t] * r[t]))
        qq = f32(0.0)
        for t in range(C):
            qq = f32(qq + f32(q[t] * q[t]))
        value = f32(f32(1048576.0) * f32(dot - f32(f32(0.5) * r2)))
        qr_n = f32(np.sqrt(f32(qq * r2)))
        seed = f32(value - f32(f32(f32(4e-5) * f32(f32(1048576.0) * f32(qr_n + f32(f32(0.5) * r2)))) + qr_n + f32(16.0)))
        assert float(seed) <= kernel_lowest, (case, float(seed), kernel_lowest, exact3)
        worst = min(worst, kernel_lowest - float(seed))
    assert worst >= 0.0
