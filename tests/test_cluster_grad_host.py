"""What can be checked without a GPU about the training-time cluster matching: that the numpy reference of tests/cluster_grad_bounds.py IS
the reference's function (it reproduces the outputs and gradients the reference's own autograd recorded, tests/golden/cluster_grad_*.npz),
the conditions the fixtures have to meet, the argument checks of the new entry points (they return before any launch), the workspace
formula and cluster_train's host-side behaviour."""
import ctypes

import numpy as np
import pytest
import torch

import aoc_amd
import cluster_grad_bounds as cgb
from conftest import load_golden

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4


def _close(got, want, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(np.asarray(got).reshape(np.shape(want)) - want).max())
    assert err <= 1e-10 * scale, f"{what}: numpy reference and recorded value differ by {err / scale:.2e} relative"


@pytest.mark.parametrize("name", cgb.FIXTURES)
def test_numpy_reference_reproduces_the_recorded_gradients(name):
    fx = load_golden(name)
    ref = cgb.fixture_ref_by_name(name)
    _close(ref["out"], fx["out"], name + " out")
    _close(ref["grad_query"], fx["grad_query"], name + " grad_query")
    _close(ref["grad_ref"], fx["grad_ref"], name + " grad_ref")
    _close(ref["grad_bias"], fx["grad_bias"], name + " grad_bias")
    assert np.abs(fx["grad_query"]).max() > 1e-2 and np.abs(fx["grad_ref"]).max() > 1e-2, "the fixture's gradients vanish: it tests nothing"


@pytest.mark.parametrize("name", cgb.FIXTURES)
def test_fixture_inputs_meet_the_conditions(name):
    fx = load_golden(name)
    ref = cgb.fixture_ref_by_name(name)
    cgb.check_fixture_conditions(name, fx, ref)
    assert ref["out"].shape == fx["out"].shape and ref["grad_ref"].shape == fx["in_ref"].shape      # nothing is left out of a comparison
    st = ref["state"]
    if name == "cluster_grad_C100_O4_bias":
        assert 0 < min(c for c in st["counts"] if c > 0) < 16 and st["seg_k"][-1] < 16, "no object with fewer rows than K: the sticky rule is not covered"
    if name == "cluster_grad_absent":
        assert st["counts"][2] == 0 and (ref["out"][..., 2, :] == 1.0).all() and fx["grad_bias"][2] == 0.0 and ref["grad_bias"][2] == 0.0
        assert (ref["fwd"]["arg"][4:6] == -1).all()
    if name == "cluster_grad_dup_empty":
        km_labels, km_cents, _ = cgb.fixture_km(fx)
        assert np.unique(km_cents[0], axis=0).shape[0] < km_cents[0].shape[0], "no bit-equal code-book entries"
        empty = sorted(set(range(km_cents[0].shape[0])) - set(np.unique(km_labels[0]).tolist()))
        assert empty and not st["live"][0, 1, empty].any() and st["live"][0, 0, empty].all(), "no empty cluster: set 1 has every slot"
        assert (ref["grad_proxies"].reshape(st["proxies"].shape)[0, 1, empty] == 0.0).all()
    if name == "cluster_grad_atrous2":
        assert int(fx["atrous_rate"]) == 2 and int(fx["atrous_obj_pixel_num"]) > 0 and fx["in_query"].shape[0] % 2 == 1


def test_unlabelled_fixture_is_the_constant_without_a_graph():
    fx = load_golden(cgb.FIXTURE_UNLABELLED)
    assert fx["in_labels"].sum() == 0 and (fx["out"] == 1.0).all() and fx["out"].shape[-1] == 2 and "grad_query" not in fx
    assert (cgb.fixture_ref(fx)["out"] == 1.0).all()


def test_workspace_formula():
    L = aoc_amd._lib.lib()
    for m, C, n_slot in ((1, 4, 1), (31, 36, 21), (257, 100, 128), (13689, 100, 128), (25773, 256, 4096)):
        assert L.aoc_proxy_set_match_grad_workspace_bytes(m, C, n_slot) == cgb.set_grad_workspace_bytes(m, C, n_slot)
    # bounded in m: no [m, n_proxy, C] term
    assert L.aoc_proxy_set_match_grad_workspace_bytes(10 ** 7, 100, 128) == L.aoc_proxy_set_match_grad_workspace_bytes(4096, 100, 128)
    assert L.aoc_centroid_avg_grad_workspace_bytes(8, 16) == cgb.centroid_grad_workspace_bytes(8, 16)
    assert L.aoc_proxy_set_match_grad_workspace_bytes(0, 100, 1) == 0 and L.aoc_centroid_avg_grad_workspace_bytes(0, 16) == 0


def _sets(begin, size, off):
    b, s, o = np.asarray(begin, np.int32), np.asarray(size, np.int32), np.asarray(off, np.int64)
    return b, s, o, [x.ctypes.data_as(ctypes.c_void_p) for x in (b, s, o)]


def test_argmin_rejects_bad_arguments_before_any_launch():
    L = aoc_amd._lib.lib()
    p = ctypes.c_void_p(256)                         # never dereferenced: every call here returns before a launch
    *_, (b, s, o) = _sets([0], [4], [0])
    call = lambda q=p, C=36, px=p, out=p, arg=p, n_proxy=8, bb=b, ss=s, oo=o: L.aoc_proxy_set_match_argmin(q, 16, C, px, None, n_proxy, 1, bb, ss, oo, None, out, arg, 1, 1, None)
    assert call(q=None) == INVALID and call(px=None) == INVALID and call(out=None) == INVALID and call(arg=None) == INVALID
    assert call(bb=None) == INVALID and call(ss=None) == INVALID and call(oo=None) == INVALID
    assert call(C=0) == INVALID and call(C=38) == UNSUPPORTED and call(C=260) == UNSUPPORTED
    assert call(n_proxy=3) == INVALID
    *_, (b2, s2, o2) = _sets([0], [65], [0])
    assert call(n_proxy=100, bb=b2, ss=s2, oo=o2) == UNSUPPORTED          # above AOC_MAX_CLUSTERS


def test_set_grad_rejects_bad_arguments_before_any_launch():
    L = aoc_amd._lib.lib()
    p = ctypes.c_void_p(256)
    *_, (b, s, o) = _sets([0], [4], [0])
    bi = np.zeros(1, np.int32)
    bip = bi.ctypes.data_as(ctypes.c_void_p)
    need = L.aoc_proxy_set_match_grad_workspace_bytes(16, 36, 4)

    def call(go=p, T=p, arg=p, q=p, C=36, px=p, n_proxy=8, bb=b, ss=s, oo=o, bidx=bip, n_bias=1, gb=p, ws=p, nbytes=need):
        return L.aoc_proxy_set_match_grad(go, T, arg, 1, q, 16, C, px, n_proxy, 1, bb, ss, oo, bidx, n_bias, p, p, gb, ws, nbytes, None)
    assert call(go=None) == INVALID and call(T=None) == INVALID and call(arg=None) == INVALID and call(q=None) == INVALID and call(px=None) == INVALID
    assert call(bb=None) == INVALID and call(bidx=None) == INVALID and call(n_bias=0) == INVALID
    assert call(C=38) == UNSUPPORTED and call(C=260) == UNSUPPORTED and call(C=0) == INVALID
    assert call(ws=None) == WORKSPACE and call(nbytes=need - 1) == WORKSPACE
    bad = np.asarray([1], np.int32)
    assert call(bidx=bad.ctypes.data_as(ctypes.c_void_p)) == INVALID           # names a bias element outside [0, n_bias)
    *_, (b2, s2, o2) = _sets([0], [65], [0])
    assert call(n_proxy=100, bb=b2, ss=s2, oo=o2) == UNSUPPORTED


def test_centroid_grad_rejects_bad_arguments_before_any_launch():
    L = aoc_amd._lib.lib()
    p = ctypes.c_void_p(256)
    need = L.aoc_centroid_avg_grad_workspace_bytes(4, 16)

    def call(gp=p, C=36, fg=p, nfg=p, off=p, sk=p, lab=p, n_seg=4, kmax=16, cap=100, out=p, rows=100, ws=p, nbytes=need):
        return L.aoc_centroid_avg_grad(gp, C, fg, nfg, off, sk, lab, n_seg, kmax, cap, out, rows, ws, nbytes, None)
    for k in ("gp", "fg", "nfg", "off", "sk", "lab", "out"):
        assert call(**{k: None}) == INVALID, k
    assert call(C=0) == INVALID and call(C=257) == UNSUPPORTED and call(kmax=65, nbytes=1 << 20) == UNSUPPORTED and call(n_seg=0) == INVALID
    assert call(ws=None) == WORKSPACE and call(nbytes=need - 1) == WORKSPACE


def _cpu_args():
    return torch.randn(3, 4, 4, requires_grad=True), torch.randn(3, 4, 4), torch.ones(3, 4, 2)


def test_cluster_train_guards():
    ct = aoc_amd.cluster_train
    ref, q, lab = _cpu_args()
    assert ct.global_matching_cluster is ct.global_matching_cluster2
    with pytest.raises(aoc_amd._lib.AocHipError, match="use_float16"):
        ct.global_matching_cluster2(ref, q, lab)                                # the reference's default argument is use_float16=True
    with pytest.raises(aoc_amd._lib.AocHipError, match="no CPU fallback"):
        ct.global_matching_cluster2(ref, q, lab, 1, 0., None, 1, False, 0)
    with pytest.raises(aoc_amd._lib.AocHipError, match="cluster_train.global_matching_cluster2 is the differentiable form"):
        aoc_amd.matching_train.global_matching_cluster2(ref, q, lab, 1, 0., None, 1, False, 0)
    import inspect
    names = list(inspect.signature(ct.global_matching_cluster2).parameters)
    assert names == ["reference_embeddings", "query_embeddings", "reference_labels", "n_chunks", "dis_bias", "ori_size", "atrous_rate",
                     "use_float16", "atrous_obj_pixel_num", "init_rows", "cluster_num"]
