#!/usr/bin/env python3
"""Golden vectors for the differentiable global matching (tests/test_match_grad_host.py, tests/test_gpu_match_grad.py), recorded by running
the reference's OWN ``global_matching`` (AEM:616-685) and ``global_matching_proxy`` (AEM:336-402) unmodified on the CPU, in float64, under
autograd, with the loss ``(out * weight).sum()`` for a fixed random ``weight``.  The file is imported by path; none of its text is stored.

Recorded per case (match_grad_*.npz): the inputs (embeddings as float16-representable values, stored as float16: widening them is exact;
the one-hot labels as uint8; dis_bias and weight as float32), the arguments, the reference's output and its gradients for the query, the
reference embeddings (or proxies) and the bias, all float64.  The all-unlabelled case has no graph and records the output only.

The embedding scale matters: unit-variance embeddings at C = 100 saturate the sigmoid and every gradient is exactly zero.  With the scales
below the nearest distances are about 1.4 to 2.5 and most outputs lie in (0.05, 0.95).  The gradient jumps where the nearest row changes,
so a fixture must not sit near a tie: a query pixel one of whose best / runner-up gaps is under 120 x the forward distance bound of
tests/match_grad_bounds.py (a few percent of the draws) is drawn again from the same distribution until none is left.
tests/test_match_grad_host.py checks both conditions on the recorded inputs.

    python tests/golden/make_golden_match_grad.py <the reference's AOC-Net directory>
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import match_grad_bounds as mgb  # noqa: E402
warnings.simplefilter("ignore")
torch.set_num_threads(4)


def load(name, path):
    sys.dont_write_bytecode = True                       # never write into the reference tree
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def label_map(rs, h, w, n_obj, unlabelled=0.15, absent=None):
    """-> one-hot [h, w, O] uint8: every present object owns at least one pixel, about `unlabelled` of the pixels belong to nobody."""
    present = [o for o in range(n_obj) if o != absent]
    owner = np.asarray(present)[rs.randint(0, len(present), h * w)]
    owner[rs.permutation(h * w)[:len(present)]] = present
    free = rs.random_sample(h * w) < unlabelled
    free[rs.permutation(h * w)[:len(present)]] = False       # may free an owner's only pixel: re-planted below
    owner[free] = -1
    for o in present:
        if not (owner == o).any():
            owner[rs.randint(0, h * w)] = o
    assert (owner == -1).any() or unlabelled == 0
    lab = np.zeros((h * w, n_obj), np.uint8)
    lab[owner >= 0, owner[owner >= 0]] = 1
    return lab.reshape(h, w, n_obj)


def record(name, fn, ref, query, labels, bias, weight, n_chunks, atrous_rate=1, obj_pix=0):
    ref64 = torch.from_numpy(ref.astype(np.float64)).requires_grad_(True)
    q64 = torch.from_numpy(query.astype(np.float64)).requires_grad_(True)
    b64 = torch.from_numpy(bias.astype(np.float64)).view(-1, 1, 1, 1).requires_grad_(True)       # aocnet.py:144
    lab = torch.from_numpy(labels.astype(np.float64)).clone()                                    # the reference writes into its labels
    out = fn(ref64, q64, lab, n_chunks, b64, None, atrous_rate, False, obj_pix)
    arrays = dict(in_ref=ref, in_query=query, in_labels=labels, in_bias=bias, weight=weight, n_chunks=np.int64(n_chunks),
                  atrous_rate=np.int64(atrous_rate), atrous_obj_pixel_num=np.int64(obj_pix), out=out.detach().numpy().astype(np.float64))
    if out.requires_grad:
        (out * torch.from_numpy(weight.astype(np.float64))).sum().backward()
        arrays.update(grad_query=q64.grad.numpy(), grad_ref=ref64.grad.numpy(), grad_bias=b64.grad.numpy().reshape(-1))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    T = arrays["out"]
    print(f"{name}: {os.path.getsize(path)} bytes, out {tuple(out.shape)}, {float(((T > 0.05) & (T < 0.95)).mean()):.2f} of the outputs in (0.05, 0.95)"
          + (f", |grad_query| up to {np.abs(arrays['grad_query']).max():.3e}" if out.requires_grad else ", no graph"))


def dense_case(aem, name, seed, h, w, C, n_obj, scale, n_chunks=3, atrous_rate=1, obj_pix=0, absent=None, unlabelled=0.15):
    rs = np.random.RandomState(seed)
    ref, query = h16(scale * rs.standard_normal((h, w, C))), h16(scale * rs.standard_normal((h, w, C)))
    labels = label_map(rs, h, w, n_obj, unlabelled, absent) if unlabelled < 1 else np.zeros((h, w, n_obj), np.uint8)
    bias = (0.3 * rs.standard_normal(n_obj)).astype(np.float32)
    weight = rs.standard_normal((1, h, w, n_obj, 1)).astype(np.float32)
    redrawn = 0
    while labels.any():
        fwd = mgb.dense_forward_ref(query.reshape(-1, C).astype(np.float32), ref.reshape(-1, C).astype(np.float32),
                                    mgb.twin_labels(labels, atrous_rate, obj_pix).reshape(-1, n_obj), bias)
        near = ((fwd["gap"] < 1.2 * mgb.GAP_FACTOR * fwd["e_best"]) & (fwd["arg"] >= 0)).any(0).reshape(h, w)
        if not near.any():
            break
        query[near] = h16(scale * rs.standard_normal((int(near.sum()), C)))
        redrawn += int(near.sum())
    print(f"{name}: {redrawn} query pixels drawn again")
    record(name, aem.global_matching, ref, query, labels, bias, weight, n_chunks, atrous_rate, obj_pix)


def proxy_case(aem, name, seed, h, w, C, n_obj, scale):
    rs = np.random.RandomState(seed)
    proxies, query = h16(scale * rs.standard_normal((n_obj, C))), h16(scale * rs.standard_normal((h, w, C)))
    labels = label_map(rs, h, w, n_obj)
    bias = (0.3 * rs.standard_normal(n_obj)).astype(np.float32)
    weight = rs.standard_normal((1, h, w, n_obj, 1)).astype(np.float32)
    record(name, aem.global_matching_proxy, proxies, query, labels, bias, weight, 2)


def main(ref_root):
    aem = load("ref_aem_match_grad", os.path.join(ref_root, "adaptive_embedding_for_matching.py"))
    dense_case(aem, "match_grad_dense_C100_O3", 101, 9, 11, 100, 3, 0.12)
    dense_case(aem, "match_grad_dense_C36_O4", 102, 5, 7, 36, 4, 0.2, n_chunks=1)
    dense_case(aem, "match_grad_dense_C4_O2", 103, 3, 3, 4, 2, 0.6)
    dense_case(aem, "match_grad_dense_C128_O17", 104, 9, 11, 128, 17, 0.1, n_chunks=100)
    dense_case(aem, "match_grad_atrous2", 105, 5, 7, 36, 3, 0.2, atrous_rate=2, obj_pix=0)
    dense_case(aem, "match_grad_atrous2_objpix", 106, 5, 7, 36, 3, 0.2, atrous_rate=2, obj_pix=2)
    dense_case(aem, "match_grad_absent", 107, 5, 7, 36, 4, 0.2, absent=2)
    dense_case(aem, "match_grad_unlabelled", 108, 5, 7, 36, 3, 0.2, unlabelled=1.0)
    proxy_case(aem, "match_grad_proxy", 109, 5, 7, 36, 3, 0.2)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
