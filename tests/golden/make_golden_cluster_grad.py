#!/usr/bin/env python3
"""Golden vectors for the differentiable cluster matching (tests/test_cluster_grad_host.py, tests/test_gpu_cluster_grad.py), recorded by
running the reference's OWN ``global_matching_cluster2`` (networks/layers/matching.py:1324-1404 over 506-640) unmodified on the CPU, in
float64, under autograd, with the loss ``(out * weight).sum()`` for a fixed random ``weight``.  The file is imported by path; none of its
text is stored.

``kmeans2`` in the loaded module is replaced by ``make_golden.recording_kmeans2`` behind a cast: the data is cast to float32 before the
call (exact: the inputs are float16-representable) and the code book is widened back to float64 after it, so the clustering is the
float32 one the device chain reproduces bit for bit while the gradients are float64.  ``np.random.seed(seed)`` precedes the call.

Recorded per case (cluster_grad_*.npz): the inputs (embeddings as float16, one-hot labels as uint8, dis_bias and weight as float32), the
arguments and the seed, the km log (per kmeans2 call the drawn rows, the labels and the code book), the reference's output and its
gradients for the query, the reference embeddings and the bias, all float64.  The all-unlabelled case has no graph: output only.

The embedding scale keeps most outputs in (0.05, 0.95); a query pixel one of whose best / runner-up gaps is under 120 x the forward
distance bound of tests/cluster_grad_bounds.py is drawn again (the clustering depends on the reference embeddings alone, so it stays);
bit-equal code-book entries (cluster_grad_dup_empty) count as one candidate there: whichever wins, value and gradients are the same.
tests/test_cluster_grad_host.py re-checks the conditions on the recorded inputs.

    python tests/golden/make_golden_cluster_grad.py <the reference's AOC-Net directory>
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True                            # never write into the reference tree
import cluster_grad_bounds as cgb  # noqa: E402
import make_golden as mg  # noqa: E402  (recording_kmeans2 and its KM_LOG)
from make_golden_match_grad import h16, label_map, load  # noqa: E402
warnings.simplefilter("ignore")
torch.set_num_threads(4)


def kmeans2_float32(data, k, iter=10, minit='random', **kw):
    data32 = np.ascontiguousarray(np.asarray(data, np.float32))
    assert np.array_equal(data32.astype(np.float64), data)
    centroid, label = mg.recording_kmeans2(data32, k, iter=iter, minit=minit, **kw)
    return centroid.astype(np.float64), label


def run(fn, ref, query, labels, bias, weight, seed, atrous_rate, obj_pix):
    ref64 = torch.from_numpy(ref.astype(np.float64)).requires_grad_(True)
    q64 = torch.from_numpy(query.astype(np.float64)).requires_grad_(True)
    b64 = torch.from_numpy(bias.astype(np.float64)).view(-1, 1, 1, 1).requires_grad_(True)       # aocnet.py:144
    lab = torch.from_numpy(labels.astype(np.float64)).clone()                                    # the reference writes into its labels
    del mg.KM_LOG[:]
    np.random.seed(seed)
    out = fn(ref64, q64, lab, 3, b64, None, atrous_rate, False, obj_pix)
    arrays = dict(in_ref=ref, in_query=query, in_labels=labels, in_bias=bias, weight=weight, n_chunks=np.int64(3), seed=np.int64(seed),
                  cluster_num=np.int64(16), atrous_rate=np.int64(atrous_rate), atrous_obj_pixel_num=np.int64(obj_pix),
                  out=out.detach().numpy().astype(np.float64), km_calls=np.int64(len(mg.KM_LOG)))
    for i, e in enumerate(mg.KM_LOG):
        arrays[f"km{i}_rows"], arrays[f"km{i}_labels"], arrays[f"km{i}_centroid"] = e["rows"], e["labels"], e["centroid"]
    if out.requires_grad:
        (out * torch.from_numpy(weight.astype(np.float64))).sum().backward()
        arrays.update(grad_query=q64.grad.numpy(), grad_ref=ref64.grad.numpy(), grad_bias=b64.grad.numpy().reshape(-1))
    return arrays


def case(mt, name, seed, h, w, C, n_obj, scale, atrous_rate=1, obj_pix=0, absent=None, unlabelled=0.15, few=None, dup=False):
    rs = np.random.RandomState(seed)
    ref, query = h16(scale * rs.standard_normal((h, w, C))), h16(scale * rs.standard_normal((h, w, C)))
    labels = label_map(rs, h, w, n_obj, unlabelled, absent) if unlabelled < 1 else np.zeros((h, w, n_obj), np.uint8)
    if few is not None:                                    # object `few` keeps 5 pixels: fewer than 16, so K sticks at 5 for the objects after it
        ys, xs = np.nonzero(labels[:, :, few])
        for y, x in list(zip(ys, xs))[5:]:
            labels[y, x, few] = 0
            labels[y, x, (few + 1) % n_obj] = 1
    if dup:                                                # object 0's rows are copies of three vectors: its 16 drawn rows repeat, the code book
        ys, xs = np.nonzero(labels[:, :, 0])               # holds bit-equal entries and the later copy of each ends as an empty cluster
        three = h16(scale * rs.standard_normal((3, C)))
        for i, (y, x) in enumerate(zip(ys, xs)):
            ref[y, x] = three[i % 3]
    bias = (0.3 * rs.standard_normal(n_obj)).astype(np.float32)
    weight = rs.standard_normal((1, h, w, n_obj, 2)).astype(np.float32)
    redrawn = 0
    for _ in range(50):                                    # a pixel that stays near a tie for 50 draws means the case itself is wrong
        arrays = run(mt.global_matching_cluster2, ref, query, labels, bias, weight, seed, atrous_rate, obj_pix)
        if not labels.any():
            break
        fwd = cgb.fixture_ref({k: (v.astype(np.float32) if v.dtype == np.float16 else v) for k, v in arrays.items()})["fwd"]
        near = ((fwd["gap"] < 1.2 * cgb.GAP_FACTOR * fwd["e_best"]) & (fwd["arg"] >= 0)).any(0).reshape(h, w)
        if not near.any():
            break
        query[near] = h16(scale * rs.standard_normal((int(near.sum()), C)))
        redrawn += int(near.sum())
    else:
        raise AssertionError(name + ": near-ties remain after 50 redraws")
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    T = arrays["out"]
    print(f"{name}: {os.path.getsize(path)} bytes, out {T.shape}, {redrawn} query pixels drawn again, {int(arrays['km_calls'])} kmeans2 calls, "
          f"{float(((T > 0.05) & (T < 0.95)).mean()):.2f} of the outputs in (0.05, 0.95)"
          + (f", |grad_ref| up to {np.abs(arrays['grad_ref']).max():.3e}" if "grad_ref" in arrays else ", no graph"))


def main(ref_root):
    mt = load("ref_matching_cluster_grad", os.path.join(ref_root, "complete_project", "AOCNet", "networks", "layers", "matching.py"))
    mt.kmeans2 = kmeans2_float32
    case(mt, "cluster_grad_C36_O3", 201, 9, 11, 36, 3, 0.2)
    case(mt, "cluster_grad_C100_O4_bias", 202, 11, 13, 100, 4, 0.12, few=1)
    case(mt, "cluster_grad_absent", 203, 9, 11, 36, 4, 0.2, absent=2)
    case(mt, "cluster_grad_atrous2", 204, 11, 13, 36, 3, 0.2, atrous_rate=2, obj_pix=3)
    case(mt, "cluster_grad_dup_empty", 205, 9, 11, 36, 3, 0.2, dup=True)
    case(mt, "cluster_grad_unlabelled", 206, 5, 7, 36, 3, 0.2, unlabelled=1.0)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
