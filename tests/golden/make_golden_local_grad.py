#!/usr/bin/env python3
"""Golden vectors for the differentiable local matching (tests/test_local_grad_host.py, tests/test_gpu_local_grad.py), recorded by running
the reference's OWN ``local_matching`` (AEM:968-1060) unmodified on the CPU, in float64, under autograd, with the loss
``(out * weight).sum()`` for a fixed random ``weight``.  The file is imported by path; none of its text is stored.

Every case runs with allow_parallel=True.  The reference's for-loop path (AEM:875-919) shadows both embeddings with its loop variables:
its "distances" are computed from loop integers and the query gets no gradient, so nothing is recorded from it.

Recorded per case (local_grad_*.npz): the inputs (embeddings as float16-representable values, stored as float16: widening them is exact;
the one-hot labels as uint8; dis_bias and weight as float32), the arguments (ori_size (0, 0) = None), the reference's output and its
gradients for the query, the previous frame's embedding and the bias, all float64.

The embedding scale is 1 / sqrt(C): unit-variance embeddings saturate the sigmoid and every gradient is exactly zero.  The gradient jumps
where the nearest pixel changes, so a fixture must not sit near a tie: a query pixel one of whose best / runner-up gaps (at matching
resolution) is under 120 x the forward distance bound of tests/local_grad_bounds.py is drawn again from the same distribution until none
is left.  Map sizes are odd, so the stride-2 down-sample (AEM:938-941) has weights 0 and 1 only.  tests/test_local_grad_host.py checks the
conditions on the recorded inputs.  In four dimensions the nearest of a window's candidates lies at a distance of about 0.1, where
T = 2 sigmoid(d + b) - 1 is near zero for b around 0: the C = 4 case draws its biases around 0.6.

    python tests/golden/make_golden_local_grad.py <the reference's AOC-Net directory>
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import local_grad_bounds as lgb  # noqa: E402
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
    """-> one-hot [h, w, O] uint8: about `unlabelled` of the pixels belong to nobody, an absent object owns none."""
    present = [o for o in range(n_obj) if o != absent]
    owner = np.asarray(present)[rs.randint(0, len(present), h * w)]
    owner[rs.random_sample(h * w) < unlabelled] = -1
    lab = np.zeros((h * w, n_obj), np.uint8)
    lab[owner >= 0, owner[owner >= 0]] = 1
    return lab.reshape(h, w, n_obj)


def case(aem, name, seed, h, w, C, n_obj, radii, ori_size=None, atrous_rate=1, down=True, absent=None, unlabelled=0.15, bias_mean=0.0):
    rs = np.random.RandomState(seed)
    s = 1.0 / np.sqrt(C)
    prev, query = h16(s * rs.standard_normal((h, w, C))), h16(s * rs.standard_normal((h, w, C)))
    labels = label_map(rs, h, w, n_obj, unlabelled, absent) if unlabelled < 1 else np.zeros((h, w, n_obj), np.uint8)
    bias = (bias_mean + 0.3 * rs.standard_normal(n_obj)).astype(np.float32)
    Ho, Wo = (h, w) if ori_size is None else ori_size
    weight = rs.standard_normal((1, Ho, Wo, n_obj, len(radii))).astype(np.float32)
    arrays = dict(in_prev=prev, in_query=query, in_labels=labels, in_bias=bias, weight=weight, multi_local_distance=np.asarray(radii, np.int64),
                  ori_size=np.asarray(ori_size if ori_size is not None else (0, 0), np.int64), atrous_rate=np.int64(atrous_rate),
                  allow_downsample=np.bool_(down))
    redrawn = 0
    while labels.any():
        fx = {k: (v.astype(np.float32) if v.dtype == np.float16 else v) for k, v in arrays.items()}
        ref = lgb.fixture_ref(fx)
        fwd = ref["fwd"]
        near = ((fwd["gap"] < 1.2 * lgb.GAP_FACTOR * fwd["e_best"]) & (fwd["arg"] >= 0)).any((0, 1)).reshape(-1)
        if not near.any():
            break
        full = near if ref["Wd"] is None else (ref["Wd"][near] != 0).any(0)       # the full-resolution pixels behind them
        query.reshape(-1, C)[full] = h16(s * rs.standard_normal((int(full.sum()), C)))
        redrawn += int(full.sum())
    print(f"{name}: {redrawn} query pixels drawn again")
    p64 = torch.from_numpy(prev.astype(np.float64)).requires_grad_(True)
    q64 = torch.from_numpy(query.astype(np.float64)).requires_grad_(True)
    b64 = torch.from_numpy(bias.astype(np.float64)).view(-1, 1, 1, 1).requires_grad_(True)       # aocnet.py:144
    lab = torch.from_numpy(labels.astype(np.float64)).clone()
    out = aem.local_matching(p64, q64, lab, b64, list(radii), ori_size, atrous_rate, False, down, True)
    (out * torch.from_numpy(weight.astype(np.float64))).sum().backward()
    arrays.update(out=out.detach().numpy().astype(np.float64), grad_query=q64.grad.numpy(), grad_prev=p64.grad.numpy(),
                  grad_bias=b64.grad.numpy().reshape(-1))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    T = arrays["out"]
    print(f"{name}: {os.path.getsize(path)} bytes, out {tuple(out.shape)}, {float(((T > 0.05) & (T < 0.95)).mean()):.2f} of the outputs in (0.05, 0.95), "
          f"{float((T == 1.0).mean()):.2f} exactly 1, |grad_query| up to {np.abs(arrays['grad_query']).max():.3e}")


def main(ref_root):
    aem = load("ref_aem_local_grad", os.path.join(ref_root, "adaptive_embedding_for_matching.py"))
    case(aem, "local_grad_down_O3", 201, 9, 11, 36, 3, [1, 2, 3])
    case(aem, "local_grad_nodown_O3", 202, 9, 11, 36, 3, [1, 2, 3], down=False)
    case(aem, "local_grad_down_orisize_C100", 203, 13, 15, 100, 4, [2, 4, 6, 8, 10, 12], ori_size=(13, 29))
    case(aem, "local_grad_atrous2", 204, 9, 11, 36, 3, [2, 4, 5], atrous_rate=2, down=False)
    case(aem, "local_grad_absent", 205, 7, 9, 4, 2, [1, 3], absent=1, bias_mean=0.6)
    case(aem, "local_grad_unlabelled", 206, 5, 7, 4, 3, [1, 2], unlabelled=1.0)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
