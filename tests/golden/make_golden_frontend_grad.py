#!/usr/bin/env python3
"""Golden vectors for the differentiable front end (tests/test_frontend_grad_host.py, tests/test_gpu_frontend_grad.py), recorded by running
the reference's OWN ``calculate_attention_head_p_m`` (networks/layers/attention.py:134-153) and ``foreground2background``
(networks/layers/matching.py:9-23) unmodified on the CPU, in float64, under autograd, with the loss ``(out * weight).sum()`` for a fixed
random ``weight``.  The files are imported by path; none of their text is stored, and nothing is written into the reference tree.

Recorded per case (frontend_grad_*.npz): the inputs (embeddings as float16, one-hot labels as uint8, the other floats as float32), the
reference's outputs and its gradients, all float64.

  frontend_grad_heads_*   ref / prev embeddings [C, h, w], labels [O, 1, h, w]; one object owns no pixel of the previous frame; in the
                          one-object case the object owns every pixel (its negative head divides by epsilon alone)
  frontend_grad_fg2bg_*   dis [O, c, h, w] drawn without ties, so torch.min's winner is the only one

The end-to-end cases (``before_seghead_process`` in training mode) are NOT recorded: the reference's networks/aoc/aocnet.py imports
``networks.p2t.decoding_module``, which the reference tree does not contain, so that branch does not import unmodified (STATUS.md).

    python tests/golden/make_golden_frontend_grad.py <the reference's AOC-Net directory>
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
from make_golden_match_grad import h16, load  # noqa: E402
warnings.simplefilter("ignore")
torch.set_num_threads(4)


def save(name, arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, " + ", ".join(f"{k} {v.shape}" for k, v in arrays.items() if k.startswith(("out", "grad"))))


def heads_case(att, name, seed, h, w, C, n_obj, scale, epsilon=1e-5):
    rs = np.random.RandomState(seed)
    ref, prev = h16(scale * rs.standard_normal((C, h, w))), h16(scale * rs.standard_normal((C, h, w)))
    owner_ref, owner_prev = rs.randint(0, n_obj, (h, w)), rs.randint(0, n_obj, (h, w))
    if n_obj > 1:
        owner_prev[owner_prev == n_obj - 1] = 0                                 # the last object is absent from the previous frame
    lab_ref, lab_prev = (np.eye(n_obj, dtype=np.uint8)[o].transpose(2, 0, 1)[:, None].copy() for o in (owner_ref, owner_prev))
    weight = rs.standard_normal((n_obj, 4 * C)).astype(np.float32)
    r64 = torch.from_numpy(ref.astype(np.float64)).requires_grad_(True)
    p64 = torch.from_numpy(prev.astype(np.float64)).requires_grad_(True)
    outs = att.calculate_attention_head_p_m(r64.unsqueeze(0).expand(n_obj, -1, -1, -1), torch.from_numpy(lab_ref.astype(np.float64)),
                                            p64.unsqueeze(0).expand(n_obj, -1, -1, -1), torch.from_numpy(lab_prev.astype(np.float64)),
                                            epsilon=float(np.float32(epsilon)))   # the kernels take epsilon as a float
    (outs[0] * torch.from_numpy(weight.astype(np.float64))).sum().backward()
    save(name, dict(in_ref=ref, in_prev=prev, in_ref_label=lab_ref, in_prev_label=lab_prev, weight=weight, epsilon=np.float32(epsilon),
                    out_head=outs[0].detach().numpy(), grad_ref=r64.grad.numpy(), grad_prev=p64.grad.numpy()))


def fg2bg_case(mt, name, seed, h, w, n_obj, n_ch):
    rs = np.random.RandomState(seed)
    dis = np.tanh(rs.standard_normal((n_obj, n_ch, h, w))).astype(np.float32)
    assert np.unique(dis).size == dis.size, "a tie: draw again with another seed"
    weight = rs.standard_normal((n_obj, 1, h, w)).astype(np.float32)
    d64 = torch.from_numpy(dis.astype(np.float64)).requires_grad_(True)
    out = mt.foreground2background(d64, n_obj)
    (out * torch.from_numpy(weight.astype(np.float64))).sum().backward()
    save(name, dict(in_dis=dis, weight=weight, out=out.detach().numpy(), grad_dis=d64.grad.numpy()))


def main(ref_root):
    layers = os.path.join(ref_root, "complete_project", "AOCNet", "networks", "layers")
    att = load("ref_attention_frontend_grad", os.path.join(layers, "attention.py"))
    mt = load("ref_matching_frontend_grad", os.path.join(layers, "matching.py"))
    heads_case(att, "frontend_grad_heads_C36_O4", 301, 11, 13, 36, 4, 0.2)
    heads_case(att, "frontend_grad_heads_C100_O1", 302, 5, 7, 100, 1, 0.12)
    fg2bg_case(mt, "frontend_grad_fg2bg_O4_c1", 303, 11, 13, 4, 1)
    fg2bg_case(mt, "frontend_grad_fg2bg_O3_c6", 304, 5, 7, 3, 6)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
