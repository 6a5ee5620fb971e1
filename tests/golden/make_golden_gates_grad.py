#!/usr/bin/env python3
"""Golden vectors for the differentiable calibration gates (tests/test_gates_grad_host.py), recorded by running the reference's OWN
``IA_gate`` (networks/layers/attention.py:7-17), ``GCT`` (networks/layers/gct.py:7-36) and ``conditioning_block``
(networks/aoc/conditioning_layer.py:50-86) on the CPU, in float64, under autograd, with the loss ``(out * weight).sum()`` for a fixed random
``weight``.  The files are imported by path; none of their text is stored, and nothing is written into the reference tree.

  * gct.py imports ``networks.p2t.center_module``, which the reference does not ship: an empty stand-in module object is registered under
    that name (nothing of it is called), as tests/golden/make_golden_r2.py does;
  * conditioning_block.forward reads ``CL_1`` / ``CL_2`` / ``CL_3`` and conditioning_layer.forward reads ``mlp_layer`` as module GLOBALS: the
    reference's forward runs UNMODIFIED once those four names exist in its module, as tests/golden/make_golden_r6.py does -- ``CL_1`` = the
    block's own reference layer, ``mlp_layer`` = its MLP, ``CL_2`` / ``CL_3`` = the documented vector repair ``v -> CL_k.mlp_layer(v)``.

Recorded per case (gates_grad_*.npz): float32-representable inputs and parameters (float16 where the name starts with ``in_``; the
parameters are rounded to float16 and stored as float32), the output, and every input and parameter gradient, float64.  A gradient the
reference's autograd leaves at None -- ``phi_layer`` of every conditioning layer (CLB:36 compares), the unused halves of CL_2 / CL_3 -- is
recorded under ``none_grads``, a list of parameter names.

The conditioning cases assert that the k-th largest score is separated from both neighbours by at least 100 times the float32 score
bound of tests/float64_bounds.cond_scores_ref, so a float32 forward draws the same mask.

    python tests/golden/make_golden_gates_grad.py <the reference's AOC-Net directory>
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True                            # never write into the reference tree
from make_golden_match_grad import h16, load  # noqa: E402
import float64_bounds as fb  # noqa: E402
warnings.simplefilter("ignore")
torch.set_num_threads(4)
torch.set_default_dtype(torch.float64)
f64 = np.float64


def save(name, arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 100_000, f"{name}: {size} bytes"
    print(f"{name}: {size} bytes, " + ", ".join(f"{k} {np.shape(v)}" for k, v in arrays.items() if k.startswith(("out", "grad"))))


def round_parameters(module):
    with torch.no_grad():
        for prm in module.parameters():
            prm.copy_(torch.from_numpy(h16(prm.numpy()).astype(f64)))


def record(module, inputs, weight):
    """-> out, the inputs' gradients, {parameter: gradient}, the names whose gradient is None"""
    leaves = [torch.from_numpy(a.astype(f64)).requires_grad_(True) for a in inputs]
    out = module(*leaves)
    (out * torch.from_numpy(weight.astype(f64))).sum().backward()
    grads = {"grad_w_" + k.replace(".", "__"): p.grad.numpy() for k, p in module.named_parameters() if p.grad is not None}
    none = [k for k, p in module.named_parameters() if p.grad is None]
    params = {"w_" + k.replace(".", "__"): p.detach().numpy().astype(np.float32) for k, p in module.named_parameters()}
    return out.detach().numpy(), [t.grad.numpy() for t in leaves], params, grads, none


def ia_case(att, name, seed, O, c, D, h, w):
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    gate = att.IA_gate(D, c)
    round_parameters(gate)
    x, head, weight = h16(rs.standard_normal((O, c, h, w))), h16(rs.standard_normal((O, D))), h16(rs.standard_normal((O, c, h, w)))
    out, (gx, gh), params, grads, none = record(gate, (x, head), weight)
    assert not none
    save(name, dict(in_x=x, in_head=head, in_weight=weight, out=out, grad_x=gx, grad_head=gh, **params, **grads))


def gct_case(gct, name, seed, N, C, h, w, mode, after_relu):
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    m = gct.GCT(C, epsilon=float(np.float32(1e-5)), mode=mode, after_relu=after_relu)      # the kernels take epsilon as a float
    with torch.no_grad():                                  # away from the constructor's gamma = beta = 0, where half the gradients vanish
        m.alpha.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, (1, C, 1, 1))))
        m.gamma.copy_(torch.from_numpy(rs.standard_normal((1, C, 1, 1))))
        m.beta.copy_(torch.from_numpy(0.5 * rs.standard_normal((1, C, 1, 1))))
    round_parameters(m)
    x, weight = h16(rs.standard_normal((N, C, h, w))), h16(rs.standard_normal((N, C, h, w)))
    out, (gx,), params, grads, none = record(m, (x,), weight)
    assert not none
    save(name, dict(in_x=x, in_weight=weight, out=out, grad_x=gx, epsilon=np.float64(m.epsilon), mode=np.array(mode), after_relu=np.array(after_relu),
                    **params, **grads))


def block_case(clb, name, seed, N, C, D, h, w, beta):
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    blk = clb.conditioning_block(in_dim=C, proxy_dim=D, beta_percentage=beta)
    round_parameters(blk)
    x, head, weight = h16(rs.standard_normal((N, C, h, w))), h16(rs.standard_normal((N, D))), h16(rs.standard_normal((N, C, h, w)))
    clb.CL_1 = blk.CL_1
    clb.mlp_layer = blk.CL_1.mlp_layer
    clb.CL_2 = lambda v, _b=blk: _b.CL_2.mlp_layer(v)
    clb.CL_3 = lambda v, _b=blk: _b.CL_3.mlp_layer(v)
    out, (gx, gh), params, grads, none = record(blk, (x, head), weight)             # the reference's forward, CLB:66-86
    assert {"CL_1.phi_layer.weight", "CL_1.phi_layer.bias"} <= set(none), none
    # the mask of a float32 forward: the k-th largest score against its two neighbours
    k = int(beta * w * h)
    z = torch.from_numpy(x.astype(f64)).reshape(N, C, h * w)
    phi_w, phi_b = blk.CL_1.phi_layer.weight.detach().reshape(-1), blk.CL_1.phi_layer.bias.detach().reshape(())
    s, _, _, _, tol = fb.cond_scores_ref(z, phi_w, phi_b, k)
    top = torch.sort(s, dim=1, descending=True).values
    gaps = [top[:, k - 1] - top[:, k]] + ([top[:, k - 2] - top[:, k - 1]] if k > 1 else [])
    assert all((g >= 100 * tol.max()).all() for g in gaps), f"{name}: the k-th largest score is too close to a neighbour: draw again with another seed"
    save(name, dict(in_x=x, in_head=head, in_weight=weight, out=out, grad_x=gx, grad_head=gh, beta=np.float64(beta), none_grads=np.array(none),
                    **params, **grads))


def main(ref_root):
    root = os.path.join(ref_root, "complete_project", "AOCNet")
    att = load("ref_attention_gates_grad", os.path.join(root, "networks", "layers", "attention.py"))
    clb = load("ref_clb_gates_grad", os.path.join(root, "networks", "aoc", "conditioning_layer.py"))
    cm = types.ModuleType("networks.p2t.center_module")
    cm.SpatialProp = type("SpatialProp", (), {})
    sys.modules.setdefault("networks", types.ModuleType("networks"))
    sys.modules.setdefault("networks.p2t", types.ModuleType("networks.p2t"))
    sys.modules.setdefault("networks.p2t.center_module", cm)
    gct = load("ref_gct_gates_grad", os.path.join(root, "networks", "layers", "gct.py"))
    ia_case(att, "gates_grad_ia_O3", 401, 3, 16, 10, 7, 9)
    ia_case(att, "gates_grad_ia_O1", 402, 1, 5, 23, 9, 11)
    gct_case(gct, "gates_grad_gct_l2", 403, 3, 16, 7, 9, "l2", False)
    gct_case(gct, "gates_grad_gct_l1", 404, 2, 7, 9, 11, "l1", False)
    block_case(clb, "gates_grad_block_N3", 405, 3, 12, 20, 9, 11, 0.3)
    block_case(clb, "gates_grad_block_N1", 406, 1, 8, 5, 9, 11, 0.5)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
