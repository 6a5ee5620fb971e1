#!/usr/bin/env python3
"""Golden vectors for the differentiable decoder forms (tests/test_decoder_grad_host.py), recorded by running the reference's OWN
``Bottleneck`` (networks/layers/gct.py:38-91) followed by its ``IA_gate`` (networks/layers/attention.py:7-17) -- the pair of
decoding_module.py:195-196 -- on the CPU, in float64, under autograd, with the loss ``(out * weight).sum()`` for a fixed random ``weight``.
The files are imported by path; none of their text is stored, and nothing is written into the reference tree.  gct.py imports
``networks.p2t.center_module``, which the reference does not ship: an empty stand-in module object is registered under that name (nothing of
it is called), as tests/golden/make_golden_gates_grad.py does.

The convolution weights are NOT stored: recorder and test draw them from the same numpy seed (decoder_grad_bounds.conv_weights).  Recorded
per case (decoder_grad_*.npz): the float16 inputs (``in_x``, ``in_head``, ``in_weight``), the GroupNorm, GCT and gate parameters (rounded to
float16, stored as float32), the loss, and the float64 gradients of x, the head and those parameters -- no gradient of a convolution weight
and no output, which keeps each file below the largest existing fixture.

    python tests/golden/make_golden_decoder_grad.py <the reference's AOC-Net directory>
    python tests/golden/make_golden_decoder_grad.py --seeds       # the seeds of decoder_grad_bounds.GN_CASES (needs no reference)
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
import decoder_grad_bounds as dgb  # noqa: E402
warnings.simplefilter("ignore")
torch.set_num_threads(4)
f64 = np.float64


def save(name, arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 250_000, f"{name}: {size} bytes"
    print(f"{name}: {size} bytes, " + ", ".join(f"{k} {np.shape(v)}" for k, v in arrays.items() if k.startswith("grad")))


def bottleneck_case(gct, att, name, seed, O, inplanes, outplanes, D, h, w):
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    blk, gate = gct.Bottleneck(inplanes, outplanes), att.IA_gate(D, outplanes)
    assert (blk.downsample is not None) == (inplanes != outplanes)
    dgb.randomize_small_parameters(blk, gate, rs)
    dgb.set_conv_weights(blk, seed)
    x, head, weight = h16(rs.standard_normal((O, inplanes, h, w))), h16(rs.standard_normal((O, D))), h16(rs.standard_normal((O, outplanes, h, w)))
    leaves = [torch.from_numpy(a.astype(f64)).requires_grad_(True) for a in (x, head)]
    out = gate(blk(leaves[0]), leaves[1])                 # the reference's forwards, unmodified
    loss = (out * torch.from_numpy(weight.astype(f64))).sum()
    loss.backward()
    named = [("blk." + k, p) for k, p in blk.named_parameters() if "conv" not in k and not k.startswith("downsample.0")]
    named += [("gate." + k, p) for k, p in gate.named_parameters()]
    assert all(p.grad is not None for _, p in named)
    params = {"w_" + k.replace(".", "__"): p.detach().numpy().astype(np.float32) for k, p in named}
    grads = {"grad_w_" + k.replace(".", "__"): p.grad.numpy() for k, p in named}
    save(name, dict(in_x=x, in_head=head, in_weight=weight, seed=np.int64(seed), planes=np.array([inplanes, outplanes]), loss=np.float64(loss.item()),
                    grad_x=leaves[0].grad.numpy(), grad_head=leaves[1].grad.numpy(), **params, **grads))


def find_seeds():
    """per case of GN_CASES the first seed for which no element of a ReLU variant is undecided"""
    for (N, C, groups, hw) in dgb.GN_CASES:
        for seed in range(1000):
            s = dgb.gn_case(N, C, groups, hw, seed)
            if all(int(dgb.groupnorm_relu_grad_ref(**dgb.gn_args(s, v, groups))[1].sum()) == 0 for v in dgb.GN_VARIANTS if v[1]):
                print(f"({N}, {C}, {groups}, {hw}): {seed}")
                break
        else:
            raise SystemExit(f"{(N, C, groups, hw)}: no seed below 1000")


def main(ref_root):
    root = os.path.join(ref_root, "complete_project", "AOCNet")
    att = load("ref_attention_decoder_grad", os.path.join(root, "networks", "layers", "attention.py"))
    cm = types.ModuleType("networks.p2t.center_module")
    cm.SpatialProp = type("SpatialProp", (), {})
    sys.modules.setdefault("networks", types.ModuleType("networks"))
    sys.modules.setdefault("networks.p2t", types.ModuleType("networks.p2t"))
    sys.modules.setdefault("networks.p2t.center_module", cm)
    gct = load("ref_gct_decoder_grad", os.path.join(root, "networks", "layers", "gct.py"))
    bottleneck_case(gct, att, dgb.BOTTLENECK_FIXTURES[0], 501, 2, 64, 128, 10, 5, 7)
    bottleneck_case(gct, att, dgb.BOTTLENECK_FIXTURES[1], 502, 3, 128, 128, 6, 7, 5)


if __name__ == "__main__":
    if sys.argv[1] == "--seeds":
        find_seeds()
    else:
        main(os.path.abspath(sys.argv[1]))
