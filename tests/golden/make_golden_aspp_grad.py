#!/usr/bin/env python3
"""Golden vectors for the differentiable ASPP (tests/test_aspp_grad_host.py, tests/test_gpu_aspp_grad.py), recorded by running the reference's
OWN ``ASPP`` (networks/layers/aspp.py:33-78) UNMODIFIED on the CPU, in float64, under autograd, with the loss ``(out * weight).sum()`` for a fixed
random ``weight``.  None of the reference's text is stored, and nothing is written into its tree.

The convolution weights are NOT stored: recorder and tests draw all of them from one numpy seed (aspp_grad_bounds.drawn_weights).  Recorded per
case (aspp_grad_*.npz): the float16 inputs (``in_x``, ``in_weight``), the small parameters (every GCT's and GroupNorm's; float16), the loss, and
the float64 gradients of x, of every GCT and GroupNorm parameter, of the pooled convolution's weight and of ``aspp1.atrous_conv.weight``.
float64 does not compress, so the three large gradients keep a regular part (aspp_grad_bounds.recorded_view): every fourth channel of
``grad_x``, every 32nd row of the two weight gradients.  A fixture must not sit near a ReLU's kink in float32: the recorder refuses a case with
an element of a branch whose float64 z lies within the float32 bound of 0 (aspp_grad_bounds.cat_grad_ref's ``undecided``).

    python tests/golden/make_golden_aspp_grad.py <the reference's complete_project/AOCNet directory>
"""
import importlib
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True                            # never write into the reference tree
from make_golden_decoder_tail import load_reference  # noqa: E402
import aspp_grad_bounds as agb  # noqa: E402
warnings.simplefilter("ignore")
torch.set_num_threads(4)
f32, f64 = np.float32, np.float64
RECORDED_WEIGHTS = ("global_avg_pool.1.weight", "aspp1.atrous_conv.weight")


def h16(a):
    return np.asarray(a, f32).astype(np.float16)


def case(ref_aspp, name, seed):
    N, h, w = agb.FIXTURE_SHAPES[name]
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    net = ref_aspp.ASPP()                                 # the reference's constructor and forward, unmodified
    small = {}
    for k, p in net.named_parameters():
        leaf = k.split(".")[-1]
        if leaf == "alpha" or (leaf == "weight" and p.dim() == 1):
            small[k] = h16(rs.uniform(0.5, 1.5, tuple(p.shape)))
        elif leaf in ("gamma", "beta", "bias"):
            small[k] = h16(0.5 * rs.standard_normal(tuple(p.shape)))
    fx = {"p_" + k: v for k, v in small.items()}
    agb.load_fixture_parameters(net, fx)
    x, weight = h16(rs.standard_normal((N, 512, h, w))), h16(rs.standard_normal((N, 256, h, w)))
    lx = torch.from_numpy(x.astype(f64)).requires_grad_(True)
    out = net(lx)
    loss = (out * torch.from_numpy(weight.astype(f64))).sum()
    loss.backward()
    # no ReLU element of a branch within the float32 bound of its kink
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    names = ("aspp1", "aspp2", "aspp3", "aspp4")
    gct = lambda pre: [sd[f"{pre}GCT.{k}"].reshape(-1) for k in ("alpha", "gamma", "beta")]
    al, ga, be = ([gct(n + ".")[i] for n in names] for i in range(3))
    vs, mean = agb.front_forward64(lx.detach().reshape(N, 512, -1), al, ga, be, 1e-5)
    us = []
    for n, d, v in zip(names, (1, 6, 12, 18), vs):
        wgt = sd[n + ".atrous_conv.weight"]
        us.append(torch.nn.functional.conv2d(v.reshape(N, 512, h, w), wgt, None, 1, 0 if wgt.shape[2] == 1 else d, d).reshape(N, 128, -1).numpy().astype(f32))
    s = dict(us=us, groups=32, weights=np.stack([small[n + ".bn.weight"] for n in names]).astype(f32), biases=np.stack([small[n + ".bn.bias"] for n in names]).astype(f32),
             gn_eps=1e-5, tail=(mean @ sd["global_avg_pool.1.weight"].reshape(128, 512).t()).numpy().astype(f32), gct_alpha=small["GCT.alpha"].reshape(-1).astype(f32),
             gct_gamma=small["GCT.gamma"].reshape(-1).astype(f32), gct_beta=small["GCT.beta"].reshape(-1).astype(f32), gct_eps=1e-5,
             grad_out=np.zeros((N, 640, h * w), f32))
    _, und = agb.cat_grad_ref(**agb.back_ref_args(s, agb.back_saved32(s)))
    assert sum(int(u.sum()) for u in und) == 0, f"{name}: elements within the float32 bound of a ReLU's kink; take another seed"
    arrays = dict(fx, in_x=x, in_weight=weight, loss=np.asarray(float(loss)), seed=np.asarray(seed))
    arrays["grad_x"] = agb.recorded_view("x", lx.grad).numpy()
    for k, p in net.named_parameters():
        if k in small or k in RECORDED_WEIGHTS:
            arrays["grad_" + k] = agb.recorded_view(k, p.grad).numpy().astype(f64)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, loss {float(loss):.6f}, {len(arrays)} arrays")
    assert os.path.getsize(path) < 250000


def main(ref_root):
    load_reference(ref_root)
    ref_aspp = importlib.import_module("networks.layers.aspp")
    case(ref_aspp, "aspp_grad_O3", 51)
    case(ref_aspp, "aspp_grad_O1", 52)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
