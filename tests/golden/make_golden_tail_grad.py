#!/usr/bin/env python3
"""Golden vectors for the differentiable decoder tail (tests/test_tail_grad_host.py, tests/test_gpu_tail_grad.py), recorded by running the
reference's OWN ``CalibrationDecoding.decoder_final``, ``IA_logit`` (twice) and ``augment_background_logit`` (networks/aoc/decoding_module.py:
151-190, 213-225) UNMODIFIED on the CPU, in float64, under autograd, with the loss ``(pred * weight).sum()`` for a fixed random ``weight``.
The methods run on the ``__new__`` holder of make_golden_decoder_tail.py (the reference's constructor cannot run), which carries exactly the
attributes they read, built by ``tail_grad_bounds.build_decoder`` from the reference's own ``GCT`` and ``IA_gate``.  None of the reference's
text is stored, and nothing is written into its tree.

The convolution weights are NOT stored: recorder and tests draw them from the same numpy seed (tail_grad_bounds.build_decoder).  Recorded per
case (tail_grad_*.npz): the float16 inputs (``in_x``, ``in_low_level_feat``, ``in_IA_head``, ``in_weight``), the small parameters (GCT_sc, the three
GroupNorms, IA10, IA11, both IA_final layers; float16), the loss, the selected object per pixel, and the float64
gradients of x, low_level_feat, IA_head and those parameters -- no gradient of a convolution weight and no activation.

A fixture must not sit near a tie of the background minimum (the gradient jumps there): the recorder refuses a case with a pixel whose two
smallest bg logits are closer than twice the float32 forward bound (tail_grad_bounds.undecided_pixels).

    python tests/golden/make_golden_tail_grad.py <the reference's complete_project/AOCNet directory>
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
from make_golden_decoder_tail import holder, load_reference  # noqa: E402
import tail_grad_bounds as tgb  # noqa: E402
warnings.simplefilter("ignore")
torch.set_num_threads(4)
f64 = np.float64


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def case(mods, name, seed, N, h, w, H, W):
    gct, att, dm = mods
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    d = tgb.FIXTURE_DIMS
    dec = tgb.build_decoder(holder(dm), gct.GCT, att.IA_gate, seed, **d)
    x, low, head = h16(rs.standard_normal((N, d["Ce"], h, w))), h16(rs.standard_normal((N, d["Cl"], H, W))), h16(0.5 * rs.standard_normal((N, d["D"])))
    weight = h16(rs.standard_normal((1, N, H, W)))
    leaves = [torch.from_numpy(a.astype(f64)).requires_grad_(True) for a in (x, low, head)]
    cls = dm.CalibrationDecoding
    feat = cls.decoder_final(dec, *leaves)                # the reference's methods, unmodified
    fg = cls.IA_logit(dec, feat, leaves[2], dec.IA_final_fg)
    bg = cls.IA_logit(dec, feat, leaves[2], dec.IA_final_bg)
    pred = cls.augment_background_logit(dec, fg, bg)
    loss = (pred * torch.from_numpy(weight.astype(f64))).sum()
    loss.backward()
    wb = lambda lin: (leaves[2] @ lin.weight.t() + lin.bias).detach()
    und = tgb.undecided_pixels(feat.detach().reshape(N, feat.shape[1], -1), wb(dec.IA_final_fg), wb(dec.IA_final_bg))
    assert int(und.sum()) == 0, f"{name}: {int(und.sum())} pixels near a tie of the background minimum; take another seed"
    sel = tgb.arg_of(tgb.select(bg.detach().reshape(N, -1))).numpy()
    named = tgb.small_parameters(dec)
    assert all(p.grad is not None or (N == 1 and k.startswith("IA_final_bg")) for k, p in named)      # one object: the bg head is never used
    params = {"w_" + k.replace(".", "__"): h16(p.detach().numpy()) for k, p in named}
    grads = {"grad_w_" + k.replace(".", "__"): p.grad.numpy() for k, p in named if p.grad is not None}
    arrays = dict(in_x=x, in_low_level_feat=low, in_IA_head=head, in_weight=weight, seed=np.int64(seed), loss=np.float64(loss.item()), arg=sel,
                  grad_x=leaves[0].grad.numpy(), grad_low_level_feat=leaves[1].grad.numpy(), grad_IA_head=leaves[2].grad.numpy(), **params, **grads)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 250_000, f"{name}: {size} bytes"
    print(f"{name}: {size} bytes, loss {loss.item():.6f}, objects selected {np.bincount(sel, minlength=N).tolist()}")


def main(ref_root):
    mods = load_reference(ref_root)
    case(mods, tgb.FIXTURES[0], 601, 3, 5, 7, 9, 14)
    case(mods, tgb.FIXTURES[1], 602, 1, 9, 6, 17, 11)
    case(mods, tgb.FIXTURES[2], 603, 4, 6, 5, 13, 9)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
