#!/usr/bin/env python3
"""Golden vectors for the training criterion (tests/test_loss_grad_host.py, tests/test_gpu_loss_grad.py), recorded from the reference's OWN
``Concat_CrossEntropyLoss`` (networks/layers/loss.py:52-97), run UNMODIFIED on the CPU behind torch's ``interpolate`` (aocnet.py:73:
bilinear, align_corners=True), in float64, under autograd.  ``all_pred`` is aocnet.py:78's ``argmax`` of the upsampled logits.

Stored per case: the coarse logits as float16 (exact: they are drawn, then rounded), the labels as uint8 (255 = ignore_index), ``size``,
``step``, the constructor arguments (``top_k_percent_pixels`` NaN for None), the loss, the float64 ``grad_pred`` and ``all_pred``.

    python tests/golden/make_golden_loss_grad.py <the reference's complete_project/AOCNet directory>
"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_decoder_tail import load_reference  # noqa: E402

#        name                       seed C  h  w   H   W   top_k  mining_step  step
CASES = (("loss_grad_half",           31, 4, 9, 11, 33, 41, 0.15, 100000, 50000),
         ("loss_grad_C2",             32, 2, 5, 7, 17, 25, 0.15, 100000, 20000),
         ("loss_grad_mean",           33, 5, 9, 11, 33, 41, None, 100000, 50000),
         ("loss_grad_mining0",        34, 3, 6, 8, 21, 30, 0.15, 0, 7),
         ("loss_grad_past",           35, 6, 8, 9, 29, 33, 0.15, 100000, 250000))


def fixture(loss_mod, name, seed, C, h, w, H, W, top_k, mining_step, step):
    gen = torch.Generator().manual_seed(seed)
    pred = (3.0 * torch.randn(C, h, w, generator=gen)).half()
    labels = torch.randint(0, C, (H, W), generator=gen).to(torch.uint8)
    labels[torch.rand(H, W, generator=gen) < 0.1] = 255
    criterion = loss_mod.Concat_CrossEntropyLoss(top_k, mining_step)
    p = pred.double()[None].requires_grad_(True)
    up = F.interpolate(p, size=(H, W), mode="bilinear", align_corners=True)                # aocnet.py:73
    loss = criterion([up], [labels.long()[None]], step)                                     # :82
    loss.sum().backward()
    all_pred = torch.argmax(up.detach(), dim=1)[0]                                          # :78
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, pred=pred.numpy(), labels=labels.numpy(), size=np.array([H, W]), step=np.array(step),
                        top_k_percent_pixels=np.array(np.nan if top_k is None else top_k), hard_example_mining_step=np.array(mining_step),
                        loss=loss.detach().numpy(), grad_pred=p.grad[0].numpy(), all_pred=all_pred.numpy().astype(np.uint8))
    print(f"{name}: {os.path.getsize(path)} bytes, loss {float(loss.detach()):.6f}")


def main(ref_root):
    torch.set_num_threads(4)
    load_reference(ref_root)
    loss_mod = importlib.import_module("networks.layers.loss")
    for case in CASES:
        fixture(loss_mod, *case)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
