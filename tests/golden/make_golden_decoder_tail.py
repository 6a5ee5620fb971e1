#!/usr/bin/env python3
"""Golden vectors for the decoder's tail (tests/test_decoder_tail_host.py, tests/test_gpu_decoder_tail.py), recorded from the reference's own
``CalibrationDecoding.decoder_final``, ``IA_logit`` and ``augment_background_logit`` (networks/aoc/decoding_module.py:151-190, 213-225), run
UNMODIFIED on the CPU.

The reference's constructor cannot run (decoding_module.py:21, :30 read undefined names), so the methods run on an instance made with
``__new__`` that carries exactly the attributes they read, built from the reference's own ``GCT`` (networks/layers/gct.py) and ``IA_gate``
(networks/layers/attention.py) and from ``nn.Conv2d`` / ``nn.GroupNorm`` / ``nn.Linear`` with the constructor's arguments (:74-89) at small
widths.  The files import ``networks.p2t.*``, which the reference does not ship: empty stand-in module objects are registered for the import.

Forward hooks on ``IA10`` record its two inputs (the concatenated tensor and the extended head) and its output: they pin the upsample, the
concatenation order, px1_delta and the gate with no convolution in between.  Every shortcut fixture also holds decoder_final's result twice:
from the float32 modules and from ``.double()`` copies of the same modules on the float64 inputs.

    python tests/golden/make_golden_decoder_tail.py <the reference's complete_project/AOCNet directory>
"""
import copy
import importlib
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(ref_root):
    sys.dont_write_bytecode = True                       # never write into the reference tree
    sys.path.insert(0, ref_root)
    cl = importlib.import_module("networks.aoc.conditioning_layer")
    p2t = types.ModuleType("networks.p2t")
    cm = types.ModuleType("networks.p2t.center_module")
    cm.SpatialProp = type("SpatialProp", (), {})
    sys.modules.setdefault("networks.p2t", p2t)
    sys.modules.setdefault("networks.p2t.center_module", cm)
    sys.modules.setdefault("networks.p2t.conditioning_layer", cl)
    return (importlib.import_module("networks.layers.gct"), importlib.import_module("networks.layers.attention"),
            importlib.import_module("networks.aoc.decoding_module"))


def holder(dm):
    dec = dm.CalibrationDecoding.__new__(dm.CalibrationDecoding)
    nn.Module.__init__(dec)
    return dec


def randomise(module, gen):
    """The defaults make GCT's gate 1 and GroupNorm's affine the identity: draw every parameter."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.split(".")[-1]
            if leaf in ("alpha",) or (leaf == "weight" and p.dim() == 1):
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=gen))
            elif leaf in ("gamma", "beta") or (leaf == "bias" and "bn" in name):
                p.copy_(0.5 * torch.randn(p.shape, generator=gen))


def shortcut_fixture(name, mods, seed, N, Ce, Cr, D, Cl, h, w, H, W):
    gct, att, dm = mods
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    dec = holder(dm)
    dec.GCT_sc = gct.GCT(Cl)                                                        # decoding_module.py:74-86 at small widths
    dec.conv_sc = nn.Conv2d(Cl, Cr, 1, bias=False)
    dec.bn_sc = nn.GroupNorm(int(Cr / 4), Cr)
    dec.relu = nn.ReLU(inplace=True)
    dec.IA10 = att.IA_gate(D + Ce + Cr, Ce + Cr)
    dec.conv1 = nn.Conv2d(Ce + Cr, int(Ce / 2), kernel_size=3, padding=1, bias=False)
    dec.bn1 = nn.GroupNorm(32, int(Ce / 2))
    dec.IA11 = att.IA_gate(D + int(Ce / 2), int(Ce / 2))
    dec.conv2 = nn.Conv2d(int(Ce / 2), int(Ce / 2), kernel_size=3, padding=1, bias=False)
    dec.bn2 = nn.GroupNorm(32, int(Ce / 2))
    randomise(dec, gen)
    dec.eval()
    x = torch.randn(N, Ce, h, w, generator=gen)
    low = torch.randn(N, Cl, H, W, generator=gen)
    head = 0.5 * torch.randn(N, D, generator=gen)
    seen = {}

    def hook(_m, inputs, output):
        seen["x"], seen["head"], seen["out"] = inputs[0].detach().clone(), inputs[1].detach().clone(), output.detach().clone()
    hd = dec.IA10.register_forward_hook(hook)
    with torch.no_grad():
        out32 = dm.CalibrationDecoding.decoder_final(dec, x, low, head)
        hd.remove()
        dec64 = copy.deepcopy(dec).double()
        out64 = dm.CalibrationDecoding.decoder_final(dec64, x.double(), low.double(), head.double())
    arrays = dict(in_x=x.numpy(), in_low_level_feat=low.numpy(), in_IA_head=head.numpy(), ia10_in_x=seen["x"].numpy(),
                  ia10_in_head=seen["head"].numpy(), ia10_out=seen["out"].numpy(), out_f32=out32.numpy(), out_f64=out64.numpy())
    for k, v in dec.state_dict().items():
        arrays["p_" + k] = v.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, max |f32 - f64| of the final output {float((out32.double() - out64).abs().max()):.3e}")


def logit_fixture(name, mods, seed, N, C, D, h, w):
    dm = mods[2]
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    dec = holder(dm)
    fg, bg = nn.Linear(D, C + 1), nn.Linear(D, C + 1)                               # :88-89: independent heads
    x = torch.randn(N, C, h, w, generator=gen)
    head = torch.randn(N, D, generator=gen)
    with torch.no_grad():
        fg_logit = dm.CalibrationDecoding.IA_logit(dec, x, head, fg)                # :144-147
        bg_logit = dm.CalibrationDecoding.IA_logit(dec, x, head, bg)
        pred = dm.CalibrationDecoding.augment_background_logit(dec, fg_logit, bg_logit)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, in_x=x.numpy(), in_IA_head=head.numpy(), p_fg_weight=fg.weight.detach().numpy(), p_fg_bias=fg.bias.detach().numpy(),
                        p_bg_weight=bg.weight.detach().numpy(), p_bg_bias=bg.bias.detach().numpy(), fg_logit=fg_logit.numpy(),
                        bg_logit=bg_logit.numpy(), pred=pred.contiguous().numpy())
    print(f"{name}: {os.path.getsize(path)} bytes, pred {tuple(pred.shape)}")


def main(ref_root):
    torch.set_num_threads(4)
    mods = load_reference(ref_root)
    shortcut_fixture("decoder_shortcut_O3", mods, 11, N=3, Ce=64, Cr=8, D=12, Cl=16, h=5, w=7, H=9, W=14)
    shortcut_fixture("decoder_shortcut_O1", mods, 12, N=1, Ce=64, Cr=8, D=12, Cl=16, h=3, w=4, H=7, W=9)         # px1_delta == 0
    shortcut_fixture("decoder_shortcut_O4_odd", mods, 13, N=4, Ce=64, Cr=8, D=12, Cl=16, h=6, w=5, H=13, W=9)
    logit_fixture("logit_head_O1", mods, 21, N=1, C=32, D=12, h=6, w=7)                                           # no augmentation branch
    logit_fixture("logit_head_O2", mods, 22, N=2, C=32, D=12, h=6, w=7)
    logit_fixture("logit_head_O4", mods, 23, N=4, C=32, D=12, h=6, w=7)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
