#!/usr/bin/env python3
"""Golden vectors for the decoder's memory block (tests/test_decoder_memory_host.py, tests/test_gpu_decoder_memory.py), recorded from the
reference's own ``CalibrationDecoding.Modulator_1`` and ``CalibrationDecoding.forward`` (networks/aoc/decoding_module.py:96-149, 192-210), run
UNMODIFIED on the CPU on a ``__new__`` holder (make_golden_decoder_tail.py says why the constructor cannot run).

modulator_O3 / modulator_O1: Modulator_1 with the reference's own ``IA_gate`` and ``Bottleneck`` at e = 128 (``GroupNorm(32, out / 4)`` allows
nothing smaller), D = 12.  A forward hook on ``M1_Reweight_Layer_1`` records what gate 1 is handed (the concatenation) and what it returns;
the result is held twice, from the float32 modules and from their ``.double()`` copies.

decoder_memory_rule: the reference's own ``forward`` over five frames with N = 2, 2, 2, 3, 3.  Every module outside lines 133-148 is a
shape-preserving stand-in, ``decoder_final`` included (an instance attribute that returns x); the Bottlenecks of the modulators are
channel-slicing stand-ins, so C = 4 is enough; the six gates and the prediction head are the reference's own.  ``torch.Tensor.cuda`` is the
identity for the call.  Recorded per frame: the inputs, the second halves of what hooks on ``M1_Reweight_Layer_1`` / ``M2_Reweight_Layer_1``
see (which memory was used), Modulator_1's result, the returned memory list, and whether the returned slots are the objects / the storage
the reference aliases.  Frame 3 separates "sticky" from "previous frame" for slot 1, frame 4 exercises the size reset.

    python tests/golden/make_golden_decoder_memory.py <the reference's complete_project/AOCNet directory>
"""
import copy
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_decoder_tail import holder, load_reference, randomise  # noqa: E402


def modulator_fixture(name, mods, seed, N, e, D, h, w):
    gct, att, dm = mods
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    dec = holder(dm)
    dec.M1_Reweight_Layer_1 = att.IA_gate(D, e * 2)                                 # decoding_module.py:55-62 at e = 128
    dec.M1_Bottleneck_1 = gct.Bottleneck(e * 2, e * 2, 1)
    dec.M1_Reweight_Layer_2 = att.IA_gate(D, e * 2)
    dec.M1_Bottleneck_2 = gct.Bottleneck(e * 2, e * 1, 1)
    dec.M1_Reweight_Layer_3 = att.IA_gate(D, e * 1)
    dec.M1_Bottleneck_3 = gct.Bottleneck(e * 1, e * 1, 1)
    randomise(dec, gen)
    dec.eval()
    x = torch.randn(N, e, h, w, generator=gen)
    mem = torch.randn(N, e, h, w, generator=gen)
    head = 0.5 * torch.randn(N, D, generator=gen)
    seen = {}

    def hook(_m, inputs, output):
        seen["x"], seen["out"] = inputs[0].detach().clone(), output.detach().clone()
    hd = dec.M1_Reweight_Layer_1.register_forward_hook(hook)
    with torch.no_grad():
        out32 = dm.CalibrationDecoding.Modulator_1(dec, x, mem, head)
        hd.remove()
        dec64 = copy.deepcopy(dec).double()
        out64 = dm.CalibrationDecoding.Modulator_1(dec64, x.double(), mem.double(), head.double())
    arrays = dict(in_x=x.numpy(), in_x_memory=mem.numpy(), in_IA_head=head.numpy(), gate1_in=seen["x"].numpy(), gate1_out=seen["out"].numpy(),
                  out_f32=out32.numpy(), out_f64=out64.numpy())
    for k, v in dec.state_dict().items():
        arrays["p_" + k] = v.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, max |f32 - f64| of the result {float((out32.double() - out64).abs().max()):.3e}")


class Same(nn.Module):
    """Shape-preserving stand-in for everything outside lines 133-148: returns its first argument."""

    def forward(self, x, *_):
        return x


class Slice(nn.Module):
    """Channel-slicing stand-in for a modulator's Bottleneck."""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return x[:, :self.out]


def rule_fixture(name, mods, seed, counts, C, D, h, w):
    gct, att, dm = mods
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    dec = holder(dm)
    for k in ("IA1", "layer1", "CLB2", "layer2", "CLB3", "layer3", "CLB4", "layer4", "CLB5", "layer5", "IA9", "ASPP"):
        setattr(dec, k, Same())
    for m in ("M1", "M2"):
        for i, (cin, cout) in enumerate(((2 * C, 2 * C), (2 * C, C), (C, C)), 1):
            setattr(dec, f"{m}_Reweight_Layer_{i}", att.IA_gate(D, cin))
            setattr(dec, f"{m}_Bottleneck_{i}", Slice(cout))
    dec.IA_final_fg, dec.IA_final_bg = nn.Linear(D, C + 1), nn.Linear(D, C + 1)
    dec.decoder_final = lambda x, low_level_feat, IA_head: x                        # shadows the method of :162
    dec.eval()
    seen = {}
    hooks = [dec.M1_Reweight_Layer_1.register_forward_hook(lambda _m, i, o: seen.__setitem__("m1", i[0][:, C:].detach().clone())),
             dec.M2_Reweight_Layer_1.register_forward_hook(lambda _m, i, o: seen.__setitem__("m2", i[0][:, C:].detach().clone())),
             dec.M1_Bottleneck_3.register_forward_hook(lambda _m, i, o: seen.__setitem__("m1_out", o.detach().clone()))]
    arrays = dict(counts=np.asarray(counts, np.int64))
    for k, v in dec.state_dict().items():
        arrays["p_" + k] = v.numpy()
    memory = [None, None]
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            for f, N in enumerate(counts):
                x = torch.randn(N, C, h, w, generator=gen)
                head = 0.5 * torch.randn(N, D, generator=gen)
                slot1_in = memory[1]
                pred, out = dm.CalibrationDecoding.forward(dec, x, head, memory, None)
                arrays.update({f"f{f}_x": x.numpy(), f"f{f}_IA_head": head.numpy(), f"f{f}_m1_memory": seen["m1"].numpy(),
                               f"f{f}_m2_memory": seen["m2"].numpy(), f"f{f}_m1_out": seen["m1_out"].numpy(), f"f{f}_pred": pred.contiguous().numpy(),
                               f"f{f}_slot0": out[0].numpy().copy(), f"f{f}_slot1": out[1].numpy().copy(),
                               f"f{f}_slot0_shares_x": np.asarray(out[0].data_ptr() == x.data_ptr()),
                               f"f{f}_slot1_is_input_slot1": np.asarray(out[1] is slot1_in)})
                memory = out
    finally:
        torch.Tensor.cuda = real_cuda
        for hd in hooks:
            hd.remove()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes; slot 1 kept:", [bool(arrays[f"f{f}_slot1_is_input_slot1"]) for f in range(len(counts))])


def main(ref_root):
    torch.set_num_threads(4)
    mods = load_reference(ref_root)
    modulator_fixture("modulator_O3", mods, 31, N=3, e=128, D=12, h=5, w=7)
    modulator_fixture("modulator_O1", mods, 32, N=1, e=128, D=12, h=6, w=5)
    rule_fixture("decoder_memory_rule", mods, 33, counts=(2, 2, 2, 3, 3), C=4, D=6, h=3, w=5)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
