#!/usr/bin/env python3
"""Golden vectors for the ASPP mirror (tests/test_aspp_host.py, tests/test_gpu_aspp.py), recorded from the reference's own ``ASPP``
(networks/layers/aspp.py:33-78), constructed and run UNMODIFIED on the CPU in float32 with forward hooks.

Recorded: the input, every branch GCT's output, every ``atrous_conv`` output, the pooled branch after its ReLU, the concatenation (the input
of ``GCT(640)``), its gated output, ``conv1``'s output and the result; every parameter except the 3 x 3 and the 640 -> 256 convolution weights
(8 MB: the stage tests start from the recorded convolution outputs instead); and the constructor's facts as plain data -- every
convolution's kernel size, padding and dilation, the GroupNorm group counts, and the ``state_dict`` names and shapes.

    python tests/golden/make_golden_aspp.py <the reference's complete_project/AOCNet directory>
"""
import importlib
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_decoder_tail import load_reference, randomise  # noqa: E402

BRANCHES = ("aspp1", "aspp2", "aspp3", "aspp4")
LEFT_OUT = ("aspp2.atrous_conv.weight", "aspp3.atrous_conv.weight", "aspp4.atrous_conv.weight", "conv1.weight")


def aspp_fixture(name, ref_aspp, seed, N, h, w):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    net = ref_aspp.ASPP()
    randomise(net, gen)
    with torch.no_grad():                                # the two recorded 1 x 1 convolution weights keep 8 mantissa bits (still exact float32
        for conv in (net.aspp1.atrous_conv, net.global_avg_pool[1]):          # values): the archive compresses them to half, below 1 MiB
            conv.weight.copy_(conv.weight.bfloat16().float())
    net.eval()
    x = torch.randn(N, 512, h, w, generator=gen)
    seen = {}

    def keep(key, with_input=None):
        def hook(_m, inputs, output):
            seen[key] = output.detach().clone()
            if with_input:
                seen[with_input] = inputs[0].detach().clone()
        return hook
    hooks = []
    for b in BRANCHES:
        hooks.append(getattr(net, b).GCT.register_forward_hook(keep(b + "_gct_out")))
        hooks.append(getattr(net, b).atrous_conv.register_forward_hook(keep(b + "_conv_out")))
    hooks.append(net.global_avg_pool.register_forward_hook(keep("pooled")))
    hooks.append(net.GCT.register_forward_hook(keep("cat_gated", with_input="cat")))
    hooks.append(net.conv1.register_forward_hook(keep("conv1_out")))
    with torch.no_grad():
        out = net(x)
    for hd in hooks:
        hd.remove()
    arrays = dict(in_x=x.numpy(), out=out.numpy())
    arrays.update({k: v.numpy() for k, v in seen.items()})
    sd = net.state_dict()
    for k, v in sd.items():
        if k not in LEFT_OUT:
            arrays["p_" + k] = v.numpy()
    convs = [(k, m) for k, m in net.named_modules() if isinstance(m, nn.Conv2d)]
    norms = [(k, m) for k, m in net.named_modules() if isinstance(m, nn.GroupNorm)]
    arrays["meta_state_names"] = np.asarray(list(sd.keys()))
    arrays["meta_state_shapes"] = np.asarray([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], np.int64)
    arrays["meta_state_dims"] = np.asarray([v.dim() for v in sd.values()], np.int64)
    arrays["meta_conv_names"] = np.asarray([k for k, _ in convs])
    # in, out, kernel, stride, padding, dilation, groups, has bias
    arrays["meta_conv_hyper"] = np.asarray([[m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.dilation[0], m.groups,
                                             int(m.bias is not None)] for _, m in convs], np.int64)
    arrays["meta_norm_names"] = np.asarray([k for k, _ in norms])
    arrays["meta_norm_groups"] = np.asarray([[m.num_groups, m.num_channels] for _, m in norms], np.int64)
    arrays["meta_norm_eps"] = np.asarray([m.eps for _, m in norms], np.float64)
    arrays["meta_gct_eps"] = np.asarray([getattr(net, b).GCT.epsilon for b in BRANCHES] + [net.GCT.epsilon], np.float64)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, out {tuple(out.shape)}, {len(sd)} state_dict entries")


def main(ref_root):
    torch.set_num_threads(4)
    load_reference(ref_root)
    ref_aspp = importlib.import_module("networks.layers.aspp")
    aspp_fixture("aspp_O3", ref_aspp, 41, N=3, h=3, w=4)
    aspp_fixture("aspp_O1", ref_aspp, 42, N=1, h=2, w=3)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
