"""Drop-in mirror of ``networks/layers/aspp.py`` (the module ``CalibrationDecoding`` runs between ``IA9`` and ``Modulator_1``,
decoding_module.py:53, :131) on the HIP library.  Constructor signatures, attribute names, parameter names and initialisation are the
reference's, so a reference ``state_dict`` loads unchanged.  The convolutions stay PyTorch-ROCm modules (MIOpen; out of scope); everything
between them runs in the HIP library.

The four branch GCTs and the pooled branch read the same ``x``: ``ASPP.forward(x, fused=True)`` takes its plane statistics once
(``ops.plane_sum_sumsq``), forms the four gates in one launch, writes the four gated copies in one pass, and normalises the four convolution
outputs straight into the concatenation, whose plane norms for ``GCT(640)`` come out of the same apply pass.  ``fused=False`` is the same
wiring from one operator per reference line."""
import torch
from torch import nn

from . import ops
from .gct import GCT


class _ASPPModule(nn.Module):
    """aspp.py:7-31: GCT -> atrous convolution -> GroupNorm(planes / 4) -> ReLU."""

    def __init__(self, inplanes, planes, kernel_size, padding, dilation):
        super(_ASPPModule, self).__init__()
        self.GCT = GCT(inplanes)
        self.atrous_conv = nn.Conv2d(inplanes, planes, kernel_size=kernel_size, stride=1, padding=padding, dilation=dilation, bias=False)
        self.bn = nn.GroupNorm(int(planes / 4), planes)
        self.relu = nn.ReLU(inplace=True)
        self._init_weight()

    def forward(self, x):
        ops.inference_only("_ASPPModule", x, *self.parameters())
        x = self.atrous_conv(self.GCT(x))                                                 # aspp.py:19-20
        return ops.groupnorm_relu(x, self.bn.num_groups, self.bn.weight.detach(), self.bn.bias.detach(), self.bn.eps)      # :21-23

    def _init_weight(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight)


def _gct_params(gcts):
    return [[getattr(g, k).detach() for g in gcts] for k in ("alpha", "gamma", "beta")]


def gate_inputs(x, gcts):
    """The inputs of the branch convolutions and the pooled branch's input from two passes over x (aspp.py:19 for every branch, :46):
    -> ([GCT_k(x) for k], plane means [N, C]).  gcts: up to 8 l2-mode GCTs with one epsilon; each copy is bit-equal to
    ``ops.channel_scale(x, ops.gct_gate(sums, ...))`` on the sums of squares this pass produces."""
    gcts = list(gcts)
    if any(g.mode != 'l2' or g.epsilon != gcts[0].epsilon for g in gcts):
        raise ValueError("aspp.gate_inputs: the GCTs that share one statistics pass are l2-mode with one epsilon (aspp.py:10)")
    _, sumsq, mean = ops.plane_sum_sumsq(x, want_sum=False)
    alpha, gamma, beta = _gct_params(gcts)
    gates = ops.gct_gate_multi(sumsq, alpha, gamma, beta, gcts[0].epsilon, False)
    return ops.channel_scale_multi(x, gates), mean


def merge(conv_outs, bns, tail, gct):
    """aspp.py:21-23 for every branch, :62-63 and :65: GroupNorm + ReLU of the branch convolutions' outputs written into the concatenation
    with the pooled branch ``tail`` [N, C_tail] (before its ReLU) broadcast behind them, then ``gct`` applied in place, its plane norms taken
    from the apply pass.  bns: the branches' nn.GroupNorm modules (one group count, one eps)."""
    bns = list(bns)
    if any(b.num_groups != bns[0].num_groups or b.eps != bns[0].eps for b in bns):
        raise ValueError("aspp.merge: the branches' GroupNorms share one group count and one eps (aspp.py:13)")
    if gct.mode != 'l2':
        raise ValueError("aspp.merge: the gate of the concatenation is an l2-mode GCT (aspp.py:50)")
    cat, sumsq = ops.groupnorm_cat_relu(conv_outs, bns[0].num_groups, [b.weight.detach() for b in bns], [b.bias.detach() for b in bns], bns[0].eps,
                                        tail, True, want_plane_sumsq=True)
    gate = ops.gct_gate(sumsq, gct.alpha.detach(), gct.gamma.detach(), gct.beta.detach(), gct.epsilon, False)
    return ops.channel_scale(cat, gate, out=cat)


class ASPP(nn.Module):
    """aspp.py:33-78."""

    def __init__(self):
        super(ASPP, self).__init__()
        inplanes = 512
        dilations = [1, 6, 12, 18]
        self.aspp1 = _ASPPModule(inplanes, 128, 1, padding=0, dilation=dilations[0])
        self.aspp2 = _ASPPModule(inplanes, 128, 3, padding=dilations[1], dilation=dilations[1])
        self.aspp3 = _ASPPModule(inplanes, 128, 3, padding=dilations[2], dilation=dilations[2])
        self.aspp4 = _ASPPModule(inplanes, 128, 3, padding=dilations[3], dilation=dilations[3])
        self.global_avg_pool = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)),
                                             nn.Conv2d(inplanes, 128, 1, stride=1, bias=False),
                                             nn.ReLU(inplace=True))
        self.GCT = GCT(640)
        self.conv1 = nn.Conv2d(640, 256, 1, bias=False)
        self.bn1 = nn.GroupNorm(32, 256)
        self.relu = nn.ReLU(inplace=True)
        self._init_weight()

    def _pooled(self, mean):
        """aspp.py:61 without its ReLU: the 1 x 1 convolution of the plane means is a [N, 512] x [512, 128] product."""
        w = self.global_avg_pool[1].weight.detach()
        return ops.linear(mean, w.view(w.shape[0], w.shape[1]), None)

    def forward(self, x, fused=True):
        ops.inference_only("ASPP", x, *self.parameters())
        branches = (self.aspp1, self.aspp2, self.aspp3, self.aspp4)
        if fused:
            gated, mean = gate_inputs(x, [b.GCT for b in branches])                       # aspp.py:19 x 4, :46
            convs = [b.atrous_conv(g) for b, g in zip(branches, gated)]                   # :20 x 4
            x = merge(convs, [b.bn for b in branches], self._pooled(mean), self.GCT)      # :21-23 x 4, :61-65
        else:
            outs = [b(x) for b in branches]                                               # :57-60
            x5 = torch.relu(self._pooled(ops.plane_mean(x)))                              # :61
            # :62: bilinear interpolation from a 1 x 1 map with align_corners=True repeats the value
            x5 = x5[:, :, None, None].expand(-1, -1, *outs[0].shape[2:])
            x = self.GCT(torch.cat(outs + [x5], dim=1))                                   # :63, :65
        x = self.conv1(x)                                                                 # :66
        return ops.groupnorm_relu(x, self.bn1.num_groups, self.bn1.weight.detach(), self.bn1.bias.detach(), self.bn1.eps)      # :67-68

    def _init_weight(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight)
