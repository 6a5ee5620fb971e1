"""Developer tool (GPU box): the ASPP mirror's fused path (b) against the same wiring from one operator per reference line (a).

1. Everything of aspp.py:56-70 that is not a convolution, the convolution outputs replaced by tensors made beforehand:
   (a) four GCTs (plane_reduce + gct_gate + channel_scale each), four groupnorm_relu, plane_mean + linear + relu + expand, torch.cat, GCT(640),
       groupnorm_relu of conv1's output;
   (b) aspp.gate_inputs (plane_sum_sumsq + gct_gate_multi + channel_scale_multi), linear, aspp.merge (groupnorm_cat_relu + gct_gate +
       channel_scale in place), groupnorm_relu of conv1's output.
2. The whole module with its MIOpen convolutions: (a) ASPP.forward(x, fused=False), (b) ASPP.forward(x, fused=True).
Shapes: N = 3 at 61 x 107 (cfg2 at half resolution) and N = 5 at 73 x 131.  The protocol is tools/bench_decoder_tail.py's: one process, (a)
and (b) alternating, every shape warmed up first; a repetition is enough back-to-back calls between two device events to last tens of
milliseconds, REPS repetitions each; median / min / max per call.  The byte counts are derived from the shapes, with X = the bytes of the
input [N, 512, h, w] and a branch tensor = X / 4: (a) moves 23.75 X outside the convolutions, (b) 13.25 X (bn1's 1.5 X, which both share,
included).  The result is APPENDED to the file.

    python tools/bench_aspp.py [out.txt]        # default: profiles/aspp_ab.txt
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import aoc_amd  # noqa: E402
from aoc_amd import aspp, ops  # noqa: E402
from bench_decoder_tail import REPS, ab, report  # noqa: E402

SHAPES = [(3, 61, 107), (5, 73, 131)]
# (a): 4 x (reduce reads X; scale reads X, writes X) = 12 X; pool X; 4 x groupnorm_relu (2 reads + 1 write of X / 4) = 3 X; cat reads and writes
#      1.25 X each = 2.5 X; GCT(640) reads 1.25 X, then reads and writes 1.25 X each = 3.75 X; bn1 on X / 2: 2 reads + 1 write = 1.5 X.    23.75 X
# (b): statistics X; scale reads X, writes 4 X = 5 X; groupnorm_cat_relu reads X twice (4 x X / 4, two passes), writes 1.25 X = 3.25 X; gate in
#      place reads and writes 1.25 X = 2.5 X; bn1 1.5 X.                                                                                  13.25 X
X_A, X_B = 23.75, 13.25


def randomise(net, g):
    with torch.no_grad():
        for name, p in net.named_parameters():
            leaf = name.split(".")[-1]
            if leaf == "alpha" or (leaf == "weight" and p.dim() == 1):
                p.copy_(0.5 + torch.rand(p.shape, device=p.device, generator=g))
            elif leaf in ("gamma", "beta") or (leaf == "bias" and p.dim() == 1):
                p.copy_(0.5 * torch.randn(p.shape, device=p.device, generator=g))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "aspp_ab.txt")
    aoc_amd._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    torch.manual_seed(0)
    net = aspp.ASPP().cuda().eval()
    randomise(net, g)
    branches = (net.aspp1, net.aspp2, net.aspp3, net.aspp4)
    gn = lambda bn, t: ops.groupnorm_relu(t, bn.num_groups, bn.weight.detach(), bn.bias.detach(), bn.eps)
    lines = [f"# ASPP (aspp.py:56-70): the fused path (b) against one operator per reference line (a); {REPS} repetitions each, alternating, us per call:",
             f"# median / min / max.  Byte counts are derived from the shapes ((a) {X_A} X, (b) {X_B} X outside the convolutions).  "
             f"Device: {torch.cuda.get_device_name(0)}", ""]
    slower = []
    with torch.no_grad():
        for N, h, w in SHAPES:
            x = rnd(N, 512, h, w)
            convs = [rnd(N, 128, h, w) for _ in range(4)]          # stand-ins for the branch convolutions' outputs
            z = rnd(N, 256, h, w)                                  # ... and for conv1's
            X = x.numel() * 4

            def rest_a():
                for b in branches:
                    b.GCT(x)
                outs = [gn(b.bn, c) for b, c in zip(branches, convs)]
                x5 = torch.relu(net._pooled(ops.plane_mean(x)))[:, :, None, None].expand(-1, -1, h, w)
                net.GCT(torch.cat(outs + [x5], dim=1))
                return gn(net.bn1, z)

            def rest_b():
                _, mean = aspp.gate_inputs(x, [b.GCT for b in branches])
                aspp.merge(convs, [b.bn for b in branches], net._pooled(mean), net.GCT)
                return gn(net.bn1, z)

            t, calls = ab(rest_a, rest_b)
            lines.append(f"1. everything but the convolutions, N = {N}, {h} x {w}; X = {X / 1e6:.2f} MB (the input)")
            report(lines, t, calls, X_A * X, X_B * X)
            if float(np.median(t["b"])) > float(np.median(t["a"])):
                slower.append(f"non-convolution part at N = {N}, {h} x {w}")

            whole_a, whole_b = (lambda: net(x, fused=False)), (lambda: net(x, fused=True))
            diff = float((whole_a() - whole_b()).abs().max())
            t, calls = ab(whole_a, whole_b)
            lines.append(f"2. the whole module, N = {N}, {h} x {w}; max |fused - unfused| = {diff:.3e}")
            report(lines, t, calls, X_A * X, X_B * X)              # the convolutions' own traffic is not in these byte counts
            lines.insert(len(lines) - 1, "  (byte counts and TB/s of 2. leave the convolutions' own traffic out)")
            if float(np.median(t["b"])) > float(np.median(t["a"])):
                slower.append(f"whole module at N = {N}, {h} x {w}")
    lines.append("fused=True is slower at: " + "; ".join(slower) if slower else "fused=True is faster than fused=False at both shapes, with and without the convolutions.")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
