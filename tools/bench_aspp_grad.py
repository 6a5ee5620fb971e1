"""Developer tool (GPU box): forward + backward of ASPP (networks/layers/aspp.py:33-78) in three arms, all in one process, alternating call by
call:
  (hip)    aoc_amd.aspp_train.ASPP with fused=True (csrc/aspp_grad.hip behind its two fused stages; the convolutions are torch's in every arm);
  (plain)  the same twin with fused=False (one differentiable operator per reference line);
  (torch)  the same lines as the reference writes them, in plain PyTorch on the device, with the same parameters.
Shapes: N = 3 on the half-resolution map 61 x 107 and N = 5 on 73 x 131.  Per arm: WARMUP calls, then RUNS calls each bracketed by two device
events (median / min / max in ms), and torch.cuda.max_memory_allocated over one more call minus what was allocated before it (the inputs
and parameters alone).  Before the timing the gradients of the arms are compared and the largest difference relative to the largest
gradient printed.  The merge condition is the HIP arm's median at or below the PyTorch arm's of the same run at both shapes (the last
column says so; it is measured against PyTorch, never against itself), and fused=True stays the default only while it is not slower than
fused=False.  Last, the new entry points alone: one wrapper call between two device events, median of RUNS.  The results are appended to the
output file.  The exit status is 1 when a row says NO or a gradient difference exceeds GRAD_TOL.

    python tools/bench_aspp_grad.py [out.txt]        # default: profiles/aspp_grad_ab.txt
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import aoc_amd  # noqa: E402
from aoc_amd import aspp_train as at, ops  # noqa: E402
from bench_gates_grad import TorchGCT, event_median, grads_of, peak_of, step_of, WARMUP, RUNS  # noqa: E402

# The arms sum float32 products over up to 9 x 512 x 9 563 terms in orders of their own, with MIOpen's convolutions between them: 1e-3 of the
# largest gradient separates that from a wrong gradient; the rounding bounds proper are the tests'.
GRAD_TOL = 1e-3
BRANCHES = ("aspp1", "aspp2", "aspp3", "aspp4")


class TorchASPP(at.ASPP):
    """the twin's parameters, aspp.py:56-70 in plain PyTorch"""

    def __init__(self):
        super().__init__()
        for b in BRANCHES:
            getattr(self, b).GCT = TorchGCT(512)
        self.GCT = TorchGCT(640)

    def forward(self, x):
        outs = []
        for name in BRANCHES:
            b = getattr(self, name)
            outs.append(torch.relu(b.bn(b.atrous_conv(b.GCT(x)))))
        x5 = self.global_avg_pool(x)
        x5 = F.interpolate(x5, size=outs[0].size()[2:], mode='bilinear', align_corners=True)
        x = self.GCT(torch.cat(outs + [x5], dim=1))
        return torch.relu(self.bn1(self.conv1(x)))


class Arm(torch.nn.Module):
    def __init__(self, net, fused):
        super().__init__()
        self.net, self.fused = net, fused

    def forward(self, x):
        return self.net(x, fused=self.fused)


def randomise(module, gen):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("alpha"):
                p.uniform_(0.5, 1.5, generator=gen)
            elif "GCT" in name or name.endswith("bias"):
                p.normal_(std=0.5, generator=gen)
            elif p.dim() == 1:
                p.copy_(1.0 + 0.25 * torch.randn(p.shape, device=p.device, generator=gen))


def bench(N, h, w, gen):
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    twin, ref = at.ASPP().cuda(), TorchASPP().cuda()
    randomise(twin, gen)
    ref.load_state_dict(twin.state_dict())
    arms = {"hip": Arm(twin, True), "plain": Arm(twin, False), "torch": ref}
    x, gy = r(N, 512, h, w), r(N, 256, h, w)
    ins = {k: [x.clone().requires_grad_(True)] for k in arms}
    steps = {k: step_of(arms[k], ins[k], gy) for k in arms}
    grads = {}
    for k in arms:
        steps[k]()
        grads[k] = [g.clone() for g in grads_of(arms[k], ins[k])]
    diff = {k: max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads[k], grads["torch"])) for k in ("hip", "plain")}
    for _ in range(WARMUP):
        for k in arms:
            steps[k]()
    ms = {k: [] for k in arms}
    for _ in range(RUNS):
        for k in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            steps[k]()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    drop = [lambda: [setattr(t[0], "grad", None) for t in ins.values()], lambda: [setattr(p, "grad", None) for m in (twin, ref) for p in m.parameters()]]
    peaks = {k: peak_of(steps[k], drop) for k in arms}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = f"ASPP forward + backward  N={N} {h:3d}x{w:3d}  " + "   ".join(
        f"{k} {med[k]:7.3f} ms [{min(ms[k]):.3f}, {max(ms[k]):.3f}] peak {peaks[k] / 2**20:7.1f} MiB" for k in arms)
    line += f"   max rel grad diff against torch: hip {diff['hip']:.1e}, plain {diff['plain']:.1e}   (measured)"
    return line, med, max(diff.values())


def kernels_alone(N, h, w, gen):
    """the new entry points one by one at the module's widths, outputs allocated by the wrappers"""
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    x, gs, dmean = r(N, 512, h, w), [r(N, 512, h, w) for _ in range(4)], r(N, 512)
    al, ga, be = 0.5 + torch.rand(4, 512, device="cuda", generator=gen), r(4, 512), 0.5 * r(4, 512)
    _, sumsq, _ = ops.plane_sum_sumsq(x, want_sum=False)
    gates = ops.gct_gate_multi(sumsq, al, ga, be, 1e-5, False)
    dots = at.plane_dot_multi(x, gs)
    dst = at.gct_gate_multi_backward(dots, gates, sumsq, al, ga, be, 1e-5)[0]
    us, w4, b4, tail = [r(N, 128, h, w) for _ in range(4)], 1 + 0.25 * r(4, 128), r(4, 128), r(N, 128)
    cal, cga, cbe, g = 0.5 + torch.rand(640, device="cuda", generator=gen), r(640), 0.5 * r(640), r(N, 640, h, w)
    _, sq, stats = at.groupnorm_cat_relu_forward(us, 32, w4, b4, 1e-5, tail)
    gate = ops.gct_gate(sq, cal, cga, cbe, 1e-5, False)
    out = torch.empty_like(x)
    rows = (("plane_dot_multi, 4 sets", lambda: at.plane_dot_multi(x, gs)),
            ("gct_gate_multi_grad, 4 sets", lambda: at.gct_gate_multi_backward(dots, gates, sumsq, al, ga, be, 1e-5)),
            ("channel_scale_multi_grad_apply, 4 sets", lambda: at.channel_scale_multi_backward_apply(gs, gates, x, dst, dmean, out)),
            ("groupnorm_cat_relu_grad, every output", lambda: at.groupnorm_cat_relu_backward(g, us, stats, 32, w4, b4, tail, sq, gate, cal, cga, 1e-5)),
            ("groupnorm_cat_relu_grad, the small outputs alone (plane pass)", lambda: at.groupnorm_cat_relu_backward(
                g, us, stats, 32, w4, b4, tail, sq, gate, cal, cga, 1e-5, want=(False, True, True, True, True, True, True))),
            ("torch.mul(g_0, x)", lambda: torch.mul(gs[0], x, out=out)))
    return (f"kernels alone    N={N} {h:3d}x{w:3d}  X = {x.numel() * 4 / 1e6:.1f} MB, Y = X / 4: "
            + "; ".join(f"{name} {event_median(call):.3f} ms" for name, call in rows) + "   (measured)")


SHAPES = [(3, 61, 107), (5, 73, 131)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "aspp_grad_ab.txt")
    aoc_amd._lib.lib()
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False      # float32 convolutions in every arm
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = ["# ASPP, forward + backward: (hip) aoc_amd.aspp_train.ASPP fused=True, (plain) the same twin fused=False, (torch) the reference's lines in plain "
             f"PyTorch; all arms in one process, alternating; median [min, max] of {RUNS} after {WARMUP} warm-up calls; peak = max_memory_allocated above the inputs",
             f"# device: {torch.cuda.get_device_name(0)}"]
    failed = []
    for N, h, w in SHAPES:
        line, med, diff = bench(N, h, w, gen)
        ok, keep = med["hip"] <= med["torch"], med["hip"] <= med["plain"]
        lines.append(line + "   hip <= torch: " + ("yes" if ok else "NO") + "   fused <= plain: " + ("yes" if keep else "NO"))
        print(lines[-1], flush=True)
        if not ok:
            failed.append(f"N={N} {h}x{w}: the HIP median exceeds the PyTorch median")
        if not diff <= GRAD_TOL:
            failed.append(f"N={N} {h}x{w}: gradients differ by {diff:.1e} of the largest, tolerance {GRAD_TOL:.0e}")
        torch.cuda.empty_cache()
    lines.append(kernels_alone(3, 61, 107, gen))
    print(lines[-1], flush=True)
    lines += ["# FAILED: " + f for f in failed]
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    for f in failed:
        print("FAILED: " + f, file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
