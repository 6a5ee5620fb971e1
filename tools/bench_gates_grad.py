"""Developer tool (GPU box): forward + backward of the calibration gates in two arms, both in one process, alternating call by call:
  (hip)   the twins of aoc_amd.gates_train (csrc/gate_grad.hip behind them);
  (torch) the same lines as the reference writes them, in plain PyTorch on the device: ATT:12-17 (IA_gate), gct.py:17-36 (GCT, l2) and
          CLB:24-86 with the vector repair (conditioning_block), with the same parameters.
Four objects.  Shapes: cfg2's map 121 x 213 at c = 164 with D = 400; its half-resolution map 61 x 107 at c = 512 with D = 912; the
117 x 117 training crop at the same two widths; the conditioning block at C = 256, D = 400 on the two cfg2 maps.  Per arm: WARMUP calls,
then RUNS calls each bracketed by two device events (median / min / max in ms), and torch.cuda.max_memory_allocated over one more call
minus what was allocated before it (the inputs and parameters alone).  Before the timing the gradients of the two arms are compared and
the largest difference relative to the largest gradient printed.  The HIP arm moves half the bytes: at the two cfg2 shapes its median may
not exceed the PyTorch arm's of the same run (the last column says so); the other rows are recorded only.  Last, the kernels alone at the
two cfg2 shapes: one wrapper call between two device events, median of RUNS, beside ``torch.mul`` over the same two streams.  The results
are appended to the output file.  The exit status is 1 when a cfg2 row says NO or a gradient difference exceeds GRAD_TOL.

    python tools/bench_gates_grad.py [out.txt]        # default: profiles/gates_grad_ab.txt
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import aoc_amd  # noqa: E402
from aoc_amd import gates_train  # noqa: E402

WARMUP, RUNS, N_OBJ = 5, 20, 4
# Both arms sum float32 products of up to hw = 25 773 terms in orders of their own; each is within hw U = 1.5e-3 of the sum of magnitudes at
# worst and a few 1e-6 of the largest gradient in practice.  1e-3 of the largest gradient separates that from a wrong gradient (a wiring
# mistake moves it by its own size); the rounding bounds proper are the tests' (tests/gates_grad_bounds.py).
GRAD_TOL = 1e-3
GATE_SHAPES = [("cfg2 map", 121, 213, 164, 400, True), ("cfg2 half-resolution map", 61, 107, 512, 912, True), ("training crop", 117, 117, 164, 400, False),
               ("training crop", 117, 117, 512, 912, False)]
BLOCK_SHAPES = [("cfg2 map", 121, 213, 256, 400, True), ("cfg2 half-resolution map", 61, 107, 256, 400, True)]


class TorchIAGate(nn.Module):
    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.IA = nn.Linear(in_dim, out_dim)

    def forward(self, x, IA_head):                                   # ATT:12-17
        a = 1. + torch.tanh(self.IA(IA_head))
        return a.unsqueeze(-1).unsqueeze(-1) * x


class TorchGCT(nn.Module):
    def __init__(self, C, epsilon=1e-5):
        super().__init__()
        self.alpha, self.gamma, self.beta = (nn.Parameter(torch.zeros(1, C, 1, 1)) for _ in range(3))
        self.epsilon = epsilon

    def forward(self, x):                                            # gct.py:19-36, mode l2
        embedding = (x.pow(2).sum((2, 3), keepdim=True) + self.epsilon).pow(0.5) * self.alpha
        norm = self.gamma / (embedding.pow(2).mean(dim=1, keepdim=True) + self.epsilon).pow(0.5)
        return x * (1. + torch.tanh(embedding * norm + self.beta))


class TorchBlock(nn.Module):
    def __init__(self, C, D, beta):
        super().__init__()
        self.twin = gates_train.conditioning_block(C, D, beta)       # the parameters only

    def forward(self, x, head):                                      # CLB:24-86 with the vector repair
        t = self.twin
        px1 = F.avg_pool2d(x, kernel_size=(x.size(-2), x.size(-1)))
        x_delta = (torch.sum(px1, dim=0, keepdim=True) - px1).squeeze(-1).squeeze(-1)
        s = t.CL_1.phi_layer(x)
        s = s.reshape(s.size(0), s.size(1), -1)
        z = x.reshape(x.size(0), x.size(1), -1)
        beta_val, _ = torch.topk(s, k=int(t.CL_1.beta_percentage * x.size(-1) * x.size(-2)), dim=-1, sorted=True)
        gap = F.avg_pool1d(z * (s > beta_val[..., -1, None]), kernel_size=z.size(-1)).squeeze(-1)
        code = torch.cat([t.CL_1.mlp_layer(gap), t.CL_2.mlp_layer(x_delta), t.CL_3.mlp_layer(head)], dim=1)
        a = 1. + torch.tanh(t.mlp_layer(code))
        return a.unsqueeze(-1).unsqueeze(-1) * x


def step_of(module, inputs, gy):
    def step():
        for t in inputs:
            t.grad = None
        for p in module.parameters():
            p.grad = None
        module(*inputs).backward(gy)
    return step


def grads_of(module, inputs):
    return [t.grad for t in inputs] + [p.grad for p in module.parameters() if p.grad is not None]


def measure(hip_step, torch_step):
    for _ in range(WARMUP):
        hip_step()
        torch_step()
    ms = {"hip": [], "torch": []}
    for _ in range(RUNS):
        for name, step in (("hip", hip_step), ("torch", torch_step)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return ms


def peak_of(step, holders):
    """one more call: the peak above what the inputs, the parameters and their gradients of the previous call hold"""
    for clear in holders:
        clear()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench(kind, where, h, w, C, D, gen):
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    x, head, gy = r(N_OBJ, C, h, w), r(N_OBJ, D), r(N_OBJ, C, h, w)
    if kind == "IA_gate":
        hip, ref = gates_train.IA_gate(D, C).cuda(), TorchIAGate(D, C).cuda()
        ref.load_state_dict(hip.state_dict())
        mk = lambda: [x.clone().requires_grad_(True), head.clone().requires_grad_(True)]
    elif kind == "GCT":
        hip, ref = gates_train.GCT(C).cuda(), TorchGCT(C).cuda()
        with torch.no_grad():
            hip.alpha.uniform_(0.5, 1.5)
            hip.gamma.normal_()
            hip.beta.normal_(std=0.5)
        ref.load_state_dict(hip.state_dict())
        mk = lambda: [x.clone().requires_grad_(True)]
    else:
        hip = gates_train.conditioning_block(C, D, 0.3).cuda()
        ref = TorchBlock(C, D, 0.3).cuda()
        ref.twin.load_state_dict(hip.state_dict())
        mk = lambda: [x.clone().requires_grad_(True), head.clone().requires_grad_(True)]
    in_hip, in_ref = mk(), mk()
    hip_step, torch_step = step_of(hip, in_hip, gy), step_of(ref, in_ref, gy)
    hip_step()
    torch_step()
    diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads_of(hip, in_hip), grads_of(ref, in_ref)))
    ms = measure(hip_step, torch_step)
    drop = lambda mod, ins: [lambda: [setattr(t, "grad", None) for t in ins], lambda: [setattr(p, "grad", None) for p in mod.parameters()]]
    peaks = peak_of(hip_step, drop(hip, in_hip) + drop(ref, in_ref)), peak_of(torch_step, drop(hip, in_hip) + drop(ref, in_ref))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = (f"{kind:18s} {where:24s} {h:3d}x{w:3d} c={C:3d} D={D:3d}  hip {med['hip']:7.3f} ms [{min(ms['hip']):.3f}, {max(ms['hip']):.3f}] peak {peaks[0] / 2**20:7.1f} MiB"
            f"   torch {med['torch']:7.3f} ms [{min(ms['torch']):.3f}, {max(ms['torch']):.3f}] peak {peaks[1] / 2**20:7.1f} MiB   max rel grad diff {diff:.1e}")
    return line, med["hip"] <= med["torch"], diff


def event_median(call):
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def kernels_alone(where, h, w, C, D, gen):
    """the launches of an IA_gate forward + backward one by one, outputs preallocated"""
    ops = aoc_amd.ops
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    x, gy, head, W, b, dgain = r(N_OBJ, C, h, w), r(N_OBJ, C, h, w), r(N_OBJ, D), r(C, D) / D ** 0.5, r(C), r(N_OBJ, C)
    gain, out, dg = ops.film_gain(head, W, b), torch.empty_like(x), torch.empty(N_OBJ, C, device="cuda")
    rows = (("film_gain", lambda: ops.film_gain(head, W, b)), ("film_scale", lambda: ops.film_scale(x, head, W, b, out=out)),
            ("channel_scale_grad, both outputs", lambda: gates_train.channel_scale_backward(gy, x, gain, out, dg)),
            ("channel_scale_grad, the plane dot alone", lambda: gates_train.channel_scale_backward(gy, x, None, None, dg, want_x=False)),
            ("channel_scale_grad, the scale alone", lambda: gates_train.channel_scale_backward(gy, None, gain, out, None, want_gain=False)),
            ("film_gain_grad", lambda: gates_train.film_gain_backward(dgain, gain, head, W)), ("torch.mul(grad_y, x)", lambda: torch.mul(gy, x, out=out)))
    return (f"kernels alone      {where:24s} {h:3d}x{w:3d} c={C:3d} D={D:3d}  {x.numel() * 4 / 1e6:.1f} MB per activation-sized stream: "
            + "; ".join(f"{name} {event_median(call):.3f} ms" for name, call in rows))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gates_grad_ab.txt")
    aoc_amd._lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"# Calibration gates, forward + backward, {N_OBJ} objects: (hip) aoc_amd.gates_train, (torch) the reference's lines in plain PyTorch; both arms "
             f"in one process, alternating; median [min, max] of {RUNS} after {WARMUP} warm-up calls; peak = max_memory_allocated above the inputs",
             f"# device: {torch.cuda.get_device_name(0)}"]
    failed = []
    for kind, shapes in (("IA_gate", GATE_SHAPES), ("GCT", GATE_SHAPES), ("conditioning_block", BLOCK_SHAPES)):
        for where, h, w, C, D, gate in shapes:
            line, ok, diff = bench(kind, where, h, w, C, D, gen)
            lines.append(line + (("   hip <= torch: " + ("yes" if ok else "NO")) if gate else ""))
            print(lines[-1], flush=True)
            if gate and not ok:
                failed.append(f"{kind} at {where}: the HIP median exceeds the PyTorch median")
            if not diff <= GRAD_TOL:
                failed.append(f"{kind} at {where} {h}x{w} c={C}: gradients differ by {diff:.1e} of the largest, tolerance {GRAD_TOL:.0e}")
            torch.cuda.empty_cache()
    for where, h, w, C, D, gate in GATE_SHAPES:
        if gate:
            lines.append(kernels_alone(where, h, w, C, D, gen))
            print(lines[-1], flush=True)
    lines += ["# FAILED: " + f for f in failed]
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    for f in failed:
        print("FAILED: " + f, file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
