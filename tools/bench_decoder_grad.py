"""Developer tool (GPU box): forward + backward of the decoder's fused forms in two arms, both in one process, alternating call by call:
  (hip)   the twins of aoc_amd.decoder_train (csrc/norm_grad.hip behind them; the convolutions are torch's in both arms);
  (torch) the same lines as the reference writes them, in plain PyTorch on the device: ``F.group_norm``, ``+=``, ``relu`` and the gate's
          ``a * x`` (gct.py:69-90, ATT:12-17), ``torch.cat`` (decoding_module.py:193, :203), with the same parameters.
Shapes: the gated GroupNorm alone (bn3 of a Bottleneck with its residual and the IA_gate behind it) at N = 3, C = 256 and 512 on the
half-resolution map 61 x 107; one Bottleneck(512, 256) there; Modulator_1 at embed_dim = 256 with N = 3 (61 x 107) and N = 5 (73 x 131).
Per arm: WARMUP calls, then RUNS calls each bracketed by two device events (median / min / max in ms), and
torch.cuda.max_memory_allocated over one more call minus what was allocated before it (the inputs and parameters alone).  Before the
timing the gradients of the two arms are compared and the largest difference relative to the largest gradient printed, and beside it what
each arm is off a float64 run of the PyTorch arm by (the convolutions between the forms are MIOpen's in both arms, with their own error;
TF32 is switched off for both).  At every listed shape the HIP arm's median may not exceed the PyTorch arm's of the same run (the last
column says so).  Last, the two new entry points alone: one wrapper call between two device events, median of RUNS.  The results are
appended to the output file.  The exit status is 1 when a row says NO or a gradient difference exceeds GRAD_TOL.

    python tools/bench_decoder_grad.py [out.txt]        # default: profiles/decoder_grad_ab.txt
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import aoc_amd  # noqa: E402
from aoc_amd import decoder_train as dt, gates_train  # noqa: E402
from bench_gates_grad import TorchGCT, TorchIAGate, event_median, grads_of, measure, peak_of, step_of, WARMUP, RUNS  # noqa: E402

# Both arms sum float32 products over up to 16 x 6 527 terms in orders of their own, and MIOpen's convolutions sit between them: a few 1e-6 of
# the largest gradient in practice.  1e-3 of the largest separates that from a wrong gradient; the rounding bounds proper are the tests'.
GRAD_TOL = 1e-3
D = 400


class TorchGatedNorm(nn.Module):
    """bn3 of a Bottleneck with the residual, the ReLU and the gate behind it, as separate PyTorch passes"""

    def __init__(self, C, head_dim):
        super().__init__()
        self.bn = nn.GroupNorm(32, C)
        self.IA = nn.Linear(head_dim, C)

    def forward(self, x, residual, IA_head):
        out = F.group_norm(x, 32, self.bn.weight, self.bn.bias, self.bn.eps)
        out += residual
        out = torch.relu(out)
        a = 1. + torch.tanh(self.IA(IA_head))
        return a.unsqueeze(-1).unsqueeze(-1) * out


class HipGatedNorm(TorchGatedNorm):
    def forward(self, x, residual, IA_head):
        return dt.groupnorm_relu(x, 32, self.bn.weight, self.bn.bias, self.bn.eps, residual, True, gate=(IA_head, self.IA.weight, self.IA.bias))


class TorchBottleneck(dt.Bottleneck):
    """the twin's parameters, gct.py:70-91 in plain PyTorch"""

    def __init__(self, *a):
        super().__init__(*a)
        self.GCT1 = TorchGCT(self.conv1.in_channels)

    def forward(self, x):
        residual = x
        out = torch.relu(self.bn1(self.conv1(self.GCT1(x))))
        out = torch.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            residual = self.downsample(x)
        out += residual
        return torch.relu(out)


class Decoder(nn.Module):
    """M1_* of CalibrationDecoding (decoding_module.py:55-62); hip: the twins bound as INTEGRATION.md says; torch: :192-200 as written"""

    def __init__(self, e, head_dim, hip):
        super().__init__()
        gate, block = (gates_train.IA_gate, dt.Bottleneck) if hip else (TorchIAGate, TorchBottleneck)
        for i, (cin, cout) in enumerate(((2 * e, 2 * e), (2 * e, e), (e, e)), 1):
            setattr(self, f"M1_Reweight_Layer_{i}", gate(head_dim, cin))
            setattr(self, f"M1_Bottleneck_{i}", block(cin, cout, 1))
        self.hip = hip

    def forward(self, x, x_memory, IA_head):
        if self.hip:
            return dt.Modulator_1(self, x, x_memory, IA_head)
        x = torch.cat([x, x_memory], dim=1)
        for i in (1, 2, 3):
            x = getattr(self, f"M1_Reweight_Layer_{i}")(x, IA_head)
            x = getattr(self, f"M1_Bottleneck_{i}")(x)
        return x


def randomise(module, gen):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if "GCT1.alpha" in name:
                p.uniform_(0.5, 1.5, generator=gen)
            elif "GCT1" in name or name.endswith("bias"):
                p.normal_(std=0.5, generator=gen)
            elif p.dim() == 1:
                p.copy_(1.0 + 0.25 * torch.randn(p.shape, device=p.device, generator=gen))


def bench(kind, N, C, h, w, gen):
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    if kind == "gated GroupNorm":
        hip, ref = HipGatedNorm(C, D).cuda(), TorchGatedNorm(C, D).cuda()
        base = [(r(N, C, h, w), True), (r(N, C, h, w), True), (r(N, D), True)]
        out_c = C
    elif kind == "Bottleneck":
        hip, ref = dt.Bottleneck(C, C // 2).cuda(), TorchBottleneck(C, C // 2).cuda()
        base = [(r(N, C, h, w), True)]
        out_c = C // 2
    else:
        hip, ref = Decoder(C, D, True).cuda(), Decoder(C, D, False).cuda()
        x = r(N, C, h, w)
        base = [(x, True), (x.clone(), False), (r(N, D), True)]                 # the first frame's self-memory, detached (decoding_module.py:133)
        out_c = C
    randomise(hip, gen)
    ref.load_state_dict(hip.state_dict())
    gy = r(N, out_c, h, w)
    mk = lambda: [t.clone().requires_grad_(g) for t, g in base]
    in_hip, in_ref = mk(), mk()
    hip_step, torch_step = step_of(hip, in_hip, gy), step_of(ref, in_ref, gy)
    hip_step()
    torch_step()
    g_hip, g_ref = grads_of(hip, in_hip), grads_of(ref, in_ref)
    assert [g is None for g in g_hip] == [g is None for g in g_ref]
    diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(g_hip, g_ref) if a is not None)
    # where the arms differ, which one is off: the PyTorch arm once more in float64 (not timed)
    ref64 = copy.deepcopy(ref).double()
    in_64 = [t.clone().double().requires_grad_(g) for t, g in base]
    step_of(ref64, in_64, gy.double())()
    off = [max(float((a.double() - c).abs().max() / c.abs().max().clamp_min(1e-300)) for a, c in zip(g, grads_of(ref64, in_64)) if a is not None)
           for g in (g_hip, g_ref)]
    del ref64, in_64
    ms = measure(hip_step, torch_step)
    drop = lambda mod, ins: [lambda: [setattr(t, "grad", None) for t in ins], lambda: [setattr(p, "grad", None) for p in mod.parameters()]]
    peaks = peak_of(hip_step, drop(hip, in_hip) + drop(ref, in_ref)), peak_of(torch_step, drop(hip, in_hip) + drop(ref, in_ref))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    what = {"gated GroupNorm": f"C={C}", "Bottleneck": f"({C}, {C // 2})", "Modulator_1": f"embed_dim={C}"}[kind]
    line = (f"{kind:16s} {what:14s} N={N} {h:3d}x{w:3d}  hip {med['hip']:7.3f} ms [{min(ms['hip']):.3f}, {max(ms['hip']):.3f}] peak {peaks[0] / 2**20:7.1f} MiB"
            f"   torch {med['torch']:7.3f} ms [{min(ms['torch']):.3f}, {max(ms['torch']):.3f}] peak {peaks[1] / 2**20:7.1f} MiB   max rel grad diff {diff:.1e}"
            f" (against float64: hip {off[0]:.1e}, torch {off[1]:.1e})   (measured)")
    return line, med["hip"] <= med["torch"], diff


def kernels_alone(N, C, h, w, gen):
    """the two new entry points one by one, outputs allocated by the wrappers"""
    ops = aoc_amd.ops
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    x, res, gy, gm, be, gain = r(N, C, h, w), r(N, C, h, w), r(N, C, h, w), 1 + 0.25 * r(C), r(C), 1 + torch.tanh(r(N, C))
    _, stats = dt.groupnorm_relu_forward(x, 32, gm, be, 1e-5, res, True)
    mem, gy2, gain2, out = r(N, C, h, w), r(N, 2 * C, h, w), 1 + torch.tanh(r(N, 2 * C)), torch.empty(N, C, h, w, device="cuda")
    rows = (("groupnorm_relu forward", lambda: ops.groupnorm_relu(x, 32, gm, be, 1e-5, res, True, out=out)),
            ("groupnorm_relu_grad, all five outputs", lambda: dt.groupnorm_relu_backward(gy, x, stats, 32, gm, be, res, True, gain)),
            ("groupnorm_relu_grad, grad_x alone", lambda: dt.groupnorm_relu_backward(gy, x, stats, 32, gm, be, res, True, gain, want=(True, False, False, False, False))),
            ("groupnorm_relu_grad, dgain alone (the plane pass)", lambda: dt.groupnorm_relu_backward(gy, x, stats, 32, gm, be, res, True, gain,
                                                                                                      want=(False, False, False, False, True))),
            ("cat_film_scale_grad, grad_x + dgain", lambda: dt.cat_film_scale_backward(gy2, x, mem, gain2)),
            ("torch.mul(grad_y, x)", lambda: torch.mul(gy, x, out=out)))
    return (f"kernels alone    C={C} N={N} {h:3d}x{w:3d}  {x.numel() * 4 / 1e6:.1f} MB per activation-sized stream: "
            + "; ".join(f"{name} {event_median(call):.3f} ms" for name, call in rows) + "   (measured)")


SHAPES = [("gated GroupNorm", 3, 256, 61, 107), ("gated GroupNorm", 3, 512, 61, 107), ("Bottleneck", 3, 512, 61, 107), ("Modulator_1", 3, 256, 61, 107),
          ("Modulator_1", 5, 256, 73, 131)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decoder_grad_ab.txt")
    aoc_amd._lib.lib()
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False      # float32 convolutions in both arms
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = ["# Decoder forms, forward + backward: (hip) aoc_amd.decoder_train, (torch) the reference's lines in plain PyTorch; both arms in one process, "
             f"alternating; median [min, max] of {RUNS} after {WARMUP} warm-up calls; peak = max_memory_allocated above the inputs",
             f"# device: {torch.cuda.get_device_name(0)}"]
    failed = []
    for kind, N, C, h, w in SHAPES:
        line, ok, diff = bench(kind, N, C, h, w, gen)
        lines.append(line + "   hip <= torch: " + ("yes" if ok else "NO"))
        print(lines[-1], flush=True)
        if not ok:
            failed.append(f"{kind} C={C} N={N}: the HIP median exceeds the PyTorch median")
        if not diff <= GRAD_TOL:
            failed.append(f"{kind} C={C} N={N} {h}x{w}: gradients differ by {diff:.1e} of the largest, tolerance {GRAD_TOL:.0e}")
        torch.cuda.empty_cache()
    for C in (256, 512):
        lines.append(kernels_alone(3, C, 61, 107, gen))
        print(lines[-1], flush=True)
    lines += ["# FAILED: " + f for f in failed]
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    for f in failed:
        print("FAILED: " + f, file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
