"""Developer tool (GPU box): forward + backward of the decoder's tail in two arms, both in one process, alternating call by call:
  (hip)   the twins of aoc_amd.tail_train (csrc/tail_grad.hip behind them; the convolutions are torch's in both arms);
  (torch) the same lines as the reference writes them, in plain PyTorch on the device: ``F.interpolate(mode='bicubic', align_corners=True)``,
          ``torch.cat``, ``avg_pool2d``, px1_delta and the gate's ``a * x`` (decoding_module.py:163, 170-176), ``IA_logit`` as the grouped
          ``F.conv2d`` and ``augment_background_logit`` with ``torch.min`` (:151-160, 213-225), with the same parameters.
Rows, all at N = 3 (tools/bench_decoder_tail.py's shapes):
  1. the shortcut stage alone at Ce = 256, Cr = 64, 61 x 107 -> 121 x 213;
  2. the logit head alone at its C = 128 and 121 x 213;
  3. decoder_final + predict whole (embed_dim 256, refine_dim 64, low_level_dim 256).
Per arm: WARMUP calls, then RUNS calls each bracketed by two device events (median / min / max in ms), and torch.cuda.max_memory_allocated
over one more call minus what was allocated before it.  Before the timing the gradients of the two arms are compared (the largest difference
relative to the largest gradient), and beside it what each arm is off a float64 run of the PyTorch arm by; TF32 is switched off for both.
On rows 1 and 2 (no ReLU, no convolution inside) the HIP arm's median may not exceed the PyTorch arm's of the same run and the gradients
must agree to GRAD_TOL, else the exit status is 1; row 3 (a chain with ReLUs, see STATUS.md) only reports.  The results are appended to the
output file.

    python tools/bench_tail_grad.py [out.txt]        # default: profiles/tail_grad_ab.txt
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
from aoc_amd import gates_train, tail_train as tt  # noqa: E402
from bench_gates_grad import GRAD_TOL, TorchGCT, TorchIAGate, grads_of, measure, peak_of, step_of, WARMUP, RUNS  # noqa: E402  (GRAD_TOL: the rationale is there)

D = 400


def _delta(x):
    px1 = F.avg_pool2d(x, kernel_size=(x.size()[-2], x.size()[-1]), padding=0)
    return (torch.sum(px1, dim=0, keepdim=True) - px1).squeeze(-1).squeeze(-1)


class Stage(nn.Module):
    def __init__(self, Ce, Cr, hip):
        super().__init__()
        self.IA10 = (gates_train.IA_gate if hip else TorchIAGate)(D + Ce + Cr, Ce + Cr)
        self.hip = hip

    def forward(self, x, low, IA_head):
        if self.hip:
            return tt.shortcut_stage(x, low, IA_head, self.IA10.IA.weight, self.IA10.IA.bias)
        x = F.interpolate(x, size=low.size()[2:], mode='bicubic', align_corners=True)
        x = torch.cat([x, low], dim=1)
        return self.IA10(x, torch.cat([IA_head, _delta(x)], dim=1))


def torch_predict(dec, x, IA_head):
    def ia_logit(IA_final):
        n, c, h, w = x.size()
        out = IA_final(IA_head)
        return F.conv2d(x.view(1, n * c, h, w), weight=out[:, :c].view(n, c, 1, 1), bias=out[:, -1].view(-1), groups=n).view(n, 1, h, w)
    fg, bg = ia_logit(dec.IA_final_fg), ia_logit(dec.IA_final_bg)
    pred = fg
    if fg.size(0) > 1:
        aug, _ = torch.min(bg[1:], dim=0, keepdim=True)
        pred = pred + torch.cat([aug, torch.zeros(aug.size(), device=aug.device).expand(fg.size(0) - 1, -1, -1, -1)], dim=0)
    return pred.permute(1, 0, 2, 3)


class Head(nn.Module):
    def __init__(self, C, hip):
        super().__init__()
        self.IA_final_fg, self.IA_final_bg = nn.Linear(D, C + 1), nn.Linear(D, C + 1)
        self.hip = hip

    def forward(self, x, IA_head):
        return tt.predict(self, x, IA_head) if self.hip else torch_predict(self, x, IA_head)


class Tail(nn.Module):
    """decoding_module.py:74-89; hip: the twins bound as INTEGRATION.md says; torch: :162-190 and :144-147 as written"""

    def __init__(self, e, r, low_dim, hip):
        super().__init__()
        gate = gates_train.IA_gate if hip else TorchIAGate
        self.GCT_sc = (gates_train.GCT if hip else TorchGCT)(low_dim + e)
        self.conv_sc = nn.Conv2d(low_dim + e, r, 1, bias=False)
        self.bn_sc = nn.GroupNorm(int(r / 4), r)
        self.IA10 = gate(D + e + r, e + r)
        self.conv1 = nn.Conv2d(e + r, int(e / 2), kernel_size=3, padding=1, bias=False)
        self.bn1 = nn.GroupNorm(32, int(e / 2))
        self.IA11 = gate(D + int(e / 2), int(e / 2))
        self.conv2 = nn.Conv2d(int(e / 2), int(e / 2), kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.GroupNorm(32, int(e / 2))
        self.IA_final_fg, self.IA_final_bg = nn.Linear(D, int(e / 2) + 1), nn.Linear(D, int(e / 2) + 1)
        self.hip = hip

    def forward(self, x, low_level_feat, IA_head):
        if self.hip:
            return tt.predict(self, tt.decoder_final(self, x, low_level_feat, IA_head), IA_head)
        x = F.interpolate(x, size=low_level_feat.size()[2:], mode='bicubic', align_corners=True)
        low = torch.relu(self.bn_sc(self.conv_sc(self.GCT_sc(low_level_feat))))
        x = torch.cat([x, low], dim=1)
        x = self.IA10(x, torch.cat([IA_head, _delta(x)], dim=1))
        x = torch.relu(self.bn1(self.conv1(x)))
        x = self.IA11(x, torch.cat([IA_head, _delta(x)], dim=1))
        x = torch.relu(self.bn2(self.conv2(x)))
        return torch_predict(self, x, IA_head)


def randomise(module, gen):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if "GCT_sc.alpha" in name:
                p.uniform_(0.5, 1.5, generator=gen)
            elif "GCT_sc" in name or (name.startswith("bn") and name.endswith("bias")):
                p.normal_(std=0.5, generator=gen)
            elif name.startswith("bn"):
                p.copy_(1.0 + 0.25 * torch.randn(p.shape, device=p.device, generator=gen))


def bench(kind, N, h, w, H, W, gen):
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    if kind == "shortcut stage":
        Ce, Cr = 256, 64
        hip, ref = Stage(Ce, Cr, True).cuda(), Stage(Ce, Cr, False).cuda()
        base = [(r(N, Ce, h, w), True), (torch.relu(r(N, Cr, H, W)), True), (r(N, D), True)]
        out_shape, what = (N, Ce + Cr, H, W), f"Ce={Ce} Cr={Cr}"
    elif kind == "logit head":
        C = 128
        hip, ref = Head(C, True).cuda(), Head(C, False).cuda()
        base = [(r(N, C, H, W), True), (r(N, D), True)]
        out_shape, what = (1, N, H, W), f"C={C}"
    else:
        e, rd, ld = 256, 64, 256
        hip, ref = Tail(e, rd, ld, True).cuda(), Tail(e, rd, ld, False).cuda()
        base = [(r(N, e, h, w), True), (r(N, ld + e, H, W), True), (r(N, D), True)]
        out_shape, what = (1, N, H, W), f"embed_dim={e}"
    randomise(hip, gen)
    ref.load_state_dict(hip.state_dict())
    gy = r(*out_shape)
    mk = lambda: [t.clone().requires_grad_(g) for t, g in base]
    in_hip, in_ref = mk(), mk()
    hip_step, torch_step = step_of(hip, in_hip, gy), step_of(ref, in_ref, gy)
    hip_step()
    torch_step()
    g_hip, g_ref = grads_of(hip, in_hip), grads_of(ref, in_ref)
    assert [g is None for g in g_hip] == [g is None for g in g_ref]
    diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(g_hip, g_ref) if a is not None)
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
    line = (f"{kind:24s} {what:14s} N={N} {h:3d}x{w:3d} -> {H:3d}x{W:3d}  hip {med['hip']:7.3f} ms [{min(ms['hip']):.3f}, {max(ms['hip']):.3f}] peak "
            f"{peaks[0] / 2**20:7.1f} MiB   torch {med['torch']:7.3f} ms [{min(ms['torch']):.3f}, {max(ms['torch']):.3f}] peak {peaks[1] / 2**20:7.1f} MiB   "
            f"max rel grad diff {diff:.1e} (against float64: hip {off[0]:.1e}, torch {off[1]:.1e})   (measured)")
    return line, med["hip"] <= med["torch"], diff


ROWS = [("shortcut stage", True), ("logit head", True), ("decoder_final + predict", False)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tail_grad_ab.txt")
    aoc_amd._lib.lib()
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False      # float32 convolutions and products in both arms
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = ["# Decoder tail, forward + backward: (hip) aoc_amd.tail_train, (torch) the reference's lines in plain PyTorch; both arms in one process, "
             f"alternating; median [min, max] of {RUNS} after {WARMUP} warm-up calls; peak = max_memory_allocated above the inputs",
             f"# device: {torch.cuda.get_device_name(0)}"]
    failed = []
    for kind, binding in ROWS:
        line, ok, diff = bench(kind, 3, 61, 107, 121, 213, gen)
        lines.append(line + "   hip <= torch: " + ("yes" if ok else "NO") + ("" if binding else "   (reported only)"))
        print(lines[-1], flush=True)
        if binding and not ok:
            failed.append(f"{kind}: the HIP median exceeds the PyTorch median")
        if binding and not diff <= GRAD_TOL:
            failed.append(f"{kind}: gradients differ by {diff:.1e} of the largest, tolerance {GRAD_TOL:.0e}")
        torch.cuda.empty_cache()
    lines += ["# FAILED: " + f for f in failed]
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    for f in failed:
        print("FAILED: " + f, file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
