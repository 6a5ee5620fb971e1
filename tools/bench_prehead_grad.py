"""Developer tool (GPU box): forward + backward of DynamicPreHead with the concatenation behind it (aocnet.py:360-362) in two arms, both in
one process, alternating call by call:
  (hip)   the twin aoc_amd.prehead_train.DynamicPreHead called as ``twin(x, cur.permute(1, 2, 0))`` (aoc_prehead forward, csrc/prehead_grad.hip
          backward);
  (torch) the reference's lines in plain PyTorch on the device: ``nn.Conv2d(24, 64, 1)``, ``nn.GroupNorm(16, 64)``, ``nn.ReLU`` and ``torch.cat``
          with the embedding expanded over the objects, with the same parameters.
Shapes: four objects, C = 100, at the 117 x 117 training crop and at cfg2's 121 x 213 map.  Per arm: WARMUP calls, then RUNS calls each
bracketed by two device events (median / min / max in ms), and torch.cuda.max_memory_allocated over one more call minus what was allocated
before it (the inputs and parameters alone).  Then the two entry points alone: one wrapper call between two device events, median of RUNS.

Before the timing the gradients of the two arms are compared element by element: they may differ by at most the sum of the two arms'
derived bounds around the float64 reference (tests/prehead_grad_bounds.prehead_grad_ref: for the HIP arm the kernels' own analysis; for
the PyTorch arm, whose kernels are not ours, the same expressions with every sum taken in float32 in whatever order -- PyTorch groups the
terms of the GroupNorm backward in its own way, which that analysis does not follow term by term; the line also says what each arm is off
the float64 reference by, relative to its bound).  At this size some elements always lie within rounding of the ReLU's corner, where either
arm may decide either way: the tool sets the cotangent to 0 on the elements that either analysis calls undecided (the count is printed), so
that they contribute to no gradient whichever way they fall; the work of both arms is unchanged.

The exit status is 1 when the HIP arm's median exceeds the PyTorch arm's of the same run at either shape (the merge condition for a
training twin) or a gradient leaves the summed bounds.  The results are appended to the output file.

    python tools/bench_prehead_grad.py [out.txt]        # default: profiles/prehead_grad_ab.txt
"""
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aoc_amd  # noqa: E402
from aoc_amd import prehead_train as pt  # noqa: E402
from bench_gates_grad import event_median, grads_of, measure, peak_of, step_of, WARMUP, RUNS  # noqa: E402
import prehead_grad_bounds as pgb  # noqa: E402

N_OBJ, C, N_IN, N_OUT = 4, 100, 24, 64
SHAPES = [("training crop", 117, 117), ("cfg2 map", 121, 213)]


class TorchPreHead(nn.Module):
    """decoding_module.py:228-240 and aocnet.py:188, 362 as separate PyTorch passes"""

    def __init__(self, in_dim, embed_dim):
        super().__init__()
        self.conv = nn.Conv2d(in_dim, embed_dim, kernel_size=1, stride=1, padding=0)
        self.bn = nn.GroupNorm(int(embed_dim / 4), embed_dim)
        self.relu = nn.ReLU(True)

    def forward(self, x, cur):
        x = self.relu(self.bn(self.conv(x)))
        return torch.cat((cur.unsqueeze(0).expand(x.shape[0], -1, -1, -1), x), 1)


class HipPreHead(pt.DynamicPreHead):
    def forward(self, x, cur):
        return super().forward(x, cur.permute(1, 2, 0))


def bench(where, h, w, gen):
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    hw = h * w
    hip, ref = HipPreHead(N_IN, N_OUT).cuda(), TorchPreHead(N_IN, N_OUT).cuda()
    with torch.no_grad():
        hip.bn.weight.copy_(1.0 + 0.25 * r(N_OUT))
        hip.bn.bias.copy_(0.5 * r(N_OUT))
        hip.conv.bias.copy_(0.2 * r(N_OUT))
    ref.load_state_dict(hip.state_dict())
    x, cur, gy = r(N_OBJ, N_IN, h, w), r(C, h, w), r(N_OBJ, C + N_OUT, h, w)
    # the float64 reference with both arms' bounds; the cotangent is 0 wherever either analysis cannot tell the side of the ReLU's corner
    host = lambda t: t.detach().cpu().numpy()
    args = dict(feat=host(x).reshape(N_OBJ, N_IN, hw), weight=host(hip.conv.weight), bias=host(hip.conv.bias), n_groups=hip.bn.num_groups,
                gn_w=host(hip.bn.weight), gn_b=host(hip.bn.bias), eps=hip.bn.eps, C=C)
    g0 = host(gy).reshape(N_OBJ, C + N_OUT, hw)
    und = pgb.prehead_grad_ref(grad_out=g0, **args)[1] | pgb.prehead_grad_ref(grad_out=g0, any_order=True, **args)[1]
    gy.view(N_OBJ, C + N_OUT, hw)[:, C:][und.to(gy.device)] = 0.0
    g0 = host(gy).reshape(N_OBJ, C + N_OUT, hw)
    ours, _ = pgb.prehead_grad_ref(grad_out=g0, **args)
    theirs, _ = pgb.prehead_grad_ref(grad_out=g0, any_order=True, **args)
    mk = lambda: [x.clone().requires_grad_(True), cur.clone().requires_grad_(True)]
    in_hip, in_ref = mk(), mk()
    hip_step, torch_step = step_of(hip, in_hip, gy), step_of(ref, in_ref, gy)
    hip_step()
    torch_step()
    g_hip, g_ref = grads_of(hip, in_hip), grads_of(ref, in_ref)
    names = ("grad_feat", "grad_emb", "grad_weight", "grad_bias", "grad_gamma", "grad_beta")        # the inputs, then conv and bn in parameter order
    shape = lambda n, t: pgb.t64(t).reshape(C, hw).t() if n == "grad_emb" else pgb.t64(t).reshape(ours[n][0].shape)
    worst, off = 0.0, [0.0, 0.0]
    for n, a, b in zip(names, g_hip, g_ref):
        a, b = shape(n, a), shape(n, b)
        want, t_ours, t_theirs = ours[n][0], ours[n][1], theirs[n][1]
        ratio = lambda err, tol: float(torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300)).max())
        worst = max(worst, ratio((a - b).abs(), t_ours + t_theirs))
        off = [max(off[0], ratio((a - want).abs(), t_ours)), max(off[1], ratio((b - want).abs(), t_theirs))]
    ms = measure(hip_step, torch_step)
    drop = lambda mod, ins: [lambda: [setattr(t, "grad", None) for t in ins], lambda: [setattr(p, "grad", None) for p in mod.parameters()]]
    peaks = peak_of(hip_step, drop(hip, in_hip) + drop(ref, in_ref)), peak_of(torch_step, drop(hip, in_hip) + drop(ref, in_ref))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = (f"DynamicPreHead + cat  {where:14s} O={N_OBJ} C={C} {N_IN}->{N_OUT} {h:3d}x{w:3d}  hip {med['hip']:7.3f} ms [{min(ms['hip']):.3f}, {max(ms['hip']):.3f}] "
            f"peak {peaks[0] / 2**20:7.1f} MiB   torch {med['torch']:7.3f} ms [{min(ms['torch']):.3f}, {max(ms['torch']):.3f}] peak {peaks[1] / 2**20:7.1f} MiB   "
            f"largest |hip - torch| / (sum of the arms' bounds) {worst:.3f} (against float64, error / own bound: hip {off[0]:.3f}, torch {off[1]:.3f}; "
            f"{int(und.sum())} of {und.numel()} cotangent elements zeroed)   (measured)")
    # the entry points alone, outputs allocated by the wrappers
    pars = [t.detach() for t in (hip.conv.weight, hip.conv.bias, hip.bn.weight, hip.bn.bias)]
    emb = cur.permute(1, 2, 0).contiguous()
    fwd = lambda: pt.prehead_forward(x, pars[0], pars[1], hip.bn.num_groups, pars[2], pars[3], hip.bn.eps, emb)
    _, stats = fwd()
    bwd = lambda want: (lambda: pt.prehead_backward(gy, x, stats, pars[0], pars[1], hip.bn.num_groups, pars[2], pars[3], C, want=want))
    rows = (("aoc_prehead", fwd), ("aoc_prehead_grad, all six outputs", bwd((True,) * 6)), ("grad_feat alone", bwd((True,) + (False,) * 5)),
            ("grad_gamma + grad_beta (plane pass + small sums)", bwd((False, False, False, True, True, False))),
            ("grad_emb alone", bwd((False,) * 5 + (True,))))
    alone = (f"entries alone         {where:14s} O={N_OBJ} C={C} {N_IN}->{N_OUT} {h:3d}x{w:3d}  "
             + "; ".join(f"{name} {event_median(call):.3f} ms" for name, call in rows) + "   (measured)")
    return line, alone, med["hip"] <= med["torch"], worst


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prehead_grad_ab.txt")
    aoc_amd._lib.lib()
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False      # a float32 convolution in the PyTorch arm
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = ["# DynamicPreHead + concatenation, forward + backward: (hip) aoc_amd.prehead_train.DynamicPreHead, (torch) the reference's lines in plain PyTorch; "
             f"both arms in one process, alternating; median [min, max] of {RUNS} after {WARMUP} warm-up calls; peak = max_memory_allocated above the inputs",
             f"# device: {torch.cuda.get_device_name(0)}"]
    failed = []
    for where, h, w in SHAPES:
        line, alone, ok, worst = bench(where, h, w, gen)
        lines += [line + "   hip <= torch: " + ("yes" if ok else "NO"), alone]
        print(lines[-2] + "\n" + lines[-1], flush=True)
        if not ok:
            failed.append(f"{where} {h}x{w}: the HIP median exceeds the PyTorch median")
        if not worst <= 1.0:
            failed.append(f"{where} {h}x{w}: the arms' gradients differ by {worst:.3f} of the sum of their bounds")
        torch.cuda.empty_cache()
    lines += ["# FAILED: " + f for f in failed]
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    for f in failed:
        print("FAILED: " + f, file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
