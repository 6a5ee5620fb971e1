"""Developer tool (GPU box): forward + backward of the training criterion for ONE sample (aocnet.py:71-82 + Concat_CrossEntropyLoss), coarse
logits 117 x 117 -> the crop 465 x 465, in two arms, both in one process, alternating call by call:
  (hip)    aoc_amd.loss_train.Concat_CrossEntropyLoss.sample (csrc/loss_grad.hip: the upsampled logits are never formed);
  (torch)  the reference's lines in plain PyTorch on the device: F.interpolate(bilinear, align_corners=True), argmax, cross_entropy with
           ignore_index=255 and reduction='none', topk, mean; autograd's backward.
Rows: C = 4 and C = 6, at step 0 (k = every pixel) and past the mining step (k = 15 % of the pixels).  Per arm: WARMUP calls, then RUNS
calls each bracketed by two device events (median / min / max in ms), and torch.cuda.max_memory_allocated over one more call minus what
was allocated before it (the inputs alone).  Before the timing the two arms' gradients are compared and the largest difference relative
to the largest gradient printed.  The merge condition is the HIP arm's median at or below the PyTorch arm's of the same run in every row;
it is measured against PyTorch, never against itself.  Last, the four entry points alone (the wrappers, outputs preallocated): one call
between two device events, median of RUNS, with torch.topk over the same losses beside them.  The results are appended to the output file.
The exit status is 1 when a row says NO or a gradient difference exceeds GRAD_TOL.

    python tools/bench_loss_grad.py [out.txt]        # default: profiles/loss_grad_ab.txt
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
from aoc_amd import loss_train as lt  # noqa: E402
from bench_gates_grad import event_median, peak_of, WARMUP, RUNS  # noqa: E402

# Both arms sum float32 terms over up to 216 225 pixels in orders of their own; 1e-3 of the largest gradient separates that from a wrong
# gradient; the rounding bounds proper are the tests' (tests/loss_grad_bounds.py).
GRAD_TOL = 1e-3
h, w, H, W = 117, 117, 465, 465
TOP_K, MINING_STEP = 0.15, 100000


def torch_sample(pred, labels, k):
    up = F.interpolate(pred, size=(H, W), mode="bilinear", align_corners=True)            # aocnet.py:73
    all_pred = torch.argmax(up, dim=1)                                                      # :78
    losses = F.cross_entropy(up.view(1, up.size(1), -1), labels.view(1, -1), ignore_index=255, reduction="none")      # loss.py:79-82
    return torch.mean(torch.topk(losses, k=k, dim=1)[0]), all_pred                          # :90-93


def bench(C, step, gen):
    pred = 3.0 * torch.randn(1, C, h, w, device="cuda", generator=gen)
    labels = torch.randint(0, C, (1, H, W), device="cuda", generator=gen)
    labels[torch.rand(1, H, W, device="cuda", generator=gen) < 0.1] = 255
    crit = lt.Concat_CrossEntropyLoss(TOP_K, MINING_STEP)
    k = lt.top_k_pixels(TOP_K, MINING_STEP, step, H * W)
    ins = {a: pred.clone().requires_grad_(True) for a in ("hip", "torch")}

    def step_of(arm):
        def run():
            ins[arm].grad = None
            loss, _ = crit.sample(ins[arm], labels, step, (H, W)) if arm == "hip" else torch_sample(ins[arm], labels, k)
            loss.backward()
            return loss
        return run
    steps = {a: step_of(a) for a in ins}
    losses = {a: float(steps[a]().detach()) for a in ins}
    diff = float((ins["hip"].grad - ins["torch"].grad).abs().max() / ins["torch"].grad.abs().max().clamp_min(1e-30))
    for _ in range(WARMUP):
        for a in ins:
            steps[a]()
    ms = {a: [] for a in ins}
    for _ in range(RUNS):
        for a in ins:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            steps[a]()
            e1.record()
            e1.synchronize()
            ms[a].append(e0.elapsed_time(e1))
    drop = [lambda: [setattr(t, "grad", None) for t in ins.values()]]
    peaks = {a: peak_of(steps[a], drop) for a in ins}
    med = {a: float(np.median(v)) for a, v in ms.items()}
    line = f"criterion forward + backward  C={C} {h}x{w} -> {H}x{W}  step {step:6d} k {k:6d}  " + "   ".join(
        f"{a} {med[a]:7.3f} ms [{min(ms[a]):.3f}, {max(ms[a]):.3f}] peak {peaks[a] / 2**20:6.2f} MiB" for a in ins)
    line += f"   loss hip {losses['hip']:.6f} torch {losses['torch']:.6f}   max rel grad diff {diff:.1e}   (measured)"
    return line, med, diff


def kernels_alone(C, step, gen):
    pred = (3.0 * torch.randn(C, h, w, device="cuda", generator=gen)).contiguous()
    labels = torch.randint(0, C, (H * W,), device="cuda", generator=gen).to(torch.int32)
    k = lt.top_k_pixels(TOP_K, MINING_STEP, step, H * W)
    n = H * W
    out = dict(loss=torch.empty(n, device="cuda"), lse=torch.empty(n, device="cuda"), argmax=torch.empty(n, dtype=torch.int32, device="cuda"))
    loss, lse, _, _, _ = lt.upsample_ce_forward(pred, labels, (H, W), out=out)
    mean, thr, n_gt = lt.topk_mean(loss, k)
    mask = lt.topk_select_mask(loss, k, thr, n_gt)
    go, grad = torch.ones(1, device="cuda"), torch.empty_like(pred)
    rows = (("upsample_ce_forward", lambda: lt.upsample_ce_forward(pred, labels, (H, W), out=out)),
            ("topk_mean", lambda: lt.topk_mean(loss, k, mean, thr, n_gt)),
            ("topk_select_mask", lambda: lt.topk_select_mask(loss, k, thr, n_gt, mask)),
            ("upsample_ce_grad", lambda: lt.upsample_ce_backward(pred, labels, lse, mask, go, (H, W), k=k, grad_pred=grad)),
            ("torch.topk of the same losses", lambda: torch.topk(loss, k)))
    return (f"entries alone    C={C} {h}x{w} -> {H}x{W}  k {k:6d}: " + "; ".join(f"{name} {event_median(call):.3f} ms" for name, call in rows)
            + "   (measured)")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loss_grad_ab.txt")
    aoc_amd._lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = ["# training criterion of one sample, forward + backward: (hip) aoc_amd.loss_train.Concat_CrossEntropyLoss.sample, (torch) the reference's lines "
             f"in plain PyTorch; both arms in one process, alternating; median [min, max] of {RUNS} after {WARMUP} warm-up calls; peak = max_memory_allocated "
             "above the inputs", f"# device: {torch.cuda.get_device_name(0)}"]
    failed = []
    for C in (4, 6):
        for step in (0, 2 * MINING_STEP):
            line, med, diff = bench(C, step, gen)
            ok = med["hip"] <= med["torch"]
            lines.append(line + "   hip <= torch: " + ("yes" if ok else "NO"))
            print(lines[-1], flush=True)
            if not ok:
                failed.append(f"C={C} step {step}: the HIP median exceeds the PyTorch median")
            if not diff <= GRAD_TOL:
                failed.append(f"C={C} step {step}: gradients differ by {diff:.1e} of the largest, tolerance {GRAD_TOL:.0e}")
            torch.cuda.empty_cache()
    for C, step in ((4, 2 * MINING_STEP), (6, 0)):
        lines.append(kernels_alone(C, step, gen))
        print(lines[-1], flush=True)
    lines += ["# FAILED: " + f for f in failed]
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    for f in failed:
        print("FAILED: " + f, file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
