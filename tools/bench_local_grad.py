"""Developer tool (GPU box): forward + backward of the differentiable local matching (aoc_amd.local_train.local_matching) against the same
function written as plain PyTorch on the device: down-sample, the previous frame unfolded into [C, (2R+1)^2, HW] neighbourhoods, masked
distances, nested-window minima, transform, up-sample, autograd.  That formulation keeps the unfolded operand and the masked distance
volume for its backward.

Shapes: the training crop, 117 x 117 (matched at 59 x 59), and cfg2's map, 121 x 213 (61 x 107); C = 100, four objects, radii
[2, 4, 6, 8, 10, 12], allow_downsample=True, 85 % of the previous frame labelled.  Per path: WARMUP calls, then RUNS calls of forward +
backward each bracketed by two device events (median / min / max in ms), and torch.cuda.max_memory_allocated over the timed calls minus
what was allocated before them: the inputs alone, the gradients of the warm-up calls are dropped first.  Before the timing the two paths'
gradients are compared; the nearest pixel is a discontinuous choice, so pixels whose query gradient differs by more than 1e-4 (near ties
that the two summation orders resolve differently) are counted and the others compared.  The one expectation that follows from the shapes
alone: the HIP path's peak holds no C (2R+1)^2 HW term (printed beside it).  The results are appended to the output file.

    python tools/bench_local_grad.py [out.txt]        # default: profiles/local_grad_ab.txt
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import aoc_amd  # noqa: E402

WARMUP, RUNS = 3, 20
C, N_OBJ = 100, 4
RADII = [2, 4, 6, 8, 10, 12]
SHAPES = [("training crop", 117, 117), ("cfg2 map", 121, 213)]
PAD = 5e4


def torch_local_matching(prev, query, labels, bias, radii):
    """Nearest right pixel per object and nested window as PyTorch composes it.  prev, query [h, w, C]; labels [h, w, O]; bias [O, 1, 1, 1].
    -> [1, h, w, O, len(radii)], channel order [largest, r_0, r_1, ...]."""
    h, w, c = query.shape
    n_obj, R = labels.shape[2], radii[-1]
    K = 2 * R + 1
    H, W = h // 2 + 1, w // 2 + 1
    x = F.interpolate(query.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=True)
    y = F.interpolate(prev.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=True)
    lab = F.interpolate(labels.permute(2, 0, 1)[:, None], size=(H, W), mode="nearest")
    near = F.unfold(F.pad(y, (R, R, R, R)), kernel_size=K).view(c, K * K, H * W)                      # the unfolded operand
    y2 = F.unfold(F.pad((y * y).sum(1, keepdim=True), (R, R, R, R), value=PAD), kernel_size=K).view(K * K, H * W)
    xf = x.view(c, H * W)
    d = (xf * xf).sum(0)[None, :] + y2 - 2.0 * (xf[:, None, :] * near).sum(0)                         # [K K, HW]
    mask = F.unfold(F.pad(lab, (R, R, R, R)), kernel_size=K).view(n_obj, K, K, H * W) > 0.9
    dm = torch.where(mask, d.view(1, K, K, H * W), torch.full((), PAD, device=d.device))
    mins = [dm.reshape(n_obj, K * K, H * W).amin(1)]
    for r in radii[:-1]:
        mins.append(dm[:, R - r:R + r + 1, R - r:R + r + 1].reshape(n_obj, -1, H * W).amin(1))
    T = (torch.sigmoid(torch.stack(mins, 1) + bias.view(-1, 1, 1)) - 0.5) * 2.0
    T = F.interpolate(T.view(n_obj, len(radii), H, W), size=(h, w), mode="bilinear", align_corners=True)
    return T.permute(2, 3, 0, 1).reshape(1, h, w, n_obj, len(radii))


def timed(step, clear):
    for _ in range(WARMUP):
        step()
    clear()                                     # nothing of the warm-up calls stays allocated: the baseline is the inputs alone
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms), torch.cuda.max_memory_allocated() - base


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "local_grad_ab.txt")
    aoc_amd._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    s = 1.0 / np.sqrt(C)
    lines = [f"# Local matching, forward + backward: local_train.local_matching (HIP) against plain PyTorch (unfold) on the device; C = {C}, "
             f"{N_OBJ} objects, radii {RADII}, allow_downsample=True;", f"# {RUNS} runs after {WARMUP}, ms per forward + backward: median / min / max; "
             f"peak = max_memory_allocated above the inputs.  Device: {torch.cuda.get_device_name(0)}"]
    for what, h, w in SHAPES:
        H, W = h // 2 + 1, w // 2 + 1
        prev = (s * torch.randn(h, w, C, device="cuda", generator=g)).requires_grad_(True)
        query = (s * torch.randn(h, w, C, device="cuda", generator=g)).requires_grad_(True)
        bias = (0.3 * torch.randn(N_OBJ, 1, 1, 1, device="cuda", generator=g)).requires_grad_(True)
        owner = torch.randint(0, N_OBJ, (h, w), device="cuda", generator=g)
        labelled = torch.rand(h, w, device="cuda", generator=g) < 0.85
        labels = F.one_hot(owner, N_OBJ).float() * labelled[:, :, None]
        weight = torch.randn(1, h, w, N_OBJ, len(RADII), device="cuda", generator=g)

        def clear():
            prev.grad = query.grad = bias.grad = None

        def hip_step():
            clear()
            out = aoc_amd.local_train.local_matching(prev, query, labels, bias, RADII, None, 1, False, True, True)
            (out * weight).sum().backward()

        def torch_step():
            clear()
            out = torch_local_matching(prev, query, labels, bias, RADII)
            (out * weight).sum().backward()

        hip_step()
        got = [t.grad.clone() for t in (query, prev, bias)]
        out_hip = aoc_amd.local_train.local_matching(prev, query, labels, bias, RADII, None, 1, False, True, True).detach()
        torch_step()
        out_diff = float((out_hip - torch_local_matching(prev, query, labels, bias, RADII).detach()).abs().max())
        per_pixel = (got[0] - query.grad).abs().reshape(h * w, C).amax(1)
        flipped = per_pixel > 1e-4
        agree = float(per_pixel[~flipped].max())
        lines.append(f"{what}: {h} x {w}, matched at {H} x {W}; the unfolded operand C (2R+1)^2 HW floats = {C * 625 * H * W * 4 / 2 ** 20:.0f} MiB")
        lines.append(f"  HIP against PyTorch: largest |out| difference {out_diff:.2e}; grad query differs by more than 1e-4 at {int(flipped.sum())} of "
                     f"{h * w} pixels (near ties resolved differently), largest difference on the others {agree:.2e}; on grad bias "
                     f"{float((got[2] - bias.grad).abs().max()):.2e}")
        for label, step in (("HIP   local_train          ", hip_step), ("torch unfold               ", torch_step)):
            med, lo, hi, peak = timed(step, clear)
            lines.append(f"  {label} {med:9.3f} / {lo:9.3f} / {hi:9.3f} ms    peak {peak / 2 ** 20:10.1f} MiB")
        clear()
        del prev, query, bias, labels, weight
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
