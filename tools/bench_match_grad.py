"""Developer tool (GPU box): forward + backward of the differentiable dense global matching (aoc_amd.matching_train.global_matching) against
the same function written as plain PyTorch on the device (distances, padded min, transform, autograd), which keeps the [m, O, n] padded
distance tensor of every chunk for its backward.

Shapes: the training crop, 117 x 117 (m = n = 13 689), and cfg2's map, 121 x 213; C = 100, three objects + background, half of the reference
rows labelled.  The PyTorch path runs with n_chunks 1 and 4.  Per path: WARMUP calls, then RUNS calls of forward + backward each bracketed by
two device events (median / min / max in ms), and torch.cuda.max_memory_allocated over the timed calls minus what was allocated before them:
the inputs alone, the gradients of the warm-up calls are dropped first, so the peak counts the output, the saved tensors, the workspaces and
the gradients of one call.  Before the timing the two paths' gradients are compared; a pixel where they differ by more than 1e-4 must be
one where the two paths chose different rows at a near tie, and the tool shows it: the float64 gap between the best and the runner-up row
of those pixels is printed beside the smallest such gap of all the other pixels.  The one expectation that follows from the shapes alone: the HIP path's peak holds no m O n term (m O n floats is printed
beside it).  The results are appended to the output file.

    python tools/bench_match_grad.py [out.txt]        # default: profiles/match_grad_ab.txt
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import aoc_amd  # noqa: E402

WARMUP, RUNS = 3, 20
C, N_OBJ = 100, 4
SHAPES = [("training crop", 117, 117), ("cfg2 map", 121, 213)]
PAD = 5e4


def torch_global_matching(ref, query, labels, bias, n_chunks):
    """Nearest labelled reference row per object as PyTorch composes it: [chunk, O, n] padded distances, min over n, 2 sigmoid(. + b) - 1."""
    c, n_obj = query.shape[-1], labels.shape[-1]
    q, r, lab = query.reshape(-1, c), ref.reshape(-1, c), labels.reshape(-1, n_obj)
    keep = lab.sum(1) > 0.9
    r, lab = r[keep], lab[keep]
    pad = (lab < 0.1).t().float() * PAD                                   # [O, n]
    r2 = (r * r).sum(1)
    rows = []
    for qc in q.chunk(n_chunks):
        d = (qc * qc).sum(1)[:, None] + r2[None, :] - 2.0 * (qc @ r.t())
        rows.append((d[:, None, :] + pad[None, :, :]).min(2).values)
    nearest = torch.cat(rows)
    return (torch.sigmoid(nearest + bias.view(1, -1)) - 0.5) * 2.0        # [m, O]


def tie_gaps(ref, query, labels, pixels):
    """float64 gap between the best and the runner-up padded distance of the given pixels, the smallest over the objects -> [len(pixels)]."""
    c, n_obj = query.shape[-1], labels.shape[-1]
    q, r, lab = query.detach().reshape(-1, c)[pixels].double(), ref.detach().reshape(-1, c).double(), labels.reshape(-1, n_obj)
    keep = lab.sum(1) > 0.9
    r, lab = r[keep], lab[keep]
    pad = (lab < 0.1).t().double() * PAD
    gaps = []
    for qc in q.split(256):
        d = (qc * qc).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2.0 * (qc @ r.t())
        two = (d[:, None, :] + pad[None, :, :]).topk(2, dim=2, largest=False).values
        gaps.append((two[..., 1] - two[..., 0]).amin(1))
    return torch.cat(gaps) if gaps else torch.zeros(0, dtype=torch.float64, device=query.device)


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "match_grad_ab.txt")
    aoc_amd._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"# Dense global matching, forward + backward: matching_train.global_matching (HIP) against plain PyTorch on the device; C = {C}, "
             f"{N_OBJ} objects, half of the rows labelled;", f"# {RUNS} runs after {WARMUP}, ms per forward + backward: median / min / max; peak = "
             f"max_memory_allocated above the inputs.  Device: {torch.cuda.get_device_name(0)}"]
    for what, h, w in SHAPES:
        m = h * w
        ref = (0.12 * torch.randn(h, w, C, device="cuda", generator=g)).requires_grad_(True)
        query = (0.12 * torch.randn(h, w, C, device="cuda", generator=g)).requires_grad_(True)
        bias = (0.3 * torch.randn(N_OBJ, 1, 1, 1, device="cuda", generator=g)).requires_grad_(True)
        owner = torch.randint(0, N_OBJ, (h, w), device="cuda", generator=g)
        labelled = torch.rand(h, w, device="cuda", generator=g) < 0.5
        labels = torch.nn.functional.one_hot(owner, N_OBJ).float() * labelled[:, :, None]
        n = int(labelled.sum())
        weight = torch.randn(1, h, w, N_OBJ, 1, device="cuda", generator=g)
        w_flat = weight.reshape(m, N_OBJ)

        def clear():
            ref.grad = query.grad = bias.grad = None

        def hip_step():
            clear()
            out = aoc_amd.matching_train.global_matching(ref, query, labels, 100, bias, None, 1, False, 0)
            (out * weight).sum().backward()

        def torch_step(n_chunks):
            clear()
            out = torch_global_matching(ref, query, labels, bias, n_chunks)
            (out * w_flat).sum().backward()

        hip_step()
        got = [t.grad.clone() for t in (query, ref, bias)]
        torch_step(4)
        # the nearest row is a discontinuous choice: on random data a few of the m O pairs sit within float32 rounding of a tie, and the two
        # paths (different summation orders) may then pick different rows for that pixel.  Those pixels are counted, the others compared.
        per_pixel = (got[0] - query.grad).abs().reshape(m, C).amax(1)
        flipped = per_pixel > 1e-4
        agree = float(per_pixel[~flipped].max())
        gaps = tie_gaps(ref, query, labels, torch.arange(m, device="cuda"))
        worst_flipped = f"{float(gaps[flipped].max()):.2e}" if bool(flipped.any()) else "-"
        lines.append(f"{what}: {h} x {w}, m = {m}, n = {n} labelled rows; m O n floats = {m * N_OBJ * n * 4 / 2 ** 20:.0f} MiB")
        lines.append(f"  HIP against PyTorch: grad query differs by more than 1e-4 at {int(flipped.sum())} of {m} pixels; float64 best / runner-up gap of "
                     f"those pixels at most {worst_flipped} (near ties: float32 distances here round at about 1e-6), smallest gap of all the other "
                     f"pixels {float(gaps[~flipped].min()):.2e}; largest |grad query| difference on the others {agree:.2e}, on grad bias "
                     f"{float((got[2] - bias.grad).abs().max()):.2e}")
        for label, step in (("HIP   matching_train        ", hip_step), ("torch n_chunks = 1         ", lambda: torch_step(1)),
                            ("torch n_chunks = 4         ", lambda: torch_step(4))):
            med, lo, hi, peak = timed(step, clear)
            lines.append(f"  {label} {med:9.3f} / {lo:9.3f} / {hi:9.3f} ms    peak {peak / 2 ** 20:10.1f} MiB")
        clear()
        del ref, query, bias, labels, weight
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
