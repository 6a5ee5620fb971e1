"""Developer tool (GPU box): forward + backward of the differentiable cluster matching (aoc_amd.cluster_train.global_matching_cluster2) in
three arms:
  (a) the HIP path: label preparation, the device k-means chain (20 Lloyd iterations), aoc_build_proxies, the set minimum with its argmin
      and the two gradient entries;
  (b) the matching part alone written as plain PyTorch on the device and fed the HIP path's labels and code books: per object the
      segmented mean of the reference rows (through the reference's indexing: segment-local positions into the global kept-row array),
      the [m, K] distances to both sets, their minima, the transform, autograd.  No clustering in this arm;
  (c) the device k-means chain alone (matching.cluster_proxies, no backward): what replaces the host kmeans2 and its device-to-host copy
      per object.
Shapes: the training crop, 117 x 117, and cfg2's map, 121 x 213; C = 100, four objects, K = 16, 85 % of the reference frame labelled, the
same initial rows in every call.  Per arm: WARMUP calls, then RUNS calls each bracketed by two device events (median / min / max in ms), and
torch.cuda.max_memory_allocated over the timed calls minus what was allocated before them (the inputs alone).  Before the timing the
outputs and gradients of (a) and (b) are compared and the largest differences printed.  No number here is a gate.  The results are
appended to the output file.

    python tools/bench_cluster_grad.py [out.txt]        # default: profiles/cluster_grad_ab.txt
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
from aoc_amd import cluster_train, matching  # noqa: E402

WARMUP, RUNS = 3, 20
C, N_OBJ, K = 100, 4, 16
SHAPES = [("training crop", 117, 117), ("cfg2 map", 121, 213)]
PAD = 5e4


def torch_cluster_matching(ref, query, bias, fg_rows, labels, offsets, seg_k, centroids):
    """The matching part as PyTorch composes it.  ref, query [h, w, C]; bias [O, 1, 1, 1]; fg_rows [n] kept rows; labels: the packed
    k-means assignment, object o's at offsets[o] : offsets[o + 1] (host list); seg_k (host list); centroids [O, K, C] (a constant).
    -> [1, h, w, O, 2]."""
    h, w, c = query.shape
    q, pool = query.reshape(-1, c), ref.reshape(-1, c)
    q2 = (q * q).sum(1)
    planes = []
    for o, k in enumerate(seg_k):
        if k == 0:
            planes += [torch.full_like(q2, PAD)] * 2
            continue
        lab = labels[offsets[o]:offsets[o + 1]]
        rows = pool[fg_rows[:lab.numel()]]                          # segment-local positions into the global kept-row array
        member = F.one_hot(lab, k).to(rows.dtype)                   # [n_o, k]
        count = member.sum(0)
        mean = (member.t() @ rows)[count > 0] / count[count > 0][:, None]
        for p in (centroids[o, :k], mean):
            d = q2[:, None] + (p * p).sum(1)[None, :] - 2.0 * (q @ p.t())
            planes.append(d.amin(1))
    d = torch.stack(planes).view(len(seg_k), 2, h, w)
    T = (torch.sigmoid(d + bias.view(-1, 1, 1, 1)) - 0.5) * 2.0
    return T.permute(2, 3, 0, 1).reshape(1, h, w, len(seg_k), 2)


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cluster_grad_ab.txt")
    aoc_amd._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    s = 1.2 / np.sqrt(C)
    lines = [f"# Cluster matching, forward + backward: (a) cluster_train.global_matching_cluster2 (HIP, clustering included), (b) the matching part "
             f"as plain PyTorch on the device fed (a)'s labels, (c) the device k-means chain alone; C = {C}, {N_OBJ} objects, K = {K};",
             f"# {RUNS} runs after {WARMUP}, ms per call: median / min / max; peak = max_memory_allocated above the inputs.  "
             f"Device: {torch.cuda.get_device_name(0)}"]
    for what, h, w in SHAPES:
        ref = (s * torch.randn(h, w, C, device="cuda", generator=g)).requires_grad_(True)
        query = (s * torch.randn(h, w, C, device="cuda", generator=g)).requires_grad_(True)
        bias = (0.3 * torch.randn(N_OBJ, 1, 1, 1, device="cuda", generator=g)).requires_grad_(True)
        owner = torch.randint(0, N_OBJ, (h, w), device="cuda", generator=g)
        labelled = torch.rand(h, w, device="cuda", generator=g) < 0.85
        labels = F.one_hot(owner, N_OBJ).float() * labelled[:, :, None]
        weight = torch.randn(1, h, w, N_OBJ, 2, device="cuda", generator=g)
        with torch.no_grad():
            pool, labels_flat = matching._flatten_pool([ref], [labels], h, w, 1, 0)
            cp = matching.cluster_proxies(pool, labels_flat, K, None, np.random.RandomState(1))
        rows = cp["init_rows"]
        fg_rows, km_labels = cp["prep"].fg_rows.long(), cp["labels"].long()
        offsets, seg_k, centroids = cp["seg_offsets"].cpu().tolist(), list(cp["seg_k"]), cp["centroids"].clone()

        def clear():
            ref.grad = query.grad = bias.grad = None

        def hip_step():
            clear()
            out = cluster_train.global_matching_cluster2(ref, query, labels, 100, bias, None, 1, False, 0, init_rows=rows, cluster_num=K)
            (out * weight).sum().backward()

        def torch_step():
            clear()
            out = torch_cluster_matching(ref, query, bias, fg_rows, km_labels, offsets, seg_k, centroids)
            (out * weight).sum().backward()

        def chain_step():
            with torch.no_grad():
                matching.cluster_proxies(pool, labels_flat, K, rows)

        hip_step()
        got = [t.grad.clone() for t in (query, ref, bias)]
        out_hip = cluster_train.global_matching_cluster2(ref, query, labels, 100, bias, None, 1, False, 0, init_rows=rows, cluster_num=K).detach()
        torch_step()
        out_diff = float((out_hip - torch_cluster_matching(ref, query, bias, fg_rows, km_labels, offsets, seg_k, centroids).detach()).abs().max())
        per_pixel = (got[0] - query.grad).abs().reshape(h * w, C).amax(1)
        flipped = per_pixel > 1e-4
        lines.append(f"{what}: {h} x {w}, {int(labelled.sum())} kept rows, K per object {seg_k}")
        lines.append(f"  (a) against (b): largest |out| difference {out_diff:.2e}; grad query differs by more than 1e-4 at {int(flipped.sum())} of {h * w} "
                     f"pixels (near ties resolved differently), largest difference on the others {float(per_pixel[~flipped].max()):.2e}; on grad ref "
                     f"{float((got[1] - ref.grad).abs().max()):.2e}; on grad bias {float((got[2] - bias.grad).abs().max()):.2e}")
        for label, step in (("(a) HIP cluster_train, clustering included", hip_step), ("(b) torch, matching part alone            ", torch_step),
                            ("(c) device k-means chain alone, no backward", chain_step)):
            med, lo, hi, peak = timed(step, clear)
            lines.append(f"  {label} {med:9.3f} / {lo:9.3f} / {hi:9.3f} ms    peak {peak / 2 ** 20:10.1f} MiB")
        clear()
        del ref, query, bias, labels, weight, cp, pool, labels_flat
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
