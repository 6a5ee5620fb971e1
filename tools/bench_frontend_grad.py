"""Developer tool (GPU box): forward + backward of one training sample's proto-mask front end (aocnet.py:141-358) in four arms:
  (a) aoc_amd.frontend_train.proto_mask_features: the five differentiable matchers, the HIP heads and the HIP aggregation;
  (b) the same five matchers, with the lines between them as the reference composes them in plain PyTorch on the device: the heads by
      ``emb * label`` at [O, C, h, w] (ATT:136-142), foreground2background by one torch.cat + torch.min per object (AEM:13-20) for the
      global map and for the local maps, and the torch.cat of aocnet.py:355-358;
  (c) the front-end lines alone on the HIP path: the heads of both frames and the aggregation of five given matching outputs;
  (d) the same lines alone in plain PyTorch.
Shapes: the training crop, 117 x 117, and cfg2's map, 121 x 213; C = 100, four objects, six radii, K = 16, the same initial k-means rows in
every call.  Per arm: WARMUP calls, then RUNS calls each bracketed by two device events (median / min / max in ms), and
torch.cuda.max_memory_allocated over the timed calls minus what was allocated before them (the inputs alone).  Before the timing the
outputs and gradients of (a) and (b) are compared and the largest differences printed.  No number here is a gate.  The results are
appended to the output file.

    python tools/bench_frontend_grad.py [out.txt]        # default: profiles/frontend_grad_ab.txt
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import aoc_amd  # noqa: E402
from aoc_amd import cluster_train, frontend_train, local_train, matching, matching_train  # noqa: E402

WARMUP, RUNS = 3, 20
C, GT_ID, K = 100, 3, 16
RADII = [2, 4, 6, 8, 10, 12]
SHAPES = [("training crop", 117, 117), ("cfg2 map", 121, 213)]
EPS = 1e-5


def torch_heads(ref_emb, to_ref, prev_emb, to_prev):
    """ATT:134-153 as written: the [O, C, h, w] products stay alive for the backward."""
    out = []
    for emb, lab in ((ref_emb, to_ref), (prev_emb, to_prev)):
        e = emb.unsqueeze(0).expand(lab.size(0), -1, -1, -1)
        pos = torch.sum(e * lab, dim=(2, 3))
        neg = torch.sum(e, dim=(2, 3)) - pos
        out += [pos / (torch.sum(lab, dim=(2, 3)) + EPS), neg / (torch.sum(1. - lab, dim=(2, 3)) + EPS)]
    return torch.cat(out, dim=1), out[0], out[2]


def torch_fg2bg(dis, obj_num):
    """AEM:9-23 as written."""
    if obj_num == 1:
        return dis
    bg = []
    for i in range(obj_num):
        others = torch.cat([dis[j].unsqueeze(0) for j in range(obj_num) if j != i], dim=1)
        bg.append(torch.min(others, dim=1, keepdim=True)[0])
    return torch.cat(bg, dim=0)


def torch_aggregate(outs, to_prev, obj_num):
    """aocnet.py:341-358 as written."""
    g, c, p, l, lp = (t.squeeze(0).permute(2, 3, 0, 1) for t in outs)
    g_bg = torch_fg2bg(g, obj_num)
    l_bg = torch_fg2bg(l.permute(0, 2, 3, 1).unsqueeze(1), obj_num).permute(0, 4, 2, 3, 1).squeeze(-1)
    return torch.cat([torch.cat((g, c, p, l, lp, to_prev), 1), l_bg, g_bg], 1)


def sample_with_torch_front_end(ref_emb, prev_emb, cur_emb, to_ref, to_prev, bg_bias, fg_bias, rows):
    obj_num = GT_ID + 1
    bias = torch.cat([bg_bias, fg_bias.expand(GT_ID, -1, -1, -1)], dim=0)
    cur, prev, ref = cur_emb.permute(1, 2, 0), prev_emb.permute(1, 2, 0), ref_emb.permute(1, 2, 0)
    sr, sp = to_ref.squeeze(1).permute(1, 2, 0), to_prev.squeeze(1).permute(1, 2, 0)
    g = matching_train.global_matching(ref, cur, sr, 1, bias, None, 1, False)
    c = cluster_train.global_matching_cluster2(ref, cur, sr, 1, bias, None, 1, False, 0, init_rows=rows, cluster_num=K)
    l = local_train.local_matching(prev, cur, sp, bias, RADII, None, 1, False, True, True)
    head, ref_pos, prev_pos = torch_heads(ref_emb, to_ref, prev_emb, to_prev)
    p = matching_train.global_matching_proxy(ref_pos, cur, sr, 1, bias, None, 1, False)
    lp = local_train.local_matching_proxy(torch.matmul(sp, prev_pos), cur, sp, bias, RADII, None, 1, False, True, True)
    return torch_aggregate((g, c, p, l, lp), to_prev, obj_num), head


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "frontend_grad_ab.txt")
    aoc_amd._lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    s = 1.2 / np.sqrt(C)
    obj_num = GT_ID + 1
    lines = [f"# Proto-mask front end of one training sample, forward + backward: (a) frontend_train.proto_mask_features, (b) the same matchers with the "
             f"heads / foreground2background / cat in plain PyTorch, (c) heads + aggregation alone on HIP, (d) the same alone in PyTorch; C = {C}, "
             f"{obj_num} objects, radii {RADII}, K = {K};",
             f"# {RUNS} runs after {WARMUP}, ms per call: median / min / max; peak = max_memory_allocated above the inputs.  "
             f"Device: {torch.cuda.get_device_name(0)}"]
    for what, h, w in SHAPES:
        embs = [(s * torch.randn(C, h, w, device="cuda", generator=gen)).requires_grad_(True) for _ in range(3)]
        ref_emb, prev_emb, cur_emb = embs
        ref_label, prev_label = (torch.randint(0, obj_num, (h, w), device="cuda", generator=gen).int() for _ in range(2))
        bg_bias = (0.3 * torch.randn(1, 1, 1, 1, device="cuda", generator=gen)).requires_grad_(True)
        fg_bias = (0.3 * torch.randn(1, 1, 1, 1, device="cuda", generator=gen)).requires_grad_(True)
        leaves = embs + [bg_bias, fg_bias]
        ids = torch.arange(obj_num, device="cuda").int().view(-1, 1, 1, 1)
        to_ref, to_prev = (ref_label.view(1, h, w) == ids).float(), (prev_label.view(1, h, w) == ids).float()
        with torch.no_grad():
            pool, labels_flat = matching._flatten_pool([ref_emb.permute(1, 2, 0)], [to_ref.squeeze(1).permute(1, 2, 0)], h, w, 1, 0)
            rows = matching.cluster_proxies(pool, labels_flat, K, None, np.random.RandomState(1))["init_rows"]
        n_ch = frontend_train.aggregate_channels(2, len(RADII))
        w_feat = torch.randn(obj_num, n_ch, h, w, device="cuda", generator=gen)
        w_head = torch.randn(obj_num, 4 * C, device="cuda", generator=gen)
        # five given matching outputs for the arms (c) and (d): leaves in the matchers' own layout
        given = [torch.tanh(torch.randn(obj_num, k, h, w, device="cuda", generator=gen)).requires_grad_(True) for k in (1, 2, 1, len(RADII), len(RADII))]

        def clear():
            for t in leaves + given:
                t.grad = None

        def emitted():
            return [t.view(-1, 1, h, w).permute(2, 3, 0, 1).reshape(1, h, w, obj_num, t.shape[1]) for t in given]

        def loss(feat, head):
            ((feat * w_feat).sum() + (head * w_head).sum()).backward()

        def hip_step():
            clear()
            loss(*frontend_train.proto_mask_features(ref_emb, prev_emb, cur_emb, ref_label, prev_label, GT_ID, bg_bias, fg_bias, RADII, init_rows=rows,
                                                     cluster_num=K))

        def torch_step():
            clear()
            loss(*sample_with_torch_front_end(ref_emb, prev_emb, cur_emb, to_ref, to_prev, bg_bias, fg_bias, rows))

        def hip_lines():
            clear()
            e = lambda t: t.unsqueeze(0).expand(obj_num, -1, -1, -1)
            head = frontend_train.calculate_attention_head_p_m(e(ref_emb), to_ref, e(prev_emb), to_prev, EPS)[0]
            loss(frontend_train.aggregate(*emitted(), to_prev), head)

        def torch_lines():
            clear()
            loss(torch_aggregate(emitted(), to_prev, obj_num), torch_heads(ref_emb, to_ref, prev_emb, to_prev)[0])

        hip_step()
        got = [t.grad.clone() for t in leaves]
        with torch.no_grad():
            feat_hip, head_hip = frontend_train.proto_mask_features(ref_emb, prev_emb, cur_emb, ref_label, prev_label, GT_ID, bg_bias, fg_bias, RADII,
                                                                    init_rows=rows, cluster_num=K)
        torch_step()
        with torch.no_grad():
            feat_t, head_t = sample_with_torch_front_end(ref_emb, prev_emb, cur_emb, to_ref, to_prev, bg_bias, fg_bias, rows)
        diffs = ", ".join(f"{n} {float((a - t.grad).abs().max()):.2e} (scale {float(t.grad.abs().max()):.2e})"
                          for n, a, t in zip(("ref", "prev", "cur", "bg_bias", "fg_bias"), got, leaves))
        lines.append(f"{what}: {h} x {w}, feat [{obj_num}, {n_ch}, {h}, {w}]")
        lines.append(f"  (a) against (b): largest |feat| difference {float((feat_hip - feat_t).abs().max()):.2e}, |head| {float((head_hip - head_t).abs().max()):.2e}; "
                     f"largest gradient differences: {diffs}")
        for label, step in (("(a) HIP proto_mask_features               ", hip_step), ("(b) HIP matchers, torch heads / fg2bg / cat", torch_step),
                            ("(c) HIP heads + aggregation alone         ", hip_lines), ("(d) torch heads / fg2bg / cat alone       ", torch_lines)):
            med, lo, hi, peak = timed(step, clear)
            lines.append(f"  {label} {med:9.3f} / {lo:9.3f} / {hi:9.3f} ms    peak {peak / 2 ** 20:10.1f} MiB")
        clear()
        del embs, ref_emb, prev_emb, cur_emb, leaves, given, w_feat, w_head, pool, labels_flat
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
