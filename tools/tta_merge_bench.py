"""Developer tool (GPU box): ops.tta_merge against the torch composition the evaluation runner uses per augmentation.

At 480 x 854, four channels, maps of 121 x 213 (157 x 277 for the scaled lanes), A = 1, 2, 4:
  (a) per augmentation F.interpolate(bilinear, align_corners=True) + softmax (eval_runner.HotPathBackend.frame), a flip for mirrored ones,
      stack().mean(0) for A > 1, then ops.confident_labels;
  (b) ops.tta_merge (one launch).
One process, (a) and (b) alternating, every shape warmed up first; a repetition is enough back-to-back calls between two device events to last
tens of milliseconds, REPS repetitions each; median / min / max per call, the bytes (b) has to move and the share of the 8 TB/s peak.

    python tools/tta_merge_bench.py [out.txt]        # default: profiles/tta_merge.txt
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
from aoc_amd import ops  # noqa: E402

H, W, N_CH, REPS, PEAK = 480, 854, 4, 20, 8.0e12
AUGS = [(121, 213, False), (121, 213, True), (157, 277, False), (157, 277, True)]


def composition(logits, flips, bits, unc):
    ps = []
    for l, f in zip(logits, flips):
        p = torch.softmax(F.interpolate(l[None], size=(H, W), mode="bilinear", align_corners=True)[0], dim=0)
        ps.append(p.flip(2) if f else p)
    mean = ps[0] if len(ps) == 1 else torch.stack(ps).mean(0)
    return ops.confident_labels(mean.reshape(N_CH, H * W), bits, None, unc)


def time_calls(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls           # us per call


def sequence_rates(frames=21):
    """frames/s of one eval_runner.run_sequence on a cfg2-shaped sequence (121 x 213 maps, 3 objects + background) with 1, 2 and 4 augmentation
    lanes, after one untimed pass of the same sequence (workspaces, code objects); the default backend for comparison."""
    from aoc_amd import eval_runner as er
    dev = torch.device("cuda", 0)
    spec = er.SequenceSpec("cfg2-shaped", 121, 213, 4, frames, seed=7, levels=(16,), mem_every=5)
    data = er.load_sequence(spec, dev)
    out = [f"# eval_runner.run_sequence, {frames - 1} frames of a cfg2-shaped sequence (121 x 213 maps, 4 channels), second pass timed"]
    for name, augs in (("default backend (no augmentations)", None), ("1 lane", AUGS[:1]), ("2 lanes", AUGS[:2]), ("4 lanes", AUGS)):
        be = er.HotPathBackend(dev, augmentations=augs)
        er.run_sequence(spec, be, dev, data=data)
        r = er.run_sequence(spec, be, dev, data=data)
        out.append(f"  {name:36s} {r['frames'] / r['gpu_seconds']:8.1f} frames/s   mean J {r['sum_iou'] / max(r['iou_count'], 1):.4f}")
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tta_merge.txt")
    aoc_amd._lib.lib()
    rng = np.random.RandomState(0)
    lines = [f"# ops.tta_merge (b) against the per-augmentation torch composition + ops.confident_labels (a); {H} x {W}, {N_CH} channels,",
             f"# {REPS} repetitions each, alternating, us per call: median / min / max.  Device: {torch.cuda.get_device_name(0)}", ""]
    for A in (1, 2, 4):
        augs = AUGS[:A]
        logits = [torch.from_numpy(rng.standard_normal((N_CH, h, w)).astype(np.float32) * 3).cuda() for h, w, _ in augs]
        flips = [f for _, _, f in augs]
        fa = lambda: composition(logits, flips, 0b0111, 0.6)
        fb = lambda: ops.tta_merge(logits, flips, H, W, 0b0111, None, 0.6, "reference")
        for fn in (fa, fb):                              # warm-up of every shape
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        calls = {}
        for key, fn in (("a", fa), ("b", fb)):           # calls per repetition: about 30 ms
            calls[key] = max(10, int(30e3 / max(time_calls(fn, 50), 1e-3)))
        t = {"a": [], "b": []}
        for _ in range(REPS):
            for key, fn in (("a", fa), ("b", fb)):
                t[key].append(time_calls(fn, calls[key]))
        read = sum(N_CH * h * w * 4 for h, w, _ in augs)
        written = 4 * H * W * 4                          # label, confident, label_flipped, entropy
        med_b = float(np.median(t["b"]))
        lines.append(f"A = {A}: maps " + ", ".join(f"{h}x{w}{'f' if f else ''}" for h, w, f in augs))
        for key in ("a", "b"):
            lines.append(f"  ({key}) {np.median(t[key]):9.2f} / {min(t[key]):9.2f} / {max(t[key]):9.2f} us   ({calls[key]} calls per repetition)")
        lines.append(f"  (b) moves {read} B read + {written} B written = {(read + written) / 1e6:.2f} MB: {(read + written) / (med_b * 1e-6) / 1e12:.3f} TB/s, "
                     f"{100 * (read + written) / (med_b * 1e-6) / PEAK:.1f} % of the 8 TB/s peak")
        lines.append(f"  (a) min / (b) max = {min(t['a']) / max(t['b']):.2f}   [(b)'s max below (a)'s min: {max(t['b']) < min(t['a'])}]")
        lines.append("")
    lines += sequence_rates()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
