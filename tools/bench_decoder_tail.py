"""Developer tool (GPU box): the decoder's tail on the HIP library against what a caller could compose before it existed.

1. Shortcut stage, N = 3, Ce = 256, Cr = 64, 61 x 107 -> 121 x 213 (cfg2):
   (a) F.interpolate(bicubic, align_corners=True) + torch.cat + ops.plane_mean + ops.head_delta + ops.film_scale;
   (b) ops.shortcut_stage (one C call).
2. Prediction head, N = 3, C = 128, hw = 121 x 213:
   (a) ops.object_logit x 2 + the torch merge (min, add);   (b) ops.logit_head (one launch).
One process, (a) and (b) alternating, every shape warmed up first; a repetition is enough back-to-back calls between two device events to
last tens of milliseconds, REPS repetitions each; median / min / max per call, and the bytes each path has to move, derived from the shapes.

    python tools/bench_decoder_tail.py [out.txt]        # default: profiles/decoder_tail_ab.txt
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

REPS, PEAK = 20, 8.0e12
N, CE, CR, D, h, w, H, W = 3, 256, 64, 400, 61, 107, 121, 213
C_HEAD = 128


def time_calls(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls           # us per call


def ab(fa, fb):
    for fn in (fa, fb):                                 # warm-up of every shape
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    calls = {k: max(10, int(30e3 / max(time_calls(fn, 20), 1e-3))) for k, fn in (("a", fa), ("b", fb))}      # about 30 ms per repetition
    t = {"a": [], "b": []}
    for _ in range(REPS):
        for k, fn in (("a", fa), ("b", fb)):
            t[k].append(time_calls(fn, calls[k]))
    return t, calls


def report(lines, t, calls, bytes_a, bytes_b):
    for k, nbytes in (("a", bytes_a), ("b", bytes_b)):
        med = float(np.median(t[k]))
        lines.append(f"  ({k}) {med:9.2f} / {min(t[k]):9.2f} / {max(t[k]):9.2f} us   ({calls[k]} calls per repetition)   moves {nbytes / 1e6:8.2f} MB: "
                     f"{nbytes / (med * 1e-6) / 1e12:.3f} TB/s, {100 * nbytes / (med * 1e-6) / PEAK:.1f} % of the 8 TB/s peak")
    ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
    lines.append(f"  (b) / (a) medians = {mb / ma:.3f}   [(b)'s max below (a)'s min: {max(t['b']) < min(t['a'])}]"
                 + ("" if mb <= ma else "   *** (b) IS SLOWER than the composition ***"))
    lines.append("")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decoder_tail_ab.txt")
    aoc_amd._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    lines = [f"# The decoder's tail: the fused entry points (b) against the composition available before them (a); {REPS} repetitions each,",
             f"# alternating, us per call: median / min / max.  Byte counts are derived from the shapes.  Device: {torch.cuda.get_device_name(0)}", ""]

    x, low, head = rnd(N, CE, h, w), rnd(N, CR, H, W).relu_(), 0.5 * rnd(N, D)
    weight, bias = rnd(CE + CR, D + CE + CR) / (D + CE + CR) ** 0.5, 0.1 * rnd(CE + CR)
    out = torch.empty(N, CE + CR, H, W, device="cuda")

    def stage_a():
        cat = torch.cat([F.interpolate(x, size=(H, W), mode="bicubic", align_corners=True), low], 1)
        return ops.film_scale(cat, ops.head_delta(head, ops.plane_mean(cat)), weight, bias, out=out)

    stage_b = lambda: ops.shortcut_stage(x, low, head, weight, bias, out=out)
    diff = float((stage_a().clone() - stage_b()).abs().max())
    S = N * (CE + CR) * H * W * 4
    coarse, up, sc = N * CE * h * w * 4, N * CE * H * W * 4, N * CR * H * W * 4
    # (a): interpolate reads the coarse map and writes the upsample; cat reads both parts and writes S; plane_mean reads S; film_scale reads and writes S
    bytes_a = (coarse + up) + (up + sc + S) + S + 2 * S
    # (b): the coarse map twice (means, resize), the shortcut planes twice (means, scale), S written once
    bytes_b = 2 * coarse + 2 * sc + S
    t, calls = ab(stage_a, stage_b)
    lines.append(f"1. shortcut stage, N = {N}, Ce = {CE}, Cr = {CR}, D = {D}, {h} x {w} -> {H} x {W}; S = {S / 1e6:.2f} MB; max |a - b| = {diff:.3e}")
    report(lines, t, calls, bytes_a, bytes_b)

    xh = rnd(N, C_HEAD, H, W)
    wb_fg, wb_bg = rnd(N, C_HEAD + 1) / C_HEAD ** 0.5, rnd(N, C_HEAD + 1) / C_HEAD ** 0.5

    def head_a():
        fg, bg = ops.object_logit(xh, wb_fg), ops.object_logit(xh, wb_bg)
        aug = torch.min(bg[1:], dim=0, keepdim=True)[0]
        return (fg + torch.cat([aug, torch.zeros_like(aug).expand(N - 1, -1, -1, -1)], 0)).permute(1, 0, 2, 3)

    head_b = lambda: ops.logit_head(xh, wb_fg, wb_bg)
    same = bool(torch.equal(head_a(), head_b()))
    X, L = N * C_HEAD * H * W * 4, N * H * W * 4
    # (a): x twice, two logit tensors written; min reads N - 1 planes and writes one; cat writes N; the add reads 2 N and writes N
    bytes_a = 2 * X + 2 * L + (L - L // N + L // N) + L + 3 * L
    bytes_b = X + L
    t, calls = ab(head_a, head_b)
    lines.append(f"2. prediction head, N = {N}, C = {C_HEAD}, hw = {H} x {W}; x = {X / 1e6:.2f} MB; bit-equal results: {same}")
    report(lines, t, calls, bytes_a, bytes_b)

    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
