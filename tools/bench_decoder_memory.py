"""Developer tool (GPU box): the fused entry points of the decoder's memory modulators against what a caller could compose before them.

1. Concatenation + gate 1 (decoding_module.py:193-194):   (a) torch.cat + ops.film_scale;   (b) ops.cat_film_scale (one launch).
2. Last GroupNorm of a Bottleneck + the gate behind it (gct.py:84-90 + decoding_module.py:196): x, residual [N, 2e, h, w];
   (a) ops.groupnorm_relu + ops.film_scale;   (b) ops.groupnorm_relu_scale.
Shapes: N = 3, e = 256, 61 x 107 (cfg2 at half resolution) and N = 5, e = 256, 73 x 131.  The protocol is tools/bench_decoder_tail.py's: one
process, (a) and (b) alternating, every shape warmed up first; a repetition is enough back-to-back calls between two device events to last
tens of milliseconds, REPS repetitions each; median / min / max per call, the bytes each path has to move (derived from the shapes), and
whether the two results have the same bits at the timed size.  The bar: (b)'s median below (a)'s with non-overlapping min / max bands.

    python tools/bench_decoder_memory.py [out.txt]        # default: profiles/decoder_memory_ab.txt
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import aoc_amd  # noqa: E402
from aoc_amd import ops  # noqa: E402
from bench_decoder_tail import REPS, ab, report  # noqa: E402

D, E = 400, 256
SHAPES = [(3, 61, 107), (5, 73, 131)]
# hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c csrc/calibration.hip (template argument = float4 per lane)
RESOURCES = """# Compile check (-Rpass-analysis=kernel-resource-usage, gfx950): no kernel of the two entry points uses scratch.
#   cat_film_scale_kernel<4>   47 VGPRs, scratch 0      cat_film_scale_kernel<8>   63 VGPRs, scratch 0
#   gn_apply_scale_kernel<4>   64 VGPRs, scratch 0      gn_apply_scale_kernel<8>   96 VGPRs, scratch 0
#   (film_scale_ahead_kernel<4> / <8>, the model: 56 / 72 VGPRs)"""


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def verdict(lines, t, what):
    met = float(np.median(t["b"])) < float(np.median(t["a"])) and max(t["b"]) < min(t["a"])
    lines.insert(len(lines) - 1, f"  bar (median below, bands apart): {'MET' if met else 'MISSED -- ' + what + ' must use the composition'}")
    return met


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decoder_memory_ab.txt")
    aoc_amd._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    lines = [f"# The decoder's memory modulators: the fused entry points (b) against the composition available before them (a); {REPS} repetitions",
             f"# each, alternating, us per call: median / min / max.  Byte counts are derived from the shapes.  Device: {torch.cuda.get_device_name(0)}",
             RESOURCES, ""]
    for N, h, w in SHAPES:
        C = 2 * E
        x, mem, head = rnd(N, E, h, w), rnd(N, E, h, w), 0.5 * rnd(N, D)
        weight, bias = rnd(C, D) / D ** 0.5, 0.1 * rnd(C)
        out_a, out_b = torch.empty(N, C, h, w, device="cuda"), torch.empty(N, C, h, w, device="cuda")
        cat_a = lambda: ops.film_scale(torch.cat([x, mem], 1), head, weight, bias, out=out_a)
        cat_b = lambda: ops.cat_film_scale(x, mem, head, weight, bias, out=out_b)
        same = same_bits(cat_a(), cat_b())
        S = N * C * h * w * 4
        t, calls = ab(cat_a, cat_b)
        lines.append(f"1. concat + gate 1, N = {N}, e = {E}, D = {D}, {h} x {w}; S = {S / 1e6:.2f} MB (the gated concatenation); same bits: {same}")
        report(lines, t, calls, 4 * S, 2 * S)              # (a) cat reads and writes S, the gate reads and writes S; (b) S read once, written once
        verdict(lines, t, "decoder_memory's step 1")

        y, res = rnd(N, C, h, w), rnd(N, C, h, w)
        gam, bet = 0.5 + torch.rand(C, device="cuda", generator=g), 0.5 * rnd(C)
        tmp = torch.empty_like(out_a)
        gn_a = lambda: ops.film_scale(ops.groupnorm_relu(y, 32, gam, bet, 1e-5, res, True, out=tmp), head, weight, bias, out=out_a)
        gn_b = lambda: ops.groupnorm_relu_scale(y, 32, gam, bet, 1e-5, res, True, head, weight, bias, out=out_b)
        same = same_bits(gn_a(), gn_b())
        t, calls = ab(gn_a, gn_b)
        lines.append(f"2. GroupNorm + residual + ReLU + gate, N = {N}, C = {C}, groups = 32, {h} x {w}; T = {S / 1e6:.2f} MB (the tensor); same bits: {same}")
        # (a) statistics read T; apply reads T and the residual, writes T; the gate reads and writes T.  (b) statistics read T; apply reads T and the residual, writes T
        report(lines, t, calls, 6 * S, 4 * S)
        verdict(lines, t, "the gated gct.Bottleneck")

    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
