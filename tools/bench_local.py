#!/usr/bin/env python3
"""Stand-alone timing of local (windowed) matching on an idle GPU at the half-resolution map of a config (AEM:938-941):

    python tools/bench_local.py [--config cfg2]

One JSON object: median launch time (HIP events) of the kernel the library takes for the config's channel count (C = 100 / 128:
local_window_reg_kernel) and flops 2 m (2R+1)^2 C."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps=40):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    args = ap.parse_args()
    import aoc_amd  # noqa: F401
    from aoc_amd import ops
    from aoc_amd import synthetic as syn
    cfg = syn.CONFIGS[args.config]
    clip = syn.make_clip(cfg, seed=3, frames=2)
    dev = torch.device("cuda")
    O = cfg.n_obj
    prev = torch.from_numpy(clip["emb"][0]).to(dev)
    cur = torch.from_numpy(clip["emb"][1]).to(dev)
    lab = torch.from_numpy(syn.one_hot(clip["lab"][0], O)).to(dev)
    H2, W2 = int(cfg.h / 2) + 1, int(cfg.w / 2) + 1
    q2 = ops.resize_bilinear_hwc(cur, H2, W2)
    p2 = ops.resize_bilinear_hwc(prev, H2, W2)
    bits, _ = ops.label_bits(lab.reshape(-1, O), want_wrong=False)
    bits2 = ops.resize_nearest_bits(bits, cfg.h, cfg.w, H2, W2)
    radii = [2, 4, 6, 8, 10, 12]
    bias = torch.zeros(O, device=dev)
    ms = timed(lambda: ops.local_window_match(q2, p2, bits2, radii, bias, O, True))
    flops = 2.0 * H2 * W2 * 25 * 25 * cfg.c
    print(json.dumps(dict(map=[H2, W2], ms=round(ms, 4), tflops=round(flops / ms * 1e-9, 2))), flush=True)


if __name__ == "__main__":
    main()
