"""Developer tool (GPU box): SHA-256 of the per-frame label maps of eval_runner.HotPathBackend built WITHOUT augmentations, on a fixed list
of short seeded sequences -> tests/golden/tta_parent_labels.json.

The committed fixture was written by this script on the commit BEFORE HotPathBackend learned about test-time augmentation; the default
backend must keep returning these bits (tests/test_gpu_tta.py asserts that, and imports the sequences from here).

    python tools/record_tta_parent_labels.py            # write the fixture (refuses when two runs of a sequence differ)
    python tools/record_tta_parent_labels.py --check    # compare with the committed fixture instead, exit status 1 on a difference

Only what the parent commit already had is used: eval_runner.SequenceSpec, load_sequence, HotPathBackend(device).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "tta_parent_labels.json")

# name -> SequenceSpec arguments (name, h, w, n_obj, frames, seed, levels, mem_every): a small map with three pool changes, one with
# multi-level proxies, and the 121 x 213 map of a DAVIS sequence with one pool change
SEQUENCES = {
    "small_24x40": ("small_24x40", 24, 40, 3, 8, 21, (16,), 3),
    "small_33x45_levels": ("small_33x45_levels", 33, 45, 4, 7, 22, (8, 16, 32), 2),
    "davis_121x213": ("davis_121x213", 121, 213, 4, 5, 23, (16,), 3),
}


def make_spec(name):
    from aoc_amd import eval_runner as er
    return er.SequenceSpec(*SEQUENCES[name])


def run_labels(backend, spec, data):
    """The label map of every frame after the first, on the host."""
    emb, gt = data
    backend.start(spec)
    backend.first_frame(emb[0], gt[0])
    out = [backend.frame(emb[t]).cpu().numpy().astype(np.int32) for t in range(1, emb.shape[0])]
    torch.cuda.synchronize()
    return out


def digest(labels):
    return [hashlib.sha256(np.ascontiguousarray(l, dtype=np.int32).tobytes()).hexdigest() for l in labels]


def main():
    import aoc_amd
    from aoc_amd import eval_runner as er
    aoc_amd._lib.lib()
    check = "--check" in sys.argv[1:]
    dev = torch.device("cuda", 0)
    hashes = {}
    for name in SEQUENCES:
        spec = make_spec(name)
        data = er.load_sequence(spec, dev)
        d = [digest(run_labels(er.HotPathBackend(dev), spec, data)) for _ in range(2)]
        print(f"{name:24s} frames={len(d[0])} " + " ".join(x[:8] for x in d[0]), flush=True)
        if d[0] != d[1]:
            raise SystemExit(f"{name}: two runs of the same build differ: nothing written")
        hashes[name] = d[0]
    if check:
        with open(FIXTURE) as f:
            want = json.load(f)
        bad = [k for k in SEQUENCES if want.get(k) != hashes[k]]
        print("differs from the fixture: " + ", ".join(bad) if bad else f"all {len(hashes)} sequences equal the fixture")
        raise SystemExit(1 if bad else 0)
    with open(FIXTURE, "w") as f:
        json.dump(hashes, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
