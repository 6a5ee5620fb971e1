"""Developer tool (GPU box): what the dense op computed WITHOUT its bound seeds -> tests/golden/dense_seed_parent.json.

dense_seed_kernel publishes, before the matrix kernel starts, one exact-minus-margin value per query pixel; the seeds may only spare work.  The
last commit whose development build could skip that kernel (AOC_DENSE_SEED=0) is fb2052a.  The committed fixture was written by this script
with that commit's development library in csrc/ under another name:

    AOC_LIB_FILE=libaoc_hip_parentdev.so AOC_DENSE_SEED=0 python tools/record_dense_seed_parent.py            # write: hash, tested, rescored
    AOC_LIB_FILE=libaoc_hip_parentdev.so AOC_DENSE_SEED=1 python tools/record_dense_seed_parent.py --seeded   # add the parent's seeded rescored count
    python tools/record_dense_seed_parent.py --check                                                           # compare the loaded library with the fixture

tests/test_gpu_dense_split.py::test_bound_seeds_change_no_result imports the cases and run_cases from here and asserts, for the one library
of today: the same hash, the same tested count, fewer rescored pairs than the recorded seeds-off count.  `rescored` varies from run to run
(the workgroups race for the shared bounds), so the fixture keeps three runs and `rescored` is the largest of them; hash and tested must be
equal in all three or nothing is written.  The library switch is read once per process, which is why the seeded figure is a run of its own.
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "dense_seed_parent.json")
RUNS = 3


def clip():
    """-> (emb [F, h, w, C], one-hot labels [F, h, w, O], h * w) on the GPU: ten frames of 45 x 77 with four objects."""
    from aoc_amd import synthetic as syn
    cfg = syn.ClipConfig("t", 45, 77, 4, 16, frames=10)
    c = syn.make_clip(cfg, 5)
    emb = torch.from_numpy(c["emb"]).cuda()
    lab = torch.from_numpy(np.stack([syn.one_hot(l, cfg.n_obj) for l in c["lab"]])).cuda()
    return emb, lab, cfg.h * cfg.w


def cases(emb, lab, hw):
    """The seven (pool [n, C], labels [n, O], query [m, C]) of the seed test, in the order their outputs are hashed."""
    C, O = emb.shape[-1], lab.shape[-1]
    for R in (1, 2, 4):                                             # growing pools, query three frames after the newest pool frame
        yield emb[:R * 2:2].reshape(-1, C), lab[:R * 2:2].reshape(-1, O), emb[R * 2 + 1].reshape(-1, C)
    yield emb[[0, 3]].reshape(-1, C), lab[[0, 3]].reshape(-1, O), emb[3].reshape(-1, C)              # the newest pool frame is the query itself
    pool = emb[[0, 3]].reshape(-1, C).clone()
    pool[100:140] = pool[hw + 100:hw + 140]                                                           # duplicates of best rows in the older frame
    yield pool, lab[[0, 3]].reshape(-1, O), emb[3].reshape(-1, C)
    moved = torch.roll(lab[3], shifts=(7, 11), dims=(0, 1))                                           # labels moved: seeds land on other objects
    yield emb[[0, 3]].reshape(-1, C), torch.stack([lab[0], moved]).reshape(-1, O), emb[4].reshape(-1, C)
    yield emb[[0, 3]].reshape(-1, C)[: 2 * hw - 333], lab[[0, 3]].reshape(-1, O)[: 2 * hw - 333], emb[4].reshape(-1, C)   # not whole frames


def run_cases(ops):
    """All seven cases through the public API -> dict(hash = SHA-256 over the seven outputs, tested, rescored) with the counters of these calls."""
    emb, lab, hw = clip()
    O = lab.shape[-1]
    h = hashlib.sha256()
    torch.cuda.synchronize()
    ops.dense_prune_stats(reset=True)
    for pool, labels, q in cases(emb, lab, hw):
        prep = ops.label_prep(labels.contiguous())
        out = torch.empty(O, q.shape[0], device="cuda")
        ps = ops.split_rows(pool.contiguous())
        qs = ops.split_rows(q.contiguous(), overflow=ps.overflow)
        ops.dense_match_min_split(q.contiguous(), qs, pool.contiguous(), ps, prep, torch.zeros(O, device="cuda"), out, 1, q.shape[0], True)
        torch.cuda.synchronize()
        h.update(out.cpu().numpy().tobytes())
    st = ops.dense_prune_stats(reset=True)
    return dict(hash=h.hexdigest(), tested=st["tested"], rescored=st["rescored"])


def main():
    import aoc_amd
    from aoc_amd import ops
    aoc_amd._lib.lib()
    mode = ([a for a in sys.argv[1:] if a in ("--check", "--seeded")] + ["--write"])[0]
    runs = [run_cases(ops) for _ in range(RUNS)]
    for r in runs:
        print(r["hash"][:16], "tested", r["tested"], "rescored", r["rescored"], flush=True)
    if any((r["hash"], r["tested"]) != (runs[0]["hash"], runs[0]["tested"]) for r in runs):
        raise SystemExit("hash or tested count differ between runs of the same build: nothing written")
    rescored = [r["rescored"] for r in runs]
    if mode == "--write":
        if not os.environ.get("AOC_LIB_FILE") or os.environ.get("AOC_DENSE_SEED") != "0":
            raise SystemExit("writing needs a development library of the parent commit (AOC_LIB_FILE=...) run with AOC_DENSE_SEED=0")
        fix = dict(hash=runs[0]["hash"], tested=runs[0]["tested"], rescored=max(rescored), rescored_runs=rescored)
    else:
        with open(FIXTURE) as f:
            fix = json.load(f)
        same = (fix["hash"], fix["tested"]) == (runs[0]["hash"], runs[0]["tested"])
        print(("equal to" if same else "DIFFERS from") + f" the fixture; rescored {rescored} against {fix['rescored']} without seeds")
        if not same or mode == "--check":
            raise SystemExit(0 if same else 1)
        fix["parent_seeded_rescored_runs"] = rescored                # information only: no test reads it
    with open(FIXTURE, "w") as f:
        json.dump(fix, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
