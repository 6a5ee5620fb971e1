"""Developer tool (GPU box): SHA-256 of the dense op's fp32 output for a fixed list of seeded cases -> tests/golden/dense_hi_ring_parent.json.

The committed fixture was written by this script on the commit BEFORE the dense kernel staged hi planes only; a change of the kernel that keeps
every pair's operation order must reproduce it bit for bit (tests/test_gpu_dense_hi_ring.py asserts that, and imports the cases from here).

    python tools/record_dense_hashes.py            # write the fixture (refuses when two runs of a case differ)
    python tools/record_dense_hashes.py --check    # compare with the committed fixture instead, exit status 1 on a difference

Only the public API is used: ops.label_prep, ops.split_rows, ops.dense_match_min_split, ops.dense_prune_stats.  Every case must take the split
path (tested pairs > 0), so a take-over by the exact-fp32 kernels cannot hide behind an equal hash.
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "dense_hi_ring_parent.json")

POOL_STRIDE, QUERY_OFFSET = 5, 3          # the bench's memory policy: every 5th frame joins the pool; the query is three frames after the newest
ORACLE_LIMIT = 2e7                        # n * m up to which the test also asks the CPU oracle (as test_split_matches_fp32_and_oracle)


def _clip_case(cfg_name, R, seed=0, query_frame=None, pool_rows=None):
    """Pool = frames 0, 5, ..., 5 (R - 1) of a synthetic clip, query = newest pool frame + 3 (or the given frame; pool_rows cuts the pool)."""
    from aoc_amd import synthetic as syn
    cfg = syn.CONFIGS[cfg_name]
    last = (R - 1) * POOL_STRIDE
    qf = last + QUERY_OFFSET if query_frame is None else query_frame
    clip = syn.make_clip(cfg, seed, frames=max(last, qf) + 1)
    pool = clip["emb"][0:last + 1:POOL_STRIDE].reshape(-1, cfg.c)
    lab = np.concatenate([syn.one_hot(clip["lab"][i], cfg.n_obj).reshape(-1, cfg.n_obj) for i in range(0, last + 1, POOL_STRIDE)])
    if pool_rows is not None:
        pool, lab = pool[:pool_rows], lab[:pool_rows]
    return clip["emb"][qf].reshape(-1, cfg.c).copy(), np.ascontiguousarray(pool), np.ascontiguousarray(lab)


def _random_case(seed, counts, m, c=100, scale=0.3):
    """counts[o] pool rows of object o (shuffled), m query rows; non-negative values like the embeddings after a ReLU."""
    rng = np.random.RandomState(seed)
    n, o = int(sum(counts)), len(counts)
    pool = (np.maximum(rng.randn(n, c), 0) * scale).astype(np.float32)
    q = (np.maximum(rng.randn(m, c), 0) * scale).astype(np.float32)
    ids = np.repeat(np.arange(o), counts)
    rng.shuffle(ids)
    return q, pool, (ids[:, None] == np.arange(o)).astype(np.float32)


def _tiles_case(j):
    """512 query rows = one row block, for which the launch cuts the tile list into 64 splits.  64 j + 32 tiles in all: the splits 0..31 own
    j + 1 tiles, the splits 32..63 own j.  j = 7..15 -> 7 | 8, 8 | 9, ..., 15 | 16 tiles per split: below one chunk of eight, exactly one, one
    more, and every residue mod 8.  Three objects with partial last tiles (a partial tile is filled up with copies of its first row)."""
    tiles = 64 * j + 32
    t0, t1 = tiles // 2, tiles // 3
    counts = [32 * t0 - 5, 32 * t1 - 17, 32 * (tiles - t0 - t1) - 31]
    assert sum((c + 31) // 32 for c in counts) == tiles
    return _random_case(1000 + j, counts, 512)


def _ties_case():
    """The pool of test_pruning_with_ties_duplicates_and_mixed_norms: exact duplicates of query pixels, near-duplicates that differ in the lo
    plane only, norms over two orders of magnitude."""
    rng = np.random.RandomState(11)
    m, c, o = 1500, 100, 3
    q = (np.maximum(rng.randn(m, c), 0) * 0.3).astype(np.float32)
    dup = q[rng.randint(0, m, 6000)]
    near = dup[:3000] * np.float32(1.0 + 2.0 ** -13) + np.float32(2.0 ** -15)
    big = (np.maximum(rng.randn(4000, c), 0) * 3.0).astype(np.float32)
    tiny = (np.maximum(rng.randn(3000, c), 0) * 0.003).astype(np.float32)
    pool = np.concatenate([dup, near, big, tiny, q[::-1].copy()]).astype(np.float32)
    rng.shuffle(pool)
    ids = rng.randint(0, o, pool.shape[0])
    return q, pool, (ids[:, None] == np.arange(o)).astype(np.float32)


def _absent_case():
    q, pool, lab = _random_case(5, [150, 100, 50, 0, 0], 200)       # objects 3 and 4 absent: 5e4 + the nearest other pixel
    return q, pool, lab


# name -> builder of (query [m, C], pool [n, C], one-hot labels [n, O]) as float32 numpy arrays
CASES = {
    "cfg2_R1": lambda: _clip_case("cfg2", 1),
    "cfg2_R6": lambda: _clip_case("cfg2", 6),
    "cfg2_R12": lambda: _clip_case("cfg2", 12),
    "cfg4_R1_nine_objects": lambda: _clip_case("cfg4", 1),
    **{f"tiles_per_split_{j}_{j + 1}": (lambda j=j: _tiles_case(j)) for j in range(7, 16)},
    "absent_objects": _absent_case,
    "object_of_7_rows": lambda: _random_case(6, [400, 7, 250], 300),
    "pool_not_whole_frames": lambda: _clip_case("tiny", 3, seed=4, pool_rows=2 * 24 * 40 + 137),
    "ties_duplicates_mixed_norms": _ties_case,
    "query_frame_inside_pool": lambda: _clip_case("tiny", 3, seed=7, query_frame=5),
}
# the cases whose n * m the CPU oracle can afford (the test compares them with it as well)
SMALL = [k for k in CASES if not k.startswith("cfg") and k != "ties_duplicates_mixed_norms"]
# cases in which every pair might be decided without a rescoring (none at present: even a pool of one tile rescores its first pair, because
# nothing is known about a pixel before that); kept as the place to say so should a case be added whose rescored count may be zero
DEGENERATE = frozenset()


def run_case(ops, q, pool, lab, bias=None, transform=False):
    """One call of the dense op through the public API -> (fp32 output [O, m] on the host, the kernel's pair counters of that call)."""
    q, pool = torch.from_numpy(q).cuda(), torch.from_numpy(pool).cuda()
    prep = ops.label_prep(torch.from_numpy(lab).cuda())
    m, n_obj = q.shape[0], lab.shape[1]
    out = torch.empty(n_obj, m, device="cuda")
    ps = ops.split_rows(pool)
    qs = ops.split_rows(q, overflow=ps.overflow)
    torch.cuda.synchronize()
    ops.dense_prune_stats(reset=True)
    ops.dense_match_min_split(q, qs, pool, ps, prep, None if bias is None else bias.cuda(), out, 1, m, transform)
    torch.cuda.synchronize()
    return out.cpu(), ops.dense_prune_stats(reset=True)


def digest(out):
    return hashlib.sha256(np.ascontiguousarray(out.numpy(), dtype=np.float32).tobytes()).hexdigest()


def main():
    import aoc_amd
    from aoc_amd import ops
    aoc_amd._lib.lib()
    check = "--check" in sys.argv[1:]
    hashes, bad = {}, []
    for name, build in CASES.items():
        q, pool, lab = build()
        d = []
        for _ in range(2):
            out, st = run_case(ops, q, pool, lab)
            if st["tested"] == 0 or (st["rescored"] == 0 and name not in DEGENERATE):
                raise SystemExit(f"{name}: the split path did not run (tested {st['tested']}, rescored {st['rescored']})")
            d.append(digest(out))
        print(f"{name:32s} m={q.shape[0]:6d} n={pool.shape[0]:7d} O={lab.shape[1]:2d} tested={st['tested']:9d} rescored={st['rescored']:8d} {d[0][:16]}", flush=True)
        if d[0] != d[1]:
            raise SystemExit(f"{name}: two runs of the same build differ ({d[0][:16]} / {d[1][:16]}): nothing written")
        hashes[name] = d[0]
    if check:
        with open(FIXTURE) as f:
            want = json.load(f)
        bad = [k for k in CASES if want.get(k) != hashes[k]]
        print("differs from the fixture: " + ", ".join(bad) if bad else f"all {len(hashes)} cases equal the fixture")
        raise SystemExit(1 if bad else 0)
    with open(FIXTURE, "w") as f:
        json.dump(hashes, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
