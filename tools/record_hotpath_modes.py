"""Developer tool (GPU box): SHA-256 of hotpath.proto_mask_features' two results (the proto-mask tensor and the attention head) for every frame
of every orchestration mode -> tests/golden/hotpath_modes_parent.json.

The committed fixture was written by this script on the commit BEFORE proto_mask_features was cut into stages.  The stages enqueue the same
library calls with the same arguments in the same order on the same streams, so they must reproduce it bit for bit
(tests/test_gpu_hotpath_modes.py asserts that, and imports the cases from here).  These are the modes the one-call C path
(FrameRunner / aoc_frame_enqueue) is no oracle for.

    python tools/record_hotpath_modes.py            # write the fixture (refuses when two runs of a case differ)
    python tools/record_hotpath_modes.py --check    # compare with the committed fixture instead, exit status 1 on a difference

Every case walks FRAMES query frames of a synthetic clip (query t, previous frame t - 1) whose pool is the clip's first POOL_FRAMES[t - 1]
frames: one frame twice, then two, then three -- so the caches in dense_state (split records of the pool, pooled reference heads, per-set bias
table) are built, reused and extended.  The maps are as small as the condition below allows: odd sizes from 7 x 9 up (hw odd, int(h / 2) + 1
differs from h / 2), radii [2, 4], three objects unless the case is about their number.

Condition (checked on the labels, on the host, before anything runs): every object has at least kmax labelled pixels in the first pool frame
as the k-means chain sees it, so no case degenerates into the sticky-K path by accident.  Where 7 x 9 cannot meet it the case names the next
odd size that does (SIZES_TRIED says how the sizes and seeds were walked); the fixture records each case's size.
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "hotpath_modes_parent.json")

FRAMES = 4
POOL_FRAMES = [1, 1, 2, 3]              # pool frames seen by query frame t = 1 .. 4
RADII = [2, 4]
# how a case's (size, seed) was chosen: sizes (7 + 2 i) x (9 + 2 i), i = 0, 1, ...; at each size the seeds 0 .. 199 in order; the first pair
# that meets the condition.  find_shape() repeats the walk.
SIZES_TRIED = "(7 + 2 i) x (9 + 2 i), seeds 0..199 at each size, first that meets the condition"

# name -> (h, w, seed) and what differs from: three objects, width 100, one level of 16 proxies, float32, atrous rate 1
CASES = {
    "plain_rng": dict(size=(7, 9), seed=31),
    "dense_state": dict(size=(7, 9), seed=31),
    "cluster_state_side_stream": dict(size=(7, 9), seed=31),
    "cluster_ahead_batch_of_two": dict(size=(7, 9), seed=31),
    "dense_stream": dict(size=(7, 9), seed=31),
    "deferred_two_sequences": dict(size=(7, 9), seed=31, seed_b=36),
    "dense_precision_fp32": dict(size=(7, 9), seed=31),
    "incremental_bank": dict(size=(7, 9), seed=31),
    "float16_without_clustering": dict(size=(7, 9), seed=31, f16=True),
    "float16_inline": dict(size=(7, 9), seed=31, f16=True),
    "match_pool_atrous2": dict(size=(33, 35), seed=1, grate=2),
    "levels_2_4": dict(size=(7, 9), seed=0, levels=[2, 4]),
    "seventeen_objects": dict(size=(35, 37), seed=94, n_obj=17),
    "width_104": dict(size=(7, 9), seed=31, C=104),
}


def case_config(hot, case):
    return hot.MatchingConfig(MODEL_MULTI_LOCAL_DISTANCE=list(RADII), CLUSTER_LEVELS=case.get("levels"),
                              MODEL_FLOAT16_MATCHING=case.get("f16", False), TEST_GLOBAL_ATROUS_RATE=case.get("grate", 1))


def make_clip(syn, case, seed):
    """(emb [FRAMES + 1, h, w, C], one-hot labels [FRAMES + 1, h, w, O]) as float32 numpy arrays."""
    (h, w), O = case["size"], case.get("n_obj", 3)
    clip = syn.make_clip(syn.ClipConfig("hotpath-modes", h, w, O, 16, case.get("C", 100), FRAMES + 1), seed, frames=FRAMES + 1)
    return clip["emb"], np.stack([syn.one_hot(l, O) for l in clip["lab"]])


def fewest_labelled(case, lab):
    """The smallest per-object pixel count of the first pool frame as the clustering sees it (on the atrous grid with a global rate)."""
    r = case.get("grate", 1)
    return int(lab[0][::r, ::r].sum(axis=(0, 1)).min())


def kmax_of(case):
    return max(case.get("levels") or [16])


def meets_condition(syn, case):
    seeds = [case["seed"]] + ([case["seed_b"]] if "seed_b" in case else [])
    return all(fewest_labelled(case, make_clip(syn, case, s)[1]) >= kmax_of(case) for s in seeds)


def find_shape(syn, case, max_steps=40):
    """The walk of SIZES_TRIED for one case -> ((h, w), seed)."""
    for i in range(max_steps):
        for seed in range(200):
            trial = dict(case, size=(7 + 2 * i, 9 + 2 * i), seed=seed)
            trial.pop("seed_b", None)
            if meets_condition(syn, trial):
                return trial["size"], seed
    raise SystemExit("no size meets the condition")


class _Walk:
    """The device inputs of one clip and the per-frame arguments of proto_mask_features."""

    def __init__(self, aoc, case, seed):
        self.case, self.seed = case, seed
        self.O = case.get("n_obj", 3)
        emb, lab = make_clip(aoc.synthetic, case, seed)
        self.lab_host = lab
        self.emb, self.lab = torch.from_numpy(emb).cuda(), torch.from_numpy(lab).cuda()
        self.bias = (torch.arange(self.O, dtype=torch.float32) * 0.07 - 0.2).cuda()

    def pool(self, t):
        R = POOL_FRAMES[t - 1]
        return self.emb[:R].contiguous(), self.lab[:R].contiguous()

    def frame(self, t):
        """(ref_emb, ref_labels, prev_emb, prev_labels, cur_emb, dis_bias) of query frame t."""
        return self.pool(t) + (self.emb[t - 1], self.lab[t - 1], self.emb[t], self.bias)

    def match_pool(self, t):
        r = self.case.get("grate", 1)
        ref_emb, ref_lab = self.pool(t)
        return (ref_emb[:, ::r, ::r].contiguous(), ref_lab[:, ::r, ::r].contiguous()) if r > 1 else (ref_emb, ref_lab)

    def init_rows(self, ops, mc, t, n_frames=1, pool_frames=None):
        """Initial rows of n_frames chains over query frame t's pool (or over the given pool frames), drawn on the host from the label counts."""
        r = self.case.get("grate", 1)
        ids = list(range(POOL_FRAMES[t - 1])) if pool_frames is None else pool_frames
        counts = self.lab_host[ids][:, ::r, ::r].sum(axis=(0, 1, 2)).astype(np.int64)
        rows, _ = ops.kmeans_init_rows_draw(np.random.RandomState(1000 * self.seed + t), counts, mc.cluster_levels, n_frames, max(mc.cluster_levels))
        return [torch.from_numpy(rows[f]).cuda() for f in range(n_frames)]


def run_case(aoc, name):
    """One walk of a case -> [(feat, head) per frame, on the host] (two sequences: the first's frames, then the second's)."""
    hot, ops = aoc.hotpath, aoc.ops
    case = CASES[name]
    mc = case_config(hot, case)
    wk = _Walk(aoc, case, case["seed"])
    out = []
    ds = {}
    pmf = hot.proto_mask_features

    def ahead(t, w=wk):
        m_emb, m_lab = w.match_pool(t)
        return hot.launch_cluster_proxies(mc, m_emb, m_lab, w.init_rows(ops, mc, t)[0])

    if name == "deferred_two_sequences":
        walks = [wk, _Walk(aoc, case, case["seed_b"])]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        corr, main = torch.cuda.Stream(), torch.cuda.current_stream()
        states, results = [{}, {}], [[], []]
        for s in streams:
            s.wait_stream(main)                          # the walks' inputs were uploaded on the current stream
        for t in range(1, FRAMES + 1):
            pend, got = [], []
            for w, s, st in zip(walks, streams, states):
                with torch.cuda.stream(s):
                    feat, head, aux = pmf(mc, *w.frame(t), cluster_ahead=ahead(t, w), dense_state=st, defer_correlation=True)
                    pend.append(aux["pending_correlation"])
                    got.append((feat, head))
            done = hot.launch_correlations(pend, stream=corr)
            main.wait_event(done)
            for s in streams:
                main.wait_stream(s)                      # the rest of a frame (proto_finish) is on the frame's own stream
            for k, (feat, head) in enumerate(got):
                results[k].append((feat.cpu(), head.cpu()))
        return results[0] + results[1]

    side = torch.cuda.Stream() if name in ("cluster_state_side_stream", "cluster_ahead_batch_of_two", "incremental_bank") else None
    dense = torch.cuda.Stream() if name == "dense_stream" else None
    bank = hot.IncrementalProxyBank(mc, wk.O, wk.emb.shape[-1], max(POOL_FRAMES), wk.emb.device) if name == "incremental_bank" else None
    handles = []                                             # cluster_ahead_batch_of_two: (pool frames, handles not used yet)
    for t in range(1, FRAMES + 1):
        R = POOL_FRAMES[t - 1]
        rng = np.random.RandomState(1000 * case["seed"] + t)
        args = wk.frame(t)
        if name == "plain_rng":
            res = pmf(mc, *args, rng=rng)
        elif name in ("dense_state", "levels_2_4", "width_104", "float16_inline"):
            res = pmf(mc, *args, rng=rng, dense_state=ds)
        elif name == "dense_precision_fp32":
            res = pmf(mc, *args, rng=rng, dense_state=ds, dense_precision="fp32")
        elif name == "cluster_state_side_stream":
            res = pmf(mc, *args, cluster_state=dict(init_rows=wk.init_rows(ops, mc, t)[0]), side_stream=side, dense_state=ds)
        elif name == "cluster_ahead_batch_of_two":
            if not handles or handles[0] != R:
                handles = [R] + hot.launch_cluster_proxies_batch(mc, *wk.pool(t), wk.init_rows(ops, mc, t, 2), side)
            res = pmf(mc, *args, cluster_ahead=handles.pop(1), dense_state=ds)
        elif name == "dense_stream":
            res = pmf(mc, *args, cluster_ahead=ahead(t), dense_state=ds, dense_stream=dense)
        elif name == "incremental_bank":
            while bank.R < R:
                r = bank.R
                bank.append(wk.emb[r], wk.lab[r], wk.init_rows(ops, mc, 10 + r, pool_frames=[r])[0], side)
            res = pmf(mc, *args, cluster_ahead=bank.handle(args[1]), dense_state=ds)
        elif name == "float16_without_clustering":
            res = pmf(mc, *args, cluster_ahead=hot.prepare_without_clustering(mc, *wk.pool(t)), dense_state=ds)
        elif name == "match_pool_atrous2":
            res = pmf(mc, *args, cluster_ahead=ahead(t), dense_state=ds, match_pool=wk.match_pool(t))
        elif name == "seventeen_objects":
            res = pmf(mc, *args, cluster_ahead=ahead(t), dense_state=ds)
        else:
            raise KeyError(name)
        torch.cuda.synchronize()
        out.append((res[0].cpu(), res[1].cpu()))
    return out


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy(), dtype=np.float32).tobytes()).hexdigest()


def digests(frames):
    return [dict(feat=digest(f), head=digest(h)) for f, h in frames]


def main():
    import aoc_amd
    syn = aoc_amd.synthetic
    for name, case in CASES.items():                         # on the host, before anything runs
        if not meets_condition(syn, case):
            raise SystemExit(f"{name}: an object of the first pool frame has fewer than {kmax_of(case)} labelled pixels at {case['size']}, seed {case['seed']}")
    aoc_amd._lib.lib()
    check = "--check" in sys.argv[1:]
    record = {}
    with torch.no_grad():
        for name, case in CASES.items():
            a, b = digests(run_case(aoc_amd, name)), digests(run_case(aoc_amd, name))
            print(f"{name:32s} {case['size'][0]:3d} x {case['size'][1]:3d} frames={len(a)} {a[0]['feat'][:16]} {a[-1]['head'][:16]}", flush=True)
            if a != b:
                raise SystemExit(f"{name}: two runs of the same build differ: nothing written")
            record[name] = dict(size=list(case["size"]), seed=case["seed"], frames=a)
    if check:
        with open(FIXTURE) as f:
            want = json.load(f)["cases"]
        bad = [k for k in CASES if want.get(k, {}).get("frames") != record[k]["frames"]]
        print("differs from the fixture: " + ", ".join(bad) if bad else f"all {len(record)} cases equal the fixture")
        raise SystemExit(1 if bad else 0)
    with open(FIXTURE, "w") as f:
        json.dump(dict(note="sizes: " + SIZES_TRIED + "; a case above 7 x 9 did not meet the condition at any smaller size",
                       pool_frames=POOL_FRAMES, radii=RADII, cases=record), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
