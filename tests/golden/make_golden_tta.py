#!/usr/bin/env python3
"""Golden vectors of the evaluation loop with test-time augmentation (--flip / --ms), produced by RUNNING THE REFERENCE ITSELF (build
container only; see make_golden.py).

    python tests/golden/make_golden_tta.py

``Evaluator.evaluating`` (networks/engine/eval_manager_mm.py:160-394) is called UNMODIFIED (make_golden_r4.load_evaluator) on a mock sequence
whose ``__getitem__`` returns A samples per frame, shaped like VOS_Test's after MultiRestrictSize + MultiToTensor: the image filled with
100 t + a, ``meta['flip']``, the ground truth kept at H x W for every scale and mirrored for flipped samples.  The recording model returns
scripted [1, n_ch, H, W] soft-max maps per (t, a): a shared random field plus per-augmentation noise, mirrored for flipped a.  Stored per case:
the scripted probabilities, the ground truths, per (t, a) the pool's frame ids / every confident mask / the previous frame id and mask as the
model was handed them, and the saved label maps -> tests/golden/eval_loop_tta_<case>.npz.

While recording, in float64: no pixel of any frame may have a top-two gap of the averaged probabilities <= 1e-5 nor an entropy (of the last
augmentation's own maps, the one the reference thresholds) within 1e-5 of unc_ratio -- a fixed seed list is walked until one qualifies; the seed
and the two minima are stored.  An fp32 evaluation fed log(probs) is off by a few 1e-7, so the fixture's labels can be asked for EXACTLY.

Also writes tests/golden/tta_sizes.json: MultiRestrictSize itself (dataloaders/custom_transforms.py, imported by path behind a stand-in cv2
whose resize returns zeros of the requested size) on a handful of (H, W, min_size, max_size, flip, scales).
"""
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_r4 as g4  # noqa: E402

MARGIN = 1e-5


class Seq(torch.utils.data.Dataset):
    def __init__(self, n, H, W, gt, obj_nums, augs):
        self.seq_name, self.n, self.H, self.W, self.gt, self.obj_nums, self.augs = "tta", n, H, W, gt, obj_nums, augs

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        out = []
        for a, (sc, flip) in enumerate(self.augs):
            s = {"current_img": torch.full((3, int(self.H * sc), int(self.W * sc)), float(idx * 100 + a))}
            if idx in self.gt:
                g = self.gt[idx].astype(np.uint8)
                s["current_label"] = torch.from_numpy(g[:, ::-1].copy() if flip else g)[None]
            s["meta"] = {"seq_name": "tta", "frame_num": self.n, "obj_num": int(self.obj_nums[idx]), "current_name": f"{idx:05d}.jpg",
                         "height": self.H, "width": self.W, "flip": flip, "obj_list": list(range(int(self.obj_nums[idx]) + 1))}
            out.append(s)
        return out


class Model:
    def __init__(self, probs):
        self.probs, self.calls = probs, []

    def eval(self):
        return self

    def forward_for_eval(self, mem, ref_e, ref_m, prev_e, prev_m, cur, pred_size, gt_ids):
        t, a = divmod(int(cur[0, 0, 0, 0].item()), 100)
        emb = torch.full((1, 4, 5, 7), float(100 * t + a))           # (frame, augmentation) IS the embedding: the log shows who is in the pool
        sq = lambda m: m.detach().clone().reshape(m.shape[-2], m.shape[-1]).to(torch.int64).numpy()
        self.calls.append(dict(t=t, a=a, ref=[int(e[0, 0, 0, 0]) for e in ref_e], ref_m=[sq(m) for m in ref_m],
                               prev=None if prev_e is None else int(prev_e[0, 0, 0, 0]), prev_m=None if prev_m is None else sq(prev_m)))
        if prev_e is None:
            return None, emb, mem
        return torch.from_numpy(self.probs[(t, a)])[None].clone(), emb, mem


def scripted(seed, augs, n, n_ch, H, W):
    rng = np.random.RandomState(seed)
    probs = {}
    for t in range(1, n):
        base = rng.randn(n_ch, H, W).astype(np.float32) * 2.5
        for a, (_, flip) in enumerate(augs):
            l = base + rng.randn(n_ch, H, W).astype(np.float32) * 0.7
            probs[(t, a)] = torch.softmax(torch.from_numpy(l[:, :, ::-1].copy() if flip else l), 0).numpy()
    return probs


def margins(probs, augs, n, gt, unc):
    """float64: the smallest top-two gap of the averaged (flipped-back, never-seen channels zeroed) probabilities over all frames, and the
    smallest distance of the thresholded entropy from unc_ratio.  label_all_list as the reference keeps it (updated inside the loop)."""
    A = len(augs)
    seen = set(np.unique(gt[0]).tolist())
    min_gap, min_ent = np.inf, np.inf
    for t in range(1, n):
        ps = []
        for a, (_, flip) in enumerate(augs):
            p = probs[(t, a)].astype(np.float64).copy()
            for c in range(p.shape[0]):
                if c not in seen:
                    p[c] = 0
            own, own_seen = p, sorted(seen)
            if t in gt:
                seen |= set(np.unique(gt[t]).tolist())
            ps.append(p[:, :, ::-1] if flip else p)
        mean = np.mean(ps, 0)
        top = np.sort(mean, 0)
        keep = gt[t] == 0 if t in gt else np.ones(mean.shape[1:], bool)
        min_gap = min(min_gap, float((top[-1] - top[-2])[keep].min()))
        e = -(own[own_seen] * np.log(own[own_seen] + 1e-6)).sum(0)
        min_ent = min(min_ent, float(np.abs(e - unc)[keep].min()))
    return min_gap, min_ent


def run_case(name, augs, gt, obj_nums, n=8, H=21, W=29, n_ch=4, mem_every=3, unc=0.6):
    em, log = g4.load_evaluator()
    for seed in range(1, 200):
        probs = scripted(seed, augs, n, n_ch, H, W)
        min_gap, min_ent = margins(probs, augs, n, gt, unc)
        if min_gap > MARGIN and min_ent > MARGIN:
            break
    else:
        raise SystemExit(f"{name}: no seed qualifies")
    assert min_gap > MARGIN and min_ent > MARGIN
    model = Model(probs)
    ev = em.Evaluator.__new__(em.Evaluator)
    ev.cfg = types.SimpleNamespace(BLOCK_NUM=2, TEST_WORKERS=0)
    ev.mem_every, ev.unc_ratio, ev.gpu, ev.model = mem_every, unc, 0, model
    ev.dataset = [Seq(n, H, W, gt, obj_nums, augs)]
    ev.result_root = ev.source_folder = "/tmp/aoc_golden_tta"
    ev.zip_dir = "/tmp/aoc_golden_tta.zip"
    real_cuda, real_empty = torch.Tensor.cuda, torch.cuda.empty_cache
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.empty_cache = lambda: None
    log["saved"].clear()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ev.evaluating()
    finally:
        torch.Tensor.cuda, torch.cuda.empty_cache = real_cuda, real_empty
    A = len(augs)
    out = dict(n_frames=np.int32(n), n_ch=np.int32(n_ch), n_aug=np.int32(A), flips=np.array([f for _, f in augs], np.int32),
               scales=np.array([s for s, _ in augs], np.float32), mem_every=np.int32(mem_every), unc_ratio=np.float32(unc), seed=np.int32(seed),
               min_gap=np.float64(min_gap), min_entropy_distance=np.float64(min_ent), gt_frames=np.array(sorted(gt), np.int32),
               obj_nums=np.array(obj_nums, np.int32), probs=np.stack([np.stack([probs[(t, a)] for a in range(A)]) for t in range(1, n)]))
    for t, g in gt.items():
        out[f"gt{t}"] = g.astype(np.int16)
    assert [(c["t"], c["a"]) for c in model.calls] == [(t, a) for t in range(n) for a in range(A)]
    for c in model.calls:
        k = f"f{c['t']}_a{c['a']}"
        out[k + "_ref_frames"] = np.array(c["ref"], np.int32)
        out[k + "_ref_masks"] = np.stack(c["ref_m"]).astype(np.int16) if c["ref_m"] else np.zeros((0, H, W), np.int16)
        out[k + "_prev_frame"] = np.int32(-1 if c["prev"] is None else c["prev"])
        out[k + "_prev_mask"] = (c["prev_m"] if c["prev_m"] is not None else np.zeros((0, W))).astype(np.int16)
    assert len(log["saved"]) == n - 1
    out["saved_labels"] = np.stack([m.reshape(H, W).to(torch.int64).numpy() for _, m in log["saved"]]).astype(np.int16)
    g4.save_raw("eval_loop_tta_" + name, **out)
    print(f"    seed {seed}, min gap {min_gap:.3e}, min |entropy - unc_ratio| {min_ent:.3e}")


def record_sizes():
    cv2 = types.ModuleType("cv2")
    cv2.setNumThreads = lambda n: None
    cv2.INTER_CUBIC = cv2.INTER_NEAREST = cv2.INTER_LINEAR = 0
    cv2.resize = lambda img, dsize, interpolation=None: np.zeros((dsize[1], dsize[0]) + img.shape[2:], img.dtype)
    sys.modules["cv2"] = cv2
    spec = importlib.util.spec_from_file_location("ref_custom_transforms", os.path.join(g4.CP, "dataloaders", "custom_transforms.py"))
    ct = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ct)
    cases = [(480, 854, None, 800, True, [1.0, 1.1, 1.2, 1.3]), (480, 854, None, 1040.0, False, [1.0]), (480, 854, None, 800, False, [1.0, 0.75, 1.5]),
             (720, 1280, None, 800, True, [1.0, 1.3]), (1280, 720, None, 800, True, [1.3]), (480, 854, 360, None, True, [1.0, 1.25]),
             (241, 321, None, 800, True, [1.0]), (300, 200, 480, None, False, [1.0, 2.0])]
    out = []
    for H, W, mn, mx, flip, scales in cases:
        samples = ct.MultiRestrictSize(mn, mx, flip, scales)({"current_img": np.zeros((H, W, 3), np.float32), "meta": {"flip": False}})
        out.append(dict(H=H, W=W, min_size=mn, max_size=mx, flip=flip, scales=scales,
                        sizes=[[int(s["current_img"].shape[0]), int(s["current_img"].shape[1]), bool(s["meta"]["flip"])] for s in samples]))
    with open(os.path.join(HERE, "tta_sizes.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("tta_sizes.json", len(out), "cases")


def main():
    H, W = 21, 29
    g0 = np.zeros((H, W), np.int64)
    g0[3:9, 4:12] = 1
    g0[11:18, 15:26] = 2
    g5 = np.zeros((H, W), np.int64)                # frame 5 carries ground truth that introduces object 3; channel 4 is never seen
    g5[1:6, 18:27] = 3
    run_case("flip", [(1.0, False), (1.0, True)], {0: g0}, [2] * 8)
    run_case("ms", [(1.0, False), (1.3, False)], {0: g0}, [2] * 8)
    run_case("ms_flip", [(1.0, False), (1.0, True), (1.3, False), (1.3, True)], {0: g0}, [2] * 8)
    run_case("ms_flip_join", [(1.0, False), (1.0, True), (1.3, False), (1.3, True)], {0: g0, 5: g5}, [2] * 5 + [3] * 3, n_ch=5)
    record_sizes()


if __name__ == "__main__":
    main()
