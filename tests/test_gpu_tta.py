"""aoc_tta_merge (ops.tta_merge) on the GPU: against a float64 restatement of eval_manager_mm.py's per-frame tail at real sizes, its exact
properties, and the default HotPathBackend against the label maps recorded at the parent commit.

Float results are compared under a DERIVED bound (U = 2^-24), never one read off the kernel's output:
  * the interpolated logit is off as in _bilinear_tol of tests/test_gpu_stream_kernels.py (two roundings of the source position per axis,
    2 U (in - 1) in the weight, times the interpolant's slope -- here the plane's largest neighbour difference instead of 2 max|x| -- plus
    8 U max|x| for the blend's roundings), the subtraction of the maximum adds U * 2 max|x|: eps in the exponent;
  * logits off by at most eps each move a soft-max value by at most p (1 - p) (e^(2 eps) - 1) <= (e^(2 eps) - 1) / 4 (worst case: its own logit
    up, every other one down);
  * expf (2 U), the n_ch - 1 additions of the denominator and the division: gamma(n_ch + 4) relative, on a value <= 1;
  * the A - 1 additions of s (each on a partial sum <= A, divided by A afterwards) and the division by A: A U.
Every such comparison runs the slipped-reference self-check: a flip not undone, align_corners=False, and a mean over A - 1 augmentations
must each leave the bound."""
import hashlib
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()
    return aoc_amd


def _bits(seen):
    return sum(1 << c for c in seen)


def _ref64(logits, flips, H, W, bits, join, unc, mode, align_corners=True, undo_flip=True, drop_last=False):
    """float64 restatement of aoc_tta_merge's contract (include/aoc_hip.h).  Returns mean [n_ch, H, W], label, entropy, top-two gap."""
    A, n_ch = len(logits), logits[0].shape[0]
    bits = [bits] * A if isinstance(bits, int) else bits
    ps, own = [], None
    for l, f, b in zip(logits, flips, bits):
        p = torch.softmax(F.interpolate(l[None].double(), size=(H, W), mode="bilinear", align_corners=align_corners)[0], dim=0)
        seen = torch.tensor([(b >> c) & 1 for c in range(n_ch)], dtype=torch.float64).view(-1, 1, 1)
        p = p * seen
        own = p
        ps.append(p.flip(2) if (f and undo_flip) else p)
    if drop_last and A > 1:
        ps = ps[:-1]
    mean = torch.stack(ps).sum(0) / len(ps)
    top = mean.topk(2, dim=0).values if n_ch > 1 else torch.stack([mean[0], mean[0] - 1])
    label = mean.argmax(0)
    src = own if mode == "reference" else mean
    seen_last = torch.tensor([(bits[-1] >> c) & 1 for c in range(n_ch)], dtype=torch.float64).view(-1, 1, 1)
    ent = -(seen_last * src * torch.log(src + 1e-6)).sum(0)
    if join is not None:
        keep = (join == 0)
        label = torch.where(keep, label, join.long())
        ent = torch.where(keep, ent, (join < 0).double())
    return mean, label, ent, top[0] - top[1]


def _tol(logits, H, W, n_ch):
    A = len(logits)
    eps = []
    for l in logits:
        M = float(l.abs().max())
        h, w = l.shape[1:]
        dy = 2 * U * (h - 1) if H > 1 else 0.0
        dx = 2 * U * (w - 1) if W > 1 else 0.0
        # the interpolant's slope in a weight is the difference of the two neighbours it blends: the plane's largest one per axis (<= 2 M)
        Dy = float((l[:, 1:] - l[:, :-1]).abs().max()) if h > 1 else 0.0
        Dx = float((l[:, :, 1:] - l[:, :, :-1]).abs().max()) if w > 1 else 0.0
        eps.append(Dy * dy + Dx * dx + 8 * U * M + 2 * M * U)
    soft = sum((math.exp(2 * e) - 1.0) / 4.0 for e in eps) / A
    return soft + gamma(n_ch + 4) + A * U


def _smooth_logits(rng, n_ch, h, w, amp, base):
    coarse = torch.from_numpy(base)
    l = F.interpolate(coarse[None], size=(h, w), mode="bicubic", align_corners=True)[0] * amp
    return (l + torch.from_numpy(rng.standard_normal((n_ch, h, w)).astype(np.float32)) * 0.5).contiguous()


SIZES = [(121, 213), (157, 277), (145, 261)]
#        H,   W,   A, n_ch, identity, mode,         join
CASES = [(480, 854, 1, 4, False, "reference", False),
         (480, 854, 2, 4, False, "reference", True),
         (480, 854, 4, 4, False, "reference", False),
         (480, 854, 4, 4, False, "consistent", True),
         (484, 852, 6, 2, False, "reference", False),
         (484, 852, 4, 11, False, "consistent", False),
         (480, 854, 2, 32, False, "reference", True),
         (480, 854, 6, 11, False, "reference", False),
         (121, 213, 2, 4, True, "consistent", True),
         (484, 852, 1, 32, False, "consistent", False)]


@pytest.mark.parametrize("H,W,A,n_ch,identity,mode,with_join", CASES)
def test_tta_merge_vs_float64(aoc, H, W, A, n_ch, identity, mode, with_join):
    rng = np.random.RandomState(H + 7 * A + 31 * n_ch + (mode == "consistent"))
    base = rng.standard_normal((n_ch, 31, 54)).astype(np.float32)
    flips = [bool(a % 2) for a in range(A)]
    seen = [c for c in range(n_ch) if c % 5 != 3] if n_ch > 2 else [0, 1]           # unseen channels 3, 8, 13, ...
    unseen = [c for c in range(n_ch) if c not in seen]
    logits = []
    for a in range(A):
        h, w = (H, W) if identity else SIZES[(a // 2) % len(SIZES)]
        l = _smooth_logits(rng, n_ch, h, w, 4.0, base)
        # a never-seen channel that dominates a pixel leaves the seen ones a few 1e-4 each, zeroed without renormalisation: top-two gaps below any
        # float32 margin on a quarter of the map.  Lowered by 3 it still wins often enough to be checked (asserted below) without doing that
        l[unseen] -= 3.0
        logits.append(l.flip(2).contiguous() if flips[a] else l)
    bits = _bits(seen)
    join = None
    if with_join:
        j = np.zeros((H, W), np.int32)
        j[5:40, 10:90] = min(n_ch - 1, 3)
        j[50:60, 100:160] = -1
        join = torch.from_numpy(j)
    unc = 0.6
    out = aoc.ops.tta_merge([l.cuda() for l in logits], flips, H, W, bits, None if join is None else join.cuda(), unc, mode, want_mean=True)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in out.items()}
    mean, label, ent, gap = _ref64(logits, flips, H, W, bits, join, unc, mode)
    tol = _tol(logits, H, W, n_ch)
    err = (got["mean_probs"].double() - mean).abs()
    print(f"tta_merge {H}x{W} A={A} n_ch={n_ch} {mode}: tol {tol:.3e} max err {float(err.max()):.3e}")
    assert float(err.max()) <= tol, f"mean_probs: worst error {float(err.max()):.3e} > bound {tol:.3e}"
    slips = dict(align=_ref64(logits, flips, H, W, bits, join, unc, mode, align_corners=False)[0] if not identity else None,
                 flip=_ref64(logits, flips, H, W, bits, join, unc, mode, undo_flip=False)[0] if any(flips) else None,
                 drop=_ref64(logits, flips, H, W, bits, join, unc, mode, drop_last=True)[0] if A > 1 else None)
    for name, s in slips.items():
        if s is not None:
            assert float((s - mean).abs().max()) > tol, f"slipped reference '{name}' stays inside the bound (bound too loose)"
    # labels where the float64 top-two gap exceeds twice the bound (joined pixels are exact), at most 1 % of the map left out
    joined = torch.zeros(H, W, dtype=torch.bool) if join is None else (join != 0)
    sure = (gap > 2 * tol) | joined
    assert float((~sure).float().mean()) <= 0.01
    assert torch.equal(got["label"][sure].long(), label[sure])
    if unseen:
        everything_seen = _ref64(logits, flips, H, W, _bits(range(n_ch)), join, unc, mode)[1]
        assert float((everything_seen != label).float().mean()) > 0.01          # the zeroing decides a fair share of the map (2.3 - 8.4 % in these cases)
    # the confident map's own decision, 125 or not, where the float64 entropy is further than twice the bound from unc_ratio (joined pixels are
    # exact: 0 or 1 against unc_ratio); everywhere else it IS the label, compared above
    sure_c = ((ent - unc).abs() > 2 * tol) | joined
    print(f"  left out: labels {float((~sure).float().mean()):.4%}, confident {float((~sure_c).float().mean()):.4%}")
    assert float((~sure_c).float().mean()) <= 0.01
    assert torch.equal((got["confident"] == 125)[sure_c], (ent > unc)[sure_c])
    assert torch.equal(got["confident"], torch.where(got["confident"] == 125, got["confident"], got["label"]))
    assert float((got["entropy"].double() - ent).abs().max()) <= 40 * tol       # |d(p log p)/dp| <= |log 1e-6| + 1 per channel, errors sum to 0
    assert torch.equal(got["label_flipped"], got["label"].flip(1))
    if mode == "consistent":
        assert torch.equal(got["confident_flipped"], got["confident"].flip(1))


@pytest.mark.parametrize("W", [853, 854])
@pytest.mark.parametrize("n_ch", [4, 11, 32])
def test_mirrored_twin_gives_the_same_bits(aoc, W, n_ch):
    """A = 2 with the second augmentation the exact mirror of the first and flip = 1: s = p + p and s / 2 are exact, so label and mean_probs
    have the bits of A = 1 -- at an odd and an even W, in every channel bucket."""
    rng = np.random.RandomState(W + n_ch)
    H, h, w = 97, 33, 60 + W % 2                          # identity-size part: an odd and an even width as well
    l = torch.from_numpy(rng.standard_normal((n_ch, h, w)).astype(np.float32) * 3).cuda()
    bits = _bits(range(n_ch))
    one = aoc.ops.tta_merge([l], [False], H, W, bits, None, 0.6, "consistent", want_mean=True)
    two = aoc.ops.tta_merge([l, l.flip(2).contiguous()], [False, True], H, W, bits, None, 0.6, "consistent", want_mean=True)
    # the mirrored twin samples source position scale * (W - 1 - x') of the mirrored plane: the same four values only when the grid is symmetric,
    # which align_corners=True makes it up to the rounding of the source position -- compare through the float64 margin there, bits where exact
    same = torch.equal(one["mean_probs"], two["mean_probs"])
    if not same:
        d = float((one["mean_probs"] - two["mean_probs"]).abs().max())
        assert d <= 2 * _tol([l.cpu()], H, W, n_ch), d
    ident = aoc.ops.tta_merge([l], [False], h, w, bits, None, 0.6, "consistent", want_mean=True)
    twin = aoc.ops.tta_merge([l, l.flip(2).contiguous()], [False, True], h, w, bits, None, 0.6, "consistent", want_mean=True)
    for k in ("label", "mean_probs", "confident", "entropy"):
        assert torch.equal(ident[k], twin[k]), k                # identity size: both sample the same pixel exactly


def test_null_outputs_stay_unwritten_and_one_lane_equals_the_separate_calls(aoc):
    """Every output alone, between NaN / sentinel canaries: the others are NULL and nothing else is touched; and A = 1, no flip at identity
    size equals softmax -> ops.confident_labels bit for bit in the label (same arithmetic order), entropy within the margin."""
    import ctypes
    ops = aoc.ops
    rng = np.random.RandomState(5)
    n_ch, h, w, H, W = 5, 23, 37, 45, 73
    l = torch.from_numpy(rng.standard_normal((n_ch, h, w)).astype(np.float32) * 3).cuda()
    full = ops.tta_merge([l], [False], H, W, 0b10111, None, 0.6, "consistent", want_mean=True)
    for key, n, dtype in (("label", H * W, torch.int32), ("confident", H * W, torch.int32), ("label_flipped", H * W, torch.int32),
                          ("confident_flipped", H * W, torch.int32), ("entropy", H * W, torch.float32), ("mean_probs", n_ch * H * W, torch.float32)):
        pad = 64
        buf = torch.full((n + 2 * pad,), -7, dtype=dtype, device="cuda") if dtype == torch.int32 else torch.full((n + 2 * pad,), float("nan"), device="cuda")
        d = ops._TtaDesc()
        d.n_aug, d.n_ch, d.H, d.W, d.mode, d.unc_ratio = 1, n_ch, H, W, 1, 0.6
        d.h[0], d.w[0], d.flip[0], d.exist_bits[0], d.plane_stride[0], d.logits[0] = h, w, 0, 0b10111, h * w, l.data_ptr()
        setattr(d, key, buf.data_ptr() + pad * 4)
        aoc._lib.check(aoc._lib.lib().aoc_tta_merge(ctypes.byref(d), ops._stream()), "aoc_tta_merge")
        torch.cuda.synchronize()
        assert torch.equal(buf[pad:pad + n].view(full[key].shape), full[key]) or (dtype == torch.float32 and torch.allclose(buf[pad:pad + n].view(full[key].shape), full[key], rtol=0, atol=0, equal_nan=True)), key
        edge = torch.cat([buf[:pad], buf[pad + n:]])
        assert (torch.isnan(edge).all() if dtype == torch.float32 else bool((edge == -7).all())), f"{key}: written outside the map"
    probs = torch.softmax(F.interpolate(l[None], size=(H, W), mode="bilinear", align_corners=True)[0], dim=0)
    lab, conf, ent = ops.confident_labels(probs.reshape(n_ch, -1), 0b10111, None, 0.6)
    m64, label64, ent64, gap = _ref64([l.cpu()], [False], H, W, 0b10111, None, 0.6, "consistent")
    tol = _tol([l.cpu()], H, W, n_ch)
    sure = gap > 2 * tol
    assert float((~sure).float().mean()) <= 0.01
    assert torch.equal(full["label"].cpu()[sure], lab.view(H, W).cpu()[sure])
    sure_c = sure & ((ent64 - 0.6).abs() > 2 * tol)
    assert torch.equal(full["confident"].cpu()[sure_c], conf.view(H, W).cpu()[sure_c])


@pytest.mark.parametrize("case", ["flip", "ms", "ms_flip", "ms_flip_join"])
def test_reference_goldens_through_the_kernel(aoc, golden, case):
    """tests/golden/eval_loop_tta_*.npz (the reference's own loop) with logits = log(probs) at identity size, where the bilinear step is an
    exact copy: every mask and label exactly equal, through AugmentedMemoryPolicy with the default merge (ops.tta_merge) and through
    ops.tta_merge alone against the CPU restatement on every frame."""
    from test_tta_host import _replay, check_handed, cpu_merge
    g = golden("eval_loop_tta_" + case)
    check_handed(g, _replay(g, "reference", merge=None, to_dev=lambda t: t.cuda()))
    A, H, W = int(g["n_aug"]), *g["probs"].shape[-2:]
    flips = [bool(f) for f in g["flips"]]
    for t in range(g["probs"].shape[0]):
        logits = [torch.log(torch.from_numpy(g["probs"][t, a].copy())) for a in range(A)]
        for mode in ("reference", "consistent"):
            want = cpu_merge(logits, flips, H, W, 0b0111, None, float(g["unc_ratio"]), mode)
            got = aoc.ops.tta_merge([l.cuda() for l in logits], flips, H, W, 0b0111, None, float(g["unc_ratio"]), mode)
            for k in want:
                # the fixtures' margins (1e-5, asserted while recording) cover the label and the reference mode's entropy, not the merged one's
                if k != "entropy" and (mode == "reference" or k.startswith("label")):
                    assert torch.equal(got[k].cpu(), want[k]), (t, mode, k)


def test_default_backend_returns_the_parent_commits_labels(aoc):
    """HotPathBackend built without augmentations against tests/golden/tta_parent_labels.json (SHA-256 of the per-frame label maps, written by
    tools/record_tta_parent_labels.py at the parent commit; never taken from the code under test)."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_tta_parent_labels as rec
    from aoc_amd import eval_runner as er
    with open(rec.FIXTURE) as f:
        want = json.load(f)
    dev = torch.device("cuda", 0)
    for name in rec.SEQUENCES:
        spec = rec.make_spec(name)
        got = rec.digest(rec.run_labels(er.HotPathBackend(dev), spec, er.load_sequence(spec, dev)))
        assert got == want[name], name


def _iou(a, b, n_obj):
    vals = []
    for o in range(n_obj):
        pa, pb = a == o, b == o
        union = int((pa | pb).sum())
        vals.append(1.0 if union == 0 else int((pa & pb).sum()) / union)
    return float(np.mean(vals))


def _run_backend(backend, spec, data, each_frame=None):
    emb, gt = data
    backend.start(spec)
    backend.first_frame(emb[0], gt[0])
    out = []
    for t in range(1, emb.shape[0]):
        out.append(backend.frame(emb[t]).cpu().numpy())
        if each_frame is not None:
            each_frame(t, backend)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("h,w,n_obj,levels", [(24, 40, 3, (16,)), (33, 45, 4, (8, 16, 32))])
def test_one_unflipped_lane_is_the_default_backend(aoc, h, w, n_obj, levels):
    """HotPathBackend(augmentations=[(h, w, False)]) -- the lane's logits decided by aoc_tta_merge -- against the default backend, whose tail is
    interpolate / softmax / aoc_confident_labels: per-frame mask IoU >= 1 - 1e-3 (the budget of tests/test_gpu_closed_loop.py)."""
    er = aoc.eval_runner
    dev = torch.device("cuda", 0)
    spec = er.SequenceSpec("tta-one-lane", h, w, n_obj, 8, seed=31, levels=levels, mem_every=3)
    data = er.load_sequence(spec, dev)
    want = _run_backend(er.HotPathBackend(dev), spec, data)
    got = _run_backend(er.HotPathBackend(dev, augmentations=[(h, w, False)]), spec, data)
    ious = [_iou(g, w_, n_obj) for g, w_ in zip(got, want)]
    print("one lane vs default, per-frame IoU:", ious)
    assert len(got) == spec.frames - 1 and min(ious) >= 1.0 - 1e-3, ious


@pytest.mark.parametrize("mode", ["reference", "consistent"])
def test_four_lanes_closed_loop(aoc, mode):
    """Two scales with their flipped twins on a small sequence: runs to the end, every lane's pool grows on the same frames, a flipped lane's
    previous mask is the mirror of its twin's, and a second run returns the same labels bit for bit."""
    er = aoc.eval_runner
    dev = torch.device("cuda", 0)
    h, w, n_obj = 24, 40, 3
    augs = [(h, w, False), (h, w, True), (29, 49, False), (29, 49, True)]
    spec = er.SequenceSpec("tta-four-lanes", h, w, n_obj, 8, seed=32, levels=(16,), mem_every=3)
    data = er.load_sequence(spec, dev)
    pools = []

    def each_frame(t, be):
        sizes = [len(r) for r in be.tta.ref_embeddings]
        assert len(set(sizes)) == 1 and sizes == [len(m) for m in be.tta.ref_mask_confident], (t, sizes)
        pools.append(sizes[0])
        for a in (1, 3):
            assert torch.equal(be.tta.prev_mask[a], be.tta.prev_mask[a - 1].flip(1)), (t, a)
            assert tuple(be.tta.prev_embedding[a].shape[:2]) == augs[a][:2]

    runs = [_run_backend(er.HotPathBackend(dev, augmentations=augs, tta_mode=mode), spec, data, each_frame) for _ in range(2)]
    assert pools[:7] == [1, 1, 2, 2, 2, 3, 3] and pools[7:] == pools[:7]           # frames 3 and 6 join (mem_every = 3)
    assert len(runs[0]) == 7 and all(l.shape == (4 * h, 4 * w) for l in runs[0])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    gt = data[1].cpu().numpy()
    ious = [_iou(l, gt[t + 1], n_obj) for t, l in enumerate(runs[0])]
    print(f"four lanes ({mode}), per-frame IoU against the synthetic ground truth:", ious)
