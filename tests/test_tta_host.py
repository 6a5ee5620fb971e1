"""Host side of the test-time augmentation path (CPU): the size arithmetic against MultiRestrictSize's recorded output, AugmentedMemoryPolicy
against what the reference's own loop handed its model (tests/golden/eval_loop_tta_*.npz, make_golden_tta.py), the properties of the
"consistent" mode, and aoc_tta_merge's argument validation and descriptor layout.  The merge itself has no CPU implementation in the package:
``cpu_merge`` below is this file's torch restatement of its contract (include/aoc_hip.h), used through the policy's ``merge=`` seam."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import aoc_amd
from golden_cases import check_eval_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TTA_CASES = ["flip", "ms", "ms_flip", "ms_flip_join"]


def cpu_merge(logits_list, flips, H, W, exist_bits, join_label=None, unc_ratio=1.0, mode="reference", want_mean=False):
    A, n_ch = len(logits_list), logits_list[0].shape[0]
    bits = [exist_bits] * A if isinstance(exist_bits, int) else list(exist_bits)
    s, own = None, None
    for l, f, b in zip(logits_list, flips, bits):
        p = torch.softmax(torch.nn.functional.interpolate(l[None].float(), size=(H, W), mode="bilinear", align_corners=True)[0], dim=0)
        p = p * torch.tensor([float((b >> c) & 1) for c in range(n_ch)]).view(-1, 1, 1)
        own = p
        p = p.flip(2) if f else p
        s = p if s is None else s + p
    mean = s / A
    label = torch.argmax(s, dim=0)
    seen = [c for c in range(n_ch) if (bits[-1] >> c) & 1]
    src = (own if mode == "reference" else mean)[seen]
    ent = -1.0 * torch.sum(src * torch.log(src + 1e-6), dim=0)
    if join_label is not None:
        j = join_label.long()
        keep = (j == 0).long()
        label = label * keep + j * (1 - keep)
        ent = ent * keep + (j < 0).long() * (1 - keep)
    region = (ent > unc_ratio).long()
    conf = label * (1 - region) + 125 * region
    out = dict(label=label.int(), confident=conf.int(), label_flipped=label.flip(1).int(), entropy=ent)
    if mode == "consistent":
        out["confident_flipped"] = conf.flip(1).int()
    if want_mean:
        out["mean_probs"] = mean
    return out


def test_multi_restrict_sizes_equal_the_reference():
    with open(os.path.join(ROOT, "tests", "golden", "tta_sizes.json")) as f:
        cases = json.load(f)
    assert len(cases) >= 6
    for c in cases:
        got = aoc_amd.eval_loop.multi_restrict_sizes(c["H"], c["W"], c["min_size"], c["max_size"], c["flip"], c["scales"])
        assert [list(g) for g in got] == c["sizes"], c
    got = aoc_amd.eval_loop.multi_restrict_sizes(480, 854, None, 800, True, [1.0, 1.1, 1.2, 1.3])
    assert got[::2] == [(449, 801, False), (497, 881, False), (545, 961, False), (577, 1041, False)] and all(f for _, _, f in got[1::2])
    assert aoc_amd.eval_loop.multi_restrict_sizes(480, 854, None, 1040.0, False, [1.0]) == [(481, 849, False)]
    assert aoc_amd.eval_loop.map_size(481) == 121 and aoc_amd.eval_loop.map_size(849) == 213


def _replay(g, mode, merge=cpu_merge, to_dev=lambda t: t):
    """Drives an AugmentedMemoryPolicy with the golden's scripted maps (as logits = log(probs) at identity size); yields per frame what every
    augmentation would be handed before the frame, and the label the frame returns."""
    A, n = int(g["n_aug"]), int(g["n_frames"])
    flips = [bool(f) for f in g["flips"]]
    pol = aoc_amd.eval_loop.AugmentedMemoryPolicy(A, flips, mem_every=int(g["mem_every"]), unc_ratio=float(g["unc_ratio"]), mode=mode, merge=merge)
    gt = {int(t): to_dev(torch.from_numpy(g[f"gt{int(t)}"].astype(np.int64))) for t in g["gt_frames"]}
    emb = lambda t: [to_dev(torch.full((1, 1, 4), float(100 * t + a))) for a in range(A)]
    for t in range(n):
        handed = []
        for a in range(A):
            handed.append(dict(ref=[int(e.reshape(-1)[0]) for e in pol.ref_embeddings[a]], ref_m=[m.cpu().long().numpy() for m in pol.ref_mask_confident[a]],
                               prev=-1 if pol.prev_embedding[a] is None else int(pol.prev_embedding[a].reshape(-1)[0]),
                               prev_m=None if pol.prev_mask[a] is None else pol.prev_mask[a].cpu().long().numpy()))
        if t == 0:
            pol.start(emb(0), gt[0])
            label = None
        else:
            logits = [to_dev(torch.log(torch.from_numpy(g["probs"][t - 1, a].copy()))) for a in range(A)]
            label = pol.update(emb(t), logits, gt.get(t))[0].cpu().long().numpy()
        yield t, handed, label


@pytest.mark.parametrize("case", TTA_CASES)
def test_reference_mode_hands_every_augmentation_what_the_reference_does(golden, case):
    g = golden("eval_loop_tta_" + case)
    assert float(g["min_gap"]) > 1e-5 and float(g["min_entropy_distance"]) > 1e-5
    check_handed(g, _replay(g, "reference"))


def check_handed(g, frames):
    for t, handed, label in frames:
        for a, hd in enumerate(handed):
            k = f"f{t}_a{a}"
            assert hd["ref"] == g[k + "_ref_frames"].tolist(), f"{k}: pool membership"
            assert len(hd["ref_m"]) == g[k + "_ref_masks"].shape[0]
            for r, m in enumerate(hd["ref_m"]):
                assert np.array_equal(m, g[k + "_ref_masks"][r]), f"{k}: confident reference mask {r}"
            assert hd["prev"] == int(g[k + "_prev_frame"])
            if t > 0:
                assert np.array_equal(hd["prev_m"], g[k + "_prev_mask"]), f"{k}: previous mask"
        if t > 0:
            assert np.array_equal(label, g["saved_labels"][t - 1]), f"frame {t}: saved label map"


@pytest.mark.parametrize("case", ["flip", "ms_flip", "ms_flip_join"])
def test_consistent_mode_keeps_flipped_lanes_mirrors_of_their_twins(golden, case):
    g = golden("eval_loop_tta_" + case)
    n125 = 0
    for t, handed, _ in _replay(g, "consistent"):
        for a in range(1, len(handed), 2):                       # augmentation a is the flipped twin of a - 1
            twin, me = handed[a - 1], handed[a]
            assert len(me["ref_m"]) == len(twin["ref_m"])
            for m, tm in zip(me["ref_m"], twin["ref_m"]):
                assert np.array_equal(m, tm[:, ::-1])
                n125 += int((m == 125).sum())
            if t > 0:
                assert np.array_equal(me["prev_m"], twin["prev_m"][:, ::-1])
    assert n125 > 0                                              # uncertain pixels did reach the flipped lanes


class _OneLane:
    """AugmentedMemoryPolicy with A = 1 behind MemoryPolicy's interface (probabilities in, as golden_cases.replay_eval_loop feeds them)."""

    def __init__(self, mode, mem_every, unc_ratio):
        self.p = aoc_amd.eval_loop.AugmentedMemoryPolicy(1, [False], mem_every, unc_ratio, mode=mode, merge=cpu_merge)

    ref_embeddings = property(lambda self: self.p.ref_embeddings[0])
    ref_mask_confident = property(lambda self: self.p.ref_mask_confident[0])
    prev_embedding = property(lambda self: self.p.prev_embedding[0])
    prev_mask = property(lambda self: self.p.prev_mask[0])

    def start(self, emb, gt):
        self.p.start([emb], gt)

    def update(self, emb, probs, gt=None):
        return self.p.update([emb], [torch.log(probs)], gt)


@pytest.mark.parametrize("mode", ["reference", "consistent"])
@pytest.mark.parametrize("name", ["eval_loop_mem3", "eval_loop_join_obj3"])
def test_one_augmentation_is_the_memory_policy(golden, mode, name):
    g = golden(name)
    check_eval_loop(g, _OneLane(mode, int(g["mem_every"]), float(g["unc_ratio"])))


def test_default_merge_has_no_cpu_fallback():
    pol = aoc_amd.eval_loop.AugmentedMemoryPolicy(1, [False])
    pol.start([torch.zeros(2, 2, 4)], torch.zeros(8, 8, dtype=torch.int64))
    with pytest.raises(aoc_amd._lib.AocHipError, match="no CPU fallback"):
        pol.update([torch.zeros(2, 2, 4)], [torch.zeros(2, 2, 2)])


def _desc(**kw):
    d = aoc_amd.ops._TtaDesc()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    d.n_aug, d.n_ch, d.H, d.W, d.mode, d.unc_ratio = 2, 3, 4, 4, 0, 0.5
    for a in range(2):
        d.h[a], d.w[a], d.flip[a], d.exist_bits[a], d.plane_stride[a], d.logits[a] = 2, 2, a, 7, 4, p
    d.label = p
    d._keep = buf
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def test_tta_merge_rejects_bad_arguments_without_a_gpu():
    L = aoc_amd._lib.lib()
    INVALID, UNSUPPORTED = -1, -4
    call = lambda d: L.aoc_tta_merge(ctypes.byref(d), None)
    assert L.aoc_tta_merge(None, None) == INVALID
    assert call(_desc(n_aug=0)) == INVALID
    assert call(_desc(n_aug=aoc_amd.ops.MAX_TTA_AUGS + 1)) == UNSUPPORTED
    assert call(_desc(n_ch=33)) == UNSUPPORTED
    assert call(_desc(n_ch=0)) == INVALID
    assert call(_desc(logits=(1, None))) == INVALID                      # a NULL plane
    for k in ("H", "W"):
        assert call(_desc(**{k: 0})) == INVALID
    for k in ("h", "w"):
        assert call(_desc(**{k: (1, 0)})) == INVALID
    assert call(_desc(plane_stride=(0, 3))) == INVALID                   # planes would overlap
    assert call(_desc(flip=(0, 2))) == INVALID
    assert call(_desc(mode=2)) == INVALID
    d = _desc()
    assert call(_desc(confident_flipped=d.label)) == INVALID             # mode 0 has no mirrored confident map
    assert call(_desc(label=None)) == INVALID                            # no output at all


def test_tta_desc_matches_the_header(tmp_path):
    D = aoc_amd.ops._TtaDesc
    fields = ["mode", "unc_ratio", "h", "flip", "exist_bits", "scale_h", "plane_stride", "logits", "join_label", "label", "confident_flipped", "entropy", "mean_probs"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%d", sizeof(aoc_tta_desc), AOC_MAX_TTA_AUGS);\n%s\nreturn 0;}\n'
                   % (os.path.join(ROOT, "include", "aoc_hip.h"), "\n".join('printf(" %%zu", offsetof(aoc_tta_desc, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(D), aoc_amd.ops.MAX_TTA_AUGS] + [getattr(D, f).offset for f in fields]
