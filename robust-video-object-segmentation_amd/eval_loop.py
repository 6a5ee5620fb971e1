"""Eval-loop memory policy: the immediate caller of the matching path.

Counterpart of the per-sequence state machine in ``networks/engine/eval_manager_mm.py:196-361``.  ``MemoryPolicy`` is the single-scale,
no-flip configuration the reference evaluates with by default (configs/resnet101_aocnet.py: TEST_MULTISCALE=[1.], TEST_FLIP=False);
``AugmentedMemoryPolicy`` is the same loop for the sample LIST of ``--flip`` / ``--ms`` (one pool, previous frame and memory per
augmentation, one merged decision per frame: ``aoc_tta_merge``), ``multi_restrict_sizes`` the size arithmetic of that list.  One augmentation:

* frame 0 seeds the reference pool with the ground-truth mask (:274-282);
* every later frame: channels of labels that never appeared in a ground-truth map are zeroed (:253-265), the label map is
  the arg-max (:316-318), a ground-truth map that introduces new objects overrides it where it is non-zero (:319-326);
* the *confident* map that the matching path sees replaces pixels whose Shannon entropy exceeds ``unc_ratio`` by the label
  125, which matches no object (:305-306, :339-346, :357-361; shannon_entropy.py:10-13);
* the frame joins the pool when it carries ground truth (:296-297) or every ``mem_every`` frames (:309-312);
* the previous-frame embedding / mask always advance (:314, :350-353).

All per-pixel work runs in ``libaoc_hip.so`` (``aoc_confident_labels``, ``aoc_label_onehot_nearest``); this class only keeps
the lists.  ``reference_pool(h, w)`` hands the pool over in the layout ``hotpath.proto_mask_features`` takes.
"""
import torch

from . import ops

UNCERTAIN_LABEL = 125


class MemoryPolicy:
    def __init__(self, mem_every=5, unc_ratio=1.0, max_obj=None):
        self.mem_every = int(mem_every)
        self.unc_ratio = float(unc_ratio)
        self.max_obj = max_obj
        self.reset()

    def reset(self):
        """eval_manager_mm.py:376-382: all per-sequence state is dropped between sequences."""
        self.ref_embeddings, self.ref_masks, self.ref_mask_confident = [], [], []
        self.prev_embedding = self.prev_mask = None
        self.label_all = set()
        self.frame_idx = 0

    def _see(self, gt_label):
        # :267-272 np.unique of the ground truth (a host read-back in the reference as well; only on frames that carry GT)
        self.label_all.update(int(v) for v in torch.unique(gt_label).tolist())

    def exist_bits(self):
        bits = 0
        for l in self.label_all:
            if 0 <= l < 32:
                bits |= 1 << l
        return bits

    def start(self, embedding, gt_label):
        """Frame 0 (:274-282).  embedding [h, w, C]; gt_label int [H, W]."""
        assert self.frame_idx == 0
        gt_label = gt_label.to(torch.int32).contiguous()
        self._see(gt_label)
        self.ref_embeddings.append(embedding)
        self.ref_masks.append(gt_label)
        self.ref_mask_confident.append(gt_label)
        self.prev_embedding, self.prev_mask = embedding, gt_label
        self.frame_idx = 1

    def update(self, embedding, probs, gt_label=None):
        """One frame after the first.  probs [n_ch, H, W] class probabilities (soft-max of the decoder logits);
        gt_label int [H, W] when the frame carries ground truth (new objects, :288-289).
        Returns (label [H, W] int32, confident [H, W] int32, entropy [H, W] float32)."""
        assert self.frame_idx > 0, "call start() with the first frame"
        n_ch, H, W = probs.shape
        join = None
        if gt_label is not None:
            join = gt_label.to(torch.int32).contiguous()
        # the reference updates label_all_list from the current GT only AFTER zeroing the channels (:253-272)
        label, confident, entropy = ops.confident_labels(probs.reshape(n_ch, H * W), self.exist_bits(), join, self.unc_ratio)
        label, confident, entropy = label.view(H, W), confident.view(H, W), entropy.view(H, W)
        if gt_label is not None:
            self._see(join)
            self.ref_embeddings.append(embedding)                                  # :296-297
            self.ref_masks.append(label)                                           # :333
            self.ref_mask_confident.append(confident)                              # :339-348
        elif self.mem_every > -1 and self.frame_idx % self.mem_every == 0:
            self.ref_embeddings.append(embedding)                                  # :309-312
            self.ref_masks.append(label)
            self.ref_mask_confident.append(confident)                              # :357-361
        self.prev_embedding, self.prev_mask = embedding, label                     # :314, :350-353
        self.frame_idx += 1
        return label, confident, entropy

    def reference_pool(self, h, w, n_obj):
        """The pool as proto_mask_features takes it: (ref_emb [R, h, w, C], ref_labels [R, h, w, O] one-hot float of the
        CONFIDENT maps, prev_emb, prev_labels [h, w, O])  (aocnet.py:128-156)."""
        ref_emb = torch.stack(self.ref_embeddings, dim=0)
        ref_lab = torch.stack([ops.label_onehot_nearest(m, h, w, n_obj) for m in self.ref_mask_confident], dim=0)
        return ref_emb, ref_lab, self.prev_embedding, ops.label_onehot_nearest(self.prev_mask, h, w, n_obj)


class _Lane:
    """One augmentation of an AugmentedMemoryPolicy seen as a MemoryPolicy (what a single-augmentation caller reads: the lists, the previous
    frame, frame_idx)."""

    def __init__(self, policy, a):
        self._p, self._a = policy, a

    ref_embeddings = property(lambda self: self._p.ref_embeddings[self._a])
    ref_mask_confident = property(lambda self: self._p.ref_mask_confident[self._a])
    prev_embedding = property(lambda self: self._p.prev_embedding[self._a])
    prev_mask = property(lambda self: self._p.prev_mask[self._a])
    frame_idx = property(lambda self: self._p.frame_idx)

    def reference_pool(self, h, w, n_obj):
        return self._p.reference_pool(self._a, h, w, n_obj)


class AugmentedMemoryPolicy:
    """The state machine of eval_manager_mm.py:196-361 for a list of A augmented samples per frame (--flip / --ms): every augmentation keeps its
    own reference pool, previous frame and previous mask; the per-augmentation maps are flipped back, averaged and decided ONCE per frame
    (``merge``, by default ops.tta_merge = aoc_tta_merge: one launch), and the decision is handed back to every augmentation.

    mode "reference" reproduces what the reference hands its model (tests/golden/eval_loop_tta_*.npz, recorded from its own loop):
      * previous mask of augmentation a = the label map, mirrored for a flipped a (:351-354);
      * a frame with ground truth: an un-flipped a gets the confident map, a flipped a the mirrored LABEL without any 125 (:332-349);
      * a ``mem_every`` frame: EVERY a, flipped or not, gets the same UN-mirrored confident map (:356-361);
      * the entropy behind the confident map is that of the LAST augmentation's own, not flipped-back probabilities (:306, :339), and on a
        ground-truth frame the labels it introduces count as seen from the second augmentation on (:268-272 run inside the loop).
      ``ref_masks`` (the partial-mean ``current_label_0`` of :300-311) is never handed to the model and is not kept.
    mode "consistent" is this project's (non-parity, like hotpath.IncrementalProxyBank): the entropy of the MERGED probabilities, and a flipped
    augmentation always gets the mirrored confident map, so that a flipped lane's masks are the mirror of the un-flipped lane's on every frame.

    ``merge`` is a seam for a test's stand-in with the signature and result keys of ops.tta_merge; the package ships no CPU merge."""

    def __init__(self, n_aug, flips, mem_every=5, unc_ratio=1.0, mode="reference", merge=None):
        self.n_aug = int(n_aug)
        self.flips = [bool(f) for f in flips]
        if self.n_aug < 1 or len(self.flips) != self.n_aug:
            raise ValueError("AugmentedMemoryPolicy: one flip flag per augmentation")
        if mode not in ops.TTA_MODES:
            raise ValueError(f"AugmentedMemoryPolicy: mode {mode!r} is not one of {sorted(ops.TTA_MODES)}")
        self.mem_every, self.unc_ratio, self.mode = int(mem_every), float(unc_ratio), mode
        self.merge = merge if merge is not None else ops.tta_merge
        self.reset()

    def reset(self):
        A = self.n_aug
        self.ref_embeddings, self.ref_mask_confident = [[] for _ in range(A)], [[] for _ in range(A)]
        self.prev_embedding, self.prev_mask = [None] * A, [None] * A
        self.label_all = set()
        self.frame_idx = 0
        self.size = None

    _see = MemoryPolicy._see
    exist_bits = MemoryPolicy.exist_bits

    def lane(self, a):
        return _Lane(self, a)

    def start(self, embeddings, gt_label):
        """Frame 0 (:274-282).  embeddings: one [h_a, w_a, C] per augmentation; gt_label int [H, W], un-mirrored (every scale keeps the ground
        truth at image size, custom_transforms.py:441-443; a flipped sample carries its mirror, :459)."""
        assert self.frame_idx == 0 and len(embeddings) == self.n_aug
        gt_label = gt_label.to(torch.int32).contiguous()
        self._see(gt_label)
        self.size = tuple(gt_label.shape)
        mirrored = gt_label.flip(1).contiguous() if any(self.flips) else None
        for a in range(self.n_aug):
            g = mirrored if self.flips[a] else gt_label
            self.ref_embeddings[a].append(embeddings[a])
            self.ref_mask_confident[a].append(g)
            self.prev_embedding[a], self.prev_mask[a] = embeddings[a], g
        self.frame_idx = 1

    def update(self, embeddings, logits_list, gt_label=None):
        """One frame after the first.  logits_list: the decoder's logits [n_ch, h_a, w_a] per augmentation, a flipped one's in the mirrored
        orientation; gt_label int [H, W] (un-mirrored) when the frame carries ground truth.  Returns (label, confident, entropy) [H, W]."""
        assert self.frame_idx > 0, "call start() with the first frame"
        assert len(embeddings) == self.n_aug and len(logits_list) == self.n_aug
        A, H, W = self.n_aug, *self.size
        reference = self.mode == "reference"
        join = None
        bits = self.exist_bits()
        if gt_label is not None:
            join = gt_label.to(torch.int32).contiguous()
            if reference and A > 1:
                self._see(join)                                       # :268-272: inside the augmentation loop, after augmentation 0's zeroing
                bits = [bits] + [self.exist_bits()] * (A - 1)
        out = self.merge(logits_list, self.flips, H, W, bits, join, self.unc_ratio, self.mode)
        label, confident, label_flipped = out["label"], out["confident"], out["label_flipped"]
        mirrored_confident = None if reference else out["confident_flipped"]
        joins = gt_label is not None or (self.mem_every > -1 and self.frame_idx % self.mem_every == 0)
        if gt_label is not None:
            self._see(join)
        for a in range(A):
            if joins:
                self.ref_embeddings[a].append(embeddings[a])                                # :296-297, :309-312
                if not self.flips[a]:
                    mask = confident                                                        # :336-349, :357-361
                elif not reference:
                    mask = mirrored_confident
                else:
                    mask = label_flipped if gt_label is not None else confident             # :333-335 (no 125) | :357-361 (not mirrored)
                self.ref_mask_confident[a].append(mask)
            self.prev_embedding[a] = embeddings[a]                                          # :314
            self.prev_mask[a] = label_flipped if self.flips[a] else label                   # :351-354
        self.frame_idx += 1
        return label, confident, out["entropy"]

    def reference_pool(self, a, h, w, n_obj):
        """Augmentation a's pool as proto_mask_features takes it (MemoryPolicy.reference_pool)."""
        ref_emb = torch.stack(self.ref_embeddings[a], dim=0)
        ref_lab = torch.stack([ops.label_onehot_nearest(m, h, w, n_obj) for m in self.ref_mask_confident[a]], dim=0)
        return ref_emb, ref_lab, self.prev_embedding[a], ops.label_onehot_nearest(self.prev_mask[a], h, w, n_obj)


def map_size(n):
    """Image edge -> edge of the stride-4 embedding map (resnet.py:109-115 on a 16 k + 1 edge)."""
    return (int(n) - 1) // 4 + 1


def multi_restrict_sizes(H, W, min_size, max_size, flip, multi_scale):
    """The size arithmetic of MultiRestrictSize.__call__ (dataloaders/custom_transforms.py:387-462): [(new_h, new_w, flip), ...] in the order
    of the sample list -- per scale the resized sample (edges rounded to 16 k + 1), directly followed by its flipped twin with ``flip``."""
    import numpy as np
    if (min_size is None) == (max_size is None):
        raise ValueError("multi_restrict_sizes: exactly one of min_size / max_size")
    out = []
    for scale in multi_scale:
        sc = None
        if min_size is not None:
            short_edge = W if H > W else H
            if short_edge > min_size:
                sc = float(min_size) / short_edge
        else:
            long_edge = H if H > W else W
            if long_edge > max_size:
                sc = float(max_size) / long_edge
        new_h, new_w = (H, W) if sc is None else (sc * H, sc * W)
        new_h, new_w = int(new_h * scale), int(new_w * scale)
        if (new_h - 1) % 16 != 0:
            new_h = int(np.around((new_h - 1) / 16.) * 16 + 1)
        if (new_w - 1) % 16 != 0:
            new_w = int(np.around((new_w - 1) / 16.) * 16 + 1)
        out.append((new_h, new_w, False))
        if flip:
            out.append((new_h, new_w, True))
    return out
