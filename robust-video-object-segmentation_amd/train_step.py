"""The sequential training step on csrc/train_step.hip: the loop of train_manager_mm.py:241-284 around any model with ``AOCNet.forward``'s
signature, with the hand-over between two of its frames on the device,

    train_manager_mm.py:277      iou = pytorch_iou(all_pred.unsqueeze(1), curr_labels, obj_nums)          utils/metric.py:3-34
    train_manager_mm.py:281-282  running_losses[idx].update(loss.item() * seq_len); running_ious[idx].update(iou.item())     utils/meters.py
    train_manager_mm.py:258-259  prev_labels = all_pred.unsqueeze(1), which aocnet.py:134-135 shrinks again with interpolate(mode='nearest')

    frame_handover      aoc_frame_handover     one call per frame for the whole batch, two launches: the IoU, its per-sample values, the integer
                                                counts behind it, the prediction at the embedding's size, and the frame's IoU meter
    pytorch_iou         the drop-in for :277   [bs, 1, H, W] inputs take mode "reference", [bs, H, W] take "per_object" -- what the
                                                reference's own broadcasting makes of each form (include/aoc_hip.h has the two readings)
    DeviceMeters        aoc_meters_update / aoc_meters_reset: ``AverageMeter``s that live on the device; ``read()`` is the only call that waits
    sequential_step     :241-284 for one batch

The reference waits for the device twice per frame (the two ``.item()``s), ten times per step; nothing here does when ``obj_num`` is on the
host.  A CUDA ``obj_num`` tensor is read back once per call (``sequential_step``: once per step): that read is the only host wait.  The
ctypes wrappers live here, not in ``ops`` (whose public names are a tested table).  Not built: ``process_log`` / tensorboard, distributed
training, the AOCNet and CalibrationDecoding twins (they plug into ``sequential_step`` as ``model``).
"""
import ctypes

import torch

from . import _lib, ops, optim_train

MODES = {"reference": 0, "per_object": 1}                      # AOC_IOU_PER_COLUMN, AOC_IOU_PER_OBJECT
DTYPES = {torch.int32: 0, torch.int64: 1, torch.float32: 2}    # AOC_LABEL_I32, _I64, _F32
MAX_OBJECTS = 30                                                # AOC_MAX_OBJECTS
METERS_PER_CALL = 8                                             # AOC_METERS_PER_CALL
OUTPUTS = ("iou", "iou_per_sample", "counts", "prev_small")


class _Meter(ctypes.Structure):
    """aoc_meter"""
    _fields_ = [("val", ctypes.c_float), ("avg", ctypes.c_float), ("sum", ctypes.c_double), ("count", ctypes.c_int64)]


def _obj_list(obj_nums, bs):
    """obj_nums (a list, a CPU tensor or a CUDA tensor) -> a list of bs ints.  A CUDA tensor is read back here: the only host wait."""
    nums = [int(v) for v in (obj_nums.reshape(-1).tolist() if torch.is_tensor(obj_nums) else obj_nums)]
    if len(nums) != bs:
        raise ValueError(f"obj_nums names {len(nums)} samples, the maps have {bs}")
    return nums


def _label_map(what, t):
    if not torch.is_tensor(t) or t.dtype not in DTYPES or t.dim() != 3 or t.numel() == 0 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous non-empty [bs, H, W] tensor of int32, int64 or float32 labels, got "
                         f"{tuple(t.shape) if torch.is_tensor(t) else type(t)} {getattr(t, 'dtype', '')}")
    return t


class MeterSlot:
    """One meter of a DeviceMeters: what ``frame_handover(meter=...)`` takes."""

    def __init__(self, meters, index):
        self.meters, self.index = meters, index

    @property
    def ptr(self):
        return ctypes.c_void_p(self.meters.dev.data_ptr() + self.index * ctypes.sizeof(_Meter))


def frame_handover(pred, gt, obj_nums, small_size=None, mode="reference", epsilon=1e-6, want=(True, False, False, None), out=None, meter=None,
                   workspace=None):
    """aoc_frame_handover: pred, gt [bs, H, W] label maps (int32, int64 or float32 maps of integers, each its own), obj_nums [bs] (a list, a
    CPU tensor, or a CUDA tensor, which is read back once: the only host wait) -> (iou [1], iou_per_sample [bs], counts, prev_small
    [bs, h, w] int32); None where ``want`` is false and ``out`` (a dict of caller buffers by those names) has no buffer.  counts is
    [bs, W, 2] uint32-as-int32 (I, U per column) in mode "reference" and [bs, 30, 3] (I, #pred, #gt per object) in mode "per_object".
    ``small_size`` (h, w): the size of prev_small, wanted by default when it is given.  ``meter``: a MeterSlot updated with iou."""
    what = "frame_handover"
    if mode not in MODES:
        raise ValueError(f"{what}: mode {mode!r} (one of {sorted(MODES)})")
    pred = _label_map(what + ": pred", pred)
    bs, H, W = pred.shape
    want = list(want)
    if want[3] is None:
        want[3] = small_size is not None
    out = dict(out or {})
    need_counts = any(want[:3]) or any(out.get(k) is not None for k in OUTPUTS[:3]) or meter is not None
    if need_counts:
        gt = _label_map(what + ": gt", gt)
        if gt.shape != pred.shape:
            raise ValueError(f"{what}: gt {tuple(gt.shape)} beside pred {tuple(pred.shape)}")
        nums = (ctypes.c_int32 * bs)(*_obj_list(obj_nums, bs))
    else:
        gt, nums = None, None
    if (want[3] or out.get("prev_small") is not None) and small_size is None:
        raise ValueError(f"{what}: prev_small needs small_size")
    h, w = (int(small_size[0]), int(small_size[1])) if small_size is not None else (0, 0)
    shapes = ((1,), (bs,), (bs, W, 2) if MODES[mode] == 0 else (bs, MAX_OBJECTS, 3), (bs, h, w))
    ops._need_gpu(pred, gt, workspace, *out.values())
    iou, per_sample, counts, prev_small = ops._wanted(what, OUTPUTS, shapes, want, out, pred, (torch.float32, torch.float32, torch.int32, torch.int32))
    L = _lib.lib()
    ws = None
    if need_counts:
        ws = workspace if workspace is not None else ops._ws(L.aoc_frame_handover_workspace_bytes(bs, H, W), pred.device)
    _lib.check(L.aoc_frame_handover(ops._p(pred), DTYPES[pred.dtype], ops._p(gt), DTYPES[gt.dtype] if gt is not None else 0, bs, H, W, nums,
                                    float(epsilon), MODES[mode], h, w, ops._p(iou), ops._p(per_sample), ops._p(counts), ops._p(prev_small),
                                    meter.ptr if meter is not None else None, ops._p(ws), ws.numel() * ws.element_size() if ws is not None else 0,
                                    ops._stream()), "aoc_frame_handover")
    return iou, per_sample, counts, prev_small


def pytorch_iou(pred, target, obj_num, epsilon=1e-6):
    """The drop-in for train_manager_mm.py:277 (utils/metric.py:3-34) -> a 0-d device tensor.  [bs, 1, H, W] inputs, the form the trainer
    calls it with, take mode "reference" (per column); [bs, H, W] inputs, the documented form, take "per_object": exactly what the
    reference's broadcasting makes of each.  Other ranks raise."""
    if not torch.is_tensor(pred) or not torch.is_tensor(target) or pred.dim() != target.dim():
        raise ValueError("pytorch_iou: pred and target must be tensors of one rank")
    if pred.dim() == 4 and pred.shape[1] == 1 and target.shape[1] == 1:
        mode, pred, target = "reference", pred[:, 0], target[:, 0]
    elif pred.dim() == 3:
        mode = "per_object"
    else:
        raise ValueError(f"pytorch_iou: [bs, 1, H, W] or [bs, H, W] inputs, got {tuple(pred.shape)} and {tuple(target.shape)}")
    return frame_handover(pred.contiguous(), target.contiguous(), obj_num, None, mode, epsilon)[0].view(())


class MeterReading:
    """What ``DeviceMeters.read()`` returns per meter: ``AverageMeter``'s four attributes."""

    def __init__(self, val, avg, sum, count):
        self.val, self.avg, self.sum, self.count = val, avg, sum, count

    def __repr__(self):
        return f"MeterReading(val={self.val!r}, avg={self.avg!r}, sum={self.sum!r}, count={self.count!r})"


class DeviceMeters:
    """``utils/meters.py`` AverageMeters that live on the device.  ``update`` and ``reset`` are enqueued on the current stream and wait for
    nothing; ``read()`` is the only call that waits.  A meter is named by its name or its index; at most 64 per object."""

    def __init__(self, names, device=None):
        self.names = list(names)
        if not 1 <= len(self.names) <= 64 or len(set(self.names)) != len(self.names):
            raise ValueError(f"DeviceMeters: 1 to 64 distinct names, got {len(self.names)}")
        self.index = {name: i for i, name in enumerate(self.names)}
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.dev = torch.zeros(len(self.names) * ctypes.sizeof(_Meter), dtype=torch.uint8, device=device)       # zeroed records: fresh meters
        ops._need_gpu(self.dev)

    @classmethod
    def for_sequence(cls, seq_len, device=None):
        """the meters ``sequential_step`` updates: loss_0 .. loss_{seq_len-1}, iou_0 .. (running_losses / running_ious of the trainer)"""
        return cls([f"loss_{i}" for i in range(seq_len)] + [f"iou_{i}" for i in range(seq_len)], device)

    def _idx(self, key):
        i = self.index[key] if isinstance(key, str) else int(key)
        if not 0 <= i < len(self.names):
            raise IndexError(f"DeviceMeters: meter {key!r} of {len(self.names)}")
        return i

    def slot(self, key):
        return MeterSlot(self, self._idx(key))

    def update(self, key, value, scale=1.0, n=1):
        """meter.update(value.item() * scale, n) without the ``.item()``: ``value`` is a float32 device word.  ``key`` / ``value`` / ``scale``
        / ``n`` may be lists of up to METERS_PER_CALL entries (distinct meters): still one launch."""
        many = isinstance(key, (list, tuple))
        keys = list(key) if many else [key]
        k = len(keys)
        values = list(value) if many else [value]
        scales = list(scale) if isinstance(scale, (list, tuple)) else [scale] * k
        ns = list(n) if isinstance(n, (list, tuple)) else [n] * k
        if not (len(values) == len(scales) == len(ns) == k) or not 1 <= k <= METERS_PER_CALL:
            raise ValueError(f"DeviceMeters.update: {k} meters, {len(values)} values, {len(scales)} scales, {len(ns)} counts (1 to {METERS_PER_CALL} of each)")
        words = [optim_train._word("DeviceMeters.update: value", v.detach() if torch.is_tensor(v) else v) for v in values]   # bound until the launch
        ops._need_gpu(*words)
        idx = (ctypes.c_int32 * k)(*[self._idx(key) for key in keys])
        ptrs = (ctypes.c_void_p * k)(*[ops._addr(v) for v in words])
        sc = (ctypes.c_double * k)(*[float(s) for s in scales])
        nn = (ctypes.c_int64 * k)(*[int(v) for v in ns])
        _lib.check(_lib.lib().aoc_meters_update(ops._p(self.dev), len(self.names), idx, ptrs, sc, nn, k, ops._stream()), "aoc_meters_update")

    def reset(self, keys=None):
        """``AverageMeter.reset()`` of the named meters (None: all of them), one launch"""
        keys = range(len(self.names)) if keys is None else (keys if isinstance(keys, (list, tuple, range)) else [keys])
        mask = 0
        for key in keys:
            mask |= 1 << self._idx(key)
        _lib.check(_lib.lib().aoc_meters_reset(ops._p(self.dev), len(self.names), mask, ops._stream()), "aoc_meters_reset")

    def read(self):
        """-> {name: MeterReading}.  Copies the records to the host: waits for the stream."""
        raw = self.dev.cpu().numpy().tobytes()
        recs = (_Meter * len(self.names)).from_buffer_copy(raw)
        return {name: MeterReading(r.val, r.avg, r.sum, r.count) for name, r in zip(self.names, recs)}


def _zero_grads(optimizer):
    """:246.  An optim_train.SGD that made the last update of these gradients through ``sequential_step`` zeroed them in that pass
    (``step(zero_grads=True)``): nothing to do.  Otherwise its one-launch zeroing, or torch's ``zero_grad()``."""
    if isinstance(optimizer, optim_train.SGD):
        if not getattr(optimizer, "_grads_zeroed_by_step", False):
            optimizer.zero_grad(set_to_none=False)
        optimizer._grads_zeroed_by_step = False
    else:
        optimizer.zero_grad()


def _update(optimizer, clip_grad_norm):
    """:283-284"""
    own = isinstance(optimizer, optim_train.SGD)
    if own and optimizer.clip_grad_norm is not None:
        if clip_grad_norm is not None and float(clip_grad_norm) != optimizer.clip_grad_norm:
            raise ValueError(f"sequential_step: clip_grad_norm {clip_grad_norm} beside the optimiser's own {optimizer.clip_grad_norm}")
    elif clip_grad_norm is not None:
        optim_train.clip_grad_norm_([p for g in optimizer.param_groups for p in g["params"]], clip_grad_norm)
    if own:
        optimizer.step(zero_grads=True)
        optimizer._grads_zeroed_by_step = True
    else:
        optimizer.step()


def sequential_step(model, sample, optimizer, *, step, seq_len, start_seq_training_steps, meters=None, iou_mode="reference", scaled_labels=None,
                    clip_grad_norm=None, handover=frame_handover, memory_placeholder=None):
    """train_manager_mm.py:241-284 for one batch.  ``sample`` is the loader's dict (``ref_img``, ``prev_img``, ``curr_img`` [seq_len],
    ``ref_label``, ``prev_label``, ``curr_label`` [seq_len], ``meta['obj_num']``) with its tensors on the model's device already;
    ``model(inputs, memory_prev_list, ref_labels, prev_labels, curr_labels, gt_ids=, step=, tf_board=False)`` returns ``(loss [bs], all_pred
    [bs, H, W], boards, memory_cur_list)``.  Labels: the ground truth up to and including ``start_seq_training_steps``, the previous
    frame's prediction after it (:254-263).  Per frame ``(loss.mean() / seq_len).backward()``, the loss meter ``loss_<idx>`` updated from
    the device scalar with ``scale=seq_len`` (:281) and the IoU meter ``iou_<idx>`` by the hand-over (``meters``: a
    ``DeviceMeters.for_sequence(seq_len)`` or None).  Then the update: ``optim_train.SGD.step()`` when it carries its own clip, else
    ``optim_train.clip_grad_norm_`` (with ``clip_grad_norm``) and ``optimizer.step()``.  The gradients are zero when the loop begins (:246);
    an ``optim_train.SGD`` zeroes them in its update pass, so only its first step here costs a zeroing launch -- gradients accumulated
    between two calls by anyone else are the caller's to zero.  With ``scaled_labels=(h, w)`` the model also gets
    ``scale_previous_frame_label=`` [bs, 1, h, w] int32, the previous mask as aocnet.py:134-135 would shrink it.  ``handover``:
    ``frame_handover`` or a function of its signature; ``memory_placeholder``: what the first frame finds in every slot of
    ``memory_prev_list`` (the trainer's ``[None] * cfg.BLOCK_NUM``).  Nothing here waits for the device when ``obj_num`` is on the host.
    -> (all_pred of the last frame, the list of the frames' boards)"""
    ref_imgs, prev_imgs = sample["ref_img"], sample["prev_img"]
    ref_labels, prev_labels = sample["ref_label"], sample["prev_label"]
    obj_nums = sample["meta"]["obj_num"]
    bs = prev_labels.shape[0]
    nums = _obj_list(obj_nums, bs)                              # once per step; a CUDA tensor is read back here
    all_boards = []
    curr_imgs, curr_labels = prev_imgs, prev_labels
    all_pred = prev_labels.squeeze(1)
    _zero_grads(optimizer)
    memory_prev_list = [memory_placeholder] * bs               # :247-251: the trainer's PlaceHolder ([None] * BLOCK_NUM) per sample
    small = None                                                # the mask of the next frame's prev_labels at (h, w), when a hand-over made it
    for idx in range(seq_len):
        prev_imgs = curr_imgs
        curr_imgs = sample["curr_img"][idx]
        inputs = torch.cat((ref_imgs, prev_imgs, curr_imgs), 0)
        if step > start_seq_training_steps:
            prev_labels = all_pred.unsqueeze(1)                 # the previous prediction instead of the ground-truth mask
        else:
            prev_labels, small = curr_labels, None
        curr_labels = sample["curr_label"][idx]
        extra = {}
        if scaled_labels is not None:
            if small is None:
                small = handover(prev_labels[:, 0].contiguous(), None, nums, small_size=scaled_labels, want=(False, False, False, True))[3]
            extra["scale_previous_frame_label"] = small.unsqueeze(1)
        loss, all_pred, boards, memory_cur_list = model(inputs, memory_prev_list, ref_labels, prev_labels, curr_labels, gt_ids=obj_nums, step=step,
                                                        tf_board=False, **extra)
        memory_prev_list = memory_cur_list
        small = None
        if meters is not None or scaled_labels is not None:      # else the hand-over has no taker
            small = handover(all_pred.detach().contiguous(), curr_labels[:, 0].contiguous(), nums, small_size=scaled_labels, mode=iou_mode,
                             want=(False, False, False, scaled_labels is not None),
                             meter=meters.slot(f"iou_{idx}") if meters is not None else None)[3]
        loss = torch.mean(loss) / seq_len
        loss.backward()
        all_boards.append(boards)
        if meters is not None:
            meters.update(f"loss_{idx}", loss.detach().reshape(1), scale=seq_len)
    _update(optimizer, clip_grad_norm)
    return all_pred, all_boards
