"""Developer tool (GPU box): the hand-over between two frames of a training step, in two arms that alternate call by call in one process:
  (ref)  the reference's lines in plain PyTorch on the device (train_manager_mm.py:277-282, aocnet.py:134-135): the 4-D ``pytorch_iou`` as
         utils/metric.py computes it (restated here: the broadcast comparison, the sums over (1, 2), the mean), ``loss.item()`` and
         ``iou.item()`` into host meters, and the nearest resize of the prediction;
  (hip)  one ``train_step.frame_handover`` (IoU into its device meter, prev_small) and one ``DeviceMeters.update`` for the loss.
At bs = 1 and bs = 8, 465 x 465 -> 117 x 117, five objects.  Per arm: WARMUP calls, then RUNS calls each bracketed by two device events
(device: the call as the stream sees it, host gaps included) and, separately, the host time until the call returns after a
synchronisation (for the ref arm that includes its two waits).  The condition: the hip arm's median is at or below the ref arm's in
every row, device and host (exit status 1 otherwise).

    python tools/bench_train_handover.py [out.txt]        # default: profiles/train_handover_ab.txt
"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import aoc_amd  # noqa: E402
from aoc_amd import train_step as ts  # noqa: E402

WARMUP, RUNS = 5, 20
H = W = 465
SMALL = (117, 117)
N_OBJ, SEQ_LEN = 5, 5


class HostMeter:
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def iou_4d(pred, target, obj_num, epsilon=1e-6):
    """what the trainer's call computes: [bs, 1, H, W] inputs, ids viewed [n, 1, 1], sums over dims (1, 2)"""
    vals = []
    for idx in range(obj_num.size(0)):
        ids = torch.arange(1, int(obj_num[idx]) + 1, device=pred.device).int().view(-1, 1, 1)
        if ids.size(0) == 0:
            continue
        p, t = (pred[idx].unsqueeze(0) == ids).float(), (target[idx].unsqueeze(0) == ids).float()
        inter, union = (p * t).sum((1, 2)), ((p + t) > 0).float().sum((1, 2))
        vals.append(((inter + epsilon) / (union + epsilon)).mean())
    return torch.stack(vals).mean() if vals else torch.ones(1, device=pred.device)


def make(bs, gen):
    gt = torch.randint(0, N_OBJ + 1, (bs, 1, H // 15, W // 15), device="cuda", generator=gen).float()
    gt = F.interpolate(gt, size=(H, W), mode="nearest")                         # blobs, as masks have
    flip = torch.rand(bs, 1, H, W, device="cuda", generator=gen) < 0.1
    pred = torch.where(flip, torch.randint(0, N_OBJ + 1, (bs, 1, H, W), device="cuda", generator=gen).float(), gt).long()[:, 0].contiguous()
    return pred, gt.contiguous(), torch.rand(1, device="cuda", generator=gen)


def bench(bs, gen, lines):
    pred, gt, loss = make(bs, gen)
    nums_host, nums_dev = [N_OBJ] * bs, torch.full((bs,), N_OBJ, device="cuda")
    host = {"loss": HostMeter(), "iou": HostMeter()}
    dev = ts.DeviceMeters(["loss", "iou"])
    gt3 = gt[:, 0].contiguous()
    kept = {}

    def ref():
        iou = iou_4d(pred.unsqueeze(1), gt, nums_dev)
        host["loss"].update(loss.item() * SEQ_LEN)
        host["iou"].update(iou.item())
        kept["ref"] = F.interpolate(pred.unsqueeze(1).float(), size=SMALL, mode="nearest").int()

    def hip():
        kept["hip"] = ts.frame_handover(pred, gt3, nums_host, small_size=SMALL, want=(False, False, False, True), meter=dev.slot("iou"))[3]
        dev.update("loss", loss, scale=SEQ_LEN)

    arms = {"ref": ref, "hip": hip}
    for _ in range(WARMUP):
        for call in arms.values():
            call()
    torch.cuda.synchronize()
    same_small = torch.equal(kept["ref"][:, 0], kept["hip"])
    got = dev.read()
    drift = abs(got["iou"].avg - host["iou"].avg)
    ms, host_ms = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(RUNS):
        for k, call in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
        for k, call in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            host_ms[k].append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
    lines.append(f"bs = {bs}, {H} x {W} -> {SMALL[0]} x {SMALL[1]}, {N_OBJ} objects ({2 * bs * H * W * 6 / 1e6:.1f} MB of labels: int64 prediction, float ground truth); "
                 f"prev_small equal: {same_small}; |iou avg hip - ref| {drift:.1e}")
    ok = same_small and drift < 1e-5
    for what, t in (("device", ms), ("host until the call returns", host_ms)):
        r, h = float(np.median(t["ref"])), float(np.median(t["hip"]))
        lines.append(f"  {what:28s} (ref) {r:7.3f} ms [{min(t['ref']):.3f}, {max(t['ref']):.3f}]   (hip) {h:7.3f} ms [{min(t['hip']):.3f}, {max(t['hip']):.3f}]   "
                     f"hip <= ref: {'yes' if h <= r else 'NO'} ({r / h:.1f}x)")
        ok = ok and h <= r
    return ok


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_handover_ab.txt")
    aoc_amd._lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"# The frame hand-over of a training step: the reference's lines in plain PyTorch (4-D pytorch_iou, two .item()s, nearest resize, host meters) "
             f"against frame_handover + one meter update (three launches); arms alternating in one process, median [min, max] of {RUNS} after {WARMUP} "
             f"warm-up calls; torch {torch.__version__}", f"# device: {torch.cuda.get_device_name(0)}"]
    failed = []
    with torch.no_grad():
        for bs in (1, 8):
            if not bench(bs, gen, lines):
                failed.append(f"bs = {bs}: a row misses the condition")
    lines += ["# FAILED: " + f for f in failed]
    print("\n".join(lines), flush=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
