#!/usr/bin/env python3
"""Golden values for the frame hand-over of a training step (tests/test_train_step_host.py), recorded by running the reference's OWN
``utils/metric.py`` and ``utils/meters.py`` UNMODIFIED (they import only ``torch``), loaded by path, and torch's own nearest resize.  None of
the reference's text is stored, and nothing is written into its tree.  The inputs are the ones tests/train_step_cases.py makes.

    train_handover_iou.npz       per case of FIXTURE_GEOMETRIES: pred, gt (int16), obj_num, and what ``pytorch_iou`` returns for the form the
                                 trainer calls it with (train_manager_mm.py:277: pred int64 [bs, 1, H, W], target float [bs, 1, H, W]) and for
                                 the documented form ([bs, H, W]), each as a float32
    train_handover_nearest.npz   per case of NEAREST_GEOMETRIES: pred (int16) and ``F.interpolate(pred.float(), size, mode='nearest').int()``
                                 (aocnet.py:134-135)
    train_handover_meters.npz    METER_SEQUENCE through ``AverageMeter``: after every entry val, avg, sum as float64 and count, fed as the
                                 trainer feeds it (``.item()`` of a float32 tensor times the scale, train_manager_mm.py:281)

    python tests/golden/make_golden_train_handover.py <the reference's complete_project/AOCNet directory>
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True                            # never write into the reference tree

import train_step_cases as tc  # noqa: E402


def _load(ref_root, name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref_root, "utils", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                            # the reference's file, unmodified
    return mod


def main(ref_root):
    metric, meters = _load(ref_root, "metric"), _load(ref_root, "meters")
    out = {}
    for k, (bs, H, W, nums) in enumerate(tc.FIXTURE_GEOMETRIES):
        pred, gt = tc.make_maps(bs, H, W, nums, seed=k)
        p, g, n = torch.from_numpy(pred), torch.from_numpy(gt).float(), torch.tensor(nums)
        out[f"pred_{k}"], out[f"gt_{k}"], out[f"nums_{k}"] = pred.astype(np.int16), gt.astype(np.int16), np.asarray(nums, np.int32)
        out[f"iou4d_{k}"] = metric.pytorch_iou(p.unsqueeze(1), g.unsqueeze(1), n).reshape(()).numpy().astype(np.float32)
        out[f"iou3d_{k}"] = metric.pytorch_iou(p, g, n).reshape(()).numpy().astype(np.float32)
    _save("train_handover_iou.npz", out)
    out = {}
    for k, (bs, H, W, h, w) in enumerate(tc.NEAREST_GEOMETRIES):
        pred = tc.make_maps(bs, H, W, [5] * bs, seed=100 + k, planted=False)[0]
        out[f"pred_{k}"] = pred.astype(np.int16)
        out[f"small_{k}"] = F.interpolate(torch.from_numpy(pred).unsqueeze(1).float(), size=(h, w), mode="nearest").int()[:, 0].numpy()
    _save("train_handover_nearest.npz", out)
    m, rows = meters.AverageMeter(), []
    for entry in tc.METER_SEQUENCE:
        if entry is None:
            m.reset()
        else:
            value, scale, n = entry
            m.update(torch.tensor(value, dtype=torch.float32).item() * scale, n)
        rows.append((float(m.val), float(m.avg), float(m.sum), float(m.count)))
    _save("train_handover_meters.npz", {"state": np.asarray(rows, np.float64)})


def _save(name, arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
