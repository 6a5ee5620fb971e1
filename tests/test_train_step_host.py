"""The host half of the frame hand-over (aoc_amd.train_step, csrc/train_step.hip; tests/train_step_cases.py holds the restatement, the
reference and the bound; tests/test_gpu_train_step.py is the device half).

1. the float32 restatement and the float64 reference against what the reference's own pytorch_iou returned for both call forms
   (tests/golden/train_handover_iou.npz), each slipped twin outside the bound on every fixture;
2. the nearest maps against F.interpolate(...).int() as recorded and as this torch computes it; rounding in place of floor differs on every fixture;
3. the host meter against AverageMeter in double, bit for bit; count += 1 in place of n differs;
4. sequential_step on CPU tensors with the restatement as its hand-over and a recording model: labels, memory lists, meters, gradients;
5. the C ABI's rejections that need no device.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import train_step_cases as tc
from aoc_amd import _lib
from aoc_amd import train_step as ts

f32 = np.float32


@pytest.fixture(scope="module")
def iou_fix(golden):
    z = golden("train_handover_iou")
    return [(z[f"pred_{k}"].astype(np.int64), z[f"gt_{k}"].astype(np.int64), [int(n) for n in z[f"nums_{k}"]], float(z[f"iou4d_{k}"]), float(z[f"iou3d_{k}"]))
            for k in range(len(tc.FIXTURE_GEOMETRIES))]


# ------------------------------------------------------------------------------------------ 1
def test_fixture_inputs_are_the_cases(iou_fix):
    for k, ((bs, H, W, nums), (pred, gt, got_nums, _, _)) in enumerate(zip(tc.FIXTURE_GEOMETRIES, iou_fix)):
        want_pred, want_gt = tc.make_maps(bs, H, W, nums, seed=k)
        assert got_nums == nums and np.array_equal(pred, want_pred) and np.array_equal(gt, want_gt)
        assert bs <= 3 and H <= 33 and W <= 31


@pytest.mark.parametrize("mode", tc.MODES)
def test_restatement_and_reference_inside_the_bound_of_the_reference_code(iou_fix, mode):
    for k, (pred, gt, nums, iou4d, iou3d) in enumerate(iou_fix):
        ref = iou4d if mode == "reference" else iou3d
        want, tol, per, per_tol = tc.handover64(pred, gt, nums, mode)
        got, got_per, _ = tc.handover32(pred, gt, nums, mode)
        print(f"case {k} {mode}: reference code {ref!r}, float64 {want!r}, bound {tol:.3e}, restatement off by {abs(float(got) - want):.3e}, "
              f"reference code off by {abs(ref - want):.3e}")
        assert 0.0 < tol < 4e-6, "the bound is a few float32 roundings of a value near 1"
        assert abs(ref - want) <= tol, f"case {k}: the reference's own value leaves the bound of the float64 reference"
        assert abs(float(got) - want) <= tol, f"case {k}: the float32 restatement leaves the bound"
        assert (np.abs(got_per.astype(np.float64) - per) <= per_tol).all()
        for dt in (np.int32, np.float32):                                      # the dtype of a map changes no count
            assert float(tc.handover32(pred.astype(dt), gt.astype(np.float32), nums, mode)[0]) == float(got)


@pytest.mark.parametrize("mode", tc.MODES)
def test_slipped_twins_leave_the_bound_on_every_fixture(iou_fix, mode):
    other = "per_object" if mode == "reference" else "reference"
    for k, (pred, gt, nums, iou4d, iou3d) in enumerate(iou_fix):
        want, tol, _, _ = tc.handover64(pred, gt, nums, mode)
        wrong_reading = tc.handover64(pred, gt, nums, other)[0]
        assert abs(wrong_reading - want) > tol, f"case {k}: the {other} reading stays inside the bound of the {mode} one"
        assert abs((iou3d if mode == "reference" else iou4d) - want) > tol, f"case {k}: the reference's other call form stays inside the bound"
        slipped = float(tc.handover32(pred, gt, nums, mode, slip="eps_on_intersection_only")[0])
        assert not abs(slipped - want) <= tol, f"case {k}: eps on the intersection only stays inside the bound ({slipped!r})"


def test_planted_ratios():
    H, W = 6, 5
    gt = np.zeros((1, H, W), np.int64)
    gt[0, :, 1:3] = 1
    gt[0, :3, 3] = 2
    for mode in tc.MODES:
        assert tc.handover32(gt, gt, [2], mode)[0] == f32(1.0)                  # pred == gt: every ratio (I + eps) / (I + eps)
        assert tc.handover32(gt, gt, [0], mode)[0] == f32(1.0)                  # only background: torch.ones
    disjoint = np.where(gt == 1, 2, np.where(gt == 2, 1, 0))
    iou, per, counts = tc.handover32(disjoint, gt, [2], "reference")
    assert (counts[0, :, 0] == 0).all() and iou < f32(0.5)                      # columns 0 and 4 hold nothing: eps / eps == 1.0f
    ratios = tc.ratio32(counts[0, :, 0].astype(np.int64), counts[0, :, 1].astype(np.int64), 1e-6)
    assert ratios[0] == f32(1.0) and ratios[4] == f32(1.0) and (ratios[1:4] < f32(1e-6)).all()
    odd = gt.astype(np.float32)
    odd[0, 0, 1] = 1.5                                                          # a non-integer names nothing
    assert tc.column_counts(odd[0], gt[0], 2)[1].tolist() == [H - 1, H]
    assert tc.column_counts(np.full((H, W), 255), np.full((H, W), 255), 30).sum() == 0


# ------------------------------------------------------------------------------------------ 2
def test_nearest_maps_equal_interpolate(golden):
    z = golden("train_handover_nearest")
    for k, (bs, H, W, h, w) in enumerate(tc.NEAREST_GEOMETRIES):
        pred = z[f"pred_{k}"].astype(np.int64)
        assert np.array_equal(pred, tc.make_maps(bs, H, W, [5] * bs, seed=100 + k, planted=False)[0])
        got = tc.nearest32(pred, (h, w))
        assert got.dtype == np.int32 and np.array_equal(got, z[f"small_{k}"]), f"case {k}: the nearest rule differs from the recorded interpolate"
        now = F.interpolate(torch.from_numpy(pred).unsqueeze(1).float(), size=(h, w), mode="nearest").int()[:, 0].numpy()
        assert np.array_equal(got, now)
        assert np.array_equal(tc.nearest32(pred.astype(np.float32), (h, w)), got)
        assert not np.array_equal(tc.nearest32(pred, (h, w), slip="round"), got), f"case {k}: rounding in place of floor does not show"
    for k, (bs, H, W, h, w) in enumerate(tc.NEAREST_WHOLE + [(1, 465, 465, 117, 117)]):
        pred = tc.make_maps(bs, H, W, [5] * bs, seed=200 + k, planted=False)[0]
        now = F.interpolate(torch.from_numpy(pred).unsqueeze(1).float(), size=(h, w), mode="nearest").int()[:, 0].numpy()
        assert np.array_equal(tc.nearest32(pred, (h, w)), now)
    assert [tc.nearest_index(y, 465, 117) for y in (0, 1, 116)] == [0, 3, 461]


# ------------------------------------------------------------------------------------------ 3
def test_meter_equals_average_meter_bit_for_bit(golden):
    want = golden("train_handover_meters")["state"]
    m, slipped, differs = tc.Meter(), tc.Meter(), False
    for entry, row in zip(tc.METER_SEQUENCE, want):
        if entry is None:
            m.reset(), slipped.reset()
        else:
            m.update(*entry)
            slipped.update(*entry, slip="count_plus_one")
        val, avg, total, count = m.state()
        assert np.float64(total).tobytes() == np.float64(row[2]).tobytes() and count == int(row[3])
        assert val == float(f32(row[0])) and avg == float(f32(row[1]))
        differs |= slipped.state()[1:] != m.state()[1:]
    assert differs, "count += 1 in place of n must show"
    assert ctypes.sizeof(ts._Meter) == 24 and ts._Meter.sum.offset == 8 and ts._Meter.count.offset == 16


def test_meter_struct_matches_the_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "m.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu %%d %%d\\n", sizeof(aoc_meter), '
                   'offsetof(aoc_meter, avg), offsetof(aoc_meter, sum), offsetof(aoc_meter, count), offsetof(aoc_meter, val), AOC_MAX_OBJECTS, '
                   'AOC_METERS_PER_CALL);return 0;}\n' % os.path.join(root, "include", "aoc_hip.h"))
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    M = ts._Meter
    assert got == [ctypes.sizeof(M), M.avg.offset, M.sum.offset, M.count.offset, M.val.offset, ts.MAX_OBJECTS, ts.METERS_PER_CALL]


# ------------------------------------------------------------------------------------------ 4
class Recorder(nn.Module):
    """AOCNet.forward's signature; records what every call received and returns a prediction that is a function of the frame alone"""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.tensor([0.5, -0.25]))
        self.calls = []

    def forward(self, inputs, memory_prev_list, ref_labels, prev_labels, curr_labels, gt_ids=None, step=0, tf_board=False, **extra):
        k = len(self.calls)
        self.calls.append(dict(inputs=inputs.clone(), memory=memory_prev_list, ref=ref_labels, prev=prev_labels.clone(), curr=curr_labels.clone(), gt_ids=gt_ids,
                               step=step, tf_board=tf_board, extra={n: v.clone() for n, v in extra.items()},
                               grad=None if self.w.grad is None else self.w.grad.clone()))
        bs = curr_labels.shape[0]
        all_pred = ((curr_labels[:, 0].long() + k) % 3)
        loss = (self.w[0] * inputs.mean() + self.w[1] * (k + 1)) * torch.ones(bs) + torch.arange(bs)
        return loss, all_pred, {"frame": k}, [f"memory of call {k}"] * bs


def _sample(bs, H, W, seq_len, seed):
    r = np.random.RandomState(seed)
    img = lambda: torch.from_numpy(r.rand(bs, 3, H, W).astype(f32))
    lab = lambda: torch.from_numpy(r.randint(0, 3, (bs, 1, H, W)).astype(f32))
    return {"ref_img": img(), "prev_img": img(), "curr_img": [img() for _ in range(seq_len)], "ref_label": lab(), "prev_label": lab(),
            "curr_label": [lab() for _ in range(seq_len)], "meta": {"obj_num": torch.tensor([2, 1][:bs])}}


@pytest.mark.parametrize("step,uses_prediction", [(10, False), (11, True)])
def test_sequential_step_label_flow_memory_and_meters(step, uses_prediction):
    bs, H, W, seq_len, small = 2, 9, 7, 3, (4, 3)
    model, sample = Recorder(), _sample(bs, H, W, 3, seed=3)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    meters = tc.HostMeters.for_sequence(seq_len)
    w0 = model.w.detach().clone()
    all_pred, boards = ts.sequential_step(model, sample, opt, step=step, seq_len=seq_len, start_seq_training_steps=10, meters=meters, scaled_labels=small,
                                          handover=tc.host_handover, memory_placeholder="placeholder")
    calls = model.calls
    assert len(calls) == seq_len and boards == [{"frame": k} for k in range(seq_len)]
    imgs = [sample["prev_img"]] + sample["curr_img"]
    preds = [((sample["curr_label"][k][:, 0].long() + k) % 3) for k in range(seq_len)]
    assert torch.equal(all_pred, preds[-1])
    for k, c in enumerate(calls):
        assert torch.equal(c["inputs"], torch.cat((sample["ref_img"], imgs[k], imgs[k + 1]), 0))
        assert c["ref"] is sample["ref_label"] and torch.equal(c["curr"], sample["curr_label"][k])
        assert c["step"] == step and c["tf_board"] is False and c["gt_ids"] is sample["meta"]["obj_num"]
        if k == 0 or not uses_prediction:                                      # :243-245 and the else of :257-262: the previous ground truth
            want_prev = sample["prev_label"] if k == 0 else sample["curr_label"][k - 1]
        else:                                                                   # :258-259
            want_prev = preds[k - 1].unsqueeze(1)
        assert c["prev"].shape == (bs, 1, H, W) and torch.equal(c["prev"].double(), want_prev.double()), f"frame {k}: wrong previous labels"
        want_small = F.interpolate(want_prev.float(), size=small, mode="nearest").int()
        got_small = c["extra"]["scale_previous_frame_label"]
        assert got_small.dtype == torch.int32 and torch.equal(got_small, want_small)
        assert c["memory"] == (["placeholder"] * bs if k == 0 else [f"memory of call {k - 1}"] * bs)          # :247-251, :275
    assert calls[0]["grad"] is None                                             # :246
    # meters: the loss from the scalar that was differentiated, times seq_len (:278, :281); the IoU of the frame's prediction (:277, :282)
    log = meters.log
    assert [e[0] for e in log] == [n for k in range(seq_len) for n in (f"iou_{k}", f"loss_{k}")]
    for k in range(seq_len):
        want_iou = tc.handover32(preds[k].numpy(), sample["curr_label"][k][:, 0].numpy(), [2, 1], "reference")[0]
        assert log[2 * k][1:] == (float(want_iou), 1.0, 1)
        per_sample = (w0[0] * calls[k]["inputs"].mean() + w0[1] * (k + 1)) * torch.ones(bs) + torch.arange(bs)
        want_loss = torch.mean(per_sample) / seq_len
        assert log[2 * k + 1][1:] == (float(want_loss), seq_len, 1)
        m = meters.meters[f"loss_{k}"]
        assert m.sum == float(want_loss) * seq_len and m.count == 1
    # the update: the three frames' gradients accumulated, one step
    g = torch.stack([sum(c["inputs"].mean() for c in calls), torch.tensor(float(sum(range(1, seq_len + 1))))]) / seq_len
    assert torch.allclose(model.w.detach(), w0 - 0.1 * g, rtol=1e-6, atol=0)


def test_sequential_step_zeroes_the_gradients_of_the_step_before():
    model, sample = Recorder(), _sample(2, 5, 6, 2, seed=4)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    model.w.grad = torch.tensor([3.0, 4.0])                                     # someone else's leftovers
    for _ in range(2):
        ts.sequential_step(model, sample, opt, step=0, seq_len=2, start_seq_training_steps=5, handover=tc.host_handover)
    first = [c["grad"] for c in model.calls[0::2]]
    assert all(g is None or not g.any() for g in first), "a step began with gradients that were not zero"
    assert all(c["grad"] is not None and c["grad"].any() for c in model.calls[1::2])      # the second frame accumulates onto the first
    assert all(not c["extra"] for c in model.calls)                             # no scaled_labels: the model gets no extra keyword
    assert all(c["memory"] == [None, None] for c in model.calls[0::2])


def test_wrappers_refuse_what_they_cannot_run():
    a = torch.zeros(2, 3, 4, dtype=torch.int64)
    with pytest.raises(_lib.AocHipError):
        ts.frame_handover(a, a, [1, 1])                                         # CPU tensors: no fallback
    with pytest.raises(ValueError):
        ts.frame_handover(a, a, [1, 1], mode="per_pixel")
    with pytest.raises(ValueError):
        ts.frame_handover(a.to(torch.int16), a, [1, 1])
    with pytest.raises(ValueError):
        ts.frame_handover(a, a, [1])
    with pytest.raises(ValueError):
        ts.frame_handover(a, a, [1, 1], want=(True, False, False, True))        # prev_small without a size
    for bad in (torch.zeros(3, 4), torch.zeros(1, 2, 3, 4), torch.zeros(1, 1, 1, 3, 4)):
        with pytest.raises(ValueError):
            ts.pytorch_iou(bad, bad, [1])


# ------------------------------------------------------------------------------------------ 5
def test_c_abi_rejections_without_a_device():
    L = _lib.lib()
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nums = (ctypes.c_int32 * 2)(1, 1)

    def call(pred=p, pd=0, gt=p, gd=0, bs=2, H=2, W=2, n=nums, eps=1e-6, mode=0, sh=0, sw=0, iou=p, per=None, counts=None, small=None, meter=None, ws=p, nbytes=256):
        return L.aoc_frame_handover(pred, pd, gt, gd, bs, H, W, n, eps, mode, sh, sw, iou, per, counts, small, meter, ws, nbytes, None)

    assert call(iou=None) == INVALID                                            # all outputs NULL
    assert call(pd=3) == INVALID and call(gd=-1) == INVALID                     # dtype codes
    assert call(mode=2) == INVALID and call(bs=0) == INVALID and call(pred=None) == INVALID and call(n=None) == INVALID
    assert call(n=(ctypes.c_int32 * 2)(1, 31)) == UNSUPPORTED and call(n=(ctypes.c_int32 * 2)(-1, 1)) == INVALID
    assert call(bs=1, H=4097, W=4096) == UNSUPPORTED                            # H * W above 2^24, by arguments only
    assert call(bs=128, H=4096, W=4096) == UNSUPPORTED                          # bs * H * W == 2^31
    assert call(nbytes=L.aoc_frame_handover_workspace_bytes(2, 2, 2) - 1) == WORKSPACE and call(ws=None) == INVALID
    assert call(small=p, sh=0, sw=3) == INVALID
    assert call(pred=ctypes.c_void_p(p.value + 2)) == INVALID                   # off the 4-byte grid
    assert L.aoc_frame_handover_workspace_bytes(1, 4097, 4096) == 0 and L.aoc_frame_handover_workspace_bytes(0, 4, 4) == 0
    assert L.aoc_frame_handover_workspace_bytes(1, 4096, 4096) > 0
    idx, ptrs = (ctypes.c_int32 * 2)(0, 0), (ctypes.c_void_p * 2)(p.value, p.value)
    sc, nn_ = (ctypes.c_double * 2)(1.0, 1.0), (ctypes.c_int64 * 2)(1, 1)
    assert L.aoc_meters_update(p, 2, idx, ptrs, sc, nn_, 2, None) == INVALID    # one meter twice
    assert L.aoc_meters_update(p, 2, (ctypes.c_int32 * 1)(2), ptrs, sc, nn_, 1, None) == INVALID
    assert L.aoc_meters_update(p, 2, idx, ptrs, sc, (ctypes.c_int64 * 1)(0), 1, None) == INVALID
    assert L.aoc_meters_update(p, 16, idx, ptrs, sc, nn_, 9, None) == UNSUPPORTED
    assert L.aoc_meters_update(None, 2, idx, ptrs, sc, nn_, 1, None) == INVALID
    assert L.aoc_meters_reset(p, 65, 1, None) == UNSUPPORTED and L.aoc_meters_reset(p, 2, 4, None) == INVALID and L.aoc_meters_reset(None, 2, 1, None) == INVALID
    assert L.aoc_meters_reset(p, 2, 0, None) == 0                               # nothing to reset: nothing launched
    assert not any(buf)
