"""The frame hand-over of a training step on the device (csrc/train_step.hip, aoc_amd.train_step; tests/train_step_cases.py holds the
restatement, the references and the bound; tests/test_train_step_host.py is the host half).

1. aoc_frame_handover through its C entry on label maps inside 0xFF-filled arenas at the four misalignments, every dtype, both modes: the
   counts numpy's, iou and iou_per_sample bit for bit the float32 restatement and inside the bound of the float64 reference, prev_small torch's
   own nearest resize on the device, margins untouched, each output alone with the bits it has with the others, the same bits from a second
   run and from a workspace of all-ones bytes;  2. the training crop once;  3. planted maps;  4. nearest geometries;  5. meters;
6. rejections;  7. no synchronisation;  8. sequential_step around a stand-in model against the same lines written out with ``.item()``.
"""
import ctypes
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import stream_order_cases as soc
import train_step_cases as tc
from aoc_amd import _lib, loss_train
from aoc_amd import optim_train as ot
from aoc_amd import train_step as ts

pytestmark = pytest.mark.gpu
f32 = np.float32
CODES = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.float32): 2}
NP_DTYPES = (np.int32, np.int64, np.float32)
OUTS = ("iou", "per", "counts", "small")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    _lib.lib()
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------ arenas and the raw call
class Buf:
    """nbytes of payload inside a device buffer filled with one byte value, starting `off` floats behind the 16-byte grid, 32 bytes of margin"""

    def __init__(self, dev, nbytes, off=0, data=None, fill=0xFF):
        self.lo, self.n = 32 + 4 * off, int(nbytes)
        self.host = np.full(self.lo + self.n + 32, fill, np.uint8)
        if data is not None:
            self.host[self.lo:self.lo + self.n] = np.frombuffer(np.ascontiguousarray(data).tobytes(), np.uint8)
        self.dev = torch.from_numpy(self.host).to(dev)
        assert self.dev.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr() + self.lo)

    def read(self, dtype, shape):
        raw = self.dev.cpu().numpy()
        assert (raw[:self.lo] == self.host[:self.lo]).all() and (raw[self.lo + self.n:] == self.host[self.lo + self.n:]).all(), "a margin was written"
        return np.frombuffer(raw[self.lo:self.lo + self.n].tobytes(), dtype).reshape(shape)

    def untouched(self):
        return bool((self.dev.cpu().numpy() == self.host).all())


def counts_shape(bs, W, mode):
    return (bs, W, 2) if mode == "reference" else (bs, tc.MAX_OBJECTS, 3)


class Call:
    """one aoc_frame_handover call on arenas; results as numpy arrays"""

    def __init__(self, dev, pred, gt, nums, mode, off=0, small=None, outs=OUTS, eps=1e-6, ws_fill=0x00, meter=None, expect=0, ws_bytes=None,
                 shape=None, codes=None, nums_raw=None):
        bs, H, W = shape or pred.shape
        L = _lib.lib()
        self.pred, self.gt = Buf(dev, pred.nbytes, off, pred), Buf(dev, gt.nbytes, (off + 1) % 4, gt)
        h, w = small or (0, 0)
        self.bufs = {"iou": Buf(dev, 4, (off + 2) % 4), "per": Buf(dev, 4 * pred.shape[0], (off + 3) % 4),
                     "counts": Buf(dev, 4 * int(np.prod(counts_shape(pred.shape[0], pred.shape[2], mode))), off),
                     "small": Buf(dev, 4 * pred.shape[0] * max(h * w, 1), (off + 1) % 4)}
        need = L.aoc_frame_handover_workspace_bytes(*pred.shape)
        self.ws = Buf(dev, need if ws_bytes is None else ws_bytes, off, fill=ws_fill)
        ptr = lambda k: self.bufs[k].ptr if k in outs else None
        n_arr = (ctypes.c_int32 * len(nums))(*(nums_raw or nums))
        pc, gc = codes or (CODES[pred.dtype], CODES[gt.dtype])
        self.rc = L.aoc_frame_handover(self.pred.ptr, pc, self.gt.ptr, gc, bs, H, W, n_arr, float(eps), tc.MODES.index(mode), h, w, ptr("iou"), ptr("per"),
                                       ptr("counts"), ptr("small") if small else None, meter, self.ws.ptr, self.ws.n, None)
        assert self.rc == expect, f"aoc_frame_handover returned {_lib.STATUS.get(self.rc, self.rc)}"
        torch.cuda.synchronize()
        self.outs, self.small_size, self.mode, self.shape = outs, small, mode, pred.shape

    def result(self):
        bs, H, W = self.shape
        r = {}
        for k, dtype, shape in (("iou", f32, ()), ("per", f32, (bs,)), ("counts", np.uint32, counts_shape(bs, W, self.mode)),
                                ("small", np.int32, (bs,) + tuple(self.small_size or (1, 1)))):
            if k in self.outs and (k != "small" or self.small_size):
                r[k] = self.bufs[k].read(dtype, shape)
            else:
                assert self.bufs[k].untouched(), f"{k} was not asked for and was written"
        assert self.pred.untouched() and self.gt.untouched()
        return r


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def small_of(H, W):
    return max(1, (H + 3) // 4), max(1, (W + 2) // 3)


def check_against_references(r, pred, gt, nums, mode, small, what):
    iou, per, counts = tc.handover32(pred, gt, nums, mode)
    want, tol, per64, per_tol = tc.handover64(pred, gt, nums, mode)
    assert same(r["counts"], counts), f"{what}: the counts are not numpy's"
    assert r["iou"].tobytes() == f32(iou).tobytes(), f"{what}: iou {float(r['iou'])!r} is not the restatement's {float(iou)!r}"
    assert same(r["per"], per), f"{what}: iou_per_sample differs from the restatement"
    assert abs(float(r["iou"]) - want) <= tol and (np.abs(r["per"].astype(np.float64) - per64) <= per_tol).all(), f"{what}: outside the float64 bound"
    assert all(v == f32(1.0) for v, n in zip(r["per"], nums) if n == 0)
    if small:
        assert same(r["small"], tc.nearest32(pred, small)), f"{what}: prev_small is not the nearest rule's"


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("g", range(len(tc.GPU_GEOMETRIES)))
def test_geometries_bit_for_bit_at_every_alignment(dev, g, mode):
    bs, H, W, nums = tc.GPU_GEOMETRIES[g]
    pred64, gt64 = tc.make_maps(bs, H, W, nums, seed=40 + g)
    small = small_of(H, W)
    first = None
    for off in range(4):                                                        # every misalignment, the dtypes rotating with it
        pd, gd = NP_DTYPES[(g + off) % 3], NP_DTYPES[(g + off + 1 + (off >> 1)) % 3]
        pred, gt = pred64.astype(pd), gt64.astype(gd)
        r = Call(dev, pred, gt, nums, mode, off, small).result()
        check_against_references(r, pred, gt, nums, mode, small, f"geometry {g} {mode} off {off} {pd.__name__}/{gd.__name__}")
        on_dev = F.interpolate(torch.from_numpy(pred64).to(dev).unsqueeze(1).float(), size=small, mode="nearest").int()[:, 0]
        assert torch.equal(torch.from_numpy(r["small"].copy()).to(dev), on_dev), "prev_small differs from torch's nearest resize on the device"
        first = first or r
        assert all(same(r[k], first[k]) for k in OUTS), "the bits depend on a pointer's alignment or a map's dtype"
    pred, gt = pred64.astype(np.int64), gt64.astype(np.float32)                 # the trainer's pair: upsampled_criterion's int64, the loader's float
    for k in OUTS:                                                              # each output alone
        alone = Call(dev, pred, gt, nums, mode, 1, small, outs=(k,)).result()
        assert list(alone) == [k] and same(alone[k], first[k]), f"{k} alone differs from {k} beside the others"
    again = Call(dev, pred, gt, nums, mode, 1, small, ws_fill=0xFF).result()    # a second run, in a workspace of all-ones bytes
    assert all(same(again[k], first[k]) for k in OUTS), "the bits depend on what the workspace held"
    if all(n == 0 for n in nums):
        assert first["iou"] == f32(1.0)


@pytest.mark.parametrize("mode", tc.MODES)
def test_training_crop(dev, mode):
    bs, H, W, nums = tc.CROP
    pred64, gt64 = tc.make_maps(bs, H, W, nums, seed=7)
    pred, gt = pred64.astype(np.int64), gt64.astype(np.float32)
    r = Call(dev, pred, gt, nums, mode, 3, tc.CROP_SMALL).result()
    check_against_references(r, pred, gt, nums, mode, tc.CROP_SMALL, f"crop {mode}")
    on_dev = F.interpolate(torch.from_numpy(pred64).to(dev).unsqueeze(1).float(), size=tc.CROP_SMALL, mode="nearest").int()[:, 0]
    assert torch.equal(torch.from_numpy(r["small"].copy()).to(dev), on_dev)
    # the wrappers on ordinary tensors: the drop-in takes the mode from the rank, as the reference's broadcasting does
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    got = ts.pytorch_iou(p.unsqueeze(1), t.unsqueeze(1), torch.tensor(nums)) if mode == "reference" else ts.pytorch_iou(p, t, torch.tensor(nums, device=dev))
    assert got.shape == () and got.is_cuda and got.cpu().numpy().tobytes() == r["iou"].tobytes()
    with pytest.raises(ValueError):
        ts.pytorch_iou(p[0], t[0], nums)


# ------------------------------------------------------------------------------------------ 3: planted maps
def test_planted_maps(dev):
    H, W = 9, 6
    gt = np.zeros((2, H, W), np.int64)
    gt[:, :, 1:3] = 1
    gt[:, :4, 3] = 2
    gt[1, 5:, 4] = 3
    nums = [2, 3]
    for mode in tc.MODES:
        r = Call(dev, gt.astype(np.int32), gt.astype(np.float32), nums, mode).result()
        assert r["iou"] == f32(1.0) and (r["per"] == f32(1.0)).all(), "pred == gt must give exactly 1.0f"
    disjoint = np.where(gt == 1, 2, np.where(gt == 2, 1, 0))
    r = Call(dev, disjoint, gt.astype(np.float32), nums, "reference").result()
    assert (r["counts"][..., 0] == 0).all() and (r["counts"][0, :, 1] == [0, 2 * H, 2 * H, 8, 0, 0]).all()
    check_against_references(r, disjoint, gt.astype(np.float32), nums, "reference", None, "disjoint")
    e = f32(1e-6)
    ratios = (r["counts"][0, :, 0].astype(f32) + e) / (r["counts"][0, :, 1].astype(f32) + e)
    assert ratios[0] == f32(1.0) and ratios[5] == f32(1.0)                      # a column with no object: eps / eps
    r = Call(dev, disjoint, gt.astype(np.float32), nums, "per_object").result()
    assert (r["counts"][0, :2] == [[0, 4, 2 * H], [0, 2 * H, 4]]).all() and (r["counts"][0, 2:] == 0).all() and r["per"][0] < f32(1e-6)
    # 255, negatives, ids above obj_num and non-integers name nothing, in either map
    noisy_p, noisy_g = gt.astype(np.float32), gt.astype(np.float32)
    noisy_p[0, 0, :] = [255, -1, 3, 1.5, 0.5, 31]
    noisy_g[0, 1, :] = [255, -2, 3, 2.5, 1e9, -0.0]
    noisy_g[1, 8, 0] = np.nan
    for mode in tc.MODES:
        r = Call(dev, noisy_p, noisy_g, nums, mode, 2).result()
        check_against_references(r, noisy_p, noisy_g, nums, mode, None, f"noisy {mode}")
    r = Call(dev, np.full((1, H, W), 255, np.int64), np.full((1, H, W), 255, np.int32), [30], "reference").result()
    assert r["iou"] == f32(1.0) and not r["counts"].any()


# ------------------------------------------------------------------------------------------ 4: nearest geometries
def test_prev_small_alone_equals_torch_on_the_device(dev):
    for k, (bs, H, W, h, w) in enumerate(tc.NEAREST_GEOMETRIES + tc.NEAREST_WHOLE):
        pred = tc.make_maps(bs, H, W, [5] * bs, seed=300 + k, planted=False)[0]
        for dt in (torch.int64, torch.int32, torch.float32):
            p = torch.from_numpy(pred).to(dev).to(dt)
            got = ts.frame_handover(p, None, None, small_size=(h, w), want=(False, False, False, True))      # one launch: no gt, no obj_nums
            assert got[:3] == (None, None, None) and got[3].dtype == torch.int32
            assert torch.equal(got[3], F.interpolate(p.unsqueeze(1).float(), size=(h, w), mode="nearest").int()[:, 0]), f"{(bs, H, W, h, w)} {dt}"


# ------------------------------------------------------------------------------------------ 5: meters
def test_meters_against_average_meter(dev, golden):
    want = golden("train_handover_meters")["state"]                             # AverageMeter's own arithmetic, recorded
    meters = ts.DeviceMeters(["a", "b", "c"], dev)
    other = tc.Meter()
    for entry, row in zip(tc.METER_SEQUENCE, want):
        if entry is None:
            meters.reset("a")
        else:
            value, scale, n = entry
            word, twin = torch.tensor([value], device=dev), torch.tensor([1.0 - value], device=dev)
            meters.update(["a", "b"], [word, twin], [scale, 1.0], [n, 2])       # two meters, one launch
            other.update(1.0 - value, 1.0, 2)
        got = meters.read()
        a, b = got["a"], got["b"]
        assert np.float64(a.sum).tobytes() == np.float64(row[2]).tobytes() and a.count == int(row[3]), f"sum / count after {entry}"
        assert a.val == float(f32(row[0])) and a.avg == float(f32(row[1]))
        assert (b.val, b.avg, b.sum, b.count) == other.state(), "a reset or an update of one meter touched another"
        assert (got["c"].val, got["c"].avg, got["c"].sum, got["c"].count) == (0.0, 0.0, 0.0, 0)
    pred, gt = (torch.from_numpy(m).to(dev) for m in tc.make_maps(2, 7, 9, [3, 0], seed=1))
    iou = ts.frame_handover(pred, gt, [3, 0], meter=meters.slot("c"))[0]
    meters.update(2, iou, scale=2.0, n=3)                                       # by index
    c = meters.read()["c"]
    v = float(iou.cpu()[0])
    assert c.sum == v + v * 2.0 * 3 and c.count == 4 and c.val == float(f32(v * 2.0)) and c.avg == float(f32(c.sum / 4))
    meters.reset()
    assert all((m.val, m.avg, m.sum, m.count) == (0.0, 0.0, 0.0, 0) for m in meters.read().values())
    with pytest.raises(ValueError):
        meters.update("a", torch.ones(2, device=dev))
    with pytest.raises(_lib.AocHipError):
        meters.update(["a", "a"], [iou, iou])


# ------------------------------------------------------------------------------------------ 6: rejections
def test_rejections_leave_the_outputs_alone(dev):
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    pred, gt = (m.astype(np.int32) for m in tc.make_maps(2, 7, 9, [3, 1], seed=2))
    calls = [Call(dev, pred, gt, [3, 31], "reference", 1, (2, 3), expect=UNSUPPORTED),                      # obj_num 31
             Call(dev, pred, gt, [3, 1], "reference", 1, (2, 3), expect=INVALID, nums_raw=[3, -1]),
             Call(dev, pred, gt, [3, 1], "per_object", 1, (2, 3), expect=UNSUPPORTED, shape=(1, 4097, 4096)),  # H * W above 2^24: arguments only
             Call(dev, pred, gt, [3, 1], "reference", 1, (2, 3), expect=UNSUPPORTED, shape=(128, 4096, 4096)),
             Call(dev, pred, gt, [3, 1], "reference", 1, (2, 3), expect=INVALID, codes=(3, 0)),                # bad dtype code
             Call(dev, pred, gt, [3, 1], "reference", 1, (2, 3), expect=INVALID, codes=(0, -1)),
             Call(dev, pred, gt, [3, 1], "reference", 1, None, outs=(), expect=INVALID),                       # all outputs NULL
             Call(dev, pred, gt, [3, 1], "per_object", 1, (2, 3), expect=WORKSPACE, ws_bytes=_lib.lib().aoc_frame_handover_workspace_bytes(2, 7, 9) - 4),
             Call(dev, pred, gt, [3, 1], "reference", 1, (0, 3), outs=("small",), expect=INVALID)]
    torch.cuda.synchronize()
    for c in calls:
        assert all(b.untouched() for b in list(c.bufs.values()) + [c.ws, c.pred, c.gt]), "a rejected call wrote something"


# ------------------------------------------------------------------------------------------ 7: no synchronisation
def test_handover_and_meter_update_do_not_wait(dev):
    pred, gt = (torch.from_numpy(m).to(dev) for m in tc.make_maps(2, 65, 129, [3, 2], seed=3))
    gt = gt.float()
    word = torch.tensor([0.25], device=dev)

    def run(stall_ms, cycles_per_ms):
        meters = ts.DeviceMeters(["loss", "iou"], dev)
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        if stall_ms:
            torch.cuda._sleep(int(stall_ms * cycles_per_ms))
        ev.record()
        t0 = time.perf_counter()
        out = ts.frame_handover(pred, gt, [3, 2], small_size=(17, 33), meter=meters.slot("iou"))
        meters.update("loss", word, scale=3)
        t_enq = time.perf_counter() - t0
        stalled = not ev.query()
        state = meters.read()
        return (out[0].clone(), out[3].clone(), state["iou"].sum, state["loss"].sum), t_enq, stalled

    cpm = soc.calibrate_cycles_per_ms()
    run(0, cpm)                                                                 # loads the kernels, fills the allocator's cache
    want, t_enq, _ = run(0, cpm)
    stall_ms = max(soc.STALL_MIN_MS, soc.STALL_T_ENQ_FACTOR * t_enq * 1e3)
    assert stall_ms <= soc.STALL_MAX_MS, f"the two calls took {t_enq * 1e3:.1f} ms on the host"
    got, _, stalled = run(stall_ms, cpm)
    assert stalled, "frame_handover + DeviceMeters.update returned only after the spin in front of them was over: something waits for the device"
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:]


# ------------------------------------------------------------------------------------------ 8: the loop
H8, W8, SMALL8, NUMS8, SEQ = 33, 31, (9, 8), [3, 1], 3


class StandIn(nn.Module):
    """AOCNet.forward's signature: a 1 x 1 convolution over the pooled image and the scaled previous mask to [1, O + 1, h, w] logits per sample,
    through loss_train.upsampled_criterion.  Written with broadcasting and sums, so equal inputs give equal bits."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.weight = nn.Parameter(torch.randn(tc.MAX_OBJECTS + 1, 4, generator=g) * 0.5)
        self.bias = nn.Parameter(torch.zeros(tc.MAX_OBJECTS + 1))
        self.criterion = loss_train.Concat_CrossEntropyLoss(top_k_percent_pixels=0.15, hard_example_mining_step=100)
        self.seen, self.preds = [], []

    def forward(self, inputs, memory_prev_list, ref_labels, prev_labels, curr_labels, gt_ids=None, step=0, tf_board=False, scale_previous_frame_label=None):
        bs = curr_labels.shape[0]
        self.seen.append((prev_labels.detach().clone(), scale_previous_frame_label.clone(), list(memory_prev_list)))
        x = torch.cat((F.adaptive_avg_pool2d(inputs[2 * bs:], SMALL8), scale_previous_frame_label.float()), 1)
        tmp = []
        for i in range(bs):
            n = int(gt_ids[i]) + 1
            tmp.append(((self.weight[:n, :, None, None] * x[i][None]).sum(1) + self.bias[:n, None, None]).unsqueeze(0).contiguous())
        losses, all_pred = loss_train.upsampled_criterion(self.criterion, tmp, [curr_labels[i] for i in range(bs)], step, (H8, W8))
        self.preds.append(all_pred.clone())
        return losses, all_pred, {}, [len(self.seen)] * bs


def plain_iou(pred4, gt4, nums, eps=1e-6):
    """the per-column reading in plain torch, float32"""
    vals = []
    for s, n in enumerate(nums):
        if n == 0:
            continue
        p, g = pred4[s, 0], gt4[s, 0]
        pin, gin = (p >= 1) & (p <= n), (g >= 1) & (g <= n)
        both = pin & (p == g)
        inter, union = both.float().sum(0), (pin.float() + gin.float() - both.float()).sum(0)
        vals.append(((inter + eps) / (union + eps)).mean())
    return torch.stack(vals).mean() if vals else torch.ones((), device=pred4.device)


def written_out(model, sample, opt, step, start, meters):
    """train_manager_mm.py:241-284 as the trainer has them: .item(), host meters, the nearest resize and the IoU in plain torch"""
    ref_imgs, prev_imgs, ref_labels, prev_labels = sample["ref_img"], sample["prev_img"], sample["ref_label"], sample["prev_label"]
    obj_nums = sample["meta"]["obj_num"]
    curr_imgs, curr_labels, all_pred = prev_imgs, prev_labels, prev_labels.squeeze(1)
    opt.zero_grad(set_to_none=False)
    memory_prev_list = [None] * len(NUMS8)
    for idx in range(SEQ):
        prev_imgs, curr_imgs = curr_imgs, sample["curr_img"][idx]
        inputs = torch.cat((ref_imgs, prev_imgs, curr_imgs), 0)
        prev_labels = all_pred.unsqueeze(1) if step > start else curr_labels
        curr_labels = sample["curr_label"][idx]
        scaled = F.interpolate(prev_labels.float(), size=SMALL8, mode="nearest").int()
        loss, all_pred, _, memory_prev_list = model(inputs, memory_prev_list, ref_labels, prev_labels, curr_labels, gt_ids=obj_nums, step=step, tf_board=False,
                                                    scale_previous_frame_label=scaled)
        iou = plain_iou(all_pred.unsqueeze(1), curr_labels, NUMS8)
        loss = torch.mean(loss) / SEQ
        loss.backward()
        meters[f"loss_{idx}"].update(loss.item(), SEQ)
        meters[f"iou_{idx}"].update(iou.item())
    opt.step()


def make_sample(dev, seed):
    r = np.random.RandomState(seed)
    img = lambda: torch.from_numpy(r.rand(2, 3, H8, W8).astype(f32)).to(dev)

    def lab():
        m = np.stack([r.randint(0, n + 1, (H8 // 3, W8 // 3 + 1)).repeat(3, 0).repeat(3, 1)[:H8, :W8] for n in NUMS8])
        return torch.from_numpy(m[:, None].astype(f32)).to(dev)
    return {"ref_img": img(), "prev_img": img(), "curr_img": [img() for _ in range(SEQ)], "ref_label": lab(), "prev_label": lab(),
            "curr_label": [lab() for _ in range(SEQ)], "meta": {"obj_num": torch.tensor(NUMS8)}}


@pytest.mark.parametrize("steps,uses_prediction", [((9, 10), False), ((11, 12), True)])
def test_sequential_step_against_the_written_out_loop(dev, steps, uses_prediction):
    start = 10
    samples = [make_sample(dev, 20 + s) for s in steps]
    with torch.enable_grad():                                                   # conftest wraps GPU tests in no_grad
        a, b = StandIn().to(dev), StandIn().to(dev)
        new_opt = lambda m: ot.SGD(ot.get_trainable_params(m, 0.05, 1e-4), lr=0.05, momentum=0.9, nesterov=True, clip_grad_norm=5.0)
        opt_a, opt_b = new_opt(a), new_opt(b)
        dev_meters = ts.DeviceMeters.for_sequence(SEQ, dev)
        host_meters = {name: tc.Meter() for name in dev_meters.names}
        for step, sample in zip(steps, samples):
            ts.sequential_step(a, sample, opt_a, step=step, seq_len=SEQ, start_seq_training_steps=start, meters=dev_meters, scaled_labels=SMALL8)
            written_out(b, sample, opt_b, step, start, host_meters)
    got = dev_meters.read()                                                     # the first wait
    assert all(p.grad is not None and not p.grad.any() for p in a.parameters()), "the update pass left the gradients zeroed for the next step"
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb), "the hand-over changes only integers: the parameters must agree bit for bit"
    assert not torch.equal(a.weight, StandIn().weight.to(dev))
    assert len(a.seen) == len(b.seen) == 2 * SEQ
    for k, ((prev_a, small_a, mem_a), (prev_b, small_b, mem_b)) in enumerate(zip(a.seen, b.seen)):
        assert prev_a.shape == prev_b.shape == (2, 1, H8, W8) and torch.equal(prev_a.double(), prev_b.double()), f"call {k}: other previous labels"
        assert small_a.dtype == torch.int32 and small_a.shape == (2, 1) + SMALL8 and torch.equal(small_a, small_b), f"call {k}: other scaled labels"
        assert mem_a == mem_b == ([None, None] if k % SEQ == 0 else [k, k])
        uses = uses_prediction and k % SEQ > 0
        assert (prev_a.dtype == torch.int64) == uses and (not uses or torch.equal(prev_a[:, 0], a.preds[k - 1]))
    for idx in range(SEQ):
        m, h = got[f"loss_{idx}"], host_meters[f"loss_{idx}"]
        assert (m.val, m.avg, m.sum, m.count) == h.state() and m.count == 2, f"loss meter {idx}"
        want = tol = 0.0
        for s, sample in enumerate(samples):
            w, t = tc.handover64(a.preds[s * SEQ + idx].cpu().numpy(), sample["curr_label"][idx][:, 0].cpu().numpy(), NUMS8, "reference")[:2]
            want, tol = want + w, tol + t
        m, h = got[f"iou_{idx}"], host_meters[f"iou_{idx}"]
        assert m.count == 2 and abs(m.sum - want) <= tol and abs(h.sum - want) <= tol, f"IoU meter {idx}: {m.sum!r} against {want!r} +- {tol:.2e}"
        assert 0.0 < m.avg <= 1.0
