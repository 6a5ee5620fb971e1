"""The frame hand-over of a training step (csrc/train_step.hip, aoc_amd.train_step), shared by tests/test_train_step_host.py and
tests/test_gpu_train_step.py: the float32 restatement in the order include/aoc_hip.h states, a float64 reference, the bound between them,
host meters, the slipped twins and the cases.

Counts are integers.  A ratio is ((float)I + eps) / ((float)U + eps): two additions and a division, one rounding each.  A sample's mean
over its n terms: thread t of 256 adds the terms t, t + 256, ... ascending from 0.0f (ceil(n / 256) additions, the first one exact), the
xor butterfly over the wave (6 levels), the four wave sums as (w0 + w1) + (w2 + w3) (2 levels), a division by (float)n.  The batch mean: the
counted samples serially (as many additions as samples), a division.  The bound is that analysis carried by gates_grad_bounds.E at
U = 2^-24 against a float64 evaluation that uses the float32 eps widened; no constant is fitted.  The reference's own pytorch_iou sums its
terms in torch's order, which is no deeper than this one at the fixtures' sizes (at most 31 terms), so it has to lie inside the same bound.
"""
import numpy as np
import torch

from float64_bounds import gamma
from gates_grad_bounds import E

f32, f64 = np.float32, np.float64
MAX_OBJECTS = 30
MODES = ("reference", "per_object")
DTYPES = {"i32": torch.int32, "i64": torch.int64, "f32": torch.float32}


# ------------------------------------------------------------------------------------------ counts (integers: any order)
def ids(m, n):
    """the object each label names among 1 .. n, else 0: v == o as numbers"""
    v = np.asarray(m)
    ok = (v >= 1) & (v <= n)
    if v.dtype.kind == "f":
        ok &= v == np.floor(v)
    return np.where(ok, v, 0).astype(np.int64)


def column_counts(pred, gt, n):
    """one sample [H, W] -> [W, 2]: I[x], U[x]"""
    p, g = ids(pred, n), ids(gt, n)
    both = (p != 0) & (p == g)
    return np.stack([both.sum(0), ((p != 0).astype(np.int64) + (g != 0) - both).sum(0)], 1).astype(np.uint32)


def object_counts(pred, gt, n):
    """one sample [H, W] -> [30, 3]: I[o], #pred[o], #gt[o], zero behind n"""
    p, g = ids(pred, n), ids(gt, n)
    out = np.zeros((MAX_OBJECTS, 3), np.uint32)
    for o in range(1, n + 1):
        out[o - 1] = ((p == o) & (g == o)).sum(), (p == o).sum(), (g == o).sum()
    return out


def counts_of(pred, gt, nums, mode):
    return np.stack([(column_counts if mode == "reference" else object_counts)(pred[s], gt[s], int(n)) for s, n in enumerate(nums)])


def _terms(counts, n, mode):
    """(I, U) of a sample's terms as integer vectors"""
    if mode == "reference":
        return counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
    c = counts[:n].astype(np.int64)
    return c[:, 0], c[:, 1] + c[:, 2] - c[:, 0]


# ------------------------------------------------------------------------------------------ the float32 restatement
def block_mean32(terms, n):
    """aoc_frame_handover's mean of a sample: 256 per-thread sums, the xor butterfly per wave, (w0 + w1) + (w2 + w3), / (float)n"""
    terms = np.asarray(terms, f32)
    acc = np.zeros(256, f32)
    for k in range(0, len(terms), 256):
        chunk = terms[k:k + 256]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    v = acc.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    total = f32(f32(v[0, 0] + v[1, 0]) + f32(v[2, 0] + v[3, 0]))
    return f32(total / f32(n))


def ratio32(I, U, eps, slip=None):
    e = f32(eps)
    if slip == "eps_on_intersection_only":
        with np.errstate(divide="ignore", invalid="ignore"):
            return (I.astype(f32) + e) / U.astype(f32)
    return (I.astype(f32) + e) / (U.astype(f32) + e)


def handover32(pred, gt, nums, mode="reference", eps=1e-6, slip=None):
    """-> (iou float32, iou_per_sample [bs] float32, counts) bit for bit what the device gives"""
    counts = counts_of(pred, gt, nums, mode)
    per = np.ones(len(nums), f32)
    batch, counted = f32(0.0), 0
    for s, n in enumerate(nums):
        if n == 0:
            continue
        I, U = _terms(counts[s], int(n), mode)
        per[s] = block_mean32(ratio32(I, U, eps, slip), len(I))
        batch = f32(batch + per[s])
        counted += 1
    return (f32(batch / f32(counted)) if counted else f32(1.0)), per, counts


# ------------------------------------------------------------------------------------------ the float64 reference and its bound
def handover64(pred, gt, nums, mode="reference", eps=1e-6):
    """-> (iou, tol, iou_per_sample [bs], tol [bs]) in float64"""
    e = E(torch.tensor(float(f32(eps)), dtype=torch.float64))
    per, per_tol = np.ones(len(nums)), np.zeros(len(nums))
    batch, counted = None, 0
    counts = counts_of(pred, gt, nums, mode)
    for s, n in enumerate(nums):
        if n == 0:
            continue
        I, U = _terms(counts[s], int(n), mode)
        r = (E(torch.from_numpy(I).double()) + e) / (E(torch.from_numpy(U).double()) + e)
        depth = -(-len(I) // 256) + 6 + 2
        m = r.sum(0, depth) / E(torch.tensor(float(len(I)), dtype=torch.float64))
        per[s], per_tol[s] = float(m.v), float(m.e)
        batch = m if batch is None else E(batch.v + m.v, batch.e + m.e)
        counted += 1
    if not counted:
        return 1.0, 0.0, per, per_tol
    total = E(batch.v, batch.e + gamma(counted) * (batch.v.abs() + batch.e))      # the serial sum
    out = total / E(torch.tensor(float(counted), dtype=torch.float64))
    return float(out.v), float(out.e), per, per_tol


# ------------------------------------------------------------------------------------------ torch's nearest rule
def nearest_index(dst, src_size, dst_size, slip=None):
    """source index of destination index `dst`: min((int)floorf((float)dst * ((float)src / (float)dst_size)), src - 1) in float32"""
    scale = f32(f32(src_size) / f32(dst_size))
    v = f32(dst) * scale
    i = int(np.floor(v + f32(0.5))) if slip == "round" else int(np.floor(v))
    return min(i, src_size - 1)


def nearest32(pred, size, slip=None):
    """pred [bs, H, W] -> [bs, h, w] int32 through the nearest rule; float labels through (int)v"""
    pred = np.asarray(pred)
    H, W = pred.shape[1:]
    ys = [nearest_index(y, H, size[0], slip) for y in range(size[0])]
    xs = [nearest_index(x, W, size[1], slip) for x in range(size[1])]
    return pred[:, ys][:, :, xs].astype(np.int32)


# ------------------------------------------------------------------------------------------ meters
class Meter:
    """aoc_meter on the host: utils/meters.py in doubles, val and avg as the floats the device stores"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val, self.avg, self.sum, self.count = f32(0.0), f32(0.0), 0.0, 0

    def update(self, value, scale=1.0, n=1, slip=None):
        x = float(f32(value)) * float(scale)
        self.val = f32(x)
        self.sum += x * n
        self.count += 1 if slip == "count_plus_one" else n
        self.avg = f32(self.sum / self.count)

    def state(self):
        return float(self.val), float(self.avg), self.sum, self.count


class HostMeters:
    """what sequential_step needs of a DeviceMeters, on the host, recording every update"""

    class Slot:
        def __init__(self, owner, name):
            self.owner, self.name = owner, name

        def update(self, value):
            self.owner.update(self.name, value)

    def __init__(self, names):
        self.meters = {name: Meter() for name in names}
        self.log = []

    @classmethod
    def for_sequence(cls, seq_len):
        return cls([f"loss_{i}" for i in range(seq_len)] + [f"iou_{i}" for i in range(seq_len)])

    def slot(self, name):
        return HostMeters.Slot(self, name)

    def update(self, name, value, scale=1.0, n=1):
        value = float(value.reshape(-1)[0]) if torch.is_tensor(value) else float(value)
        self.log.append((name, value, scale, n))
        self.meters[name].update(value, scale, n)


def host_handover(pred, gt, obj_nums, small_size=None, mode="reference", epsilon=1e-6, want=(True, False, False, None), out=None, meter=None):
    """frame_handover's signature on CPU tensors, by the restatement"""
    prev_small = None
    if small_size is not None and (want[3] is None or want[3]):
        prev_small = torch.from_numpy(nearest32(pred.numpy(), small_size))
    if gt is None:
        return None, None, None, prev_small
    iou, per, counts = handover32(pred.numpy(), gt.numpy(), [int(n) for n in obj_nums], mode, epsilon)
    if meter is not None:
        meter.update(iou)
    return torch.tensor([iou]), torch.from_numpy(per), torch.from_numpy(counts.astype(np.int32)), prev_small


# ------------------------------------------------------------------------------------------ cases
def make_maps(bs, H, W, nums, seed, planted=True):
    """(pred, gt) [bs, H, W] int64: gt random ids in 0 .. n with a background majority, pred = gt with a quarter of the pixels drawn again;
    then 255, -1 and n + 1 sprinkled into both.  planted: column 0 holds no object and the sample's largest id appears nowhere (an empty
    union in either reading), wherever the map has room for it."""
    r = np.random.RandomState([17, bs, H, W, seed])
    pred, gt = np.zeros((bs, H, W), np.int64), np.zeros((bs, H, W), np.int64)
    for s, n in enumerate(nums):
        g = r.randint(0, n + 1, (H, W)) * (r.rand(H, W) < 0.6)
        p = np.where(r.rand(H, W) < 0.25, r.randint(0, n + 1, (H, W)), g)
        for m in (p, g):
            k = r.rand(H, W)
            m[k < 0.03] = 255
            m[(k >= 0.03) & (k < 0.05)] = -1
            m[(k >= 0.05) & (k < 0.07)] = n + 1
        if planted:
            if W > 1:
                p[:, 0], g[:, 0] = 0, 255
            if n > 1:
                p[p == n], g[g == n] = 0, 0
        pred[s], gt[s] = p, g
    return pred, gt


# (bs, H, W, obj_nums): tests/test_gpu_train_step.py
GPU_GEOMETRIES = [
    (1, 1, 1, [1]),
    (1, 3, 5, [2]),
    (2, 7, 9, [3, 0]),                      # the second sample starts 12 bytes off the 16-byte grid
    (3, 33, 31, [30, 1, 0]),
    (2, 17, 260, [4, 2]),                   # two column strips
    (1, 300, 5, [5]),                       # many row bands
    (8, 65, 129, [5, 0, 3, 1, 4, 2, 5, 1]),
    (4, 17, 16, [0, 0, 0, 0]),              # iou == 1.0f
]
CROP = (1, 465, 465, [5])
CROP_SMALL = (117, 117)

# the fixtures of tests/golden/train_handover_iou.npz: maps <= 33 x 31, bs <= 3
FIXTURE_GEOMETRIES = [(1, 3, 5, [2]), (2, 7, 9, [3, 0]), (3, 33, 31, [30, 1, 0]), (2, 17, 16, [4, 2])]
# (bs, H, W, h, w): train_handover_nearest.npz -- down- and up-scaling with fractional steps, where rounding and floor part
NEAREST_GEOMETRIES = [(2, 33, 31, 9, 8), (1, 7, 9, 16, 20), (3, 31, 33, 8, 9), (1, 30, 30, 7, 13)]
# the geometries on which rounding cannot show (identity, a single source pixel, whole factors), checked against torch as it runs
NEAREST_WHOLE = [(1, 5, 7, 5, 7), (1, 1, 1, 3, 2), (2, 4, 6, 8, 12)]
# (value, scale, n) and None = reset: train_handover_meters.npz
METER_SEQUENCE = [(0.75, 1.0, 1), (0.1, 3.0, 1), (1.0 / 3.0, 5.0, 4), (2.5e-3, 3.0, 2), None, (0.3, 5.0, 3), (0.7, 1.0, 1)]
