"""The training update on csrc/optim.hip: what the reference trainer runs between ``loss.backward()`` and the next forward,

    train_manager_mm.py:283      torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.TRAIN_CLIP_GRAD_NORM)
    train_manager_mm.py:68-72    optim.SGD(trainable_params, lr, momentum=0.9, nesterov=True)
    train_manager_mm.py:284      optimizer.step()
    utils/learning.py:4-34       adjust_learning_rate (warm-up, then poly or cosine), get_trainable_params

``get_trainable_params`` puts every parameter into a group of its own (the GCT ``beta``s can then get another weight decay), which leaves torch
no multi-tensor path: several small launches per tensor over several hundred tensors.  Here the gradients, parameters and momentum buffers of
the whole model are described by ONE table (include/aoc_hip.h: aoc_mt_tensor) and a step is three launches:

    SGD.step()          aoc_clip_sgd_step       the three entries below as ONE call (``clip_grad_norm`` set), or aoc_sgd_step alone
                        aoc_grad_sumsq_partials  the sum of g^2 per chunk of 4096 floats, in a fixed order
                        aoc_grad_norm_finish     total_norm and the clip coefficient, left on the device
                        aoc_sgd_step             clip, weight decay, momentum, Nesterov and the parameter update in one pass; zeroes g where asked
    clip_grad_norm_     the first two, then aoc_multi_tensor_scale: the drop-in for train_manager_mm.py:283
    SGD.zero_grad(set_to_none=False)             aoc_multi_tensor_zero

The table is built in pinned memory and uploaded with a non-blocking copy, and only when a pointer, a size, a weight decay or a flag has
changed (``SGD.table_uploads`` counts the uploads); nothing in ``step`` synchronises.  The update's order of operations is torch's
``_single_tensor_sgd`` behind ``clip_grad_norm_`` (the clip first, the weight decay second), one rounding per operation; there are no float
atomics, so equal buffers give equal bits, and no pointer's alignment enters a sum.  The state key is ``momentum_buffer``: a checkpoint written
by ``torch.optim.SGD`` loads here and the other way round.  The tensors the kernels write (parameters, zeroed or scaled gradients) get their
autograd version counters advanced, as after torch's in-place operators.  The ctypes wrappers live here, not in ``ops`` (whose public names are a tested
table).  Not built: ``maximize``, ``differentiable``, sparse gradients, parameters that are not contiguous float32, momentum / dampening /
nesterov that differ between groups (lr and weight_decay may), norms other than 2.
"""
import ctypes
import math

import torch

from . import _lib, ops

CHUNK = 4096                    # AOC_MT_CHUNK
HAS_MOMENTUM = 1                # AOC_MT_HAS_MOMENTUM


class _MtTensor(ctypes.Structure):
    """aoc_mt_tensor"""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("momentum", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("chunk_begin", ctypes.c_int64), ("weight_decay", ctypes.c_float), ("flags", ctypes.c_int32)]


def chunk_prefix(sizes):
    """(chunk_begin of every tensor, n_chunks): a tensor of n floats owns ceil(n / CHUNK) chunks, an empty one none."""
    begins, at = [], 0
    for n in sizes:
        if n < 0:
            raise ValueError(f"a tensor of {n} elements")
        begins.append(at)
        at += (n + CHUNK - 1) // CHUNK
    return begins, at


# ------------------------------------------------------------------------------------------ the table and the C ABI
class TensorTable:
    """A device array of aoc_mt_tensor records and the host mirror the library validates a call against.  ``records``: tuples
    (param, grad, momentum, n, weight_decay, flags) of integer addresses (None: NULL).  ``keep`` holds whatever owns those addresses."""

    def __init__(self, records, device, keep=None):
        self.n_tensors = len(records)
        self.begins, self.n_chunks = chunk_prefix([r[3] for r in records])
        if self.n_chunks > 2 ** 31 - 1:
            raise ValueError(f"{self.n_chunks} chunks (at most 2^31 - 1)")
        self.host = (_MtTensor * max(self.n_tensors, 1))()
        for rec, begin, r in zip(self.host, self.begins, records):
            rec.param, rec.grad, rec.momentum, rec.n, rec.chunk_begin, rec.weight_decay, rec.flags = r[0], r[1], r[2], r[3], begin, r[4], r[5]
        self.device = device
        self.keep = keep
        self.fresh = []
        self.dev = None
        self.upload()

    def upload(self):
        """Pinned staging memory and a non-blocking copy.  The staging block is a fresh one per upload (torch's pinned allocator hands it out
        again only when the copy has run), and it is NOT the mirror: the library sets flags in the mirror right after it enqueues a step,
        which a copy still in flight must not see."""
        nbytes = ctypes.sizeof(self.host)
        stage = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        ctypes.memmove(stage.data_ptr(), ctypes.addressof(self.host), nbytes)
        if self.dev is None:
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.dev.copy_(stage, non_blocking=True)

    def args(self):
        return ctypes.c_void_p(self.dev.data_ptr()), ctypes.c_void_p(ctypes.addressof(self.host)), self.n_tensors, self.n_chunks


def _word(what, t, dtype=torch.float32):
    if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != 1 or not t.is_contiguous():
        raise ValueError(f"{what} must be a single {str(dtype).replace('torch.', '')} device word")
    return t


def grad_sumsq_partials(table, partial=None):
    """aoc_grad_sumsq_partials -> partial [n_chunks] float64"""
    if partial is None:
        partial = torch.empty(max(table.n_chunks, 1), dtype=torch.float64, device=table.device)
    elif partial.dtype != torch.float64 or not partial.is_contiguous() or partial.numel() < table.n_chunks:
        raise ValueError(f"grad_sumsq_partials: partial must be a contiguous float64 tensor of {table.n_chunks} elements")
    ops._need_gpu(table.dev, partial)
    _lib.check(_lib.lib().aoc_grad_sumsq_partials(*table.args(), ops._p(partial), ops._stream()), "aoc_grad_sumsq_partials")
    return partial


def grad_norm_finish(partial, n_chunks, max_norm, total_norm=None, coef=None):
    """aoc_grad_norm_finish -> (total_norm [1], coef [1]) on the device"""
    if partial.dtype != torch.float64 or not partial.is_contiguous() or partial.numel() < n_chunks:
        raise ValueError(f"grad_norm_finish: partial must be a contiguous float64 tensor of {n_chunks} elements")
    total_norm = torch.empty(1, device=partial.device) if total_norm is None else _word("grad_norm_finish: total_norm", total_norm)
    coef = torch.empty(1, device=partial.device) if coef is None else _word("grad_norm_finish: coef", coef)
    ops._need_gpu(partial, total_norm, coef)
    _lib.check(_lib.lib().aoc_grad_norm_finish(ops._p(partial), int(n_chunks), float(max_norm), ops._p(total_norm), ops._p(coef), ops._stream()),
               "aoc_grad_norm_finish")
    return total_norm, coef


def multi_tensor_scale(table, coef):
    """aoc_multi_tensor_scale: g *= coef[0] in place"""
    _word("multi_tensor_scale: coef", coef)
    ops._need_gpu(table.dev, coef)
    _lib.check(_lib.lib().aoc_multi_tensor_scale(*table.args(), ops._p(coef), ops._stream()), "aoc_multi_tensor_scale")


def multi_tensor_zero(table):
    """aoc_multi_tensor_zero: g = 0 in place"""
    ops._need_gpu(table.dev)
    _lib.check(_lib.lib().aoc_multi_tensor_zero(*table.args(), ops._stream()), "aoc_multi_tensor_zero")


def _lr_dev(table, lr_dev):
    if lr_dev is not None and (lr_dev.dtype != torch.float32 or not lr_dev.is_contiguous() or lr_dev.numel() != table.n_tensors):
        raise ValueError(f"lr_dev must be a contiguous float32 tensor of {table.n_tensors} elements")
    return lr_dev


def sgd_step(table, lr, momentum=0.0, dampening=0.0, nesterov=False, coef=None, lr_dev=None, zero_grad=False):
    """aoc_sgd_step: one update of every tensor of the table that has a gradient"""
    if coef is not None:
        _word("sgd_step: coef", coef)
    _lr_dev(table, lr_dev)
    ops._need_gpu(table.dev, coef, lr_dev)
    _lib.check(_lib.lib().aoc_sgd_step(*table.args(), ops._p(coef), float(lr), ops._p(lr_dev), float(momentum), float(dampening), int(bool(nesterov)),
                                       int(bool(zero_grad)), ops._stream()), "aoc_sgd_step")


def clip_sgd_step(table, max_norm, lr, momentum=0.0, dampening=0.0, nesterov=False, lr_dev=None, zero_grad=False, total_norm=None, workspace=None):
    """aoc_clip_sgd_step: the sums, the finish and the step as one call -> total_norm [1] on the device"""
    _lr_dev(table, lr_dev)
    total_norm = torch.empty(1, device=table.device) if total_norm is None else _word("clip_sgd_step: total_norm", total_norm)
    L = _lib.lib()
    ws = workspace if workspace is not None else ops._ws(L.aoc_clip_sgd_step_workspace_bytes(table.n_chunks), table.device)
    ops._need_gpu(table.dev, lr_dev, total_norm, ws)
    _lib.check(L.aoc_clip_sgd_step(*table.args(), float(max_norm), ops._p(total_norm), float(lr), ops._p(lr_dev), float(momentum), float(dampening),
                                   int(bool(nesterov)), int(bool(zero_grad)), ops._p(ws), ws.numel() * ws.element_size(), ops._stream()),
               "aoc_clip_sgd_step")
    return total_norm


# ------------------------------------------------------------------------------------------ the tensors a table may point at
def _check_param(p):
    if not torch.is_tensor(p) or p.dtype != torch.float32:
        raise ValueError(f"optim_train: parameters are float32 tensors, got {getattr(p, 'dtype', type(p))}")
    if p.is_sparse or not p.is_contiguous():
        raise ValueError("optim_train: a parameter must be dense and contiguous (the kernels walk it through its bare pointer)")


def _check_grad(p, g):
    if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
        raise ValueError(f"optim_train: the gradient of a {tuple(p.shape)} float32 parameter on {p.device} must be a dense contiguous float32 tensor "
                         f"of that shape on that device, got {tuple(g.shape)} {g.dtype} on {g.device}")


def _one_device(tensors):
    devs = {t.device for t in tensors}
    if len(devs) > 1:
        raise ValueError(f"optim_train: the parameters lie on several devices ({sorted(map(str, devs))}); one table describes one device")
    return devs.pop() if devs else None


def _written(*lists):
    """The kernels write through bare pointers: tell autograd that these tensors changed in place, as torch's own in-place operators do (a graph
    that saved one of them then refuses a late backward instead of using the new values)."""
    for tensors in lists:
        torch.autograd.graph.increment_version(tensors)


# ------------------------------------------------------------------------------------------ clip_grad_norm_
_CLIP_CACHE = {}                # one entry: the key of the last list of gradients -> its table


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """The drop-in for train_manager_mm.py:283 (torch.nn.utils.clip_grad_norm_): scales the gradients in place by
    min(1, max_norm / (total_norm + 1e-6)) and returns total_norm as a 0-d device tensor.  Three launches, no synchronisation unless
    ``error_if_nonfinite`` asks to read the norm back.  Only norm_type 2 is built; ``foreach`` is accepted and means nothing here."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_: norm_type {norm_type} is not built (only 2)")
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.zeros(())
    for p in params:
        _check_param(p)
        _check_grad(p, p.grad)
    device = _one_device(params)
    ops._need_gpu(*params)
    key = tuple((p.grad.data_ptr(), p.numel()) for p in params)
    table = _CLIP_CACHE.get(key)
    if table is None or table.device != device:
        _CLIP_CACHE.clear()
        table = _CLIP_CACHE[key] = TensorTable([(None, p.grad.data_ptr(), None, p.numel(), 0.0, 0) for p in params], device)
    table.keep = [p.grad for p in params]
    total_norm, coef = grad_norm_finish(grad_sumsq_partials(table), table.n_chunks, max_norm)
    if error_if_nonfinite and not bool(torch.isfinite(total_norm)):           # reads the norm back: synchronises
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped.")
    multi_tensor_scale(table, coef)
    _written(table.keep)
    table.keep = None
    return total_norm.view(())


# ------------------------------------------------------------------------------------------ the optimiser
class SGD(torch.optim.Optimizer):
    """``torch.optim.SGD`` (momentum, dampening, weight decay, Nesterov) with the gradient-norm clip folded in, over one tensor table.
    Takes torch's argument forms, the one-group-per-parameter list of ``get_trainable_params`` included; ``param_groups`` is the ordinary
    list (``adjust_learning_rate`` works on it), the state key is ``momentum_buffer``.  ``clip_grad_norm``: the max_norm of
    train_manager_mm.py:283, applied inside ``step``; ``self.total_norm`` is then the 0-d device tensor of the last step's norm."""

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, clip_grad_norm=None, maximize=False,
                 differentiable=False):
        if maximize or differentiable:
            raise ValueError("optim_train.SGD: maximize and differentiable are not built")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if clip_grad_norm is not None and not float(clip_grad_norm) > 0.0:
            raise ValueError(f"Invalid clip_grad_norm: {clip_grad_norm}")
        # the keys torch.optim.SGD keeps in a group, so that a checkpoint of either loads into the other
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False, foreach=None,
                        differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.clip_grad_norm = None if clip_grad_norm is None else float(clip_grad_norm)
        self.total_norm = None
        self.table_uploads = 0
        self._table = self._key = self._ws = self._lr_key = self._lr_vec = None
        _one_device([p for g in self.param_groups for p in g["params"]])

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            _check_param(p)
        _one_device([p for g in self.param_groups for p in g["params"]])

    # ---- the table
    def _hyper(self):
        """momentum, dampening, nesterov: one value each for the whole table"""
        first = self.param_groups[0]
        m, d, n = first["momentum"], first["dampening"], first["nesterov"]
        for g in self.param_groups:
            if g["momentum"] != m or g["dampening"] != d or g["nesterov"] != n:
                raise ValueError("optim_train.SGD: momentum, dampening and nesterov must agree between the groups, got "
                                 f"{(g['momentum'], g['dampening'], g['nesterov'])} beside {(m, d, n)}")
            if g.get("maximize") or g.get("differentiable"):
                raise ValueError("optim_train.SGD: maximize and differentiable are not built")
        return float(m), float(d), bool(n)

    def _scan(self, with_momentum):
        """One pass over the groups, the host's share of a step: the parameters that have a gradient with their gradients, the momentum buffers
        the state holds for them (None: not yet), weight decays and learning rates, and the key -- what the device table depends on."""
        ps, gs, bs, wds, lrs, key = [], [], [], [], [], [with_momentum]
        get = self.state.get
        for group in self.param_groups:
            wd, lr = float(group["weight_decay"]), float(group["lr"])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or not g.is_contiguous():
                    _check_grad(p, g)                         # raises; shape, dtype and device are held by torch when a gradient is assigned
                b = None
                if with_momentum:
                    st = get(p)
                    if st:
                        b = st.get("momentum_buffer")
                ps.append(p), gs.append(g), bs.append(b), wds.append(wd), lrs.append(lr)
                key.append((p.data_ptr(), g.data_ptr(), 0 if b is None else b.data_ptr(), p.numel(), wd))
        return ps, gs, bs, wds, lrs, key

    def _sync_table(self, scan):
        """The table of this scan, uploaded again only when a pointer, a size, a weight decay or a flag differs from the last one."""
        ps, gs, bs, wds, _, key = scan
        if key == self._key:
            return self._table
        with_momentum = key[0]
        fresh, records = [], []
        for p, g, b, wd in zip(ps, gs, bs, wds):
            _check_grad(p, g)
            if b is not None and (b.dtype != torch.float32 or not b.is_contiguous() or b.shape != p.shape or b.device != p.device):
                raise ValueError("optim_train.SGD: a momentum_buffer must be a contiguous float32 tensor of its parameter's shape and device")
            flags = HAS_MOMENTUM if b is not None else 0
            if with_momentum and b is None:
                b = torch.empty_like(p)                       # flags == 0: the first step writes it and reads nothing of it
                fresh.append((p, b))
            records.append((p.data_ptr(), g.data_ptr(), None if b is None else b.data_ptr(), p.numel(), wd, flags))
        device = ps[0].device
        self._key = None                                      # set by _stepped, once the new buffers are part of the state
        self._table = TensorTable(records, device)
        self._table.fresh = fresh
        self.table_uploads += 1
        self._ws = ops._ws(_lib.lib().aoc_clip_sgd_step_workspace_bytes(self._table.n_chunks), device)
        return self._table

    def _stepped(self, key):
        """The step is enqueued: the buffers allocated for it are state now (the library has set their flags in the table and in its mirror),
        and the next step's key is the one of this table."""
        table = self._table
        if table.fresh:
            for p, b in table.fresh:
                self.state[p]["momentum_buffer"] = b
            table.fresh = []
            key = self._scan(key[0])[-1]
        self._key = key

    def _lr(self, lrs, device):
        """(lr by value, None) when every tensor has the same, which is the reference's case; else (0, a device vector), uploaded when it changed"""
        first = lrs[0]
        for v in lrs:
            if v != first:
                break
        else:
            return first, None
        if lrs != self._lr_key:
            stage = torch.tensor(lrs, dtype=torch.float32).pin_memory()
            self._lr_vec = torch.empty(len(lrs), dtype=torch.float32, device=device)
            self._lr_vec.copy_(stage, non_blocking=True)
            self._lr_key = lrs
        return 0.0, self._lr_vec

    # ---- the step
    def step(self, closure=None, zero_grads=False):
        """One update.  ``zero_grads=True`` zeroes the gradients in the update pass itself and keeps their tensors, so the next step finds the
        same pointers and uploads nothing.  Nothing here synchronises with the device."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        momentum, dampening, nesterov = self._hyper()
        scan = self._scan(momentum != 0.0)
        ps, lrs, key = scan[0], scan[4], scan[5]
        if not ps:
            if self.clip_grad_norm is not None:
                self.total_norm = torch.zeros(())
            return loss
        ops._need_gpu(ps[0])                                  # one device for all of them: the constructor's rule
        table = self._sync_table(scan)
        lr, lr_dev = self._lr(lrs, ps[0].device)
        if self.clip_grad_norm is not None:
            self.total_norm = clip_sgd_step(table, self.clip_grad_norm, lr, momentum, dampening, nesterov, lr_dev, zero_grads, workspace=self._ws).view(())
        else:
            sgd_step(table, lr, momentum, dampening, nesterov, None, lr_dev, zero_grads)
        self._stepped(key)
        _written(ps, scan[1] if zero_grads else ())
        return loss

    def zero_grad(self, set_to_none=True):
        """torch's default drops the gradient tensors (the table is then rebuilt by the next step).  ``set_to_none=False`` keeps them and
        zeroes them with one launch."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        ps, gs = self._scan(False)[:2]
        if not ps:
            return
        ops._need_gpu(ps[0])
        grads = [(g.data_ptr(), g.numel()) for g in gs]
        table = self._table
        if table is None or self._key is None or [(k[1], k[3]) for k in self._key[1:]] != grads:
            table = TensorTable([(None, ptr, None, n, 0.0, 0) for ptr, n in grads], ps[0].device)
        multi_tensor_zero(table)
        _written(gs)


# ------------------------------------------------------------------------------------------ utils/learning.py (host Python)
def adjust_learning_rate(optimizer, base_lr, p, itr, max_itr, warm_up_steps=1000, is_cosine_decay=False, min_lr=1e-5):
    """utils/learning.py:4-21 with its signature and defaults: a linear warm-up over ``warm_up_steps``, then over the remaining steps the
    polynomial ``(1 - t / (T + 1)) ** p`` or the half cosine, floored at ``min_lr``; written into every group and returned."""
    if itr < warm_up_steps:
        lr = base_lr * itr / warm_up_steps
    else:
        t, total = itr - warm_up_steps, max_itr - warm_up_steps
        if is_cosine_decay:
            lr = base_lr * (math.cos(math.pi * t / (total + 1)) + 1.) * 0.5
        else:
            lr = base_lr * (1 - t / (total + 1)) ** p
    if lr < min_lr:
        lr = min_lr
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def get_trainable_params(model, base_lr, weight_decay, beta_wd=True):
    """utils/learning.py:24-34: one group per parameter that requires a gradient, in ``named_parameters`` order; a parameter whose name
    contains ``beta`` (the GCT gates) gets weight decay 0 when ``beta_wd`` is false."""
    groups = []
    for name, value in model.named_parameters():
        if value.requires_grad:
            wd = 0. if ("beta" in name and not beta_wd) else weight_decay
            groups.append({"params": [value], "lr": base_lr, "weight_decay": wd})
    return groups
