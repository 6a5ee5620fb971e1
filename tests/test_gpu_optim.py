"""The training update on the device (csrc/optim.hip, aoc_amd.optim_train; tests/optim_bounds.py holds the restatement, the references and the
bounds; tests/test_optim_host.py is the host half).

1. the entries through their wrappers, on tensors inside NaN-filled arenas at every misalignment: the update bit for bit the float32
   restatement at the coefficient the device produced, the chunk sums bit for bit the stated order, margins and skipped tensors untouched,
   the norm inside its bound, the same bits from two runs, from all four alignments and from aoc_clip_sgd_step;
2. the coefficient's edges; 3. the module against torch on the device, each inside the bound of a float64 reference at its own state;
4. gradient handling and the upload counter; 5. learning rates; 6. checkpoints both ways; 7. no synchronisation; 8. rejections.
"""
import io
import time

import numpy as np
import pytest
import torch
from torch import nn

import optim_bounds as ob
import stream_order_cases as soc
from aoc_amd import _lib
from aoc_amd import optim_train as ot

pytestmark = pytest.mark.gpu
f32 = np.float32
LR, MAX_NORM = 0.01, 5.0
MOM = dict(momentum=0.9, dampening=0.0, nesterov=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    _lib.lib()
    return torch.device("cuda", torch.cuda.current_device())


def same_bits(a, b):
    """equal bit for bit, except that a NaN equals any NaN (the host's 0 * inf and the device's differ in the sign bit)"""
    a, b = np.ascontiguousarray(a, f32).reshape(-1), np.ascontiguousarray(b, f32).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.int32)[~na] == b.view(np.int32)[~na]).all())


# ------------------------------------------------------------------------------------------ arenas
class Arena:
    """tensors of the given sizes inside one NaN-filled device buffer, each starting `off` floats behind the 16-byte grid, with NaN margins"""

    def __init__(self, sizes, off, dev, values=None):
        self.sizes, self.starts, at = list(sizes), [], 8
        for n in sizes:
            at = (at + 3) // 4 * 4 + off
            self.starts.append(at)
            at += n + 5
        self.host = np.full(at + 8, np.nan, f32)
        if values is not None:
            for s, n, v in zip(self.starts, sizes, values):
                if v is not None:
                    self.host[s:s + n] = v
        self.dev = torch.from_numpy(self.host).to(dev)
        assert self.dev.data_ptr() % 16 == 0
        assert all((self.ptr(i) % 16) == 4 * off for i in range(len(sizes)))

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.starts[i]

    def read(self):
        return self.dev.cpu().numpy()

    def expect(self, values):
        """the arena as it must look when tensor i holds values[i] (None: what it held at the start) and nothing else was written"""
        out = self.host.copy()
        for s, n, v in zip(self.starts, self.sizes, values):
            if v is not None:
                out[s:s + n] = v
        return out

    def tensors(self, flat):
        return [flat[s:s + n] for s, n in zip(self.starts, self.sizes)]


LISTS = {1: (4097,), 2: (8193, 0), 37: tuple((ob.SIZES * 3)[:37]), 700: tuple((5 * i) % 9 for i in range(700))}
OFFSETS = {0: (0, 0, 0), 1: (1, 2, 0), 2: (2, 3, 1), 3: (3, 1, 2)}          # by the gradient's misalignment: (grad, param, buffer) in floats


class Case:
    """one list: host values, which tensors have a gradient and which a filled buffer"""

    def __init__(self, count, seed=5, scale=1.0):
        self.sizes = LISTS[count]
        n = len(self.sizes)
        self.g, self.p = ob.make_list(self.sizes, seed, scale)
        self.b = ob.make_list(self.sizes, seed + 1)[0]
        self.has_g = [not (n >= 4 and i % 5 == 3) for i in range(n)]
        self.has_b = [i % 2 == 0 for i in range(n)]
        self.wd = [0.0 if i % 3 == 2 else 1e-4 for i in range(n)]                 # every third tensor a `beta`; the first one decays

    def build(self, off, dev):
        og, op, ob_ = OFFSETS[off]
        ga = Arena(self.sizes, og, dev, [g if h else None for g, h in zip(self.g, self.has_g)])
        pa = Arena(self.sizes, op, dev, self.p)
        ba = Arena(self.sizes, ob_, dev, [b if h else None for b, h in zip(self.b, self.has_b)])       # no value yet: the buffer holds NaN
        records = [(pa.ptr(i), ga.ptr(i) if self.has_g[i] else None, ba.ptr(i), self.sizes[i], self.wd[i], ot.HAS_MOMENTUM if self.has_b[i] else 0)
                   for i in range(len(self.sizes))]
        return ga, pa, ba, ot.TensorTable(records, dev, keep=(ga, pa, ba))

    def grads(self):
        return [g if h else None for g, h in zip(self.g, self.has_g)]

    def expected(self, coef, zero_grad=False, **mode):
        mode = mode or MOM
        ps, bs, gs = [], [], []
        for g, p, b, hg, hb, wd in zip(self.g, self.p, self.b, self.has_g, self.has_b, self.wd):
            if not hg:
                ps.append(None), bs.append(None), gs.append(None)
                continue
            p2, b2 = ob.step32(g, p, b if hb else None, coef, wd, LR, mode["momentum"], mode["dampening"], mode["nesterov"])
            ps.append(p2), bs.append(b2), gs.append(np.zeros_like(g) if zero_grad else None)
        return ps, bs, gs


def _table_bytes(table):
    import ctypes
    return bytes(table.dev.cpu().numpy()), ctypes.string_at(ctypes.addressof(table.host), ctypes.sizeof(table.host))


@pytest.mark.parametrize("count", sorted(LISTS))
def test_entries_bit_for_bit_at_every_alignment(dev, count):
    case = Case(count)
    want_partial = ob.partials32(case.grads(), case.sizes)
    S, dS, N, dN = ob.norm_ref(case.grads(), case.sizes)
    seen = {}
    for off in sorted(OFFSETS):
        ga, pa, ba, table = case.build(off, dev)
        assert table.n_chunks == ob.chunk_prefix(case.sizes)[1] == want_partial.size
        partial = ot.grad_sumsq_partials(table)
        norm, coef = ot.grad_norm_finish(partial, table.n_chunks, MAX_NORM)
        ot.sgd_step(table, LR, coef=coef, **MOM)
        got_partial = partial.cpu().numpy()[:table.n_chunks]
        assert np.array_equal(got_partial.view(np.int64), want_partial.view(np.int64)), f"offset {off}: the chunk sums are not in the stated order"
        norm_h, coef_h = f32(norm.item()), f32(coef.item())
        assert abs(float(norm_h) - N) <= dN, f"offset {off}: total_norm {norm_h} against {N} +- {dN}"
        c = f32(MAX_NORM) / (norm_h + f32(1e-6))
        assert coef_h == (f32(1.0) if c > 1 else c) and coef_h < 1
        ps, bs, _ = case.expected(coef_h)
        assert same_bits(pa.read(), pa.expect(ps)), f"offset {off}: parameters (or their margins, or a skipped tensor)"
        assert same_bits(ba.read(), ba.expect(bs)), f"offset {off}: momentum buffers (or their margins, or a skipped tensor)"
        assert same_bits(ga.read(), ga.host), f"offset {off}: the gradients were written without zero_grad"
        dev_bytes, host_bytes = _table_bytes(table)
        assert dev_bytes == host_bytes, "the host mirror no longer describes the device table"
        assert all(bool(r.flags & 1) == (hb or (hg and n > 0)) for r, hb, hg, n in zip(table.host, case.has_b, case.has_g, case.sizes))
        # the same buffers again: the same bits; then aoc_clip_sgd_step on a fresh copy, with the gradients zeroed in the pass
        ga2, pa2, ba2, table2 = case.build(off, dev)
        p2 = ot.grad_sumsq_partials(table2)
        n2, c2 = ot.grad_norm_finish(p2, table2.n_chunks, MAX_NORM)
        ot.sgd_step(table2, LR, coef=c2, **MOM)
        ga3, pa3, ba3, table3 = case.build(off, dev)
        n3 = ot.clip_sgd_step(table3, MAX_NORM, LR, zero_grad=True, **MOM)
        for what, a, b in (("partial", p2, partial), ("norm", n2, norm), ("coef", c2, coef), ("params", pa2.dev, pa.dev), ("buffers", ba2.dev, ba.dev),
                           ("fused norm", n3, norm), ("fused params", pa3.dev, pa.dev), ("fused buffers", ba3.dev, ba.dev)):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64),
                               b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64)), f"offset {off}: {what} differs between runs"
        assert same_bits(ga3.read(), ga3.expect(case.expected(coef_h, zero_grad=True)[2])), f"offset {off}: zero_grad"
        seen[off] = (got_partial, norm_h, pa.tensors(pa.read()), ba.tensors(ba.read()))
    for off in seen:
        assert np.array_equal(seen[off][0], seen[0][0]) and seen[off][1] == seen[0][1], f"the norm depends on the alignment ({off})"
        for a, b in zip(seen[off][2] + seen[off][3], seen[0][2] + seen[0][3]):
            assert same_bits(a, b), f"the update depends on the alignment ({off})"


@pytest.mark.parametrize("mode", ["momentum", "plain", "dampening"])
def test_entries_other_modes_and_scale(dev, mode):
    m = {k: v for k, v in ob.MODES[mode].items() if k != "wd"}
    case = Case(37, seed=9)
    ga, pa, ba, table = case.build(1, dev)
    partial = ot.grad_sumsq_partials(table)
    norm, coef = ot.grad_norm_finish(partial, table.n_chunks, MAX_NORM)
    ot.sgd_step(table, LR, coef=coef, **m)
    ps, bs, _ = case.expected(f32(coef.item()), **m)
    assert same_bits(pa.read(), pa.expect(ps))
    assert same_bits(ba.read(), ba.expect(bs if m["momentum"] else [None] * len(bs))), "momentum == 0 leaves every buffer alone"
    assert all(bool(r.flags & 1) == (hb or (m["momentum"] != 0 and hg and n > 0)) for r, hb, hg, n in zip(table.host, case.has_b, case.has_g, case.sizes))
    # the stand-alone scale and the zeroing
    ot.multi_tensor_scale(table, coef)
    want = [None if g is None else g * f32(coef.item()) for g in case.grads()]
    assert same_bits(ga.read(), ga.expect(want))
    ot.multi_tensor_zero(table)
    assert same_bits(ga.read(), ga.expect([None if g is None else np.zeros_like(g) for g in case.grads()]))


# ------------------------------------------------------------------------------------------ 2: the coefficient's edges
def _run(case, dev, max_norm, off=2):
    ga, pa, ba, table = case.build(off, dev)
    norm = ot.clip_sgd_step(table, max_norm, LR, **MOM)
    return f32(norm.item()), pa, ba


def test_coefficient_edges(dev):
    zero = Case(37)
    zero.g = [np.zeros_like(g) for g in zero.g]
    partial = ot.grad_sumsq_partials(zero.build(0, dev)[3])
    norm, coef = ot.grad_norm_finish(partial, ob.chunk_prefix(zero.sizes)[1], MAX_NORM)
    assert norm.item() == 0.0 and coef.item() == 1.0
    # a norm below max_norm: the coefficient is exactly 1 and the update that of aoc_sgd_step without one
    small = Case(37, scale=1e-3)
    ga, pa, ba, table = small.build(2, dev)
    partial = ot.grad_sumsq_partials(table)
    norm, coef = ot.grad_norm_finish(partial, table.n_chunks, MAX_NORM)
    assert 0 < norm.item() < MAX_NORM and coef.item() == 1.0
    ot.sgd_step(table, LR, coef=coef, **MOM)
    ga2, pa2, ba2, table2 = small.build(2, dev)
    ot.sgd_step(table2, LR, coef=None, **MOM)
    assert torch.equal(pa.dev.view(torch.int32), pa2.dev.view(torch.int32)) and torch.equal(ba.dev.view(torch.int32), ba2.dev.view(torch.int32))
    ps, bs, _ = small.expected(f32(1.0))
    assert same_bits(pa.read(), pa.expect(ps)) and same_bits(ba.read(), ba.expect(bs))
    # a norm above it
    big = Case(37)
    norm_h, pa, ba = _run(big, dev, MAX_NORM)
    assert norm_h > MAX_NORM
    c = f32(MAX_NORM) / (norm_h + f32(1e-6))
    ps, bs, _ = big.expected(c)
    assert c < 1 and same_bits(pa.read(), pa.expect(ps)) and same_bits(ba.read(), ba.expect(bs))


def test_one_infinite_gradient_element(dev):
    case = Case(37)
    case.has_g = [True] * len(case.sizes)
    case.g[4][2] = np.inf
    norm_h, pa, ba = _run(case, dev, MAX_NORM)
    assert np.isinf(norm_h)
    ps, bs, _ = case.expected(f32(0.0))                     # max_norm / inf
    assert same_bits(pa.read(), pa.expect(ps)) and same_bits(ba.read(), ba.expect(bs))
    # NaN exactly where torch's clip_grad_norm_ + SGD gives NaN
    tp = [nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in case.p]
    topt = torch.optim.SGD([{"params": [p], "weight_decay": wd} for p, wd in zip(tp, case.wd)], lr=LR, **MOM)
    for i, p in enumerate(tp):
        p.grad = torch.from_numpy(case.g[i].copy()).to(dev)
        if case.has_b[i]:
            topt.state[p]["momentum_buffer"] = torch.from_numpy(case.b[i].copy()).to(dev)
    torch.nn.utils.clip_grad_norm_(tp, MAX_NORM)
    topt.step()
    mine = pa.tensors(pa.read())
    for i, p in enumerate(tp):
        assert np.array_equal(np.isnan(p.detach().cpu().numpy()), np.isnan(mine[i])), f"tensor {i}: NaN where torch has none, or the other way round"
    assert sum(int(np.isnan(m).sum()) for m in mine) == 1


# ------------------------------------------------------------------------------------------ 3: the module against torch
class _Gate(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.alpha, self.gamma, self.beta = nn.Parameter(torch.ones(1, c, 1, 1)), nn.Parameter(torch.zeros(1, c, 1, 1)), nn.Parameter(torch.zeros(1, c, 1, 1))


class Toy(nn.Module):
    def __init__(self, frozen):
        super().__init__()
        self.conv = nn.Conv2d(3, 64, 3)
        self.gct = _Gate(24)
        self.wide = nn.Linear(65, 128)                         # 8320 weights: three chunks, the last one short
        self.empty = nn.Parameter(torch.zeros(0))
        self.odd = nn.Parameter(torch.zeros(4097))
        if frozen:
            self.cold = nn.Parameter(torch.zeros(33))          # trainable, but never given a gradient
            self.conv.bias.requires_grad_(False)


def _toy(seed, frozen, dev):
    torch.manual_seed(seed)
    toy = Toy(frozen)
    with torch.no_grad():
        for p in toy.parameters():
            p.copy_(torch.randn_like(p))
    return toy.to(dev)


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _state(opt, params):
    return [_np(p) for p in params], [_np(opt.state[p].get("momentum_buffer")) if p in opt.state else None for p in params]


def _give_grads(params, seed, scale, skip=()):
    torch.manual_seed(seed)
    out = []
    for p in params:
        g = torch.randn(p.shape) * scale
        out.append(None if id(p) in skip else g)
    return out


def _inside(opt, params, before, grads, wds, lrs, norm, mode, what, max_norm=MAX_NORM):
    """params, buffers and the norm after a step against the float64 reference at the state before it"""
    p0, b0 = before
    N, dN, coef, ref = ob.clip_sgd_ref([_np(g) for g in grads], p0, b0, wds, lrs, max_norm, mode["momentum"], mode["dampening"], mode["nesterov"])
    if norm is not None:
        assert abs(float(norm) - N) <= dN, f"{what}: norm {float(norm)} against {N} +- {dN}"
    p1, b1 = _state(opt, params)
    worst = 0.0
    for i, r in enumerate(ref):
        if r is None:
            assert np.array_equal(p1[i], p0[i]) and b1[i] is None and b0[i] is None, f"{what}: a parameter without a gradient was touched or got state"
            continue
        worst = max(worst, ob.check(p1[i], r[0].v, r[0].e))
        if r[1] is not None:
            worst = max(worst, ob.check(b1[i], r[1].v, r[1].e))
    assert worst <= 1.0, f"{what}: {worst:.3f} of the bound"
    return coef.v


@pytest.mark.parametrize("frozen", [False, True])
def test_module_against_torch_on_the_device(dev, frozen):
    mine_m, torch_m = _toy(3, frozen, dev), _toy(3, frozen, dev)
    opts = []
    for model, make in ((mine_m, lambda g: ot.SGD(g, lr=LR, clip_grad_norm=MAX_NORM, **MOM)), (torch_m, lambda g: torch.optim.SGD(g, lr=LR, **MOM))):
        groups = ot.get_trainable_params(model, LR, 1e-4, beta_wd=False)                  # one group per parameter, the betas at wd = 0
        assert len(groups) == sum(p.requires_grad for p in model.parameters()) and any(g["weight_decay"] == 0.0 for g in groups)
        opts.append((make(groups), [g["params"][0] for g in groups], [g["weight_decay"] for g in groups]))
    skip_names = {"cold"} if frozen else set()
    for step, scale in enumerate((1.0, 0.5, 1e-4)):                                       # the first step, a clipped one, an unclipped one
        for k, (opt, params, wds) in enumerate(opts):
            names = {id(p): n for n, p in (mine_m if k == 0 else torch_m).named_parameters()}
            grads = _give_grads(params, 40 + step, scale, skip={id(p) for p in params if names[id(p)] in skip_names})
            for p, g in zip(params, grads):
                p.grad = None if g is None else g.to(dev)
            before = _state(opt, params)
            if k == 0:
                opt.step()
                norm = opt.total_norm
                assert norm.dim() == 0 and norm.is_cuda
            else:
                norm = torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], MAX_NORM)
                opt.step()
            c = _inside(opt, params, before, grads, wds, [LR] * len(params), norm.item(), MOM, f"{'mine' if k == 0 else 'torch'} step {step}")
            assert (c < 1.0) == (step < 2)
    if frozen:
        assert torch.equal(mine_m.conv.bias, torch_m.conv.bias) and torch.equal(mine_m.cold, torch_m.cold)      # untouched by either
        assert mine_m.cold not in opts[0][0].state or not opts[0][0].state[mine_m.cold]


def test_drop_in_clip_grad_norm(dev):
    mine_m, torch_m = _toy(4, False, dev), _toy(4, False, dev)
    for scale, clipped in ((1.0, True), (1e-4, False)):
        for model in (mine_m, torch_m):
            for p, g in zip(model.parameters(), _give_grads(list(model.parameters()), 77, scale)):
                p.grad = g.to(dev)
        grads = [_np(p.grad) for p in mine_m.parameters()]
        got = ot.clip_grad_norm_(mine_m.parameters(), MAX_NORM)
        want = torch.nn.utils.clip_grad_norm_(torch_m.parameters(), MAX_NORM)
        _, _, N, dN = ob.norm_ref(grads)
        assert got.dim() == 0 and got.is_cuda and abs(got.item() - N) <= dN and abs(want.item() - N) <= dN
        c = f32(MAX_NORM) / (f32(got.item()) + f32(1e-6))
        c = f32(1.0) if c > 1 else c
        assert (c < 1) == clipped
        for p, g in zip(mine_m.parameters(), grads):
            assert same_bits(_np(p.grad), g * c)
    mine_m.odd.grad[7] = float("inf")
    with pytest.raises(RuntimeError):
        ot.clip_grad_norm_(mine_m.parameters(), MAX_NORM, error_if_nonfinite=True)


# ------------------------------------------------------------------------------------------ 4, 5: gradients, uploads, learning rates
def _fresh(dev, seed=6, sizes=((33, 7), (4097,), (0,), (5,)), **kw):
    torch.manual_seed(seed)
    params = [nn.Parameter(torch.randn(s).to(dev)) for s in sizes]
    groups = [{"params": [p], "weight_decay": wd} for p, wd in zip(params, (1e-4, 0.0, 1e-4, 1e-4))]
    return params, ot.SGD(groups, lr=LR, **{**MOM, **kw})


def _grads_for(params, step, dev):
    torch.manual_seed(500 + step)
    return [torch.randn(p.shape).to(dev) for p in params]


def test_gradient_handling_and_upload_counter(dev):
    # kept pointers: zeroed by the update pass itself, one upload over three steps
    pa, a = _fresh(dev, clip_grad_norm=MAX_NORM)
    for p, g in zip(pa, _grads_for(pa, 0, dev)):
        p.grad = g
    ptrs = [p.grad.data_ptr() for p in pa]
    for step in range(3):
        if step:
            for p, g in zip(pa, _grads_for(pa, step, dev)):
                p.grad.copy_(g)
        a.step(zero_grads=True)
        assert all(not p.grad.any() for p in pa) and [p.grad.data_ptr() for p in pa] == ptrs
    assert a.table_uploads == 1
    assert all(p._version >= 3 and p.grad._version >= 3 for p in pa), "autograd was not told that the kernels wrote the parameters and the gradients"
    # torch's default zero_grad(): the tensors go, the table is rebuilt, the results are the same bits
    pb, b = _fresh(dev, clip_grad_norm=MAX_NORM)
    held = []
    for step in range(3):
        grads = _grads_for(pb, step, dev)
        held.append(grads)                                                  # kept alive: the next step's gradients cannot land on these addresses
        for p, g in zip(pb, grads):
            p.grad = g
        b.step()
        b.zero_grad()
        assert all(p.grad is None for p in pb)
    assert b.table_uploads == 3
    for p, q in zip(pa, pb):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)) and torch.equal(a.state[p]["momentum_buffer"], b.state[q]["momentum_buffer"])
    assert torch.equal(a.total_norm, b.total_norm)
    # zero_grad(set_to_none=False): one launch, the tensors stay
    for p, g in zip(pa, _grads_for(pa, 9, dev)):
        p.grad.copy_(g)
    a.zero_grad(set_to_none=False)
    assert all(not p.grad.any() for p in pa) and [p.grad.data_ptr() for p in pa] == ptrs and a.table_uploads == 1


def test_learning_rates(dev):
    params, opt = _fresh(dev)                                               # no clip: the coefficient is exactly 1
    state_p, state_b = [_np(p) for p in params], [None] * len(params)
    wds = [g["weight_decay"] for g in opt.param_groups]
    for p, g in zip(params, _grads_for(params, 0, dev)):
        p.grad = g
    plans = (lambda: ot.adjust_learning_rate(opt, LR, 0.9, 500, 50000), lambda: ot.adjust_learning_rate(opt, LR, 0.9, 30000, 50000, is_cosine_decay=True),
             lambda: [g.__setitem__("lr", 0.02 * (i + 1)) for i, g in enumerate(opt.param_groups)],          # a vector of learning rates
             lambda: opt.param_groups[1].__setitem__("lr", 0.5))
    for step, plan in enumerate(plans):
        plan()
        lrs = [g["lr"] for g in opt.param_groups]
        assert (len(set(lrs)) == 1) == (step < 2)
        if step:
            for p, g in zip(params, _grads_for(params, step, dev)):
                p.grad.copy_(g)
        grads = [_np(p.grad) for p in params]
        opt.step(zero_grads=True)
        for i, p in enumerate(params):
            state_p[i], state_b[i] = ob.step32(grads[i], state_p[i], state_b[i], f32(1.0), wds[i], lrs[i], **MOM)
            assert same_bits(_np(p), state_p[i]) and same_bits(_np(opt.state[p]["momentum_buffer"]), state_b[i]), f"step {step}, tensor {i}"
    assert opt.table_uploads == 1 and opt.total_norm is None, "a learning rate is no reason to upload the table again"


# ------------------------------------------------------------------------------------------ 6: checkpoints
def _through_a_file(state_dict):
    buf = io.BytesIO()
    torch.save(state_dict, buf)
    buf.seek(0)
    return torch.load(buf)


@pytest.mark.parametrize("direction", ["torch_to_here", "here_to_torch"])
def test_checkpoint_interop(dev, direction):
    def make(kind, params):
        groups = [{"params": [p], "weight_decay": wd} for p, wd in zip(params, (1e-4, 0.0, 1e-4, 1e-4))]
        return ot.SGD(groups, lr=LR, **MOM) if kind == "here" else torch.optim.SGD(groups, lr=LR, **MOM)

    first, second = ("torch", "here") if direction == "torch_to_here" else ("here", "torch")
    pa, _ = _fresh(dev, seed=8)
    a = make(first, pa)
    for p, g in zip(pa, _grads_for(pa, 0, dev)):
        p.grad = g
    a.step()
    pb = [nn.Parameter(p.detach().clone()) for p in pa]
    b = make(second, pb)
    b.load_state_dict(_through_a_file(a.state_dict()))
    wds = [g["weight_decay"] for g in a.param_groups]
    for opt, params, what in ((a, pa, first + " continuing"), (b, pb, second + " from the checkpoint")):
        grads = _grads_for(params, 1, dev)
        for p, g in zip(params, grads):
            p.grad = g.clone()                                               # torch's Nesterov step adds the buffer into the gradient in place
        before = _state(opt, params)
        assert all(x is not None for x, p in zip(before[1], params))
        opt.step()
        _inside(opt, params, before, grads, wds, [LR] * len(params), None, MOM, what, max_norm=None)
    # both started this step from the same state and lie inside the bound of the same reference: within twice the bound of each other


# ------------------------------------------------------------------------------------------ 7: no synchronisation
def test_step_does_not_synchronise(dev):
    def run(stall_ms, cycles_per_ms):
        params, opt = _fresh(dev, seed=12, clip_grad_norm=MAX_NORM)
        opt.param_groups[2]["lr"] = 0.5 * LR                                # the vector path: its upload must not synchronise either
        for p, g in zip(params, _grads_for(params, 0, dev)):
            p.grad = g
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        if stall_ms:
            torch.cuda._sleep(int(stall_ms * cycles_per_ms))
        ev.record()
        t0 = time.perf_counter()
        opt.step(zero_grads=True)                                           # builds and uploads the table, allocates the buffers, three launches
        opt.step(zero_grads=True)
        t_enq = time.perf_counter() - t0
        stalled = not ev.query()
        torch.cuda.synchronize()
        return [p.detach().clone() for p in params], opt.total_norm.clone(), t_enq, stalled

    cpm = soc.calibrate_cycles_per_ms()
    run(0, cpm)                                                             # loads the kernels, fills the allocators' caches
    want, want_norm, t_enq, _ = run(0, cpm)
    stall_ms = max(soc.STALL_MIN_MS, soc.STALL_T_ENQ_FACTOR * t_enq * 1e3)
    assert stall_ms <= soc.STALL_MAX_MS, f"two steps took {t_enq * 1e3:.1f} ms on the host"
    got, got_norm, _, stalled = run(stall_ms, cpm)
    assert stalled, "step() returned only after the spin in front of it was over: something in it waits for the device"
    assert torch.equal(got_norm, want_norm) and all(torch.equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------ 8: rejections
def test_rejections_leave_the_buffers_alone(dev):
    sizes = (5, 4097)
    g, p, b = (Arena(sizes, 1, dev, [np.full(n, 7.0, f32) for n in sizes]) for _ in range(3))
    table = ot.TensorTable([(p.ptr(i), g.ptr(i), b.ptr(i), n, 1e-4, 1) for i, n in enumerate(sizes)], dev, keep=(g, p, b))
    word = torch.ones(1, device=dev)
    with pytest.raises(_lib.AocHipError, match="AOC_ERR_INVALID_ARG"):
        ot.sgd_step(table, LR, momentum=0.0, nesterov=True)
    with pytest.raises(_lib.AocHipError, match="AOC_ERR_INVALID_ARG"):
        ot.sgd_step(table, LR, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(_lib.AocHipError, match="AOC_ERR_INVALID_ARG"):
        ot.clip_sgd_step(table, MAX_NORM, LR, momentum=-0.9)
    with pytest.raises(_lib.AocHipError, match="AOC_ERR_WORKSPACE"):
        ot.clip_sgd_step(table, MAX_NORM, LR, momentum=0.9, workspace=torch.empty(8, dtype=torch.uint8, device=dev))
    for wrong in (torch.ones(1, dtype=torch.float64, device=dev), torch.ones(2, device=dev)):
        with pytest.raises(ValueError):
            ot.sgd_step(table, LR, coef=wrong)
        with pytest.raises(ValueError):
            ot.multi_tensor_scale(table, wrong)
    with pytest.raises(ValueError):
        ot.sgd_step(table, LR, lr_dev=torch.ones(3, device=dev))
    with pytest.raises(ValueError):
        ot.grad_sumsq_partials(table, torch.empty(1, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.AocHipError):
        ot.sgd_step(table, LR, coef=torch.ones(1))                          # a host tensor
    table.host[1].chunk_begin = 2                                           # the mirror says the prefix is wrong
    for call in (lambda: ot.sgd_step(table, LR, momentum=0.9), lambda: ot.clip_sgd_step(table, MAX_NORM, LR, momentum=0.9), lambda: ot.multi_tensor_zero(table),
                 lambda: ot.multi_tensor_scale(table, word), lambda: ot.grad_sumsq_partials(table)):
        with pytest.raises(_lib.AocHipError, match="AOC_ERR_INVALID_ARG"):
            call()
    table.host[1].chunk_begin = 1
    table.host[0].n = -5
    with pytest.raises(_lib.AocHipError, match="AOC_ERR_INVALID_ARG"):
        ot.sgd_step(table, LR, momentum=0.9)
    torch.cuda.synchronize()
    for arena in (g, p, b):
        assert same_bits(arena.read(), arena.host), "a rejected call wrote something"
    pr, opt = _fresh(dev)
    pr[0].grad = torch.ones(7, 33, device=dev).t()                          # not contiguous
    with pytest.raises(ValueError):
        opt.step()
    assert not opt.state[pr[0]] and opt.table_uploads == 0
