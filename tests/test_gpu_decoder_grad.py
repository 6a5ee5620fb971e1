"""The differentiable decoder forms on the device: the two entry points of csrc/norm_grad.hip through their wrappers, and the twins of
aoc_amd.decoder_train through ``backward()``, against the float64 references and derived bounds of tests/decoder_grad_bounds.py.  The module
tests record what every wrapper received and returned during the backward (the tape of tests/test_gpu_gates_grad.py, extended by this
module's wrappers), hold each call to its float64 reference AT THOSE TENSORS and read the wiring off the tape, so no tolerance is added for
the chain; the convolutions are torch's.  Each test prints its largest error / bound per output before it asserts."""
import numpy as np
import pytest
import torch
from torch import nn

import aoc_amd
import decoder_grad_bounds as dgb
import gates_grad_bounds as ggb
import test_gpu_gates_grad as tgg
from aoc_amd import _lib, decoder_memory, decoder_train as dt, gates_train as gt, gct, ops
from test_gpu_gates_grad import DEV, FROM, dev, margins, shifted, untouched, _np

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
INVALID, WORKSPACE, UNSUPPORTED = "AOC_ERR_INVALID_ARG", "AOC_ERR_WORKSPACE", "AOC_ERR_UNSUPPORTED"
WORST = {}


def held(entry, got, want_tol, what):
    want, tol = want_tol
    r = ggb.check(_np(got), want, tol, what)
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, f"{what}: error / bound {r:.3f}"
    return r


def worst(prefix):
    return ", ".join(f"{k[len(prefix):]} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith(prefix))


# ------------------------------------------------------------------------------------------ 1 aoc_groupnorm_relu_grad
def _gn_device(s, variant, groups, off):
    """one variant of a case on the device, every buffer `off` floats past a 16-byte boundary -> the wrapper's positional arguments"""
    res, relu, gain, affine = variant
    x = shifted(s["x"], off)
    r = shifted(s["residual"], off) if res else None
    w, b = (shifted(s["weight"], off), shifted(s["bias"], off)) if affine else (None, None)
    _, stats = dt.groupnorm_relu_forward(x, groups, w, b, 1e-5, r, relu)
    return [shifted(s["grad_y"], off), x, shifted(_np(stats), off), groups, w, b, r, relu, shifted(s["gain"], off) if gain else None]


def _gn_shapes(N, C, hw):
    return {"grad_x": (N, C, hw), "grad_residual": (N, C, hw), "grad_gamma": (C,), "grad_beta": (C,), "dgain": (N, C)}


@pytest.mark.parametrize("N,C,groups,hw", tuple(dgb.GN_CASES))
def test_groupnorm_relu_grad(N, C, groups, hw):
    s = dgb.gn_case(N, C, groups, hw)
    shapes = _gn_shapes(N, C, hw)
    for variant in dgb.GN_VARIANTS:
        ref, und = dgb.groupnorm_relu_grad_ref(**dgb.gn_args(s, variant, groups))
        assert int(und.sum()) == 0
        for off in (0, 1):
            args = _gn_device(s, variant, groups, off)
            held("gn stats", args[2], dgb.stats_ref(s["x"], groups, 1e-5), "the forward's statistics")
            runs = []
            for _ in range(2):
                bufs = {k: margins(shape, off) for k, shape in shapes.items()}
                got = dt.groupnorm_relu_backward(*args, want=(True,) * 5, out={k: v for k, (_, v) in bufs.items()})
                assert all(g is bufs[k][1] for g, k in zip(got, dgb.GN_OUTS)) and all(untouched(bufs[k][0], shapes[k], off) for k in shapes), \
                    "written outside the outputs"
                runs.append([g.clone() for g in got])
            what = f"groupnorm_relu_grad {N},{C},{groups},{hw} {variant} off={off}"
            for k, (name, a, b) in enumerate(zip(dgb.GN_OUTS, *runs)):
                assert torch.equal(a, b), f"{what} {name}: two runs differ"
                held("gn " + name, a, ref[name], f"{what} {name}")
                alone = dt.groupnorm_relu_backward(*args, want=tuple(j == k for j in range(5)))       # each output alone: the same bits
                assert all((g is None) == (j != k) for j, g in enumerate(alone)) and torch.equal(alone[k], a), f"{what}: {name} alone differs"
    print(f"groupnorm_relu_grad {N},{C},{groups},{hw}: worst error / bound so far: {worst('gn ')}")


def test_groupnorm_relu_grad_planted():
    N, C, groups, hw = 2, 64, 32, 35
    s = dgb.gn_case(N, C, groups, hw, seed=11)
    s["weight"][5] = s["bias"][5] = 0.0                                       # z is exactly 0 on channel 5 of sample 0 (residual 0 there)
    s["residual"][0, 5] = 0.0
    s["gain"][1, :] = 0.0                                                     # a whole sample gated off: no gradient reaches x
    s["x"][0, 8:10] = 3.25                                                    # a group (channels 8, 9) whose channels are constant: var = 0
    variant = (True, True, True, True)
    ref, und = dgb.groupnorm_relu_grad_ref(**dgb.gn_args(s, variant, groups))
    assert int(und.sum()) <= dgb.MASK_CAP * und.numel()
    args = _gn_device(s, variant, groups, 0)
    gx, gr, gg, gb, dg = dt.groupnorm_relu_backward(*args)
    for name, g in zip(dgb.GN_OUTS, (gx, gr, gg, gb, dg)):
        held("gn planted " + name, g, ref[name], "planted " + name)
    assert float(gr[0, 5].abs().max()) == 0.0, "z == 0 exactly: the mask is off (torch's > 0) and grad_residual is exactly 0"
    assert float(gx[1].abs().max()) == 0.0 and float(gr[1].abs().max()) == 0.0, "gain == 0.0: grad_x and grad_residual are exactly 0"
    assert float(dg[0, 5].abs()) == 0.0
    stats = _np(args[2]).reshape(N, groups, 2)
    assert stats[0, 4, 0] == f32(3.25) and abs(stats[0, 4, 1] - 1e-5 ** -0.5) <= 1e-4 * 1e-5 ** -0.5, "a constant group: mean exact, rstd = eps^-1/2"
    assert bool(torch.isfinite(gx).all())
    print(f"groupnorm_relu_grad planted: {worst('gn planted ')}")


def test_groupnorm_relu_grad_rejections():
    N, C, groups, hw = 2, 64, 32, 35
    s = dgb.gn_case(N, C, groups, hw)
    args = _gn_device(s, (True, True, True, True), groups, 0)
    shapes = _gn_shapes(N, C, hw)
    L = _lib.lib()
    p = ops._p

    def call(N=N, C=C, hw=hw, groups=groups, ws_bytes=None):
        bufs = {k: margins(shape) for k, shape in shapes.items()}
        ws = ops._ws(L.aoc_groupnorm_relu_grad_workspace_bytes(2, 64, 32), DEV)
        o = [bufs[k][1] for k in dgb.GN_OUTS]
        gy, x, st, _, w, b, r, _, g = args
        rc = L.aoc_groupnorm_relu_grad(p(gy), p(x), p(r), p(st), p(w), p(b), p(g), N, C, hw, groups, 1, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(ws),
                                       ws.numel() if ws_bytes is None else ws_bytes, ops._stream())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(b_).all()) for b_, _ in bufs.values()), "a rejected call wrote something"
        return _lib.STATUS[rc]
    assert call(groups=5) == INVALID and call(hw=0) == INVALID and call(N=ops.MAX_OBJECTS + 1) == UNSUPPORTED and call(ws_bytes=64) == WORKSPACE
    with pytest.raises(ValueError, match="do not divide"):
        dt.groupnorm_relu_backward(args[0], args[1], args[2], 5)
    with pytest.raises(_lib.AocHipError, match="AOC_ERR_UNSUPPORTED"):
        big = torch.zeros(31, 32, 1, device=DEV)
        dt.groupnorm_relu_backward(big, big, torch.zeros(31 * 32, 2, device=DEV), 32)


# ------------------------------------------------------------------------------------------ 2 aoc_cat_film_scale_grad
@pytest.mark.parametrize("O,Cx,Cm,hw", dgb.CAT_CASES)
def test_cat_film_scale_grad(O, Cx, Cm, hw):
    s = dgb.cat_case(O, Cx, Cm, hw)
    for alias in ((False, True) if Cm == Cx else (False,)):
        mem_np = s["x"] if alias else s["mem"]
        ref = dgb.cat_film_scale_grad_ref(s["grad_y"], s["x"], mem_np, s["gain"])
        for offs in ((0, 0, 0), (1, 2, 3)):                                   # the three base pointers at different misalignments
            gy, x = shifted(s["grad_y"], offs[0]), shifted(s["x"], offs[1])
            mem = x if alias else (shifted(mem_np, offs[2]) if Cm else None)
            gain = dev(s["gain"])
            runs = []
            for _ in range(2):
                bx, ox = margins(x.shape, offs[1])
                bm, om = margins(mem.shape, offs[2]) if Cm else (None, None)
                bg, og = margins(s["gain"].shape)
                got = dt.cat_film_scale_backward(gy, x, mem, gain, ox, om, og)
                assert got[0] is ox and got[1] is om and got[2] is og and untouched(bx, x.shape, offs[1]) and untouched(bg, s["gain"].shape)
                assert om is None or untouched(bm, mem.shape, offs[2]), "written outside the outputs"
                runs.append([g.clone() if g is not None else None for g in got])
            what = f"cat_film_scale_grad {O},{Cx},{Cm},{hw} alias={alias} offs={offs}"
            for k, name in enumerate(("grad_x", "grad_mem", "dgain")):
                if runs[0][k] is None:
                    continue
                assert torch.equal(runs[0][k], runs[1][k]), f"{what} {name}: two runs differ"
                held("cat " + name, runs[0][k], ref[name], f"{what} {name}")
            only_x = dt.cat_film_scale_backward(gy, x, mem, gain, want_gain=False)            # grad_mem not wanted; each output alone: the same bits
            only_g = dt.cat_film_scale_backward(gy, x, mem, None, want_x=False)
            assert only_x[1] is None and only_x[2] is None and only_g[0] is None and only_g[1] is None
            assert torch.equal(only_x[0], runs[0][0]) and torch.equal(only_g[2], runs[0][2]), f"{what}: an output alone differs"
            if Cm:
                only_m = dt.cat_film_scale_backward(gy, x, mem, gain, want_x=False, want_mem=True, want_gain=False)
                assert only_m[0] is None and only_m[2] is None and torch.equal(only_m[1], runs[0][1])
            # the plane dots of aoc_channel_scale_grad on the materialised concatenation
            cat = torch.cat([x, mem], 1).contiguous() if Cm else x.contiguous()
            _, dg2 = gt.channel_scale_backward(gy.contiguous(), cat, None, want_x=False)
            held("cat dgain", dg2, ref["dgain"], f"{what}: channel_scale_backward on the concatenation")
    with pytest.raises(ValueError, match="do not concatenate"):
        dt.cat_film_scale_backward(dev(s["grad_y"]), dev(s["x"])[:, :, :-1] if hw > 1 else dev(s["x"]).repeat(1, 2, 1), None, dev(s["gain"]))
    print(f"cat_film_scale_grad {O},{Cx},{Cm},{hw}: worst error / bound so far: {worst('cat ')}")


# ------------------------------------------------------------------------------------------ modules: every wrapper call on tape
class Tape(tgg.Tape):
    """tgg.Tape (the wrappers of gates_train) plus this module's two"""
    MINE = ("groupnorm_relu_backward", "cat_film_scale_backward")

    def __enter__(self):
        super().__enter__()
        self._mine = {n: getattr(dt, n) for n in self.MINE}
        for n, f in self._mine.items():
            setattr(dt, n, lambda *a, _n=n, _f=f, **k: self._note(_n, _f, a, k))
        return self

    def __exit__(self, *exc):
        for n, f in self._mine.items():
            setattr(dt, n, f)
        super().__exit__(*exc)


def _p3(t):
    return _np(t).reshape(t.shape[0], t.shape[1], -1) if t is not None else None


def hold_call(name, a, k, res):
    """one recorded wrapper call against its float64 reference at the tensors it received"""
    if name == "groupnorm_relu_backward":
        gy, x, stats, groups, gamma, beta, residual, relu, gain = a[:9]
        held("module gn stats", stats, dgb.stats_ref(_p3(x), groups, 1e-5), "the saved statistics")
        ref, und = dgb.groupnorm_relu_grad_ref(_p3(gy), _p3(x), _p3(residual), groups, _np(gamma), _np(beta), 1e-5, relu, _np(gain))
        assert int(und.sum()) <= dgb.MASK_CAP * und.numel(), f"{int(und.sum())} of {und.numel()} elements undecided"
        for g, n in zip(res, dgb.GN_OUTS):
            if g is not None:
                held("module gn " + n, g.reshape(ref[n][0].shape), ref[n], n)
    elif name == "cat_film_scale_backward":
        gy, x, mem, gain = a[:4]
        ref = dgb.cat_film_scale_grad_ref(_p3(gy), _p3(x), _p3(mem), _np(gain))
        for g, n in zip(res, ("grad_x", "grad_mem", "dgain")):
            if g is not None:
                held("module cat " + n, g.reshape(ref[n][0].shape), ref[n], n)
    else:
        tgg.hold_call(name, a, k, res)


def backward_taped(forward, leaves, params, grad_y):
    """forward + backward on fresh leaves -> (y, leaf gradients, parameter gradients, tape); every taped call is held to its reference.  (That two
    runs give the same bits is tested entry by entry above: MIOpen does not promise it for the convolutions in between.)"""
    for p in params.values():
        p.grad = None
    ls = [t.clone().requires_grad_(True) for t in leaves]
    with Tape() as tape, torch.enable_grad():
        y = forward(*ls)
        y.backward(grad_y)
    for c in tape.calls:
        hold_call(*c)
    return y.detach(), [l.grad for l in ls], {n: (p.grad.clone() if p.grad is not None else None) for n, p in params.items()}, tape


class Replay(nn.Module):
    """stands in for a convolution of the mirror: demands the bits the twin's convolution received and returns the bits it returned.  MIOpen may
    pick another solver for a second execution of the same convolution, so `the twin's forward has the mirror's bits` is stated for what the
    library computes: equal bits into every convolution, equal bits out of the last form, the convolutions' own results shared."""

    def __init__(self, name, inp, out):
        super().__init__()
        self.name, self.inp, self.out = name, inp, out

    def forward(self, x):
        assert torch.equal(x, self.inp), f"{self.name}: the mirror hands this convolution other bits than the twin did"
        return self.out


def record_convs(module):
    """-> (records name -> (input, output) of every Conv2d of `module`, filled by its next forward; the hooks to remove)"""
    records = {}
    hooks = [m.register_forward_hook(lambda mod, inp, out, _n=n: records.__setitem__(_n, (inp[0].detach(), out.detach())))
             for n, m in module.named_modules() if isinstance(m, nn.Conv2d)]
    return records, hooks


def replayed(mirror, twin, records):
    """the mirror with the twin's parameters and every convolution replaced by the replay of the twin's"""
    mirror.load_state_dict(twin.state_dict())
    for n, m in list(mirror.named_modules()):
        if isinstance(m, nn.Conv2d):
            parent, _, child = n.rpartition(".")
            setattr(mirror.get_submodule(parent) if parent else mirror, child, Replay(n, *records[n]))
    return mirror.to(DEV)


def mirror_bits(twin, make_mirror, call):
    """call(module) under no_grad on the twin, then on the replaying mirror: the same bits"""
    records, hooks = record_convs(twin)
    with torch.no_grad():
        yt = call(twin)
    for hk in hooks:
        hk.remove()
    with torch.no_grad():
        ym = call(replayed(make_mirror(), twin, records))
    assert not yt.requires_grad and torch.equal(yt, ym), "without a graph the twin does not give the mirror's bits"


def _bottleneck(cin, cout, seed):
    blk = dt.Bottleneck(cin, cout)
    dgb.randomize_small_parameters(blk, None, np.random.RandomState(seed))
    dgb.set_conv_weights(blk, seed)
    return blk.to(DEV)


def _wired(tape, *specs, skip_none=False):
    """tgg.wired, where a None in a spec means `not checked` (skip_none) and an empty spec skips the call"""
    assert len(tape.calls) == len(specs)
    for (name, a, _, _), spec in zip(tape.calls, specs):
        for pos, want in enumerate(spec):
            got, where = a[pos], f"{name}, argument {pos}"
            if isinstance(want, tuple) and len(want) == 3 and want[0] == "from":
                src = tape.calls[want[1]][3][want[2]]
                assert got is src or (got.data_ptr() == src.data_ptr() and got.shape == src.shape), where + ": not the tensor the earlier stage returned"
            elif want is None:
                assert skip_none or got is None, where
            elif torch.is_tensor(want):
                assert torch.is_tensor(got) and got.numel() == want.numel() and torch.equal(got.reshape(want.shape), want), where + ": another tensor"
            else:
                assert not torch.is_tensor(got) and got == want, f"{where}: {got!r}, expected {want!r}"


GN_CHAIN = ["groupnorm_relu_backward"]
GCT_CHAIN = ["channel_scale_backward", "gct_gate_backward", "gct_scale_backward"]


@pytest.mark.parametrize("gated", (False, True))
@pytest.mark.parametrize("cin,cout", ((64, 128), (128, 128)))
def test_bottleneck_backward(cin, cout, gated):
    N, D, h, w = 2, 10, 5, 7
    rs = ggb.rng(cin, cout, int(gated), 5)
    blk = _bottleneck(cin, cout, 600 + cin)
    gate = gt.IA_gate(D, cout).to(DEV)
    x, head, gy = (dev(rs.standard_normal(s).astype(f32)) for s in ((N, cin, h, w), (N, D), (N, cout, h, w)))
    mgate = lambda: (head, gate.IA.weight.detach(), gate.IA.bias.detach()) if gated else None
    # without a graph: the mirror's bits
    mirror_bits(blk, lambda: gct.Bottleneck(cin, cout), lambda m: m(x, gate=mgate()))
    records, hooks = record_convs(blk)
    params = dict(blk.named_parameters(), **({"gate." + k: v for k, v in gate.named_parameters()} if gated else {}))
    fwd = (lambda lx, lh: blk(lx, gate=(lh, gate.IA.weight, gate.IA.bias))) if gated else (lambda lx, lh: blk(lx))
    y, (gx, gh), pg, tape = backward_taped(fwd, (x, head), params, gy)
    for hk in hooks:
        hk.remove()
    seen = {n: out for n, (_, out) in records.items()}
    with torch.no_grad():
        ym = replayed(gct.Bottleneck(cin, cout), blk, records)(x, gate=mgate())
    assert y.shape == ym.shape and torch.equal(y, ym), "the forward with a graph is not the mirror's"
    down = blk.downsample is not None
    assert tape.names() == GN_CHAIN + (["film_gain_backward"] if gated else []) + (GN_CHAIN if down else []) + 2 * GN_CHAIN + GCT_CHAIN
    c = tape.calls
    nxt = 2 if gated else 1
    with torch.no_grad():
        residual = ops.groupnorm_relu(seen["downsample.0"], 32, blk.downsample[1].weight, blk.downsample[1].bias, 1e-5, None, False) if down else x
        gain = ops.film_gain(head, gate.IA.weight, gate.IA.bias) if gated else None
    # bn3 (+ the gate): the cotangent, conv3's output, the residual, the gain; then the gate's small backward on its dgain
    _wired(tape, *([(gy, seen["conv3"], None, 32, blk.bn3.weight.detach(), blk.bn3.bias.detach(), residual, True, gain)]
                      + ([(FROM(0, 4), gain, head, gate.IA.weight.detach())] if gated else [])
                      + ([(FROM(0, 1), seen["downsample.0"], None, 32, blk.downsample[1].weight.detach(), blk.downsample[1].bias.detach(), None, False, None)] if down else [])
                      + [(None, seen["conv2"], None, 32, blk.bn2.weight.detach(), blk.bn2.bias.detach(), None, True, None),
                         (None, seen["conv1"], None, 32, blk.bn1.weight.detach(), blk.bn1.bias.detach(), None, True, None)]
                      + [()] * 3), skip_none=True)
    assert torch.equal(pg["bn3.weight"], c[0][3][2]) and torch.equal(pg["bn3.bias"], c[0][3][3])
    k2 = nxt + (1 if down else 0)
    assert torch.equal(pg["bn2.weight"], c[k2][3][2]) and torch.equal(pg["bn1.bias"], c[k2 + 1][3][3])
    if down:
        assert torch.equal(pg["downsample.1.weight"], c[nxt][3][2]) and c[nxt][3][1] is None and c[nxt][3][4] is None
    else:
        assert c[0][3][1] is not None, "no downsample: the residual is x and wants its gradient"
    if gated:
        assert torch.equal(gh, c[1][3][0]) and torch.equal(pg["gate.IA.weight"], c[1][3][1]) and torch.equal(pg["gate.IA.bias"], c[1][3][2])
    else:
        assert gh is None and c[0][3][4] is None
    assert gx is not None and bool(torch.isfinite(gx).all()) and all(v is not None for v in pg.values())
    print(f"Bottleneck {cin}->{cout} gated={gated}: worst error / bound so far: {worst('module ')}")


class Decoder(nn.Module):
    """carries the twins as methods, the way INTEGRATION.md binds them onto the reference's class"""
    Modulator_1 = dt.Modulator_1
    Modulator_2 = dt.Modulator_2
    modulate = dt.modulate


class MirrorDecoder(nn.Module):
    Modulator_1 = decoder_memory.Modulator_1
    Modulator_2 = decoder_memory.Modulator_2
    modulate = decoder_memory.modulate


# decoding_module.py:55-71 with the smallest embed_dim its Bottlenecks can be built with: GroupNorm(32, embed_dim / 4) needs embed_dim / 4 to be a
# multiple of 32 (nn.GroupNorm refuses 32 groups of 8 or 16 channels in the constructor), so 128: channels 256 -> 256 -> 128 -> 128
EMBED = 128


def _decoder(D, seed, prefixes=("M1",), twin=True):
    dec = Decoder() if twin else MirrorDecoder()
    e = EMBED
    for prefix in prefixes:
        for i, (cin, cout) in enumerate(((2 * e, 2 * e), (2 * e, e), (e, e)), 1):
            torch.manual_seed(seed + i)
            setattr(dec, f"{prefix}_Reweight_Layer_{i}", (gt.IA_gate if twin else aoc_amd.attention.IA_gate)(D, cin))
            blk = (dt.Bottleneck if twin else gct.Bottleneck)(cin, cout, 1)
            if twin:
                dgb.randomize_small_parameters(blk, None, np.random.RandomState(seed + i))
                dgb.set_conv_weights(blk, seed + i)
            setattr(dec, f"{prefix}_Bottleneck_{i}", blk)
    return dec.to(DEV)


def _block_chain(down, gated):
    return GN_CHAIN + (["film_gain_backward"] if gated else []) + (GN_CHAIN if down else []) + 2 * GN_CHAIN + GCT_CHAIN


M_CHAIN = _block_chain(False, False) + _block_chain(True, True) + _block_chain(False, True) + ["cat_film_scale_backward", "film_gain_backward"]


def test_modulator_backward():
    N, D, h, w = 2, 10, 5, 7
    rs = ggb.rng(N, D, 6)
    dec = _decoder(D, 700)
    x, mem, head, gy = (dev(rs.standard_normal(s).astype(f32)) for s in ((N, EMBED, h, w), (N, EMBED, h, w), (N, D), (N, EMBED, h, w)))
    mirror_bits(dec, lambda: _decoder(D, 700, twin=False), lambda m: m.Modulator_1(x, mem, head))
    records, hooks = record_convs(dec)
    y, (gx, gh), pg, tape = backward_taped(lambda lx, lh: dec.Modulator_1(lx, mem, lh), (x, head), dict(dec.named_parameters()), gy)
    for hk in hooks:
        hk.remove()
    with torch.no_grad():
        ym = replayed(_decoder(D, 700, twin=False), dec, records).Modulator_1(x, mem, head)
    assert torch.equal(y, ym) and tape.names() == M_CHAIN
    cat = tape.calls[-2]
    with torch.no_grad():
        gain1 = ops.film_gain(head, dec.M1_Reweight_Layer_1.IA.weight, dec.M1_Reweight_Layer_1.IA.bias)
    assert torch.equal(cat[1][1], x) and torch.equal(cat[1][2], mem) and torch.equal(cat[1][3], gain1) and cat[3][1] is None, "the memory gets no gradient"
    assert torch.equal(gx, cat[3][0]) and tape.calls[-1][1][0] is cat[3][2] and torch.equal(pg["M1_Reweight_Layer_1.IA.weight"], tape.calls[-1][3][1])
    assert gh is not None and all(v is not None and bool(torch.isfinite(v).all()) for v in pg.values())
    print(f"Modulator_1 embed_dim={EMBED}: worst error / bound so far: {worst('module ')}")


def test_modulate_two_frames():
    N, D, h, w = 2, 10, 5, 7
    rs = ggb.rng(N, D, 7)
    dec = _decoder(D, 800, ("M1", "M2"))
    head = dev(rs.standard_normal((N, D)).astype(f32))
    frames = [dev(rs.standard_normal((N, EMBED, h, w)).astype(f32)) for _ in range(2)]
    gy = dev(rs.standard_normal((N, EMBED, h, w)).astype(f32))
    mem_t, mem_m = [None, None], [None, None]
    for f, x in enumerate(frames):                                            # frame 0: both self-memories; frame 1: slot 0 = frame 0's x, slot 1 kept
        keep, box = list(mem_t), {}

        def fwd(lx, lh):
            out, box["mem"] = dec.modulate(lx, lh, keep)
            return out
        records, hooks = record_convs(dec)
        y, (gx, gh), pg, tape = backward_taped(fwd, (x, head), dict(dec.named_parameters()), gy)
        for hk in hooks:
            hk.remove()
        mem_t = box["mem"]
        with torch.no_grad():
            ym, mem_m = replayed(_decoder(D, 800, ("M1", "M2"), twin=False), dec, records).modulate(x, head, mem_m)
        assert torch.equal(y, ym) and tape.names() == M_CHAIN + M_CHAIN, f"frame {f}"
        assert all(not m.requires_grad and m.is_cuda for m in mem_t) and torch.equal(mem_t[0], x) and torch.equal(mem_t[1], mem_m[1])
        cat2, cat1 = tape.calls[len(M_CHAIN) - 2], tape.calls[-2]
        assert cat1[3][1] is None and cat2[3][1] is None, "the memories are detached: no gradient is computed for them"
        assert torch.equal(cat1[1][2], x if f == 0 else frames[0]) and torch.equal(gx, cat1[3][0])
        if f == 1:
            assert torch.equal(cat2[1][2], keep[1]) and keep[1].data_ptr() == mem_t[1].data_ptr(), "slot 1 is kept"
    print(f"modulate, two frames: worst error / bound so far: {worst('module ')}")


class Slice(nn.Module):
    """not this module's Bottleneck: the gate follows through gates_train's film scale"""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return x[:, :self.out]


def test_modulator_falls_back_behind_a_foreign_block():
    N, D, e, h, w = 3, 6, 4, 3, 5
    rs = ggb.rng(N, D, 8)
    dec = Decoder()
    for i, (cin, cout) in enumerate(((2 * e, 2 * e), (2 * e, e), (e, e)), 1):
        setattr(dec, f"M1_Reweight_Layer_{i}", gt.IA_gate(D, cin))
        setattr(dec, f"M1_Bottleneck_{i}", Slice(cout))
    dec = dec.to(DEV)
    x, head, gy = (dev(rs.standard_normal(s).astype(f32)) for s in ((N, e, h, w), (N, D), (N, e, h, w)))
    y, (gx, gh), pg, tape = backward_taped(lambda lx, lh: dec.Modulator_1(lx, lx.detach(), lh), (x, head), dict(dec.named_parameters()), gy)
    assert tape.names() == 2 * ["channel_scale_backward", "film_gain_backward"] + ["cat_film_scale_backward", "film_gain_backward"]
    with torch.no_grad():
        ia1, ia2, ia3 = (getattr(dec, f"M1_Reweight_Layer_{i}").IA for i in (1, 2, 3))
        want = ops.cat_film_scale(x, x, head, ia1.weight, ia1.bias)
        want = ops.film_scale(want, head, ia2.weight, ia2.bias)               # Slice(2 e) keeps everything
        want = ops.film_scale(want[:, :e], head, ia3.weight, ia3.bias)
    assert torch.equal(y, want)


def test_mirrors_raise_under_autograd_and_name_the_twins():
    x = torch.randn(2, 128, 3, 3, device=DEV, requires_grad=True)
    head = torch.randn(2, 6, device=DEV)
    with torch.enable_grad():
        with pytest.raises(_lib.AocHipError, match="inference-only.*decoder_train.Bottleneck is the differentiable form"):
            gct.Bottleneck(128, 128).to(DEV)(x)
        mir = _decoder(6, 900, twin=False)
        with pytest.raises(_lib.AocHipError, match="inference-only.*decoder_train.Modulator_1 is the differentiable form"):
            mir.Modulator_1(x, x.detach(), head)


def test_double_backward_raises():
    x = torch.randn(2, 32, 4, 4, device=DEV, requires_grad=True)
    w = torch.ones(32, device=DEV)
    with torch.enable_grad():
        y = dt.groupnorm_relu(x, 32, w, w)
        g, = torch.autograd.grad((y * y).sum(), x, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()


def test_bottleneck_peak_memory():
    N, C, h, w = 4, 128, 31, 33
    blk = _bottleneck(C, C, 31)
    rs = ggb.rng(N, C, 9)
    x, gy = dev(rs.standard_normal((N, C, h, w)).astype(f32)).requires_grad_(True), dev(rs.standard_normal((N, C, h, w)).astype(f32))

    def run():
        with torch.enable_grad():
            y = blk(x)
            y.backward(gy)
        return y.detach()
    run()                                                                      # warm-up: library, MIOpen and allocator
    x.grad = None
    for p in blk.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    hw, P = h * w, C // 4
    plane = N * hw * 4
    output = C * plane
    saved = (C + P + P) * plane + (P + P + C) * plane                          # the convolutions' inputs (GCT1's output, bn1's, bn2's); the normalisations' (conv1..3's outputs)
    saved += 3 * N * 32 * 2 * 4 + 2 * N * C * 4                                # the statistics; GCT1's plane sums and gate
    grads = C * plane + sum(p.numel() for p in blk.parameters()) * 4           # x's and the parameters'
    L = _lib.lib()
    work = sum(L.aoc_groupnorm_relu_workspace_bytes(N, 32) + L.aoc_groupnorm_relu_grad_workspace_bytes(N, c, 32) for c in (P, P, C)) + 2 * N * C * 4
    budget = output + saved + grads + work
    print(f"Bottleneck {N},{C},{h}x{w}: peak {peak} bytes above the inputs, output + saved + gradients + workspaces {budget}")
    assert peak < 2 * budget, f"peak {peak} bytes, twice the accounted tensors is {2 * budget}"
    del y
