"""The decoder's memory block on the GPU: aoc_cat_film_scale and aoc_groupnorm_relu_scale return exactly the bits of the compositions they
replace (torch.cat + ops.film_scale, ops.groupnorm_relu + ops.film_scale), the gated gct.Bottleneck equals the Bottleneck followed by the
gate, the mirror Modulator_1 stays within 4 x the reference float32 run's own error of the float64 result (fixtures modulator_*), and
decoder_memory.modulate follows the reference's memory rule over the five-frame fixture with every memory on the device.

Bit equality is checked on the int32 view (it tells -0 from +0); outputs are pre-filled with NaN where the operator takes a buffer."""
import numpy as np
import pytest
import torch
from torch import nn

from decoder_memory_bounds import cat_gate_ref, gate1_args, gate_chain_ref
from float64_bounds import _check_bound, t64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    return aoc_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu()


def nan_like(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    assert not torch.isnan(got).any(), f"{what}: elements left unwritten"
    diff = got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.numel()} elements differ in their bits"


def gate_inputs(rng, N, C, D):
    return (dev((0.5 * rng.standard_normal((N, D))).astype(np.float32)), dev((rng.standard_normal((C, D)) / np.sqrt(D)).astype(np.float32)),
            dev((0.3 * rng.standard_normal(C)).astype(np.float32)))


def offset_view(t, start):
    """A contiguous copy of t that starts `start` floats into a larger buffer (16-byte misalignment 4 * start)."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    v = buf[start:start + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------ 1. concat + gate 1
# (N, Cx, Cm, hw, D): the smallest tensor; odd hw with Cx, Cm odd (source and destination planes at different misalignments, the dot product
# longer than one trip of 1024); the half-resolution plane (one workgroup, U = 8); a plane that spans several workgroups (U = 4)
CAT_CASES = [(1, 1, 1, 1, 5), (2, 3, 5, 7, 1100), (3, 4, 4, 6527, 400), (2, 8, 8, 25773, 37)]
CAT_MODES = ["plain", "no_memory", "alias", "offset_views", "no_bias"]


@pytest.mark.parametrize("mode", CAT_MODES)
@pytest.mark.parametrize("N,Cx,Cm,hw,D", CAT_CASES)
def test_cat_film_scale_bits(aoc, N, Cx, Cm, hw, D, mode):
    rng = np.random.RandomState(Cx * 1000 + hw)
    ops = aoc.ops
    if mode == "no_memory":
        Cm = 0
    if mode == "alias":
        Cm = Cx
    x = dev(rng.standard_normal((N, Cx, hw, 1)).astype(np.float32))
    mem = None if Cm == 0 else (x if mode == "alias" else dev(rng.standard_normal((N, Cm, hw, 1)).astype(np.float32)))
    head, weight, bias = gate_inputs(rng, N, Cx + Cm, D)
    if mode == "no_bias":
        bias = None
    want = ops.film_scale(x if mem is None else torch.cat([x, mem], 1), head, weight, bias)
    out = nan_like(N, Cx + Cm, hw, 1)
    if mode == "offset_views":
        x, mem = offset_view(x, 1), offset_view(mem, 2)
        out = offset_view(out, 3)
        assert x.data_ptr() % 16 == 4 and mem.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 12
    got = ops.cat_film_scale(x, mem, head, weight, bias, out=out)
    assert got.data_ptr() == out.data_ptr()
    same_bits(got, want, f"cat_film_scale {mode} N={N} Cx={Cx} Cm={Cm} hw={hw}")
    if mode == "plain":
        same_bits(ops.cat_film_scale(x, mem, head, weight, bias), want, "cat_film_scale, own output")


# ------------------------------------------------------------------------------------------ 2. GroupNorm apply + gate
GN_CASES = [(1, 32, 32, 1, 5), (2, 8, 4, 7, 1100), (3, 64, 32, 6527, 400), (2, 8, 2, 9563, 37)]          # (N, C, groups, hw, D); the last: U = 4


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_residual", [True, False])
@pytest.mark.parametrize("N,C,groups,hw,D", GN_CASES)
def test_groupnorm_relu_scale_bits(aoc, N, C, groups, hw, D, with_residual, relu, inplace):
    rng = np.random.RandomState(C * 100 + hw)
    ops = aoc.ops
    x = dev((rng.standard_normal((N, C, hw, 1)) * 2 + 0.5).astype(np.float32))
    res = dev(rng.standard_normal((N, C, hw, 1)).astype(np.float32)) if with_residual else None
    gam, bet = dev(rng.uniform(0.5, 1.5, C).astype(np.float32)), dev((0.5 * rng.standard_normal(C)).astype(np.float32))
    head, weight, gbias = gate_inputs(rng, N, C, D)
    want = ops.film_scale(ops.groupnorm_relu(x, groups, gam, bet, 1e-5, res, relu), head, weight, gbias)
    out = x.clone() if inplace else nan_like(N, C, hw, 1)
    src = out if inplace else x
    got = ops.groupnorm_relu_scale(src, groups, gam, bet, 1e-5, res, relu, head, weight, gbias, out=out)
    assert got.data_ptr() == out.data_ptr()
    same_bits(got, want, f"groupnorm_relu_scale N={N} C={C} hw={hw} residual={with_residual} relu={relu} inplace={inplace}")
    if not relu:
        assert bool((got < 0).any())                           # the ReLU really was off


def test_groupnorm_relu_scale_misaligned_views(aoc):
    """x, the residual and y at three different 16-byte misalignments, odd hw."""
    rng = np.random.RandomState(3)
    ops = aoc.ops
    N, C, groups, hw, D = 2, 8, 4, 1031, 37
    x, res = (dev(rng.standard_normal((N, C, hw, 1)).astype(np.float32)) for _ in range(2))
    gam, bet = dev(rng.uniform(0.5, 1.5, C).astype(np.float32)), dev((0.5 * rng.standard_normal(C)).astype(np.float32))
    head, weight, gbias = gate_inputs(rng, N, C, D)
    want = ops.film_scale(ops.groupnorm_relu(x, groups, gam, bet, 1e-5, res, True), head, weight, gbias)
    out = offset_view(nan_like(N, C, hw, 1), 3)
    got = ops.groupnorm_relu_scale(offset_view(x, 1), groups, gam, bet, 1e-5, offset_view(res, 2), True, head, weight, gbias, out=out)
    same_bits(got, want, "groupnorm_relu_scale, misaligned views")


# ------------------------------------------------------------------------------------------ 3. the gated Bottleneck
def randomise(module, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.split(".")[-1]
            if leaf == "alpha" or (leaf == "weight" and p.dim() == 1):
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=gen))
            elif leaf in ("gamma", "beta") or (leaf == "bias" and p.dim() == 1 and "IA" not in name):
                p.copy_(0.5 * torch.randn(p.shape, generator=gen))


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 128)])                  # with and without the downsample branch
def test_gated_bottleneck_equals_bottleneck_then_gate(aoc, cin, cout):
    torch.manual_seed(cin)
    block = aoc.gct.Bottleneck(cin, cout)
    gate = aoc.attention.IA_gate(12, cout)
    randomise(block, cin)
    block, gate = block.cuda().eval(), gate.cuda().eval()
    assert (block.downsample is not None) == (cin != cout)
    x, head = torch.randn(3, cin, 9, 11).cuda(), (0.5 * torch.randn(3, 12)).cuda()
    want = gate(block(x), head)
    got = block(x, gate=(head, gate.IA.weight, gate.IA.bias))
    same_bits(got, want, f"gated Bottleneck {cin}->{cout}")
    same_bits(block(x, gate=None), block(x), "Bottleneck, gate=None")


# ------------------------------------------------------------------------------------------ 4. the modulator fixtures
def mirror_decoder(aoc):
    """A class that carries the mirrors as methods, the way INTEGRATION.md binds them onto the reference's class."""
    class Decoder(nn.Module):
        Modulator_1 = aoc.decoder_memory.Modulator_1
        Modulator_2 = aoc.decoder_memory.Modulator_2
        modulate = aoc.decoder_memory.modulate
    return Decoder()


def modulator_of(aoc, g):
    e = g["in_x"].shape[1]
    D = g["in_IA_head"].shape[1]
    dec = mirror_decoder(aoc)
    for i, (cin, cout) in enumerate(((2 * e, 2 * e), (2 * e, e), (e, e)), 1):
        setattr(dec, f"M1_Reweight_Layer_{i}", aoc.attention.IA_gate(D, cin))
        setattr(dec, f"M1_Bottleneck_{i}", aoc.gct.Bottleneck(cin, cout, 1))
    dec.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p_")})
    return dec.cuda().eval()


@pytest.mark.parametrize("name", ["modulator_O3", "modulator_O1"])
def test_modulator_golden(aoc, golden, name):
    """max |mirror - float64| <= 4 max |reference float32 - float64|, both sides from the fixture: the factor 4 leaves MIOpen's convolutions
    another summation order than the CPU's; a wiring mistake is O(1).  Gate 1, which has no convolution in front of it, is held to the
    float32 bound of the host test."""
    g = golden(name)
    dec = modulator_of(aoc, g)
    x, mem, head = dev(g["in_x"]), dev(g["in_x_memory"]), dev(g["in_IA_head"])
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        got = dec.Modulator_1(x, mem, head)
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
    f64 = torch.from_numpy(g["out_f64"])
    ref_err = float((torch.from_numpy(g["out_f32"]).double() - f64).abs().max())
    err = float((host(got).double() - f64).abs().max())
    print(f"{name}: mirror {err:.3e}, reference float32 {ref_err:.3e}")
    assert got.shape == f64.shape and err <= 4 * ref_err, (err, ref_err)
    ia = dec.M1_Reweight_Layer_1.IA
    gate1 = aoc.ops.cat_film_scale(x, mem, head, ia.weight.detach(), ia.bias.detach())
    args = gate1_args(g)
    want, tol = cat_gate_ref(*args)
    _check_bound(host(gate1), want, tol, cat_gate_ref(*args, reverse=True)[0], f"{name}: gate 1 on the device, concat reversed")


# ------------------------------------------------------------------------------------------ 5. modulate
class Slice(nn.Module):
    """Channel-slicing stand-in for a modulator's Bottleneck (the fixture's): not a gct.Bottleneck, so the gate follows as ops.film_scale."""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return x[:, :self.out]


def test_modulate_keeps_the_memories_on_the_device(aoc, golden):
    g = golden("decoder_memory_rule")
    C, D = g["f0_x"].shape[1], g["f0_IA_head"].shape[1]
    dec = mirror_decoder(aoc)
    widths = (2 * C, C, C)
    for m in ("M1", "M2"):
        for i, (cin, cout) in enumerate(((2 * C, 2 * C), (2 * C, C), (C, C)), 1):
            setattr(dec, f"{m}_Reweight_Layer_{i}", aoc.attention.IA_gate(D, cin))
            setattr(dec, f"{m}_Bottleneck_{i}", Slice(cout))
    dec.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p_") and "IA_final" not in k})
    dec = dec.cuda().eval()
    seen = {}
    inner = {1: dec.Modulator_1, 2: dec.Modulator_2}

    def spy(k):
        def call(x, x_memory, IA_head):
            seen[k] = x_memory
            return inner[k](x, x_memory, IA_head)
        return call
    dec.Modulator_1, dec.Modulator_2 = spy(1), spy(2)                 # instance attributes in front of the class's methods
    gates = lambda m: [(t64(g[f"p_{m}_Reweight_Layer_{i}.IA.weight"]), t64(g[f"p_{m}_Reweight_Layer_{i}.IA.bias"])) for i in (1, 2, 3)]
    memory, slot1 = [None, None], []
    device = torch.device("cuda", torch.cuda.current_device())
    for f in range(5):
        x, head = dev(g[f"f{f}_x"]), dev(g[f"f{f}_IA_head"])
        given = list(memory)
        out, memory = dec.modulate(x, head, memory)
        for t in (out, memory[0], memory[1], seen[1], seen[2]):
            assert t.device == device
        assert memory[0].data_ptr() == x.data_ptr()                                      # held by reference: no copy of any kind
        assert torch.equal(host(seen[1]), torch.from_numpy(g[f"f{f}_m1_memory"])), f"frame {f}: Modulator_1's memory"
        assert (memory[1] is given[1]) == bool(g[f"f{f}_slot1_is_input_slot1"])
        assert seen[2] is memory[1]
        # slot 1 against float64 from the frame that made it (0 for frames 0-2, 3 afterwards), and against the recording's choice
        src = 0 if f < 3 else 3
        cat = torch.cat([t64(g[f"f{src}_x"]), t64(g[f"f{src}_m1_memory"])], 1)
        want, tol = gate_chain_ref(cat, t64(g[f"f{src}_IA_head"]), gates("M1"), widths)
        other = gate_chain_ref(torch.cat([t64(g[f"f{f}_x"]), t64(g[f"f{f}_m1_memory"])], 1), t64(g[f"f{f}_IA_head"]), gates("M1"), widths)[0] \
            if f != src else want * (1 + 2.0 ** -10)
        _check_bound(host(seen[2]), want, tol, other, f"frame {f}: Modulator_2's memory is Modulator_1's result of frame {src}")
        _check_bound(torch.from_numpy(g[f"f{f}_m2_memory"]), want, tol, other, f"frame {f}: the recording agrees")
        # the result: Modulator_2 of (Modulator_1's result, that memory)
        m1_out = gate_chain_ref(torch.cat([t64(g[f"f{f}_x"]), t64(g[f"f{f}_m1_memory"])], 1), t64(g[f"f{f}_IA_head"]), gates("M1"), widths)
        assert out.shape == (x.shape[0], C) + tuple(x.shape[2:])
        res, dres = gate_chain_ref(torch.cat([m1_out[0], want], 1), t64(g[f"f{f}_IA_head"]), gates("M2"), widths, torch.cat([m1_out[1], tol], 1))
        _check_bound(host(out), res, dres, res * (1 + 2.0 ** -10), f"frame {f}: the result")
        slot1.append(memory[1])
    assert slot1[0] is slot1[1] is slot1[2] and slot1[3] is slot1[4] and slot1[2] is not slot1[3]
