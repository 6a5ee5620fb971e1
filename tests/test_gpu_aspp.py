"""The ASPP mirror on the GPU (aoc_plane_sum_sumsq, aoc_gct_gate_multi, aoc_channel_scale_multi, aoc_groupnorm_cat_relu, aoc_amd.aspp):

* the plane statistics stay within the any-order float32 bounds of aspp_bounds.py against float64, carry the same bits on a second call,
  and every combination of wanted outputs returns what the full call returns;
* the multi-set gate, the multi-output scale and the GroupNorm-into-concatenation return exactly the bits of the per-set / per-output /
  per-source compositions they replace; plane_sumsq is within the bound of the y that was returned and repeats its bits;
* aspp.gate_inputs and aspp.merge, fed the recorded stage inputs of the reference's own ASPP (fixtures aspp_O3, aspp_O1), stay within the
  bounds of the float64 stages and agree with the recording to twice the bound;
* the whole module, fused and unfused, is within 4 x the error a plain-torch float32 CPU run of the same weights has against float64.

HW holds the plane sizes at which a streaming kernel changes path: one element, fewer than a float4 per lane, one float short of / exactly /
one past 256 and 2048 floats (a trip of the per-thread loops), and cfg2's own odd 61 x 107.  Bit equality is checked on the int32 view;
outputs are pre-filled with NaN where the operator takes a buffer."""
import numpy as np
import pytest
import torch

from aspp_bounds import BRANCHES, aspp_torch, cat_ref, gct_stage_ref, plane_stats_ref, plane_stats_slip, plane_sumsq_of
from float64_bounds import _check_bound, t64

pytestmark = pytest.mark.gpu

HW = [1, 35, 255, 256, 257, 2047, 2048, 2049, 6527]
FIXTURES = ["aspp_O3", "aspp_O1"]


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


def offset_view(t, start):
    """A contiguous copy of t that starts `start` floats into a larger buffer (16-byte misalignment 4 * start)."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    v = buf[start:start + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------ 1. plane statistics
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("hw", HW)
def test_plane_sum_sumsq_bounds_and_repeatability(aoc, hw, misaligned):
    rng = np.random.RandomState(hw)
    x = (rng.standard_normal((1, 7, hw, 1)) + 0.25).astype(np.float32)
    xd = dev(x)
    if misaligned:
        xd = offset_view(xd, 1)
        assert xd.data_ptr() % 16 == 4
    got = dict(zip(("sum", "sumsq", "mean"), aoc.ops.plane_sum_sumsq(xd)))
    ref, slip = plane_stats_ref(t64(x).view(7, hw)), plane_stats_slip(t64(x).view(7, hw))
    for k, v in got.items():
        assert v.shape == (1, 7)
        _check_bound(host(v).view(7), ref[k][0], ref[k][1], slip[k], f"plane_sum_sumsq {k} hw={hw} misaligned={misaligned}, last quarter dropped")
    again = aoc.ops.plane_sum_sumsq(xd)
    for (k, v), w in zip(got.items(), again):
        same_bits(w, v, f"plane_sum_sumsq {k} hw={hw}: second call")
    # every combination of wanted outputs: None where not wanted, the full call's bits elsewhere
    for mask in range(1, 7):
        wants = [bool(mask & 1), bool(mask & 2), bool(mask & 4)]
        part = aoc.ops.plane_sum_sumsq(xd, *wants)
        for k, w, p in zip(got, wants, part):
            assert (p is None) == (not w)
            if w:
                same_bits(p, got[k], f"plane_sum_sumsq {k} hw={hw} wanted={wants}")


# ------------------------------------------------------------------------------------------ 2. the gates of several GCTs
@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("C", [5, 512, 640])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("n_sets", [1, 4])
def test_gct_gate_multi_bits(aoc, n_sets, N, C, l1):
    rng = np.random.RandomState(C + 7 * N + n_sets)
    ops = aoc.ops
    sums = dev((np.abs(rng.standard_normal((N, C))) * 40 + (0 if l1 else 0.5)).astype(np.float32))
    al = dev(rng.uniform(0.5, 1.5, (n_sets, C)).astype(np.float32))
    ga, be = (dev((0.5 * rng.standard_normal((n_sets, C))).astype(np.float32)) for _ in range(2))
    got = ops.gct_gate_multi(sums, al, ga, be, 1e-5, l1)
    assert got.shape == (n_sets, N, C)
    for k in range(n_sets):
        same_bits(got[k], ops.gct_gate(sums, al[k], ga[k], be[k], 1e-5, l1), f"gct_gate_multi set {k} of {n_sets} N={N} C={C} l1={l1}")
    # the reference's parameter layout, one [1, C, 1, 1] tensor per GCT
    lists = [[t[k].view(1, C, 1, 1) for k in range(n_sets)] for t in (al, ga, be)]
    same_bits(ops.gct_gate_multi(sums, *lists, 1e-5, l1), got, "gct_gate_multi from per-GCT parameter lists")
    if n_sets == 4:
        assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------ 3. the gated copies
@pytest.mark.parametrize("mode", ["own", "buffers", "misaligned"])
@pytest.mark.parametrize("hw", HW)
@pytest.mark.parametrize("n_out", [1, 4, 8])
def test_channel_scale_multi_bits(aoc, n_out, hw, mode):
    rng = np.random.RandomState(hw + n_out)
    ops = aoc.ops
    N, C = 1, 3
    x = dev(rng.standard_normal((N, C, hw, 1)).astype(np.float32))
    gains = dev((1.0 + np.tanh(rng.standard_normal((n_out, N, C)))).astype(np.float32))
    want = [ops.channel_scale(x, gains[k]) for k in range(n_out)]
    outs = None
    if mode == "buffers":
        outs = [nan_like(N, C, hw, 1) for _ in range(n_out)]
    if mode == "misaligned":                                   # x one float in; the outputs at 3, 0, 1, 2, ... floats: not all at y_0's misalignment
        x = offset_view(x, 1)
        outs = [offset_view(nan_like(N, C, hw, 1), (3 + k) % 4) for k in range(n_out)]
        assert x.data_ptr() % 16 == 4 and outs[0].data_ptr() % 16 == 12
    got = ops.channel_scale_multi(x, gains, outs)
    assert len(got) == n_out
    for k in range(n_out):
        if outs is not None:
            assert got[k].data_ptr() == outs[k].data_ptr()
        same_bits(got[k], want[k], f"channel_scale_multi output {k} of {n_out} hw={hw} {mode}")
    if n_out == 1:                                              # in place
        y = x.clone() if mode != "misaligned" else offset_view(x, 2)
        res = ops.channel_scale_multi(y, gains, [y])
        assert res[0].data_ptr() == y.data_ptr()
        same_bits(y, want[0], f"channel_scale_multi in place hw={hw} {mode}")


# ------------------------------------------------------------------------------------------ 4. GroupNorm + ReLU into the concatenation
GN_CASES = [(1, 8, 2), (4, 128, 32), (8, 4, 1)]                 # (n_src, C_src, groups)
# (C_tail, N, relu, affine, misaligned): every value of the issue's lists, not their product
GN_VARIANTS = [(0, 1, True, True, False), (3, 3, False, True, False), (128, 3, True, False, False), (3, 1, True, True, True), (128, 1, False, False, True)]


@pytest.mark.parametrize("hw", HW)
@pytest.mark.parametrize("n_src,C_src,groups", GN_CASES)
def test_groupnorm_cat_relu_bits_and_plane_sumsq(aoc, n_src, C_src, groups, hw):
    ops = aoc.ops
    for C_tail, N, relu, affine, misaligned in GN_VARIANTS:
        what = f"groupnorm_cat_relu n_src={n_src} C_src={C_src} G={groups} hw={hw} C_tail={C_tail} N={N} relu={relu} affine={affine} misaligned={misaligned}"
        rng = np.random.RandomState(hw * 10 + n_src + C_tail)
        xs = [dev((rng.standard_normal((N, C_src, hw, 1)) * 2 + 0.5).astype(np.float32)) for _ in range(n_src)]
        gam = dev(rng.uniform(0.5, 1.5, (n_src, C_src)).astype(np.float32)) if affine else None
        bet = dev((0.5 * rng.standard_normal((n_src, C_src))).astype(np.float32)) if affine else None
        tail = dev(rng.standard_normal((N, C_tail)).astype(np.float32)) if C_tail else None
        parts = [ops.groupnorm_relu(x, groups, gam[k] if affine else None, bet[k] if affine else None, 1e-5, None, relu) for k, x in enumerate(xs)]
        if C_tail:
            t = torch.relu(tail) if relu else tail
            parts.append(t[:, :, None, None].expand(-1, -1, hw, 1))
        want = torch.cat(parts, 1)
        C_total = n_src * C_src + C_tail
        out = nan_like(N, C_total, hw, 1)
        if misaligned:
            xs = [offset_view(x, 1 + k % 3) for k, x in enumerate(xs)]
            out = offset_view(out, 3)
            assert out.data_ptr() % 16 == 12
        got, sq = ops.groupnorm_cat_relu(xs, groups, gam, bet, 1e-5, tail, relu, want_plane_sumsq=True, out=out)
        assert got.data_ptr() == out.data_ptr() and sq.shape == (N, C_total)
        same_bits(got, want, what)
        if not relu:
            assert bool((got < 0).any())                        # the ReLU really was off
        y64 = got.double().view(N, C_total, hw)               # the float64 sums are torch's, taken on the device
        q, tol = plane_sumsq_of(y64)
        _check_bound(sq, q, tol, plane_stats_slip(y64.view(N * C_total, hw))["sumsq"].view(N, C_total), what + ": plane_sumsq, last quarter dropped")
        # a second call with the same arguments: the same bits (the order of the plane sums follows y's 16-byte alignment, so the same buffer)
        first = sq.clone()
        out.fill_(float("nan"))
        got2, sq2 = ops.groupnorm_cat_relu(xs, groups, gam, bet, 1e-5, tail, relu, want_plane_sumsq=True, out=out)
        same_bits(got2, want, what + ": second call")
        same_bits(sq2, first, what + ": plane_sumsq on a second call")
        got3, sq3 = ops.groupnorm_cat_relu(xs, groups, gam, bet, 1e-5, tail, relu, want_plane_sumsq=True)
        same_bits(got3, want, what + ": own output")
        _check_bound(sq3, q, tol, plane_stats_slip(y64.view(N * C_total, hw))["sumsq"].view(N, C_total), what + ": plane_sumsq of the own output")
        same_bits(ops.groupnorm_cat_relu(xs, groups, gam, bet, 1e-5, tail, relu), want, what + ": without plane_sumsq")


# ------------------------------------------------------------------------------------------ 5. the recorded stages
def flat(a):
    a = np.asarray(a)
    return t64(a.reshape(a.shape[0], a.shape[1], -1))


def mirror_of(aoc, g):
    net = aoc.aspp.ASPP()
    missing, unexpected = net.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p_")}, strict=False)
    assert not unexpected and all(k.endswith("weight") for k in missing) and len(missing) == 4
    return net.cuda().eval()


def gct_params(g, prefix):
    return tuple(t64(g[f"p_{prefix}{k}"]).reshape(-1) for k in ("alpha", "gamma", "beta"))


@pytest.mark.parametrize("name", FIXTURES)
def test_gate_inputs_golden(aoc, golden, name):
    g = golden(name)
    net = mirror_of(aoc, g)
    x = dev(g["in_x"])
    gated, mean = aoc.aspp.gate_inputs(x, [getattr(net, b).GCT for b in BRANCHES])
    x64 = flat(g["in_x"])
    N, C, hw = x64.shape
    for k, b in enumerate(BRANCHES):
        want, tol, _, _ = gct_stage_ref(x64, 0.0, *gct_params(g, b + ".GCT."), float(g["meta_gct_eps"][k]))
        other = gct_stage_ref(x64, 0.0, *gct_params(g, BRANCHES[(k + 1) % 4] + ".GCT."), float(g["meta_gct_eps"][k]))[0]
        got = host(gated[k]).double().view(N, C, hw)
        _check_bound(got, want, tol, other, f"{name}: gate_inputs branch {b}, the next branch's parameters")
        assert bool(((got - flat(g[b + "_gct_out"])).abs() <= 2 * tol).all()), f"{name}: {b} against the recording"
    ref = plane_stats_ref(x64.view(N * C, hw))["mean"]
    _check_bound(host(mean).view(-1), ref[0], ref[1], plane_stats_slip(x64.view(N * C, hw))["mean"], f"{name}: gate_inputs mean")


@pytest.mark.parametrize("name", FIXTURES)
def test_merge_golden(aoc, golden, name):
    g = golden(name)
    net = mirror_of(aoc, g)
    convs = [dev(g[b + "_conv_out"]) for b in BRANCHES]
    N = convs[0].shape[0]
    tail = dev(g["pooled"]).view(N, -1)                          # recorded after its ReLU; relu(relu(v)) = relu(v)
    got = aoc.aspp.merge(convs, [getattr(net, b).bn for b in BRANCHES], tail, net.GCT)
    args = ([flat(g[b + "_conv_out"]) for b in BRANCHES], 32, [t64(g[f"p_{b}.bn.weight"]) for b in BRANCHES],
            [t64(g[f"p_{b}.bn.bias"]) for b in BRANCHES], float(g["meta_norm_eps"][0]), t64(g["pooled"]).reshape(N, -1))
    cat, dcat = cat_ref(*args)
    p, eps = gct_params(g, "GCT."), float(g["meta_gct_eps"][4])
    want, tol, _, _ = gct_stage_ref(cat, dcat, *p, eps)
    other = gct_stage_ref(cat_ref(*args, order=[3, 2, 1, 0, 4])[0], dcat, *p, eps)[0]
    got64 = host(got).double().view(want.shape)
    assert got.shape == g["cat_gated"].shape
    _check_bound(got64, want, tol, other, f"{name}: merge, branches reversed")
    # the recording's side of the comparison carries torch's float32 GroupNorm statistics (test_aspp_host.py holds it to that bound)
    rec_tol = gct_stage_ref(cat, cat_ref(*args, f32_stats=True)[1], *p, eps)[1]
    assert bool(((got64 - flat(g["cat_gated"])).abs() <= tol + rec_tol).all()), f"{name}: merge against the recording"


# ------------------------------------------------------------------------------------------ 6. the module
def randomise(module, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.split(".")[-1]
            if leaf == "alpha" or (leaf == "weight" and p.dim() == 1):
                p.copy_(torch.empty_like(p).uniform_(0.5, 1.5, generator=gen))
            elif leaf in ("gamma", "beta") or (leaf == "bias" and p.dim() == 1):
                p.copy_(0.5 * torch.randn(p.shape, generator=gen))


@pytest.fixture(scope="module")
def module_case(aoc):
    """One randomised ASPP and, per shape, the float64 and float32 plain-torch CPU results (computed once, shared, never changed)."""
    torch.manual_seed(17)
    net = aoc.aspp.ASPP()
    randomise(net, 17)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    cases = {}
    for N, h, w in ((3, 9, 13), (1, 5, 7)):
        x = torch.randn(N, 512, h, w, generator=torch.Generator().manual_seed(N * 100 + h))
        cases[(N, h, w)] = (x, aspp_torch(x, sd, torch.float64), aspp_torch(x, sd, torch.float32))
    return net.cuda().eval(), sd, cases


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("shape", [(3, 9, 13), (1, 5, 7)])
def test_aspp_module_against_float64(aoc, module_case, shape, fused):
    """max |out - f64| <= 4 max |f32 - f64|: both yardsticks are aspp_torch on the CPU with the same weights; the factor 4 leaves MIOpen's
    convolutions another summation order than the CPU's (test_decoder_final_golden); a wiring mistake is O(1)."""
    net, _, cases = module_case
    x, f64, f32 = cases[shape]
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        got = net(x.cuda(), fused=fused)
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
    ref_err = float((f32.double() - f64).abs().max())
    err = float((host(got).double() - f64).abs().max())
    print(f"ASPP {shape} fused={fused}: mirror {err:.3e}, plain-torch float32 {ref_err:.3e}")
    assert got.shape == f64.shape and got.dtype == torch.float32 and ref_err > 0
    assert err <= 4 * ref_err, (err, ref_err)


def test_aspp_paths_agree(aoc, module_case):
    """Both paths are within 4 x the float32 yardstick of float64, so within 8 x of each other.  They are not expected to share bits: the
    fused sums of squares are added in another order than plane_reduce's, and MIOpen's convolutions sit between the stages."""
    import inspect
    net, _, cases = module_case
    x, f64, f32 = cases[(1, 5, 7)]
    assert isinstance(inspect.signature(net.forward).parameters["fused"].default, bool)
    a, c = net(x.cuda(), fused=True), net(x.cuda(), fused=False)
    assert float((a - c).abs().max()) <= 8 * float((f32.double() - f64).abs().max())


def test_reference_state_dict_round_trips(aoc, module_case):
    _, sd, _ = module_case
    fresh = aoc.aspp.ASPP()
    assert list(fresh.state_dict().keys()) == list(sd.keys()) and "global_avg_pool.1.weight" in sd
    fresh.load_state_dict(sd)                                   # strict
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_requires_grad_input_raises(aoc, module_case):
    net, _, cases = module_case
    x = cases[(1, 5, 7)][0].cuda().requires_grad_(True)
    with torch.enable_grad():
        for fused in (True, False):
            with pytest.raises(aoc._lib.AocHipError):
                net(x, fused=fused)
        with pytest.raises(aoc._lib.AocHipError):
            net.aspp1(x)
    net(x.detach())
