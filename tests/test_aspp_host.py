"""The ASPP mirror without a GPU:

1. the float64 stage references of aspp_bounds.py, fed what the reference's own ASPP recorded as each stage's input (fixtures aspp_O3,
   aspp_O1), reproduce what it recorded as that stage's float32 output within the float32 bounds -- and leave them with the branches'
   parameters swapped, the concatenation reordered, the pooled branch not broadcast or GroupNorm statistics per channel: this pins the
   wiring the GPU tests hold the kernels to;
2. aoc_amd.aspp.ASPP() has the recorded state_dict names and shapes and the recorded convolution and GroupNorm hyper-parameters;
3. the four new entry points reject bad arguments before any launch, and their ops wrappers raise ValueError for mismatched shapes."""
import ctypes

import numpy as np
import pytest
import torch

from aspp_bounds import BRANCHES, aspp_torch, cat_ref, gct_stage_ref, plane_stats_ref
from float64_bounds import U, _check_bound, gamma, t64

FIXTURES = ["aspp_O3", "aspp_O1"]


def flat(a):
    """[N, C, h, w] -> float64 [N, C, hw]"""
    a = np.asarray(a)
    return t64(a.reshape(a.shape[0], a.shape[1], -1))


def gct_params(g, prefix):
    return tuple(t64(g[f"p_{prefix}{k}"]).reshape(-1) for k in ("alpha", "gamma", "beta"))


# ------------------------------------------------------------------------------------------ 1. the fixtures against the float64 stages
@pytest.mark.parametrize("name", FIXTURES)
def test_branch_gcts_reproduce_the_recording(name, golden):
    g = golden(name)
    x = flat(g["in_x"])
    eps = [float(e) for e in g["meta_gct_eps"]]
    for k, b in enumerate(BRANCHES):
        want, tol, _, _ = gct_stage_ref(x, 0.0, *gct_params(g, b + ".GCT."), eps[k])
        other = gct_stage_ref(x, 0.0, *gct_params(g, BRANCHES[(k + 1) % 4] + ".GCT."), eps[k])[0]
        _check_bound(flat(g[b + "_gct_out"]), want, tol, other, f"{name}: {b}.GCT, the next branch's parameters")
        assert float((tol / want.abs().clamp_min(1e-30)).median()) < 64 * U                  # of the size of float32 roundings


@pytest.mark.parametrize("name", FIXTURES)
def test_pooled_branch_reproduces_the_recording(name, golden):
    """relu(W mean(x)) (aspp.py:46-48): the mean to its bound, then 512 products and additions in any order."""
    g = golden(name)
    x = flat(g["in_x"])
    N, C, hw = x.shape
    W = t64(g["p_global_avg_pool.1.weight"]).reshape(128, C)
    mean, dmean = plane_stats_ref(x.reshape(N * C, hw))["mean"]
    mean, dmean = mean.view(N, C), dmean.view(N, C)
    want = torch.relu(mean @ W.t())
    tol = dmean @ W.abs().t() + gamma(C + 1) * ((mean.abs() + dmean) @ W.abs().t())
    slip = torch.relu((x[:, :, :-1].sum(2) / hw) @ W.t())                                  # the last pixel left out of the pool
    got = t64(g["pooled"])
    assert got.shape == (N, 128, 1, 1)
    _check_bound(got.view(N, 128), want, tol, slip, f"{name}: pooled branch")


def merge_args(g):
    xs = [flat(g[b + "_conv_out"]) for b in BRANCHES]
    ws = [t64(g[f"p_{b}.bn.weight"]) for b in BRANCHES]
    bs = [t64(g[f"p_{b}.bn.bias"]) for b in BRANCHES]
    groups = {int(n) for n, c in g["meta_norm_groups"][:4]}
    assert groups == {32} and all(int(c) == 128 for n, c in g["meta_norm_groups"][:4])       # planes / 4 (aspp.py:13)
    return xs, 32, ws, bs, float(g["meta_norm_eps"][0]), t64(g["pooled"]).reshape(xs[0].shape[0], -1)


@pytest.mark.parametrize("name", FIXTURES)
def test_concatenation_reproduces_the_recording(name, golden):
    g = golden(name)
    args = merge_args(g)
    want, tol = cat_ref(*args, f32_stats=True)
    got = flat(g["cat"])
    assert got.shape[1] == 640
    for what, slip in (("branches reversed", cat_ref(*args, order=[3, 2, 1, 0, 4])[0]), ("the pooled branch first", cat_ref(*args, order=[4, 0, 1, 2, 3])[0]),
                       ("statistics per channel", cat_ref(*args, slip="per_channel")[0]), ("the pooled branch at pixel 0 only", cat_ref(*args, slip="tail_first_pixel")[0])):
        _check_bound(got, want, tol, slip, f"{name}: concatenation, {what}")
    # the broadcast is exact: every pixel of a pooled plane holds the recorded value
    assert np.array_equal(g["cat"][:, 512:], np.broadcast_to(g["pooled"], g["cat"][:, 512:].shape))
    # GCT(640) on top of it, from the recorded concatenation (exact input) ...
    p = gct_params(g, "GCT.")
    eps = float(g["meta_gct_eps"][4])
    gated, gtol, _, _ = gct_stage_ref(got, 0.0, *p, eps)
    rolled = tuple(t.roll(1) for t in p)
    _check_bound(flat(g["cat_gated"]), gated, gtol, gct_stage_ref(got, 0.0, *rolled, eps)[0], f"{name}: GCT(640), parameters rolled by one channel")
    # ... and as a chain from the convolution outputs, the concatenation's own bound carried through the gate
    chained, ctol, _, _ = gct_stage_ref(want, tol, *p, eps)
    _check_bound(flat(g["cat_gated"]), chained, ctol, gct_stage_ref(cat_ref(*args, order=[3, 2, 1, 0, 4])[0], tol, *p, eps)[0],
                 f"{name}: merge as a chain, branches reversed")


def test_aspp_torch_reproduces_the_recorded_tail(golden):
    """aspp_torch itself (the yardstick of the GPU module test) cannot be run on the fixture: the 3 x 3 weights are not recorded.  Its last
    lines can: GroupNorm(32) + ReLU of the recorded conv1 output is the recorded result."""
    for name in FIXTURES:
        g = golden(name)
        want, tol = cat_ref([flat(g["conv1_out"])], 32, [t64(g["p_bn1.weight"])], [t64(g["p_bn1.bias"])], float(g["meta_norm_eps"][4]), None, f32_stats=True)
        slip = cat_ref([flat(g["conv1_out"])], 32, [t64(g["p_bn1.weight"])], [t64(g["p_bn1.bias"])], 1e-5, None, slip="per_channel")[0]
        _check_bound(flat(g["out"]), want, tol, slip, f"{name}: bn1 + relu")


def test_aspp_torch_float32_is_close_to_float64():
    """The plain-torch restatement runs in both precisions from one state_dict and its float32 error is of the size of float32."""
    from aoc_amd import aspp
    torch.manual_seed(5)
    net = aspp.ASPP()
    x = torch.randn(1, 512, 3, 4)
    f64, f32 = aspp_torch(x, net.state_dict(), torch.float64), aspp_torch(x, net.state_dict(), torch.float32)
    assert f64.dtype == torch.float64 and f32.dtype == torch.float32 and f64.shape == (1, 256, 3, 4)
    assert 0 < float((f32.double() - f64).abs().max()) < 1e-4 * float(f64.abs().max())


# ------------------------------------------------------------------------------------------ 2. the mirror's constructor
@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_has_the_recorded_constructor_facts(name, golden):
    from torch import nn
    from aoc_amd import aspp
    g = golden(name)
    torch.manual_seed(0)
    net = aspp.ASPP()
    sd = net.state_dict()
    want_names = [str(n) for n in g["meta_state_names"]]
    assert list(sd.keys()) == want_names
    for k, shape, dim in zip(want_names, g["meta_state_shapes"], g["meta_state_dims"]):
        assert tuple(sd[k].shape) == tuple(int(v) for v in shape[:int(dim)]), k
    convs = [(k, m) for k, m in net.named_modules() if isinstance(m, nn.Conv2d)]
    assert [k for k, _ in convs] == [str(n) for n in g["meta_conv_names"]]
    for (k, m), row in zip(convs, g["meta_conv_hyper"]):
        have = [m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.dilation[0], m.groups, int(m.bias is not None)]
        assert have == [int(v) for v in row] and m.kernel_size[0] == m.kernel_size[1] and m.padding[0] == m.padding[1] and m.dilation[0] == m.dilation[1], k
    norms = [(k, m) for k, m in net.named_modules() if isinstance(m, nn.GroupNorm)]
    assert [k for k, _ in norms] == [str(n) for n in g["meta_norm_names"]]
    for (k, m), row, eps in zip(norms, g["meta_norm_groups"], g["meta_norm_eps"]):
        assert [m.num_groups, m.num_channels] == [int(v) for v in row] and m.eps == float(eps), k
    assert [b.GCT.epsilon for b in (net.aspp1, net.aspp2, net.aspp3, net.aspp4)] + [net.GCT.epsilon] == [float(e) for e in g["meta_gct_eps"]]
    assert isinstance(net.global_avg_pool, nn.Sequential) and isinstance(net.global_avg_pool[0], nn.AdaptiveAvgPool2d)
    # the recorded parameters load; the four weights the fixture leaves out are the only ones missing
    missing, unexpected = net.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p_")}, strict=False)
    assert sorted(missing) == sorted(["aspp2.atrous_conv.weight", "aspp3.atrous_conv.weight", "aspp4.atrous_conv.weight", "conv1.weight"]) and not unexpected
    # kaiming_normal_ (fan_in, gain sqrt(2)) on every convolution: std = sqrt(2 / (in * k * k)), within 10 % on >= 65 536 draws
    for k, m in convs:
        assert abs(float(m.weight.detach().std()) / (2.0 / (m.in_channels * m.kernel_size[0] ** 2)) ** 0.5 - 1.0) < 0.1, k


# ------------------------------------------------------------------------------------------ 3. argument validation
@pytest.fixture(scope="module")
def L():
    """The rejections need no device, only the library: one that cannot be loaded fails these tests."""
    import aoc_amd
    return aoc_amd._lib.lib()


INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4


def ptrs(*bufs):
    return (ctypes.c_void_p * len(bufs))(*[ctypes.cast(b, ctypes.c_void_p).value if b is not None else None for b in bufs])


def test_plane_sum_sumsq_and_gct_gate_multi_reject_bad_arguments(L):
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ps = lambda x=p, planes=3, hw=7, s=p, q=p, m=p: L.aoc_plane_sum_sumsq(x, planes, hw, s, q, m, None)
    assert ps(x=None) == INVALID and ps(planes=0) == INVALID and ps(hw=0) == INVALID and ps(hw=-3) == INVALID
    assert ps(s=None, q=None, m=None) == INVALID                                           # all three outputs NULL
    assert ps(planes=2 ** 31) == UNSUPPORTED
    gg = lambda s=p, a=p, g=p, b=p, n_sets=4, N=2, C=5, gate=p: L.aoc_gct_gate_multi(s, a, g, b, n_sets, N, C, 1e-5, 0, gate, None)
    assert gg(s=None) == INVALID and gg(a=None) == INVALID and gg(g=None) == INVALID and gg(b=None) == INVALID and gg(gate=None) == INVALID
    assert gg(n_sets=0) == INVALID and gg(N=0) == INVALID and gg(C=0) == INVALID and gg(n_sets=-1) == INVALID


def test_channel_scale_multi_rejects_bad_arguments(L):
    bufs = [(ctypes.c_float * 64)() for _ in range(10)]
    x, gains = bufs[8], ctypes.cast(bufs[9], ctypes.c_void_p)
    xp = ctypes.cast(x, ctypes.c_void_p)
    cs = lambda x=xp, g=gains, n_out=2, planes=3, hw=7, ys=ptrs(bufs[0], bufs[1]): L.aoc_channel_scale_multi(x, g, n_out, planes, hw, ys, None)
    assert cs(x=None) == INVALID and cs(g=None) == INVALID and cs(ys=None) == INVALID and cs(planes=0) == INVALID and cs(hw=0) == INVALID
    assert cs(n_out=0) == INVALID and cs(n_out=9, ys=ptrs(*bufs[:8], bufs[0])) == INVALID
    assert cs(ys=ptrs(bufs[0], None)) == INVALID
    assert cs(planes=70000) == UNSUPPORTED
    # aliasing: an output on x with a second output, two outputs on one buffer, an output that overlaps x without being x
    assert cs(ys=ptrs(x, bufs[1])) == INVALID and cs(ys=ptrs(bufs[0], bufs[0])) == INVALID
    shifted = ctypes.c_void_p(xp.value + 4)
    assert L.aoc_channel_scale_multi(xp, gains, 1, 3, 7, (ctypes.c_void_p * 1)(shifted), None) == INVALID
    assert L.aoc_channel_scale_multi(xp, gains, 2, 3, 7, (ctypes.c_void_p * 2)(ctypes.cast(bufs[0], ctypes.c_void_p).value, shifted), None) == INVALID


def test_groupnorm_cat_relu_rejects_bad_arguments(L):
    bufs = [(ctypes.c_float * 512)() for _ in range(12)]
    p = lambda i: ctypes.cast(bufs[i], ctypes.c_void_p)
    need = L.aoc_groupnorm_cat_relu_workspace_bytes(2, 2, 4)
    assert need >= 2 * 2 * 4 * 2 * 4 and L.aoc_groupnorm_cat_relu_workspace_bytes(0, 2, 4) == 0 and L.aoc_groupnorm_cat_relu_workspace_bytes(9, 2, 4) == 0
    assert L.aoc_groupnorm_cat_relu_workspace_bytes(2, 0, 4) == 0 and L.aoc_groupnorm_cat_relu_workspace_bytes(2, 2, 0) == 0

    def gn(xs=ptrs(bufs[0], bufs[1]), n_src=2, N=2, C=8, hw=3, groups=4, tail=p(8), C_tail=3, y=p(9), sq=p(10), ws=p(11), nbytes=need):
        return L.aoc_groupnorm_cat_relu(xs, n_src, N, C, hw, groups, p(6), p(7), 1e-5, tail, C_tail, 1, y, sq, ws, nbytes, None)
    assert gn(xs=None) == INVALID and gn(y=None) == INVALID and gn(ws=None) == INVALID and gn(xs=ptrs(bufs[0], None)) == INVALID
    assert gn(n_src=0) == INVALID and gn(n_src=9, xs=ptrs(*bufs[:8], bufs[0])) == INVALID
    assert gn(N=0) == INVALID and gn(C=0) == INVALID and gn(hw=0) == INVALID and gn(groups=0) == INVALID
    assert gn(C=8, groups=3) == INVALID                                                     # C_src % groups != 0
    assert gn(C_tail=-1) == INVALID and gn(tail=None, C_tail=3) == INVALID
    assert gn(nbytes=need - 1) == WORKSPACE and gn(nbytes=0) == WORKSPACE
    assert gn(y=p(0)) == INVALID and gn(y=p(1)) == INVALID and gn(y=p(8)) == INVALID        # y on a source, on the tail
    assert gn(y=ctypes.c_void_p(p(1).value + 4 * 40)) == INVALID                            # y begins inside a source
    assert gn(y=p(6)) == INVALID and gn(y=p(7)) == INVALID and gn(y=p(11)) == INVALID       # y on gamma, on beta, on the workspace
    assert gn(sq=p(9)) == INVALID and gn(sq=p(0)) == INVALID and gn(sq=p(6)) == INVALID and gn(sq=p(8)) == INVALID and gn(sq=p(11)) == INVALID
    assert gn(ws=p(1)) == INVALID and gn(ws=p(7)) == INVALID and gn(ws=p(8)) == INVALID     # the statistics on a source, on beta, on the tail


def test_wrappers_reject_mismatched_shapes_without_a_device():
    from aoc_amd import _lib, ops
    x = torch.zeros(2, 5, 3, 4)
    with pytest.raises(ValueError):
        ops.plane_sum_sumsq(x, want_sum=False, want_sumsq=False, want_mean=False)
    with pytest.raises(ValueError):
        ops.plane_sum_sumsq(torch.zeros(7))
    s = torch.zeros(2, 5)
    with pytest.raises(ValueError):
        ops.gct_gate_multi(s, torch.zeros(4, 6), torch.zeros(4, 6), torch.zeros(4, 6), 1e-5)          # 6 channels against 5
    with pytest.raises(ValueError):
        ops.gct_gate_multi(s, torch.zeros(4, 5), torch.zeros(3, 5), torch.zeros(4, 5), 1e-5)          # 4, 3 and 4 sets
    with pytest.raises(ValueError):
        ops.gct_gate_multi(torch.zeros(2, 5, 1), torch.zeros(4, 5), torch.zeros(4, 5), torch.zeros(4, 5), 1e-5)
    with pytest.raises(ValueError):
        ops.channel_scale_multi(x, torch.zeros(4, 2, 6))
    with pytest.raises(ValueError):
        ops.channel_scale_multi(x, torch.zeros(9, 2, 5))
    with pytest.raises(ValueError):
        ops.channel_scale_multi(x, torch.zeros(2, 2, 5), outs=[torch.zeros(2, 5, 3, 4)])
    with pytest.raises(ValueError):
        ops.channel_scale_multi(x, torch.zeros(1, 2, 5), outs=[torch.zeros(2, 5, 4, 3)])
    xs = [torch.zeros(2, 8, 3, 4), torch.zeros(2, 8, 3, 4)]
    with pytest.raises(ValueError):
        ops.groupnorm_cat_relu(xs, 3, None, None)                                                       # 8 channels, 3 groups
    with pytest.raises(ValueError):
        ops.groupnorm_cat_relu([xs[0], torch.zeros(2, 8, 4, 3)], 4, None, None)
    with pytest.raises(ValueError):
        ops.groupnorm_cat_relu([], 4, None, None)
    with pytest.raises(ValueError):
        ops.groupnorm_cat_relu(xs * 5, 4, None, None)
    with pytest.raises(ValueError):
        ops.groupnorm_cat_relu(xs, 4, torch.zeros(3, 8), None)                                          # affine rows for three sources
    with pytest.raises(ValueError):
        ops.groupnorm_cat_relu(xs, 4, torch.zeros(2, 7), None)
    with pytest.raises(ValueError):
        ops.groupnorm_cat_relu(xs, 4, None, None, tail=torch.zeros(3, 5))                               # the tail of another batch
    with pytest.raises(ValueError):
        ops.groupnorm_cat_relu(xs, 4, None, None, tail=torch.zeros(2, 5), out=torch.zeros(2, 16, 3, 4)) # 21 channels wanted
    with pytest.raises(_lib.AocHipError):                                                                # well-formed, but on the CPU: no fallback
        ops.groupnorm_cat_relu(xs, 4, None, None, tail=torch.zeros(2, 5))
    with pytest.raises(_lib.AocHipError):
        ops.plane_sum_sumsq(x)
