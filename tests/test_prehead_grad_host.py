"""What can be checked without a GPU about the differentiable DynamicPreHead (aoc_amd.prehead_train, csrc/prehead_grad.hip): the float64
reference of tests/prehead_grad_bounds.py against torch's float64 autograd of ``nn.Conv2d`` / ``nn.GroupNorm`` / ``nn.ReLU`` / ``cat(expand)``
and against the gradients recorded from the reference's own DynamicPreHead (tests/golden/prehead_grad_*.npz); that every slipped reference
leaves its bound; that no element of any GPU case is undecided; the twin's surface; the entry point's argument checks (a rejected call
enqueues nothing, so they need no device)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

import aoc_amd
import prehead_grad_bounds as pgb
from aoc_amd import _lib, hotpath, ops, prehead_train as pt
from conftest import GOLDEN, load_golden

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4
f32, f64 = np.float32, np.float64


def _close(got, want, what, rel, scale=0.0):
    """scale: the size of the terms that cancel in `want`, where the result is what they leave behind"""
    got, want = pgb.t64(got), pgb.t64(want)
    got = got.reshape(want.shape)
    assert (got - want).abs().max() <= rel * max(float(want.abs().max()), scale, 1e-30), f"{what}: off by {float((got - want).abs().max()):.3e}"


def _leaf(a):
    return torch.from_numpy(np.asarray(a, f64)).requires_grad_(True) if a is not None else None


# ------------------------------------------------------------------------------------------ the reference against float64 autograd
@pytest.mark.parametrize("O,n_in,n_out,groups,h,w,C", ((2, 3, 4, 4, 1, 1, 0), (2, 5, 8, 2, 3, 5, 4), (3, 24, 64, 16, 5, 7, 6), (4, 7, 12, 3, 9, 11, 0)))
def test_reference_against_autograd(O, n_in, n_out, groups, h, w, C):
    """nn.Conv2d(n_in, n_out, 1), nn.GroupNorm, nn.ReLU and torch.cat with the expanded embedding, in float64 (2, 3, 4, 4, 1, 1: one element per
    group)"""
    rs = pgb.rng(O, n_in, n_out, groups, h, w, C)
    n = rs.standard_normal
    conv, bn = nn.Conv2d(n_in, n_out, 1).double(), nn.GroupNorm(groups, n_out, eps=pgb.eps32(1e-5)).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(1 + 0.5 * n(n_out)))
        bn.bias.copy_(torch.from_numpy(n(n_out)))
    x, emb, gy = _leaf(n((O, n_in, h, w))), _leaf(n((C, h, w)) if C else None), n((O, C + n_out, h, w))
    out = nn.ReLU()(bn(conv(x)))
    if C:
        out = torch.cat((emb.unsqueeze(0).expand(O, -1, -1, -1), out), 1)
    (out * torch.from_numpy(gy)).sum().backward()
    got, _ = pgb.prehead_grad_ref(gy.reshape(O, C + n_out, -1), x.detach().reshape(O, n_in, -1), conv.weight.detach(), conv.bias.detach(), groups,
                                  bn.weight.detach(), bn.bias.detach(), 1e-5, C)
    big = float(np.abs(gy).max()) * 1e3                   # rstd up to eps^-1/2 (one element per group) times what cancels
    _close(got["grad_feat"][0], x.grad, "grad_feat", 1e-12, big)
    _close(got["grad_weight"][0], conv.weight.grad, "grad_weight", 1e-12, big)
    _close(got["grad_bias"][0], conv.bias.grad, "grad_bias", 1e-12, big)
    _close(got["grad_gamma"][0], bn.weight.grad, "grad_gamma", 1e-12, big)
    _close(got["grad_beta"][0], bn.bias.grad, "grad_beta", 1e-12)
    if C:
        _close(got["grad_emb"][0].t(), emb.grad.reshape(C, -1), "grad_emb", 1e-12)
    else:
        assert got["grad_emb"] is None


# ------------------------------------------------------------------------------------------ the reference against the recorded gradients
@pytest.mark.parametrize("name", pgb.FIXTURES)
def test_reference_reproduces_the_recorded_gradients(name):
    """The reference's own DynamicPreHead (decoding_module.py:228-240) and aocnet.py:362 in float64, recorded by
    tests/golden/make_golden_prehead_grad.py.  nn.GroupNorm's eps is the double 1e-5, the kernels' (and the reference function's) the float 1e-5:
    4e-13 of var + eps, inside the 1e-10."""
    z = load_golden(name)
    args, C = pgb.fixture_args(z)
    got, und = pgb.prehead_grad_ref(**args)
    assert int(und.sum()) == 0
    rel = 1e-10
    scale = float(np.abs(z["in_weight"]).max()) * 10
    _close(got["grad_feat"][0], z["grad_x"], "grad_x", rel, scale)
    _close(got["grad_weight"][0], z["grad_conv_w"], "grad_conv_w", rel, scale)
    _close(got["grad_bias"][0], z["grad_conv_b"], "grad_conv_b", rel, scale)
    _close(got["grad_gamma"][0], z["grad_gn_w"], "grad_gn_w", rel, scale)
    _close(got["grad_beta"][0], z["grad_gn_b"], "grad_gn_b", rel)
    if C:
        _close(got["grad_emb"][0].t(), z["grad_emb"].reshape(C, -1), "grad_emb", rel)
    out = pgb.forward64(*(torch.from_numpy(np.asarray(a, f64)) for a in (z["in_x"], z["w_conv_w"], z["w_conv_b"])), int(z["groups"]),
                        torch.from_numpy(z["w_gn_w"].astype(f64)), torch.from_numpy(z["w_gn_b"].astype(f64)), float(z["eps"]),
                        torch.from_numpy(z["in_emb"].astype(f64)).permute(1, 2, 0) if C else None)
    loss = float((out * torch.from_numpy(z["in_weight"].astype(f64))).sum())
    assert abs(loss - float(z["loss"])) <= 1e-10 * max(abs(float(z["loss"])), 1.0)


def test_fixtures_are_small_and_cover_the_cases():
    seen = set()
    for name in pgb.FIXTURES:
        size = os.path.getsize(os.path.join(GOLDEN, name + ".npz"))
        assert size < 100_000, f"{name}: {size} bytes"
        z = load_golden(name)
        assert "out" not in z and not any(k.startswith("act") for k in z), "inputs, parameters and gradients only"
        x = z["in_x"]
        assert x.shape[2] % 2 == 1 and x.shape[3] % 2 == 1 and x.shape[2] <= 9 and x.shape[3] <= 11, "odd maps up to 9 x 11"
        for k in ("in_x", "in_weight", "w_conv_w", "w_conv_b", "w_gn_w", "w_gn_b"):
            assert np.array_equal(z[k].astype(np.float16).astype(f32), z[k]), f"{name} {k}: float16-representable"
        seen.add((x.shape[0], x.shape[1], "in_emb" in z))
    assert {s[0] for s in seen} == {1, 3, 4} and {s[1] for s in seen} == {24, 26} and {s[2] for s in seen} == {True, False}


# ------------------------------------------------------------------------------------------ the bounds
ALL_CASES = tuple((k, s, "case") for k, s in pgb.CASES.items()) + tuple((k, s, "mask") for k, s in pgb.MASK_CASES.items()) \
    + ((pgb.PLANTED, pgb.PLANTED_SEED, "planted"),)


@pytest.mark.parametrize("key,seed,kind", ALL_CASES)
def test_no_gpu_case_has_an_undecided_element_and_every_slip_leaves_its_bound(key, seed, kind):
    O, n_in, n_out, groups, hw, C = key
    s = pgb.planted_case(*key, seed) if kind == "planted" else pgb.case(*key, seed)
    args = pgb.ref_args(s, groups, C)
    ref, und = pgb.prehead_grad_ref(**args)
    assert int(und.sum()) == 0, f"{key} seed {seed}: {int(und.sum())} undecided elements"
    assert pgb.first_seed(key, pgb.planted_case if kind == "planted" else pgb.case) == seed, "the first seed without an undecided element"
    for name in pgb.OUTS:
        if ref[name] is not None:
            assert bool(torch.isfinite(ref[name][1]).all()) and bool((ref[name][1] >= 0).all())
    for slip in pgb.slips_of(n_out, groups, hw, C):
        bad, _ = pgb.prehead_grad_ref(slip=slip, **args)
        o = pgb.SLIPS[slip]
        assert bool(((bad[o][0] - ref[o][0]).abs() > ref[o][1]).any()), f"{key} {slip}: the slipped reference stays inside the bound of {o}"


def test_every_slip_is_exercised():
    seen = set()
    for (O, n_in, n_out, groups, hw, C) in pgb.CASES:
        seen.update(pgb.slips_of(n_out, groups, hw, C))
    assert seen == set(pgb.SLIPS)


# ------------------------------------------------------------------------------------------ the twin's surface
def test_twin_has_the_mirror_surface():
    twin, mirror = pt.DynamicPreHead(in_dim=24, embed_dim=64), hotpath.DynamicPreHead(in_dim=24, embed_dim=64)
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes(twin) == shapes(mirror) and set(shapes(twin)) == {"conv.weight", "conv.bias", "bn.weight", "bn.bias"}
    twin.load_state_dict(mirror.state_dict(), strict=True)
    ref_like = nn.Module()
    ref_like.conv, ref_like.bn = nn.Conv2d(24, 64, 1), nn.GroupNorm(16, 64)
    twin.load_state_dict(ref_like.state_dict(), strict=True)
    assert twin.bn.num_groups == 16
    with pytest.raises(NotImplementedError, match="kernel_size 1 only"):
        pt.DynamicPreHead(in_dim=24, embed_dim=64, kernel_size=3)
    assert "prehead_train" in aoc_amd.__all__ and ops._TRAINABLE["DynamicPreHead"] == "prehead_train.DynamicPreHead"
    assert "prehead_train" in ops.inference_only.__doc__
    with torch.enable_grad():
        with pytest.raises(_lib.AocHipError, match="prehead_train.DynamicPreHead is the differentiable form"):
            mirror(torch.zeros(1, 24, 3, 3))              # its parameters want a gradient: the guard fires before any device work
        with pytest.raises(_lib.AocHipError, match="no CPU fallback"):
            twin(torch.zeros(1, 24, 3, 3))


def test_stats_offset_is_the_forward_workspace_layout():
    L = _lib.lib()
    for O, n_out, groups, hw in ((4, 64, 16, 31 * 33), (1, 128, 128, 257), (30, 64, 16, 35)):
        n_chunks = -(-hw // pt.PIX)
        off = -(-(O * groups * n_chunks * 16) // 256) * 256
        assert L.aoc_prehead_workspace_bytes(O, n_out, n_out // groups, hw) == off + -(-(O * groups * 8) // 256) * 256


# ------------------------------------------------------------------------------------------ argument checks (nothing is enqueued)
def test_entry_point_rejections():
    L = _lib.lib()
    p = ctypes.c_void_p(4096)                              # never dereferenced: every call below is rejected before its first launch

    def call(n_obj=2, n_in=24, n_out=64, groups=16, hw=35, C=3, feat=p, stats=p, outs=(p, p, p, p, p, p), ws=p, ws_bytes=1 << 30):
        return L.aoc_prehead_grad(p, feat, stats, p, p, p, p, n_obj, n_in, n_out, groups, hw, C, *outs, ws, ws_bytes, None)
    assert call(feat=None) == INVALID and call(stats=None) == INVALID and call(hw=0) == INVALID and call(n_obj=0) == INVALID and call(C=-1) == INVALID
    assert call(n_in=33) == UNSUPPORTED and call(n_out=129, groups=3) == UNSUPPORTED and call(groups=5) == UNSUPPORTED and call(n_obj=65536) == UNSUPPORTED
    assert call(C=0) == UNSUPPORTED                        # an embedding gradient without embedding channels
    assert call(ws_bytes=64) == WORKSPACE and call(ws=None) == WORKSPACE
    assert call(outs=(None,) * 6) == OK                    # nothing asked for: nothing to do
    assert L.aoc_prehead_grad_workspace_bytes(2, 24, 64, 5, 35) == 0 and L.aoc_prehead_grad_workspace_bytes(0, 24, 64, 16, 35) == 0
    need = L.aoc_prehead_grad_workspace_bytes(2, 24, 64, 16, 513)
    assert need >= 2 * 64 * 3 * 16 + 2 * 16 * 8 + 2 * 3 * 64 * 25 * 4 and need % 256 == 0
    assert call(hw=513, ws_bytes=need - 1) == WORKSPACE
