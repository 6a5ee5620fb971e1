"""The decoder's tail without a GPU (tests/decoder_tail_bounds.py holds the references and the derivation of every bound):

1. the float64 matrix reference reproduces what the reference's own decoder_final hands to IA10 and gets back from it (golden fixtures
   decoder_shortcut_*), under the kernel bound widened by the float32 reference's own error (torch_f32 in the bounds module);
2. the same for the prediction head (logit_head_*);
3. np.float32 restatements of bicubic_scale_kernel / cat_scale_low_kernel and of logit_head_kernel, operation by operation, lie inside the
   bounds, and every slip the GPU tests use lies outside them (fmaf restated as in test_decoder_bounds_host.py);
4. the entry points reject bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import decoder_tail_bounds as tb
from decoder_tail_bounds import LOGIT_SLIPS, RESIZE_SLIPS, live_resize_slips, logit_inputs_random, resize_inputs, resize_slip
from float64_bounds import U, _check_bound, gamma, t64

f32 = np.float32
SHORTCUT_GOLDENS = ["decoder_shortcut_O3", "decoder_shortcut_O1", "decoder_shortcut_O4_odd"]
LOGIT_GOLDENS = ["logit_head_O1", "logit_head_O2", "logit_head_O4"]
def shortcut_inputs(g):
    """The golden's inputs of the shortcut stage in float64: x, the shortcut branch after its ReLU (what the reference concatenated), the
    head and IA10's Linear."""
    x = t64(g["in_x"])
    Ce = x.shape[1]
    return x, t64(g["ia10_in_x"][:, Ce:]), t64(g["in_IA_head"]), t64(g["p_IA10.IA.weight"]), t64(g["p_IA10.IA.bias"])


# ------------------------------------------------------------------------------------------ 1. golden shortcut fixtures
@pytest.mark.parametrize("name", SHORTCUT_GOLDENS)
def test_reference_reproduces_the_golden_upsample_and_concat(name, golden):
    g = golden(name)
    x, low, head, weight, bias = shortcut_inputs(g)
    N, Ce, h, w = x.shape
    H, W = low.shape[2:]
    want, tol = tb.cat_scale_ref(x, low, None, H, W, None, (tb.torch_coordinate_error(h), tb.torch_coordinate_error(w)))
    got = torch.from_numpy(g["ia10_in_x"])
    for kind in RESIZE_SLIPS:
        _check_bound(got, want, tol, torch.cat([resize_slip(kind, x, H, W), low], 1), f"{name}: IA10 input, slip {kind}")
    _check_bound(got, want, tol, torch.cat([low, want[:, :Ce]], 1), f"{name}: IA10 input, concat order reversed")
    assert float(tol.max()) < 1e-4                       # the widened bound is still of the size of float32 roundings


@pytest.mark.parametrize("name", SHORTCUT_GOLDENS)
def test_reference_reproduces_the_golden_head_and_gate(name, golden):
    g = golden(name)
    x, low, head, weight, bias = shortcut_inputs(g)
    D = head.shape[1]
    ref = tb.shortcut_stage_ref(x, low, head, weight, bias, torch_f32=True)
    no_minus = tb.shortcut_stage_ref(x, low, head, weight, bias, slip="no_minus")
    rev = tb.shortcut_stage_ref(x, low, head, weight, bias, slip="concat_reversed")
    got_head = torch.from_numpy(g["ia10_in_head"])
    assert torch.equal(got_head[:, :D].double(), head)
    _check_bound(got_head, ref["head"], ref["dhead"], no_minus["head"], f"{name}: px1_delta without - px1")
    if x.shape[0] > 1:                                   # one object: px1_delta is 0 in any channel order
        _check_bound(got_head, ref["head"], ref["dhead"], rev["head"], f"{name}: px1_delta of the reversed concatenation")
    for what, slip in (("no_minus", no_minus), ("concat_reversed", rev)):
        _check_bound(torch.from_numpy(g["ia10_out"]), ref["out"], ref["dout"], slip["out"], f"{name}: IA10 output, slip {what}")
    if x.shape[0] == 1:
        assert float(ref["head"][:, D:].abs().max()) == 0.0            # one object: px1_delta is identically 0


# ------------------------------------------------------------------------------------------ 2. golden logit fixtures
def logit_inputs(g):
    """x [N, C, hw] and the two IA_final outputs [N, C + 1] in float64, with what a float32 nn.Linear of D terms is off by."""
    x, head = t64(g["in_x"]), t64(g["in_IA_head"])
    N, C = x.shape[:2]
    D = head.shape[1]
    out = [x.reshape(N, C, -1)]
    for k in ("fg", "bg"):
        w, b = t64(g[f"p_{k}_weight"]), t64(g[f"p_{k}_bias"])
        out += [head @ w.t() + b, gamma(D + 1) * (head.abs() @ w.abs().t() + b.abs())]
    return out


@pytest.mark.parametrize("name", LOGIT_GOLDENS)
def test_reference_reproduces_the_golden_prediction(name, golden):
    g = golden(name)
    x, wb_fg, dfg, wb_bg, dbg = logit_inputs(g)
    N = x.shape[0]
    want, tol = tb.logit_head_ref(x, wb_fg, wb_bg, None, dfg, dbg)
    got = torch.from_numpy(g["pred"]).reshape(N, -1)
    assert g["pred"].shape[:2] == (1, N)
    if N == 1:
        _check_bound(got, want, tol, tb.logit_head_ref(x, wb_bg, wb_bg)[0], f"{name}: the bg head for the fg head")
        return
    for slip in LOGIT_SLIPS:
        if slip == "max" and N == 2:
            continue                                     # one other object: min and max coincide
        _check_bound(got, want, tol, tb.logit_head_ref(x, wb_fg, wb_bg, slip)[0], f"{name}: slip {slip}")


# ------------------------------------------------------------------------------------------ 3. step-by-step emulation
def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def taps_emulate(n_in, n_out):
    """bicubic_taps of decoder_tail.hip: -> i0 [out], weights [out, 4] float32."""
    o = np.arange(n_out, dtype=np.int64)
    i0, t = np.zeros(n_out, np.int64), np.zeros(n_out, f32)
    if n_out > 1:
        num = o * (n_in - 1)
        i0 = num // (n_out - 1)
        t = (num - i0 * (n_out - 1)).astype(f32) / f32(n_out - 1)
    A = f32(-0.75)
    one = f32(1)
    x0, u = t + one, one - t
    x3 = u + one
    c2 = lambda x: ((A * x - f32(-3.75)) * x + f32(-6)) * x - f32(-3)
    c1 = lambda x: (f32(1.25) * x - f32(2.25)) * x * x + one
    w = np.stack([c2(x0), c1(t), c1(u), c2(x3)], 1)
    assert w.dtype == f32 and t.dtype == f32
    return i0, w


def tap_sum_emulate(w, xs):
    """w [..., 4] broadcast against the four tap values xs: fma(w3, x3, fma(w2, x2, fma(w1, x1, w0 x0)))."""
    acc = w[0] * xs[0]
    for k in (1, 2, 3):
        acc = fma32(np.broadcast_to(w[k], acc.shape), xs[k], acc)
    return acc


def cat_scale_emulate(x, low, gain, H, W):
    N, Ce, h, w = x.shape
    iy, wy = taps_emulate(h, H)
    ix, wx = taps_emulate(w, W)
    rows = [np.clip(iy + k, 0, h - 1) for k in (-1, 0, 1, 2)]
    cols = [np.clip(ix + k, 0, w - 1) for k in (-1, 0, 1, 2)]
    v = tap_sum_emulate([wy[:, k].reshape(1, 1, H, 1) for k in range(4)], [x[:, :, r, :] for r in rows])           # [N, Ce, H, w]
    s = tap_sum_emulate([wx[:, k].reshape(1, 1, 1, W) for k in range(4)], [v[:, :, :, c] for c in cols])           # [N, Ce, H, W]
    full = s if low is None else np.concatenate([s, low], 1)
    assert full.dtype == f32
    return full if gain is None else gain[:, :, None, None] * full


def logit_head_emulate(x, wb_fg, wb_bg):
    N, C, hw = x.shape

    def head(wb, n):
        s = np.zeros(hw, f32)
        for c in range(C):
            s = s + wb[n, c] * x[n, c]
        return s + wb[n, C]
    pred = np.stack([head(wb_fg, n) for n in range(N)])
    if N > 1:
        pred[0] = pred[0] + np.stack([head(wb_bg, n) for n in range(1, N)]).min(0)
    assert pred.dtype == f32
    return pred


RESIZE_HOST_CASES = [(2, 3, 2, 5, 7, 9, 14), (2, 2, 2, 2, 2, 33, 65), (3, 5, 3, 9, 6, 4, 5), (1, 2, 1, 31, 54, 121, 213), (2, 2, 1, 3, 4, 1, 1)]


@pytest.mark.parametrize("N,Ce,Cr,h,w,H,W", RESIZE_HOST_CASES)
def test_cat_scale_bound_holds_the_emulation_and_sheds_the_slips(N, Ce, Cr, h, w, H, W):
    rng = np.random.RandomState(h * 100 + W)
    x, low, gain = resize_inputs(rng, N, Ce, Cr, h, w, H, W)
    for with_gain in (True, False):
        g = gain if with_gain else None
        got = cat_scale_emulate(x, low, g, H, W)
        want, tol = tb.cat_scale_ref(t64(x), t64(low), t64(g), H, W)
        gv = t64(g).view(N, -1, 1, 1) if with_gain else 1.0
        slips = live_resize_slips(t64(x), H, W, want[:, :Ce] / (gv[:, :Ce] if with_gain else 1.0))
        assert slips
        for kind, s in slips.items():
            _check_bound(torch.from_numpy(got), want, tol, gv * torch.cat([s, t64(low)], 1), f"cat_scale emulation {h}x{w}->{H}x{W} gain={with_gain} {kind}")
        rev = gv * torch.cat([t64(low), want[:, :Ce] / (gv[:, :Ce] if with_gain else 1.0)], 1)
        _check_bound(torch.from_numpy(got), want, tol, rev, f"cat_scale emulation {h}x{w}->{H}x{W} gain={with_gain} concat reversed")


def test_identity_size_emulation_is_bit_equal():
    rng = np.random.RandomState(5)
    x = rng.standard_normal((1, 2, 7, 9)).astype(f32)
    assert np.array_equal(cat_scale_emulate(x, None, None, 7, 9), x)


def test_cat_scale_bound_is_of_the_size_of_float32():
    rng = np.random.RandomState(1)
    x, low, gain = resize_inputs(rng, 1, 2, 1, 31, 54, 121, 213)
    want, tol = tb.cat_scale_ref(t64(x), t64(low), t64(gain), 121, 213)
    assert float(tol.max()) < 256 * U * float(want.abs().max())          # a few dozen roundings of the largest output, not a fitted 1e-3


def test_plane_mean_identity():
    """The mean of the float64 upsample equals the weighted sum of the coarse plane with the matrices' column sums."""
    rng = np.random.RandomState(2)
    for h, w, H, W in [(5, 7, 9, 14), (61, 107, 121, 213), (2, 2, 33, 65), (9, 6, 4, 5), (1, 1, 4, 6), (3, 4, 1, 1)]:
        x = torch.from_numpy(rng.standard_normal((3, h, w)))
        want, tol = tb.bicubic_plane_mean_ref(x, H, W)
        full = tb.bicubic_resize(x, H, W).mean((1, 2))
        assert float((want - full).abs().max()) < 64 * 2.0 ** -53 * float(x.abs().max())
        assert float(tol.max()) < 1e-4 * float(x.abs().max())


LOGIT_HOST_CASES = [(1, 128, 30), (2, 8, 1), (4, 13, 257), (30, 16, 65)]


@pytest.mark.parametrize("N,C,hw", LOGIT_HOST_CASES)
def test_logit_head_bound_holds_the_emulation_and_sheds_the_slips(N, C, hw):
    rng = np.random.RandomState(N * 100 + C + hw)
    x, wb_fg, wb_bg = logit_inputs_random(rng, N, C, hw)
    got = torch.from_numpy(logit_head_emulate(x, wb_fg, wb_bg))
    args = (t64(x), t64(wb_fg), t64(wb_bg))
    want, tol = tb.logit_head_ref(*args)
    if N == 1:
        _check_bound(got, want, tol, tb.logit_head_ref(args[0], args[2], args[2])[0], f"logit_head emulation N=1 C={C}: bg head for fg head")
        return
    for slip in LOGIT_SLIPS:
        if slip == "max" and N == 2:
            continue
        _check_bound(got, want, tol, tb.logit_head_ref(*args, slip)[0], f"logit_head emulation N={N} C={C} hw={hw} slip={slip}")


# ------------------------------------------------------------------------------------------ 4. argument validation
@pytest.fixture(scope="module")
def L():
    try:
        import aoc_amd
        return aoc_amd._lib.lib()
    except (OSError, ImportError, RuntimeError) as e:
        pytest.skip(f"the HIP library cannot be loaded here: {e}")


def test_entry_points_reject_bad_arguments_before_any_launch(L):
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.aoc_bicubic_plane_mean(None, 1, 2, 2, 4, 4, p, None) == INVALID
    assert L.aoc_bicubic_plane_mean(p, 1, 2, 2, 4, 4, None, None) == INVALID
    assert L.aoc_bicubic_plane_mean(p, 0, 2, 2, 4, 4, p, None) == INVALID
    assert L.aoc_bicubic_plane_mean(p, 1, 0, 2, 4, 4, p, None) == INVALID
    assert L.aoc_bicubic_plane_mean(p, 1, 2, 2, 4, -1, p, None) == INVALID
    assert L.aoc_bicubic_cat_scale(None, p, p, 1, 1, 1, 2, 2, 4, 4, p, None) == INVALID
    assert L.aoc_bicubic_cat_scale(p, None, p, 1, 1, 1, 2, 2, 4, 4, p, None) == INVALID              # Cr > 0 needs low
    assert L.aoc_bicubic_cat_scale(p, p, p, 1, 1, 1, 2, 2, 4, 4, None, None) == INVALID
    assert L.aoc_bicubic_cat_scale(p, p, p, 0, 1, 1, 2, 2, 4, 4, p, None) == INVALID
    assert L.aoc_bicubic_cat_scale(p, p, p, 1, 0, 1, 2, 2, 4, 4, p, None) == INVALID
    assert L.aoc_bicubic_cat_scale(p, p, p, 1, 1, -1, 2, 2, 4, 4, p, None) == INVALID
    assert L.aoc_bicubic_cat_scale(p, p, p, 1, 1, 1, 2, 2, 0, 4, p, None) == INVALID
    assert L.aoc_bicubic_cat_scale(p, p, p, 31, 1, 1, 2, 2, 4, 4, p, None) == UNSUPPORTED
    need = L.aoc_shortcut_stage_workspace_bytes(3, 4, 2, 5)
    assert need >= 4 * (3 * 6 + 3 * 11 + 3 * 6)
    assert L.aoc_shortcut_stage_workspace_bytes(31, 4, 2, 5) == 0 and L.aoc_shortcut_stage_workspace_bytes(3, 0, 2, 5) == 0
    stage = lambda x=p, low=p, head=p, w=p, N=3, Ce=4, Cr=2, D=5, h=2, H=4, out=p, ws=p, nbytes=need: L.aoc_shortcut_stage_enqueue(
        x, low, head, w, p, N, Ce, Cr, D, h, 2, H, 4, out, None, None, ws, nbytes, None)
    assert stage(x=None) == INVALID and stage(low=None) == INVALID and stage(head=None) == INVALID and stage(w=None) == INVALID
    assert stage(out=None) == INVALID and stage(ws=None) == INVALID
    assert stage(N=0) == INVALID and stage(Ce=0) == INVALID and stage(D=0) == INVALID and stage(h=0) == INVALID and stage(H=-3) == INVALID
    assert stage(N=31) == UNSUPPORTED
    assert stage(nbytes=need - 1) == WORKSPACE
    assert L.aoc_logit_head(None, p, p, 9, 2, 8, 16, p, None) == INVALID
    assert L.aoc_logit_head(p, None, p, 9, 2, 8, 16, p, None) == INVALID
    assert L.aoc_logit_head(p, p, None, 9, 2, 8, 16, p, None) == INVALID                             # N > 1 needs the bg head
    assert L.aoc_logit_head(p, p, p, 9, 2, 8, 16, None, None) == INVALID
    assert L.aoc_logit_head(p, p, p, 8, 2, 8, 16, p, None) == INVALID                                # rows shorter than C + 1
    assert L.aoc_logit_head(p, p, p, 9, 0, 8, 16, p, None) == INVALID
    assert L.aoc_logit_head(p, p, p, 9, 2, 0, 16, p, None) == INVALID
    assert L.aoc_logit_head(p, p, p, 9, 2, 8, 0, p, None) == INVALID
    assert L.aoc_logit_head(p, p, p, 9, 31, 8, 16, p, None) == UNSUPPORTED
    assert L.aoc_background_merge(None, p, 2, 16, p, None) == INVALID and L.aoc_background_merge(p, None, 2, 16, p, None) == INVALID
    assert L.aoc_background_merge(p, p, 2, 0, p, None) == INVALID and L.aoc_background_merge(p, p, 31, 16, p, None) == UNSUPPORTED
