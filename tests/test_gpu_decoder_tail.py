"""The kernels of csrc/decoder_tail.hip on the GPU against the float64 references and bounds of tests/decoder_tail_bounds.py: the bicubic
resize + concatenation + gain (aoc_bicubic_cat_scale), the plane means of the upsample from the coarse map (aoc_bicubic_plane_mean), the
shortcut stage as one call (aoc_shortcut_stage_enqueue), the prediction head (aoc_logit_head), and the mirrors of decoder_tail.py.

Every float comparison goes through _check_bound, which also demands that a reference with one deliberate slip leaves the bound:
align_corners=False coordinates, A = -0.5, zero padding instead of clamped taps, h / w weights swapped, the concatenation reversed,
px1_delta without its - px1, the min taken over every object, the augmentation added to every object, max for min.  Outputs are pre-filled
with NaN where the operator takes an output buffer.  test_decoder_tail_host.py checks the same bounds against step-by-step float32
restatements of the kernels and against the reference's own output, without a GPU."""
import types

import numpy as np
import pytest
import torch
from torch import nn

import decoder_tail_bounds as tb
from float64_bounds import U, _check_bound, _wave_dot_tol, t64

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


# ------------------------------------------------------------------------------------------ 1. resize + concatenation + gain
# (N, Ce, Cr, h, w, H, W)
RESIZE_CASES = [
    (2, 3, 2, 5, 7, 9, 14),            # generic non-integer ratio
    (1, 1, 0, 1, 1, 4, 6),             # one source pixel: every tap clamps
    (2, 2, 1, 3, 4, 1, 1),             # H = W = 1: the scale-0 guard
    (1, 2, 1, 7, 9, 7, 9),             # identity size: t = 0 everywhere, output bit-equal to the input
    (2, 2, 2, 2, 2, 33, 65),           # all-border taps at 32x; three bands of 16, 16 and 1 rows
    (3, 5, 3, 9, 6, 4, 5),             # downsampling
    (3, 8, 4, 61, 107, 121, 213),      # map geometry, few channels: eight bands per plane
    # bicubic_scale_kernel walks a band as one run of floats, 256 per workgroup turn and 64 per wave-wide store: rows of one float less
    # than a turn, exactly a turn, and one more (a row then starts 255 / 0 / 1 floats into a turn, and a store straddles two rows)
    (1, 2, 1, 4, 9, 3, 255), (1, 2, 1, 4, 9, 3, 256), (1, 2, 1, 4, 9, 3, 257),
]
RESIZE_MODES = ["gain", "no_gain", "no_low"]


def scaled(want):
    """Where no geometric slip changes the result (one source pixel): the reference off by 2^-10, far inside any fitted tolerance."""
    return want * (1 + 2.0 ** -10)


@pytest.mark.parametrize("mode", RESIZE_MODES)
@pytest.mark.parametrize("N,Ce,Cr,h,w,H,W", RESIZE_CASES)
def test_bicubic_cat_scale(aoc, N, Ce, Cr, h, w, H, W, mode):
    if mode == "no_low":
        Cr = 0
    rng = np.random.RandomState(h * 100 + W + N)
    x, low, gain = tb.resize_inputs(rng, N, Ce, Cr, h, w, H, W)
    if mode == "no_gain":
        gain = None
    out = nan_like(N, Ce + Cr, H, W)
    ret = aoc.ops.bicubic_cat_scale(dev(x), dev(low), dev(gain), size=(H, W), out=out)
    assert ret.data_ptr() == out.data_ptr()
    got = host(out)
    x64, low64, g64 = t64(x), t64(low), t64(gain)
    want, tol = tb.cat_scale_ref(x64, low64, g64, H, W)
    gv = g64.view(N, -1, 1, 1) if gain is not None else torch.ones(1, 1, 1, 1, dtype=torch.float64)
    up = tb.bicubic_resize(x64, H, W)
    cat = lambda u: gv * (u if low is None else torch.cat([u, low64], 1))
    slips = {k: cat(s) for k, s in tb.live_resize_slips(x64, H, W, up).items()}
    if low is not None:
        slips["concat_reversed"] = gv * torch.cat([low64, up], 1)
    if not slips:
        slips["scaled"] = scaled(want)
    for kind, s in slips.items():
        _check_bound(got, want, tol, s, f"bicubic_cat_scale {N}x{Ce}+{Cr} {h}x{w}->{H}x{W} {mode} slip={kind}")
    if (h, w) == (H, W) and gain is None:
        assert torch.equal(got[:, :Ce], torch.from_numpy(x))          # identity size: weights (0, 1, 0, 0) exactly
        if low is not None:
            assert torch.equal(got[:, Ce:], torch.from_numpy(low))


@pytest.mark.parametrize("N,Ce,Cr,h,w,H,W", RESIZE_CASES)
def test_bicubic_plane_mean(aoc, N, Ce, Cr, h, w, H, W):
    rng = np.random.RandomState(h * 100 + W + N + 1)
    x = (rng.standard_normal((N, Ce, h, w)) + 0.5).astype(np.float32)
    got = host(aoc.ops.bicubic_plane_mean(dev(x), (H, W)))
    x64 = t64(x)
    want, tol = tb.bicubic_plane_mean_ref(x64.reshape(N * Ce, h, w), H, W)
    full = tb.bicubic_resize(x64, H, W)
    assert float((want.view(N, Ce) - full.mean((2, 3))).abs().max()) < 64 * 2.0 ** -53 * float(x64.abs().max())       # the identity itself
    slips = {k: s.mean((2, 3)) for k, s in tb.live_resize_slips(x64, H, W, full).items()}
    slips["coarse_mean"] = x64.mean((2, 3))                        # the mean of the coarse plane: the border weights ignored
    # a slip counts where it moves some mean by more than 1e-3 of the largest (a 2 x 2 source is symmetric: its coarse mean IS the mean)
    slips = {k: s for k, s in slips.items() if float((s - want.view(N, Ce)).abs().max()) > 1e-3 * float(want.abs().max())}
    if not slips:
        slips["scaled"] = scaled(want.view(N, Ce))
    for kind, s in slips.items():
        _check_bound(got, want.view(N, Ce), tol.view(N, Ce), s, f"bicubic_plane_mean {N}x{Ce} {h}x{w}->{H}x{W} slip={kind}")


# ------------------------------------------------------------------------------------------ 2. the shortcut stage
def check_stage(aoc, x, low, head, weight, bias, what, golden_out=None):
    N, Ce = x.shape[:2]
    Cr, H, W = low.shape[1:]
    out = nan_like(N, Ce + Cr, H, W)
    ret, px, gain = aoc.ops.shortcut_stage(dev(x), dev(low), dev(head), dev(weight), dev(bias), want_debug=True, out=out)
    assert ret.data_ptr() == out.data_ptr()
    plain = aoc.ops.shortcut_stage(dev(x), dev(low), dev(head), dev(weight), dev(bias))
    assert torch.equal(plain, out)                                 # the optional outputs change nothing
    args = tuple(t64(a) for a in (x, low, head, weight, bias))
    ref = tb.shortcut_stage_ref(*args)
    no_minus = tb.shortcut_stage_ref(*args, slip="no_minus")
    rev = tb.shortcut_stage_ref(*args, slip="concat_reversed")
    acf = tb.shortcut_stage_ref(*args, slip=dict(align_corners=False))
    _check_bound(host(px), ref["px"], ref["dpx"], rev["px"], f"{what}: plane means, concat reversed")
    _check_bound(host(px), ref["px"], ref["dpx"], acf["px"], f"{what}: plane means, align_corners=False")
    _check_bound(host(gain), ref["gain"], ref["dgain"], no_minus["gain"], f"{what}: gain, px1_delta without - px1")
    for kind, s in (("no_minus", no_minus), ("concat_reversed", rev), ("align_corners_false", acf)):
        _check_bound(host(out), ref["out"], ref["dout"], s["out"], f"{what}: output, slip {kind}")
    if golden_out is not None:                                     # and the reference's own float32 result, each side within its own bound
        t32 = tb.shortcut_stage_ref(*args, torch_f32=True)
        assert bool(((host(out).double() - torch.from_numpy(golden_out).double()).abs() <= ref["dout"] + t32["dout"]).all())


@pytest.mark.parametrize("name", ["decoder_shortcut_O3", "decoder_shortcut_O1", "decoder_shortcut_O4_odd"])
def test_shortcut_stage_golden(aoc, golden, name):
    g = golden(name)
    Ce = g["in_x"].shape[1]
    check_stage(aoc, g["in_x"], np.ascontiguousarray(g["ia10_in_x"][:, Ce:]), g["in_IA_head"], g["p_IA10.IA.weight"], g["p_IA10.IA.bias"], name,
                g["ia10_out"])


@pytest.mark.parametrize("N,Ce,Cr,D,h,w,H,W", [(1, 5, 3, 7, 5, 7, 9, 14), (3, 6, 2, 70, 9, 6, 17, 11), (30, 4, 3, 9, 3, 4, 6, 7)])
def test_shortcut_stage_random(aoc, N, Ce, Cr, D, h, w, H, W):
    rng = np.random.RandomState(N * 10 + D)
    x, low, _ = tb.resize_inputs(rng, N, Ce, Cr, h, w, H, W)
    head = (0.5 * rng.standard_normal((N, D))).astype(np.float32)
    weight = (rng.standard_normal((Ce + Cr, D + Ce + Cr)) / np.sqrt(D + Ce + Cr)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(Ce + Cr)).astype(np.float32)
    check_stage(aoc, x, low, head, weight, bias, f"shortcut_stage N={N} {Ce}+{Cr} D={D} {h}x{w}->{H}x{W}")


# ------------------------------------------------------------------------------------------ 3. the prediction head
LOGIT_CASES = [(1, 128, 300), (2, 8, 1), (4, 128, 257), (3, 13, 1025), (30, 16, 513), (3, 128, 121 * 213)]


def check_logits(got, x, wb_fg, wb_bg, what, dwb_fg=None, dwb_bg=None):
    N = x.shape[0]
    want, tol = tb.logit_head_ref(x, wb_fg, wb_bg, None, dwb_fg, dwb_bg)
    if N == 1:
        _check_bound(got, want, tol, tb.logit_head_ref(x, wb_bg, wb_bg)[0], f"{what}: the bg head for the fg head")
        return
    for slip in tb.LOGIT_SLIPS:
        if slip == "max" and N == 2:
            continue                                               # one other object: min and max coincide
        _check_bound(got, want, tol, tb.logit_head_ref(x, wb_fg, wb_bg, slip)[0], f"{what}: slip {slip}")


@pytest.mark.parametrize("N,C,hw", LOGIT_CASES)
def test_logit_head(aoc, N, C, hw):
    rng = np.random.RandomState(N * 100 + C + hw % 1000)
    x, wb_fg, wb_bg = tb.logit_inputs_random(rng, N, C, hw)
    gx, gf, gb = dev(x).view(N, C, 1, hw), dev(wb_fg), dev(wb_bg)
    pred = aoc.ops.logit_head(gx, gf, gb)
    assert pred.shape == (1, N, 1, hw)
    # the composition a caller had before (parent code): bit-equal, the accumulation order is kept and nothing fuses
    fg, bg = aoc.ops.object_logit(gx, gf), aoc.ops.object_logit(gx, gb)
    comp = fg.clone()
    if N > 1:
        comp[0] += bg[1:].min(0)[0]
    assert torch.equal(pred.view(N, hw), comp.view(N, hw))
    assert torch.equal(aoc.ops.background_merge(fg, bg), pred)
    check_logits(host(pred).view(N, hw), t64(x), t64(wb_fg), t64(wb_bg), f"logit_head N={N} C={C} hw={hw}")


def test_logit_head_writes_every_element(aoc):
    """The raw entry point on a NaN-filled output with rows wider than C + 1 (stride)."""
    import ctypes
    N, C, hw, stride = 5, 9, 130, 12
    rng = np.random.RandomState(3)
    x = rng.standard_normal((N, C, hw)).astype(np.float32)
    rows_fg, rows_bg = (rng.standard_normal((N, stride)).astype(np.float32) for _ in range(2))
    gx, gf, gb, out = dev(x), dev(rows_fg), dev(rows_bg), nan_like(N, hw)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = aoc._lib.lib().aoc_logit_head(p(gx), p(gf), p(gb), stride, N, C, hw, p(out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    check_logits(host(out), t64(x), t64(rows_fg[:, :C + 1]), t64(rows_bg[:, :C + 1]), "logit_head with a row stride")


# ------------------------------------------------------------------------------------------ 4. the mirrors
def linear_of(g, k):
    lin = nn.Linear(g[f"p_{k}_weight"].shape[1], g[f"p_{k}_weight"].shape[0])
    lin.load_state_dict(dict(weight=torch.from_numpy(g[f"p_{k}_weight"]), bias=torch.from_numpy(g[f"p_{k}_bias"])))
    return lin.cuda()


@pytest.mark.parametrize("name", ["logit_head_O1", "logit_head_O2", "logit_head_O4"])
def test_predict_and_augment_golden(aoc, golden, name):
    g = golden(name)
    dec = types.SimpleNamespace(IA_final_fg=linear_of(g, "fg"), IA_final_bg=linear_of(g, "bg"))
    x, head = g["in_x"], g["in_IA_head"]
    N, C = x.shape[:2]
    D = head.shape[1]
    pred = aoc.decoder_tail.predict(dec, dev(x), dev(head))
    assert pred.shape == g["pred"].shape
    x64, h64 = t64(x).reshape(N, C, -1), t64(head)
    rows = []
    for k in ("fg", "bg"):                                         # aoc_linear is a wave dot product: its bound is _wave_dot_tol's
        wt, b = t64(g[f"p_{k}_weight"]), t64(g[f"p_{k}_bias"])
        rows += [h64 @ wt.t() + b, _wave_dot_tol(h64.abs(), torch.zeros_like(h64), wt.abs(), b.abs(), D)]
    check_logits(host(pred).view(N, -1), x64, rows[0], rows[2], f"predict {name}", rows[1], rows[3])
    # augment_background_logit on the reference's own logits: one float32 addition, the same one
    merged = aoc.decoder_tail.augment_background_logit(dev(g["fg_logit"]), dev(g["bg_logit"]))
    assert torch.equal(host(merged), torch.from_numpy(g["pred"]))


def decoder_of(aoc, g):
    """An object that carries what decoder_final reads, with the golden's parameters: the project's GCT and IA_gate mirrors, PyTorch
    convolutions and GroupNorms (their parameters only; the normalisation runs in the library)."""
    Cl, Cr = g["p_conv_sc.weight"].shape[1], g["p_conv_sc.weight"].shape[0]
    Ct, half = g["p_conv1.weight"].shape[1], g["p_conv1.weight"].shape[0]
    dec = nn.Module()
    dec.GCT_sc = aoc.gct.GCT(Cl)
    dec.conv_sc = nn.Conv2d(Cl, Cr, 1, bias=False)
    dec.bn_sc = nn.GroupNorm(int(Cr / 4), Cr)
    dec.IA10 = aoc.attention.IA_gate(g["p_IA10.IA.weight"].shape[1], Ct)
    dec.conv1 = nn.Conv2d(Ct, half, kernel_size=3, padding=1, bias=False)
    dec.bn1 = nn.GroupNorm(32, half)
    dec.IA11 = aoc.attention.IA_gate(g["p_IA11.IA.weight"].shape[1], half)
    dec.conv2 = nn.Conv2d(half, half, kernel_size=3, padding=1, bias=False)
    dec.bn2 = nn.GroupNorm(32, half)
    dec.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p_")})
    return dec.cuda().eval()


@pytest.mark.parametrize("name", ["decoder_shortcut_O3", "decoder_shortcut_O1", "decoder_shortcut_O4_odd"])
def test_decoder_final_golden(aoc, golden, name):
    """max |mirror - float64| <= 4 max |reference float32 - float64|, both sides from the fixture: the factor 4 leaves MIOpen's convolutions
    another summation order than the CPU's; a wiring mistake is O(1)."""
    g = golden(name)
    dec = decoder_of(aoc, g)
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        got = aoc.decoder_tail.decoder_final(dec, dev(g["in_x"]), dev(g["in_low_level_feat"]), dev(g["in_IA_head"]))
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
    f64 = torch.from_numpy(g["out_f64"])
    ref_err = float((torch.from_numpy(g["out_f32"]).double() - f64).abs().max())
    err = float((host(got).double() - f64).abs().max())
    print(f"{name}: mirror {err:.3e}, reference float32 {ref_err:.3e}")
    assert got.shape == f64.shape and err <= 4 * ref_err, (err, ref_err)
