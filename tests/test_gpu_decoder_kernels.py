"""The decoder-side kernels of calibration.hip (what runs after the proto-mask tensor is built), each called directly and compared with
a float64 reference of the same operation under the bound that tests/float64_bounds.py derives from the kernel's float32 expressions:
GroupNorm (+ residual) (+ ReLU), the pre-head, plane_reduce and the GCT gate, the object logit, the conditioning codes, head_delta,
plane_mean, and the scores, masked pooling and fused plane means of the conditioning gate.

Every float comparison goes through _check_bound, which also demands that the same reference with one deliberate slip (statistics of the
wrong scope, a dropped tail, a dropped channel, a neighbour's weights, >= for >) leaves the bound.  test_decoder_bounds_host.py checks the
GroupNorm and pre-head bounds themselves against step-by-step float32 restatements of the kernels, without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import float64_bounds as fb
from float64_bounds import _check_bound, t64

pytestmark = pytest.mark.gpu

FULL = 121 * 213


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


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------------------ 1. GroupNorm (+ residual) (+ ReLU)
GN_CASES = [
    (3, 64, 32, 391),                # the shape of test_bottleneck_golden
    (1, 4, 4, 1),                    # one element per group: variance 0, rstd = 1 / sqrt(eps)
    (2, 6, 3, 2047), (2, 6, 3, 2048), (2, 6, 3, 2049),   # 4094 / 4096 / 4098 elements per group: around two trips of the 8 x 256 loop
    (2, 12, 1, 1025),                # one group over every channel, hw one past the apply kernel's 1024-pixel block
    (1, 256, 32, FULL),              # the full map
    (5, 8, 2, 7),                    # fewer than 256 elements in a group
]
GN_MODES = {"all": (True, True, True), "no_affine": (False, True, True), "no_residual_no_relu": (True, False, False), "inplace": (True, True, True)}


@pytest.mark.parametrize("offset", [0.0, 3.0])
@pytest.mark.parametrize("mode", list(GN_MODES))
@pytest.mark.parametrize("N,C,groups,hw", GN_CASES)
def test_groupnorm_relu(aoc, N, C, groups, hw, mode, offset):
    """Noise + 0.5 x (channel index within the group), with and without a common offset of 3 sigma (E[x^2] - mean^2 cancels); gamma, beta,
    residual and ReLU on / gamma = beta = None / no residual and no ReLU / y aliasing x (bit-equal to the out-of-place call)."""
    affine, residual, relu = GN_MODES[mode]
    rng = np.random.RandomState(N * 1000 + C + hw + int(offset))
    x, w, b, res = fb.gn_inputs(rng, N, C, groups, hw, offset, affine, residual)
    gx, gw, gb, gr = dev(x), dev(w), dev(b), dev(res)
    got = aoc.ops.groupnorm_relu(gx, groups, gw, gb, 1e-5, gr, relu)
    if mode == "inplace":
        buf = gx.clone()
        ret = aoc.ops.groupnorm_relu(buf, groups, gw, gb, 1e-5, gr, relu, out=buf)
        assert ret.data_ptr() == buf.data_ptr() and torch.equal(buf, got)
    args = (t64(x), groups, t64(w), t64(b), 1e-5, t64(res), relu)
    want, tol = fb.groupnorm_ref(*args)
    if residual and relu and want.numel() >= 100:
        clipped = float((want == 0).double().mean())
        assert 0.2 < clipped < 0.8, clipped                      # the residual makes ReLU clip about half of the outputs
    for kind in fb.gn_slips(N, C, groups, hw, offset):
        _check_bound(host(got), want, tol, fb.groupnorm_slip(kind, *args), f"groupnorm_relu {N}x{C}x{hw} G={groups} {mode} offset={offset} slip={kind}")


def test_groupnorm_relu_rejections(aoc):
    """C % groups != 0 is an invalid argument; N C = 65536 planes exceed the apply kernel's grid and are refused before anything is
    enqueued: a NaN-filled output is still all NaN."""
    x = torch.zeros(2, 6, 5, device="cuda")
    with pytest.raises(aoc._lib.AocHipError, match="AOC_ERR_INVALID_ARG"):
        aoc.ops.groupnorm_relu(x, 4, None, None, 1e-5, None, True)
    x = torch.ones(256, 256, 1, device="cuda")
    out = nan_like((256, 256, 1))
    with pytest.raises(aoc._lib.AocHipError, match="AOC_ERR_UNSUPPORTED"):
        aoc.ops.groupnorm_relu(x, 32, None, None, 1e-5, None, True, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------ 2. pre-head
PH_CASES = [   # n_obj, n_in, n_out, n_groups, hw, embedding channels (None: no embedding)
    (1, 24, 64, 16, 17 * 23, 100),       # <24>, the model's setting
    (3, 26, 64, 16, 257, 3),             # <26>
    (1, 28, 64, 16, 255, None),          # <28>
    (3, 24, 64, 16, FULL, 100),          # <24>, the full map
    (3, 1, 128, 64, 1, 3),               # generic, two trips of the group loop, one pixel
    (1, 7, 128, 128, 257, None),         # generic, four trips, group size 1
    (3, 32, 128, 128, 1, 100),           # generic at PH_MAX_IN, four trips, group size 1, one pixel
    (1, 24, 128, 64, 256, None),         # <24>, two trips
    (1, 32, 64, 16, FULL, None),         # generic, the full map
    (3, 7, 64, 16, 256, 3),              # generic, the model's groups
    (1, 26, 128, 128, 255, 100),         # <26>, four trips
    (3, 28, 128, 64, 17 * 23, None),     # <28>, two trips
]


@pytest.mark.parametrize("n_obj,n_in,n_out,n_groups,hw,C", PH_CASES)
def test_prehead(aoc, n_obj, n_in, n_out, n_groups, hw, C):
    """The compiled <24 | 26 | 28> and the generic instantiation, one to four trips of the loop over PH_MAX_GROUPS groups, convolution bias up
    to +-2; the embedding channels are the transposed embedding, bit for bit, for every object."""
    rng = np.random.RandomState(n_in * 100 + n_groups + hw)
    feat, w, b, gw, gb = fb.ph_inputs(rng, n_obj, n_in, n_out, hw)
    emb = rng.standard_normal((hw, C)).astype(np.float32) if C else None
    got = aoc.ops.prehead(dev(feat).view(n_obj, n_in, hw, 1), dev(w), dev(b), n_groups, dev(gw), dev(gb), 1e-5, emb_hwc=dev(emb))
    got = host(got).view(n_obj, (C or 0) + n_out, hw)
    if C:
        assert torch.equal(got[:, :C], torch.from_numpy(emb).t().expand(n_obj, C, hw))
    args = (t64(feat), t64(w), t64(b), n_groups, t64(gw), t64(gb), 1e-5)
    want, tol = fb.prehead_ref(*args)
    kinds = fb.ph_slips(n_in, n_out, n_groups, hw)
    assert kinds
    for kind in kinds:
        _check_bound(got[:, C or 0:], want, tol, fb.prehead_slip(kind, *args), f"prehead O={n_obj} {n_in}->{n_out} G={n_groups} hw={hw} slip={kind}")


@pytest.mark.parametrize("n_in,n_out,n_groups", [(33, 64, 16), (24, 129, 3), (24, 64, 24)])
def test_prehead_rejections(aoc, n_in, n_out, n_groups):
    """More than PH_MAX_IN inputs, more than PH_MAX_OUT outputs and groups that do not divide the outputs are unsupported; the output is
    untouched."""
    L, ops = aoc._lib.lib(), aoc.ops
    hw = 300
    feat, w, b = torch.ones(2, n_in, hw, device="cuda"), torch.ones(n_out, n_in, device="cuda"), torch.ones(n_out, device="cuda")
    out = nan_like((2, n_out, hw))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    with pytest.raises(aoc._lib.AocHipError, match="AOC_ERR_UNSUPPORTED"):
        aoc._lib.check(L.aoc_prehead(ops._p(feat), 2, n_in, hw, ops._p(w), ops._p(b), n_out, n_groups, ops._p(b), ops._p(b), 1e-5, None, 0, ops._p(out),
                                     ops._p(ws), ws.numel(), ops._stream()), "aoc_prehead")
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------ 3. plane_reduce, gct_gate
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("hw", [1, 255, 256, 2047, 2048, 2049, FULL])
def test_plane_reduce(aoc, hw, mode):
    """Plane sums of x, x^2 and |x| of mixed-sign data on both sides of the 256-thread stride and the 2048-element unrolled trip."""
    rng = np.random.RandomState(hw + mode)
    x = (rng.standard_normal((2, 3, hw)) + 0.25).astype(np.float32)
    got = host(aoc.ops.plane_reduce(dev(x).view(2, 3, hw, 1), mode))
    want, tol = fb.plane_reduce_ref(t64(x), mode)
    for kind in (["as_mode0"] if mode == 2 else []) + ["tail"]:
        _check_bound(got, want, tol, fb.plane_reduce_slip(kind, t64(x), mode), f"plane_reduce hw={hw} mode={mode} slip={kind}")


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("C", [1, 12, 256, 257, 512])
def test_gct_gate(aoc, C, l1, N):
    """aoc_gct_gate from hand-made plane sums: one and two trips of the channel loop, gamma of mixed sign, and (N = 3) one row of all-zero
    sums: e = sqrt(eps) alpha in l2, 0 / eps in l1.  The slip: the mean over the channels taken over the first 256 only; where there are no
    more than 256, the last channel left out of that mean."""
    rng = np.random.RandomState(C * 4 + 2 * l1 + N)
    s = rng.uniform(0, 50, (N, C)).astype(np.float32)
    if N > 1:
        s[1] = 0.0
    alpha = (rng.uniform(0.5, 1.5, C) * rng.choice([-1, 1], C)).astype(np.float32)
    gam = rng.standard_normal(C).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    got = host(aoc.ops.gct_gate(dev(s), dev(alpha), dev(gam), dev(beta), 1e-5, l1_mode=l1))
    args = (t64(s), t64(alpha), t64(gam), t64(beta), 1e-5, l1)
    want, tol = fb.gct_gate_ref(*args)
    slip, _ = fb.gct_gate_ref(*args, mean_slip="first256" if C > 256 else "drop_last")
    _check_bound(got, want, tol, slip, f"gct_gate N={N} C={C} l1={l1}")


# ------------------------------------------------------------------------------------------ 4. object_logit
OL_CASES = [(1, 1, 1), (4, 7, 255), (4, 8, 257), (1, 9, 29 * 41), (4, 37, 29 * 41), (4, 256, 255), (1, 37, 257), (4, 1, 1), (1, 7, 1), (4, 9, 257)]


@pytest.mark.parametrize("N,C,hw", OL_CASES)
def test_object_logit(aoc, N, C, hw):
    """aoc_object_logit through ops.object_logit (weights and bias as views of one [N, C + 1] tensor) and directly with weight_stride =
    C + 5 and bias_stride = 3 from separate buffers: the same bits, inside gamma(C + 1) (sum |w x| + |b|)."""
    rng = np.random.RandomState(N * 1000 + C + hw)
    x = (rng.standard_normal((N, C, hw)) + 0.5).astype(np.float32)
    wb = rng.standard_normal((N, C + 1)).astype(np.float32)
    gx = dev(x)
    got = aoc.ops.object_logit(gx.view(N, C, 1, hw), dev(wb)).view(N, hw)
    L, ops = aoc._lib.lib(), aoc.ops
    wpad, bpad = nan_like((N, C + 5)), nan_like((N, 3))
    wpad[:, :C] = dev(wb[:, :C])
    bpad[:, 0] = dev(wb[:, C])
    out = nan_like((N, hw))
    aoc._lib.check(L.aoc_object_logit(ops._p(gx), N, C, hw, ops._p(wpad), C + 5, ops._p(bpad), 3, ops._p(out), ops._stream()), "aoc_object_logit")
    assert torch.equal(out, got)
    args = (t64(x), t64(wb[:, :C]), t64(wb[:, C]))
    want, tol = fb.object_logit_ref(*args)
    kinds = (["tail_channels"] if C % 8 else []) + (["prev_object"] if N > 1 else [])
    assert kinds
    for kind in kinds:
        _check_bound(host(got), want, tol, fb.object_logit_slip(kind, *args), f"object_logit N={N} C={C} hw={hw} slip={kind}")


# ------------------------------------------------------------------------------------------ 5. cond_codes, head_delta, plane_mean
@pytest.mark.parametrize("N,C,D", [(1, 1, 1), (3, 24, 400), (5, 65, 129), (30, 8, 64)])
def test_cond_codes(aoc, N, C, D):
    """aoc_cond_codes against the three F.linear calls and the sum(0) - px of oracle.calibration.conditioning_block in float64."""
    rng = np.random.RandomState(N + C + D)
    r = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    gap, px, head = r(N, C), r(N, C) + np.float32(0.5), r(N, D)
    params = [r(C, C), r(C), r(C, C), r(C), r(D, D), r(D)]
    got = host(aoc.ops.cond_codes(dev(gap), dev(px), dev(head), *[dev(p) for p in params]))
    args = [t64(a) for a in (gap, px, head, *params)]
    want, tol = fb.cond_codes_ref(*args)
    for kind in ("no_minus", "drop_head"):
        _check_bound(got, want, tol, fb.cond_codes_ref(*args, slip=kind)[0], f"cond_codes N={N} C={C} D={D} slip={kind}")


def test_cond_codes_rejects_wrong_shapes(aoc):
    """The library reads W3 as [D, D] from a bare pointer: ops.cond_codes refuses a [C, D] weight (and a short bias) before the launch."""
    N, C, D = 3, 8, 64
    z = lambda *shape: torch.zeros(*shape, device="cuda")
    good = [z(N, C), z(N, C), z(N, D), z(C, C), z(C), z(C, C), z(C), z(D, D), z(D)]
    assert aoc.ops.cond_codes(*good).shape == (N, 2 * C + D)
    for i, wrong in ((7, z(C, D)), (8, z(C)), (3, z(C, C + 1)), (1, z(N - 1, C))):
        args = list(good)
        args[i] = wrong
        with pytest.raises(aoc._lib.AocHipError, match="shapes"):
            aoc.ops.cond_codes(*args)


@pytest.mark.parametrize("n_obj,D,C", [(4, 400, 512), (1, 400, 320), (9, 912, 128), (30, 100, 37)])
def test_head_delta(aoc, n_obj, D, C):
    """The head half is a copy; the delta half is n_obj sequential additions and a subtraction: gamma(n_obj) sum |px|."""
    rng = np.random.RandomState(n_obj + D)
    head, px = rng.standard_normal((n_obj, D)).astype(np.float32), (rng.standard_normal((n_obj, C)) + 0.5).astype(np.float32)
    got = host(aoc.ops.head_delta(dev(head), dev(px)))
    assert got.shape == (n_obj, D + C) and torch.equal(got[:, :D], torch.from_numpy(head))
    want, tol = fb.head_delta_ref(t64(px))
    _check_bound(got[:, D:], want, tol, fb.head_delta_ref(t64(px), slip=True)[0], f"head_delta O={n_obj} D={D} C={C}")


@pytest.mark.parametrize("hw", [1, 2, 5, 255, 2049, 8193, FULL])
def test_plane_mean(aoc, hw):
    """plane_mean4_kernel at the sizes of test_plane_mean_sizes; 21 planes at every phase of a 16-byte line; the input carries a ramp, so
    the scalar tail is not an average of the rest."""
    rng = np.random.RandomState(hw)
    x = (rng.standard_normal((3, 7, hw)) + 2.0 * np.arange(hw) / hw).astype(np.float32)
    gx = dev(x)
    assert gx.data_ptr() % 16 == 0
    got = host(aoc.ops.plane_mean(gx.view(3, 7, hw, 1))).view(21)
    want, tol = fb.plane_mean_ref(t64(x).view(21, hw))
    _check_bound(got, want, tol, fb.plane_mean_slip(t64(x).view(21, hw)), f"plane_mean hw={hw}")


# ------------------------------------------------------------------------------------------ 6. cond_gate_pool: scores, gap, fused plane means
CG_EXACT = [(1, 1, 1), (3, 3, 255), (1, 4, 2047), (3, 5, 2048), (1, 31, 2049), (3, 32, 4097), (1, 33, 255), (3, 37, 2049), (1, 64, 4097),
            (3, 100, FULL), (1, 100, 2048), (3, 64, 1), (1, 5, 4097), (3, 33, 2047)]


@pytest.mark.parametrize("N,C,hw", CG_EXACT)
def test_cond_gate_pool_exact_scores(aoc, N, C, hw):
    """z = integers in [-8, 8] x 2^-4, phi_w = +- powers of two, phi_b = 1/4: every float32 partial score is exact, so the scores, the
    threshold and the mask are the reference's bit for bit (no exclusions), with ties at the threshold by construction; gap and the fused
    plane means are then checked under their own bounds.  C on both sides of the four-channel load group and the 32-channel chunk, hw on
    both sides of the 2048-pixel tile."""
    rng = np.random.RandomState(N * 1000 + C + hw)
    period = max(1, hw // 3)                                     # every pixel has at least two twins: every score is tied
    z = (rng.randint(-8, 9, (N, C, period)) / 16.0).astype(np.float32)
    z[:, :, 0][z[:, :, 0] == 0] = 1 / 16.0                      # (and the map of one pixel is not zero)
    z = np.tile(z, (1, 1, -(-hw // period)))[:, :, :hw]
    phi_w = (rng.choice([-1.0, 1.0], C) * 2.0 ** rng.randint(-2, 3, C)).astype(np.float32)
    phi_b = np.array([0.25], np.float32)
    k = max(1, int(0.3 * hw))
    gap, scores, thr, pm = aoc.ops.cond_gate_pool(dev(z).view(N, C, hw, 1), dev(phi_w), dev(phi_b), k, want_debug=True, want_plane_mean=True)
    z64 = t64(z)
    s, want_thr, mask, _, _ = fb.cond_scores_ref(z64, t64(phi_w), t64(phi_b), k)
    assert torch.equal(host(scores).double(), s)
    assert torch.equal(host(thr).double(), want_thr)
    ties = (s == want_thr[:, None]).sum(1)
    assert (ties > (1 if hw >= 255 else 0)).all(), ties
    want, tol = fb.cond_gap_ref(z64, mask)
    _check_bound(host(gap), want, tol, fb.cond_gap_ref(z64, s >= want_thr[:, None])[0], f"cond_gate_pool gap N={N} C={C} hw={hw}")
    want, tol = fb.cond_plane_mean_ref(z64)
    _check_bound(host(pm), want, tol, fb.cond_plane_mean_ref(z64, drop_last_tile=True)[0], f"cond_gate_pool plane_mean N={N} C={C} hw={hw}")


@pytest.mark.parametrize("N,C,hw", [(3, 37, 2049), (1, 100, FULL), (2, 33, 255), (3, 4, 4097), (1, 65, 2048)])
def test_cond_gate_pool_scores_bound(aoc, N, C, hw):
    """Random inputs: the scores under gamma(C + n_chunks + 1) (sum |w z| + |b|); the slip leaves the last 32-channel chunk out."""
    rng = np.random.RandomState(N + C + hw)
    z = (rng.standard_normal((N, C, hw)) + 0.3).astype(np.float32)
    phi_w = rng.standard_normal(C).astype(np.float32)
    phi_b = np.array([0.1], np.float32)
    k = max(1, int(0.3 * hw))
    _, scores, _ = aoc.ops.cond_gate_pool(dev(z).view(N, C, hw, 1), dev(phi_w), dev(phi_b), k, want_debug=True)
    args = (t64(z), t64(phi_w), t64(phi_b), k)
    s, _, _, _, tol = fb.cond_scores_ref(*args)
    _check_bound(host(scores), s, tol, fb.cond_scores_ref(*args, skip_chunk=(C - 1) // 32)[0], f"cond_gate_pool scores N={N} C={C} hw={hw}")
