"""The streaming kernels that build the rest of every frame, each called directly and compared with a plain reference of the same
operation: the J/F metric (oracle/metrics.py), masked mean pooling, the resize family and the atrous grid, the fused local-matching
operands, the proto-mask tail, fg2bg and the small dense calls.

Float results are compared with float64 references under a bound derived from the float32 error of the operation (U = 2^-24 is the
unit roundoff; gamma(n) = n U / (1 - n U) bounds the relative error of a value that went through n roundings).  Every such comparison
also runs its sensitivity self-check: the same reference with one deliberate slip (a dropped chunk, a dropped term, a shifted grid, a
disk without its rim) must fall OUTSIDE the bound, so the bound is tight enough to catch a subtly wrong kernel.  Calls that are
documented as bit-identical to other calls (the library is built with -ffp-contract=off) are compared with torch.equal."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from float64_bounds import U, _check_bound, gamma

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aoc():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import aoc_amd
    aoc_amd._lib.lib()      # raises if the HIP library is missing: no silent fallback
    return aoc_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu()


# ------------------------------------------------------------------------------------------ 1. J / F metric
def _jf_maps(rng, H, W, n_obj, r):
    """Blobby label maps over 0 .. n_obj - 1 and three labels outside that range (125, 255, -1); the prediction is the ground truth
    shifted by a few pixels with scattered errors.  Object 1 is a vertical line that the ground truth places r + 1 columns right of the
    prediction: half of its boundary pixels are exactly r apart, so a disk without its rim changes F.  Objects 3 / 5 / 7 are missing
    from the prediction / the ground truth / both."""
    vals = np.concatenate([np.arange(n_obj), [125, 255, -1]])
    cells = rng.choice(vals, size=((H + 6) // 7, (W + 8) // 9))
    gt = np.kron(cells, np.ones((7, 9), dtype=np.int64))[:H, :W]
    pred = np.roll(gt, (min(2, H - 1), -min(3, W - 1)), axis=(0, 1)).copy()
    noise = rng.rand(H, W) < 0.02
    pred[noise] = rng.choice(vals, size=int(noise.sum()))
    if n_obj > 1:
        pred[pred == 1] = 0
        gt[gt == 1] = 0
        c0 = 3
        if H >= 6 and c0 + r + 1 < W:
            pred[2:H - 2, c0] = 1
            gt[2:H - 2, c0 + r + 1] = 1
    for o, sides in ((3, (pred,)), (5, (gt,)), (7, (pred, gt))):
        if o < n_obj:
            for m in sides:
                m[m == o] = 0
    return pred.astype(np.int32), gt.astype(np.int32)


def _jf_ref(om, pred, gt, n_obj, r):
    sj = sum(om.db_eval_iou(gt == o, pred == o) for o in range(1, n_obj))
    sf = sum(om.db_eval_boundary(pred == o, gt == o, bound_th=r) for o in range(1, n_obj))
    return sj, sf


def _strict_disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (x * x + y * y) < r * r                   # the slip: '<' instead of '<=' drops the disk's rim


def _jf_add(aoc, pred, gt, n_obj, r, accum):
    """aoc_mask_jf_accumulate with an explicit bound_pix (MaskJF derives it from the map size)."""
    L, ops = aoc._lib.lib(), aoc.ops
    H, W = pred.shape
    p, g = dev(pred), dev(gt)
    ws = torch.zeros(int(L.aoc_mask_jf_workspace_bytes(H, W)), dtype=torch.uint8, device="cuda")
    aoc._lib.check(L.aoc_mask_jf_accumulate(ops._p(p), ops._p(g), H, W, int(n_obj), int(r), ops._p(ws), ws.numel(), 1, ops._p(accum),
                                            ops._stream()), "aoc_mask_jf_accumulate")


@pytest.mark.parametrize("r", [0, 1, 8, 32, 33, 40])
def test_mask_jf_bound_pix(aoc, r, monkeypatch):
    """bound_pix 0 .. 32 takes jf_match_tile_kernel, 33 and 40 jf_match_kernel; 16 objects (bits 15 and 31), foreign labels, objects
    empty on one side or both, a 61 x 93 map (not a multiple of the 32 x 8 tile), three frames accumulated."""
    from oracle import metrics as om
    rng = np.random.RandomState(100 + r)
    accum = torch.zeros(4, dtype=torch.float64, device="cuda")
    frames = [_jf_maps(rng, 61, 93, 16, r) for _ in range(3)]
    want_j = want_f = 0.0
    for pred, gt in frames:
        _jf_add(aoc, pred, gt, 16, r, accum)
        sj, sf = _jf_ref(om, pred, gt, 16, r)
        want_j, want_f = want_j + sj, want_f + sf
    sj, sf, n, nf = accum.tolist()
    assert nf == 3 and n == 3 * 15
    assert abs(sj - want_j) < 1e-9 and abs(sf - want_f) < 1e-9, (sj, want_j, sf, want_f)
    monkeypatch.setattr(om, "_disk", _strict_disk)
    slip_f = sum(_jf_ref(om, pred, gt, 16, r)[1] for pred, gt in frames)
    assert abs(slip_f - want_f) > 1e-9


def test_mask_jf_degenerate_shapes(aoc, monkeypatch):
    """1 x 1, 1 x 37, 41 x 1 and maps that are not multiples of the 32 x 8 tile, with n_obj 16, 4 and 1 (n_obj = 1 scores no object but
    counts the frame), both match kernels, one accumulator."""
    from oracle import metrics as om
    rng = np.random.RandomState(7)
    cases = []
    for (H, W) in ((1, 1), (1, 37), (41, 1), (13, 45), (40, 33), (9, 70)):
        for n_obj, r in ((16, 1), (4, 3), (1, 2), (16, 34)):
            cases.append((_jf_maps(rng, H, W, n_obj, r), n_obj, r))
    accum = torch.zeros(4, dtype=torch.float64, device="cuda")
    want_j = want_f = 0.0
    for (pred, gt), n_obj, r in cases:
        _jf_add(aoc, pred, gt, n_obj, r, accum)
        sj, sf = _jf_ref(om, pred, gt, n_obj, r)
        want_j, want_f = want_j + sj, want_f + sf
    sj, sf, n, nf = accum.tolist()
    assert nf == len(cases) and n == sum(n_obj - 1 for _, n_obj, _ in cases)
    assert abs(sj - want_j) < 1e-9 and abs(sf - want_f) < 1e-9, (sj, want_j, sf, want_f)
    monkeypatch.setattr(om, "_disk", _strict_disk)
    slip_f = sum(_jf_ref(om, pred, gt, n_obj, r)[1] for (pred, gt), n_obj, r in cases)
    assert abs(slip_f - want_f) > 1e-9


def test_mask_jf_accumulator_changes_shape(aoc, monkeypatch):
    """MaskJF (bound_pix = ceil(0.008 * hypot(H, W)): 8 at 480 x 854) over frames of three shapes: the workspace is re-made when the
    shape changes and the totals keep accumulating."""
    from oracle import metrics as om
    rng = np.random.RandomState(11)
    frames = [(_jf_maps(rng, 480, 854, 16, 8), 16), (_jf_maps(rng, 480, 854, 16, 8), 16), (_jf_maps(rng, 97, 141, 6, 2), 6),
              (_jf_maps(rng, 1, 37, 5, 1), 5), (_jf_maps(rng, 480, 854, 3, 8), 3)]
    jf = aoc.ops.MaskJF(torch.device("cuda"))
    want_j = want_f = 0.0
    for (pred, gt), n_obj in frames:
        jf.add(dev(pred), dev(gt), n_obj)
        sj, sf = om.jf_sums(pred, gt, n_obj)
        want_j, want_f = want_j + sj, want_f + sf
    tot = jf.totals()
    assert tot["frames"] == len(frames) and tot["objects"] == sum(n - 1 for _, n in frames)
    assert abs(tot["sum_j"] - want_j) < 1e-9 and abs(tot["sum_f"] - want_f) < 1e-9
    monkeypatch.setattr(om, "_disk", _strict_disk)
    slip_f = sum(om.jf_sums(pred, gt, n_obj)[1] for (pred, gt), n_obj in frames)
    assert abs(slip_f - want_f) > 1e-9


# ------------------------------------------------------------------------------------------ 2. masked mean pooling
def _pool_depth(C, n_obj, hw, n_frames, aligned):
    """Bound on the additions any term goes through in aoc_masked_mean_pool (calibration.hip): inside its thread at most the 128 * cpb
    pixels of its workgroup, at most 64 partial sums combined in the workgroup (RPP rows of the vec4 kernel, MP_SPLIT of the scalar one),
    ceil(n_blocks / 8) in its slice of the final kernel and the 8 slices."""
    cpf = -(-hw // 128)
    nb = n_frames * cpf
    vec4 = C % 4 == 0 and 16 <= C <= 256 and n_obj <= 8 and aligned
    cpb = -(-nb // 768) if vec4 else 1
    n_blocks = n_frames * -(-cpf // cpb) if vec4 else nb
    return 128 * cpb + 64 + -(-n_blocks // 8) + 8, vec4, cpb


def _pool_ref(emb, lab, eps, D):
    """float64 ATT:155-189 (sums over every frame and pixel) and the float32 error bound of the kernel's expressions
    pos = S / (cnt + eps), neg = (T - S) / ((N - cnt) + eps), |pos|^2 (sums of at most D additions, one rounding per product,
    per subtraction, per eps addition and per division)."""
    Fn, hw, C = emb.shape
    N = Fn * hw
    S = torch.einsum("fop,fpc->oc", lab, emb)
    A = torch.einsum("fop,fpc->oc", lab.abs(), emb.abs())
    T = emb.sum((0, 1))
    Ta = emb.abs().sum((0, 1))
    cnt = lab.sum((0, 2))[:, None]
    pos = S / (cnt + eps)
    den = (N - cnt) + eps
    neg = (T - S) / den
    eS = gamma(D + 1) * A
    ec = gamma(D) * cnt
    pos_tol = eS / (cnt + eps) + pos.abs() * (ec / (cnt + eps) + gamma(2))
    neg_tol = (gamma(D) * Ta + eS + U * (T - S).abs()) / den + neg.abs() * ((ec + U * den) / den + gamma(2))
    sq = (pos * pos).sum(1)
    sq_tol = (2 * pos.abs() * pos_tol + pos_tol * pos_tol).sum(1) + gamma(-(-C // 128) + 8) * sq
    return pos, neg, sq, pos_tol, neg_tol, sq_tol


POOL_CASES = [   # C, n_obj, hw, frames, pixel_major                               path
    (4, 1, 1, 1, False),                                                       # scalar <4>, C < 16
    (4, 5, 127, 1, True),                                                      # scalar <8>
    (16, 4, 128, 1, False),                                                    # vec4 <4>
    (36, 8, 129, 1, True),                                                     # vec4 <8>
    (100, 4, 121 * 213, 1, False),                                             # vec4 <4>, cpb 1
    (128, 5, 129, 12, True),                                                   # vec4 <8>, 12 frames
    (256, 1, 127, 12, False),                                                  # vec4 <4>, C = 256
    (260, 8, 128, 1, False),                                                   # scalar <8>, C > 256
    (260, 30, 129, 1, True),                                                   # scalar <32>
    (16, 30, 1, 12, False),                                                    # scalar <32>, one pixel per frame
    (128, 9, 127, 1, False),                                                   # scalar <32>
    (100, 9, 121 * 213, 12, True),                                             # scalar <32>, 2424 blocks
    (100, 4, 121 * 213, 12, False),                                            # vec4 <4>, cpb 4
    (36, 8, 121 * 213, 12, True),                                              # vec4 <8>, cpb 4
]


def _pool_inputs(rng, C, n_obj, hw, n_frames):
    """Embeddings with a ramp along the pixels and an offset per frame (the tail of a map and the last frame are not averages of the
    rest); soft labels in [0, 1], object 0 hard 0 / 1 (and owner of the last pixel), object 1 (when there is one) without a pixel:
    pos = 0 / eps."""
    ramp = 4.0 * np.arange(hw, dtype=np.float64) / hw
    emb = (rng.uniform(-1, 1, (n_frames, hw, C)) + ramp[None, :, None] + 0.25 * np.arange(n_frames)[:, None, None]).astype(np.float32)
    lab = rng.uniform(0, 1, (n_frames, n_obj, hw)).astype(np.float32)
    lab[:, 0] = lab[:, 0] > 0.5
    lab[-1, 0, -1] = 1.0
    if n_obj > 1:
        lab[:, 1] = 0.0
    return emb, lab


def _pool_check(aoc, C, n_obj, hw, n_frames, pixel_major, misaligned=False):
    rng = np.random.RandomState(C * 1000 + n_obj * 10 + n_frames)
    eps = 1e-5
    emb, lab = _pool_inputs(rng, C, n_obj, hw, n_frames)
    if misaligned:                                            # a contiguous view one float into its allocation: data_ptr % 16 == 4
        base = torch.empty(emb.size + 1, dtype=torch.float32, device="cuda")
        g_emb = base[1:].view(emb.shape)
        g_emb.copy_(dev(emb))
        assert g_emb.data_ptr() % 16 == 4
    else:
        g_emb = dev(emb)
    g_lab = dev(lab.transpose(0, 2, 1)) if pixel_major else dev(lab)
    sq = torch.empty(n_obj, dtype=torch.float32, device="cuda")
    pos, neg = aoc.ops.masked_mean_pool(g_emb, g_lab, eps, pixel_major=pixel_major, out_pos_sqnorm=sq)
    D, vec4, cpb = _pool_depth(C, n_obj, hw, n_frames, aligned=not misaligned)
    e64, l64 = torch.from_numpy(emb).double(), torch.from_numpy(lab).double()
    want_pos, want_neg, want_sq, pos_tol, neg_tol, sq_tol = _pool_ref(e64, l64, eps, D)
    # the slip: the last 128-pixel chunk of the last frame (its last min(128, hw) pixels) left out of every sum
    k = min(128, hw)
    e64[-1, hw - k:] = 0.0
    l64[-1, :, hw - k:] = 0.0
    slip_pos, slip_neg = _pool_ref(e64, l64, eps, D)[:2]
    what = f"masked_mean_pool C={C} O={n_obj} hw={hw} F={n_frames} pm={pixel_major} vec4={vec4} cpb={cpb}"
    _check_bound(torch.cat([host(pos), host(neg)]), torch.cat([want_pos, want_neg]), torch.cat([pos_tol, neg_tol]),
                 torch.cat([slip_pos, slip_neg]), what)
    # |pos|^2; its slip: the last channel left out
    _check_bound(host(sq), want_sq, sq_tol, (want_pos * want_pos)[:, :-1].sum(1) if C > 1 else 0 * want_sq, what + " |pos|^2")
    if n_obj > 1:
        assert torch.equal(host(pos)[1], torch.zeros(C))        # no pixel: 0 / eps


@pytest.mark.parametrize("C,n_obj,hw,n_frames,pixel_major", POOL_CASES)
def test_masked_mean_pool_paths(aoc, C, n_obj, hw, n_frames, pixel_major):
    """Every dispatch path of aoc_masked_mean_pool (scalar <4 | 8 | 32>, vec4 <4 | 8> with cpb 1 and > 1) against float64."""
    _pool_check(aoc, C, n_obj, hw, n_frames, pixel_major)


@pytest.mark.parametrize("pixel_major", [False, True])
def test_masked_mean_pool_misaligned_emb(aoc, pixel_major):
    """C = 100 with emb one float into its allocation: the vec4 kernel is ruled out and the scalar <8> / <4> kernels run."""
    _pool_check(aoc, 100, 5, 129, 12, pixel_major, misaligned=True)
    _pool_check(aoc, 100, 3, 121 * 213, 1, pixel_major, misaligned=True)


# ------------------------------------------------------------------------------------------ 3. resize family, atrous grid
def _interp64(x_chw, H, W, align_corners=True):
    return F.interpolate(x_chw[None].double(), size=(H, W), mode="bilinear", align_corners=align_corners)[0]


def _bilinear_tol(x, h, w, H, W):
    """float32 bilinear (align_corners=True) against float64: each axis's source position scale * dst is two roundings off (the scale
    (in - 1) / (out - 1) and the product), at most 2 U (in - 1) in the weight; the interpolant's slope in a weight is at most 2 max|x|;
    the complementary weights 1 - lambda and the four roundings of the blend add 6 U max|x| (8 U with the second-order terms)."""
    M = float(x.abs().max())
    dy = 2 * U * (h - 1) if H > 1 else 0.0
    dx = 2 * U * (w - 1) if W > 1 else 0.0
    return M * (2 * dy + 2 * dx + 8 * U)


RESIZE_CASES = [(121, 213, 61, 107, 100), (121, 213, 480, 854, 3), (121, 213, 61, 107, 36), (7, 5, 20, 13, 128), (40, 30, 3, 2, 1),
                (9, 11, 1, 1, 1), (1, 9, 4, 1, 36), (3, 4, 30, 41, 128)]


@pytest.mark.parametrize("h,w,H,W,C", RESIZE_CASES)
def test_resize_bilinear_hwc(aoc, h, w, H, W, C):
    rng = np.random.RandomState(h * w + C)
    x = rng.standard_normal((h, w, C)).astype(np.float32)
    got = host(aoc.ops.resize_bilinear_hwc(dev(x), H, W))
    xc = torch.from_numpy(x).permute(2, 0, 1)
    want = _interp64(xc, H, W).permute(1, 2, 0)
    slip = _interp64(xc, H, W, align_corners=False).permute(1, 2, 0)    # the half-pixel grid instead of the corner-aligned one
    _check_bound(got, want, _bilinear_tol(xc, h, w, H, W), slip, f"resize_bilinear_hwc {h}x{w}->{H}x{W} C={C}")


def test_resize_bilinear_hwc_exact_cases(aoc):
    """Identity size: an exact copy.  A 1-pixel input: every output is that pixel.  A 1-pixel output: the corner pixel."""
    rng = np.random.RandomState(3)
    x = dev(rng.standard_normal((17, 23, 36)).astype(np.float32))
    assert torch.equal(aoc.ops.resize_bilinear_hwc(x, 17, 23), x)
    one = dev(rng.standard_normal((1, 1, 100)).astype(np.float32))
    assert torch.equal(aoc.ops.resize_bilinear_hwc(one, 5, 7), one.expand(5, 7, 100))
    assert torch.equal(aoc.ops.resize_bilinear_hwc(x, 1, 1), x[:1, :1])


def _plane_index(P, H, W, inner, outer, group_stride, outer_stride, plane_stride, pixel_stride):
    p = np.arange(P)[:, None]
    pix = np.arange(H * W)[None, :]
    po = p // inner
    return (po // outer) * group_stride + (po % outer) * outer_stride + (p % inner) * plane_stride + pix * pixel_stride


@pytest.mark.parametrize("h,w,H,W", [(61, 107, 121, 213), (13, 9, 13, 9), (5, 6, 1, 3)])
def test_resize_bilinear_planes_strided(aoc, h, w, H, W):
    """resize_bilinear_planes and _planes_grouped into a NaN-filled strided destination: every addressed element right, every other
    element still NaN."""
    rng = np.random.RandomState(h + W)
    inner, outer, groups = 2, 3, 2
    for grouped in (False, True):
        P = inner * outer * (groups if grouped else 1)
        x = rng.standard_normal((P, h, w)).astype(np.float32)
        pixel_stride, plane_stride = 2, 1
        outer_stride = 2 * H * W + 3
        group_stride = outer * outer_stride + 7 if grouped else 0
        idx = _plane_index(P, H, W, inner, outer, group_stride, outer_stride, plane_stride, pixel_stride)
        assert len(np.unique(idx)) == idx.size
        out = torch.full((int(idx.max()) + 11,), float("nan"), dtype=torch.float32, device="cuda")
        if grouped:
            aoc.ops.resize_bilinear_planes_grouped(dev(x), H, W, out, inner, outer, group_stride, outer_stride, plane_stride, pixel_stride)
        else:
            aoc.ops.resize_bilinear_planes(dev(x), H, W, out, plane_stride, pixel_stride, inner_count=inner, out_outer_stride=outer_stride)
        o = host(out)
        sel = torch.from_numpy(idx.reshape(-1))
        mask = torch.zeros(o.numel(), dtype=torch.bool)
        mask[sel] = True
        assert torch.isnan(o[~mask]).all(), "an element outside the addressed ones was written"
        got = o[sel].view(P, H, W)
        xt = torch.from_numpy(x)
        if (h, w) == (H, W):
            assert torch.equal(got, xt)                         # identity size: an exact copy
            continue
        slip = _interp64(xt.flip(0), H, W)                      # planes written to each other's slots
        _check_bound(got, _interp64(xt, H, W), _bilinear_tol(xt, h, w, H, W), slip, f"resize_bilinear_planes grouped={grouped} {h}x{w}->{H}x{W}")


@pytest.mark.parametrize("h,w,H,W", [(121, 854, 61, 427), (3, 5, 7, 2), (5, 3, 2, 7), (7, 9, 7, 9), (4, 6, 8, 12), (121, 213, 61, 107)])
def test_resize_nearest_bits(aoc, h, w, H, W):
    """Bit-equal to F.interpolate(mode='nearest') of an index map (src = min(floor(dst * float(in / out)), in - 1)), at ratios that
    round (121 -> 61, 854 -> 427, 3 -> 7, 5 -> 2)."""
    idx = np.arange(h * w, dtype=np.int32)
    got = host(aoc.ops.resize_nearest_bits(dev(idx), h, w, H, W)).numpy()
    src = torch.from_numpy(idx.astype(np.float64)).view(1, 1, h, w)
    want = F.interpolate(src, size=(H, W), mode="nearest").view(-1).numpy().astype(np.int32)
    np.testing.assert_array_equal(got, want)
    if (h, w) != (H, W) and (2 * h, 2 * w) != (H, W):
        exact = F.interpolate(src, size=(H, W), mode="nearest-exact").view(-1).numpy().astype(np.int32)
        assert (exact != want).any()                            # the rounding grid differs from the floor grid at these ratios


@pytest.mark.parametrize("rate", [1, 2, 3, 4])
@pytest.mark.parametrize("X", [8, 100, 3, 7])
def test_atrous_subsample(aoc, rate, X):
    """x[::rate, ::rate] bit for bit, h and w not multiples of the rate, X % 4 == 0 (16-byte moves) and != 0."""
    rng = np.random.RandomState(rate * 31 + X)
    h, w = 4 * rate + 1, 6 * rate - 1
    x = dev(rng.standard_normal((h, w, X)).astype(np.float32))
    assert torch.equal(aoc.ops.atrous_subsample(x, rate), x[::rate, ::rate])


# ------------------------------------------------------------------------------------------ 4. local_prep / local_window_match_pair identities
def _near_threshold_labels(rng, n, n_obj):
    vals = np.array([0.9, np.nextafter(np.float32(0.9), np.float32(1)), np.nextafter(np.float32(0.9), np.float32(0)), 0.0, 1.0, 0.05, 0.45],
                    dtype=np.float32)
    return vals[rng.randint(0, len(vals), (n, n_obj))]


@pytest.mark.parametrize("h,w,H2,W2,C,n_obj", [(23, 37, 12, 19, 100, 1), (23, 37, 12, 19, 36, 3), (31, 17, 16, 9, 100, 16),
                                               (15, 21, 8, 11, 4, 30), (2, 3, 1, 2, 4, 30)])
def test_local_prep_equals_separate_calls(aoc, h, w, H2, W2, C, n_obj):
    """aoc_local_prep == resize_bilinear_hwc / label_mix + resize / label_bits + resize_nearest_bits bit for bit (frame.hip switches
    between the two), labels at the 0.9 threshold; its bias table = the documented formula and both copies exact -- also on a 2 x 3 map
    whose tables are longer than H2 * W2 * C (the launch is widened)."""
    ops = aoc.ops
    rng = np.random.RandomState(h * 100 + n_obj)
    cur = dev(rng.standard_normal((h, w, C)).astype(np.float32))
    prev = dev(rng.standard_normal((h, w, C)).astype(np.float32))
    labels = dev(_near_threshold_labels(rng, h * w, n_obj))
    prev_pos = dev(rng.standard_normal((n_obj, C)).astype(np.float32))
    obj_bias = dev(rng.standard_normal(n_obj).astype(np.float32))
    n_pair_sets = 2 * 3 * n_obj
    set_bias = torch.full((n_pair_sets + n_obj,), float("nan"), device="cuda")
    src_a, src_b = dev(rng.standard_normal(400).astype(np.float32)), dev(rng.standard_normal(333).astype(np.float32))
    dst_a, dst_b = torch.full_like(src_a, float("nan")), torch.full_like(src_b, float("nan"))
    q2, p2, pm2, bits2 = ops.local_prep(cur, prev, labels, prev_pos, H2, W2, obj_bias=obj_bias, n_pair_sets=n_pair_sets, set_bias_out=set_bias,
                                        copies=((src_a, dst_a), (src_b, dst_b)))
    assert torch.equal(q2, ops.resize_bilinear_hwc(cur, H2, W2))
    assert torch.equal(p2, ops.resize_bilinear_hwc(prev, H2, W2))
    assert torch.equal(pm2, ops.resize_bilinear_hwc(ops.label_mix(labels, prev_pos).view(h, w, C), H2, W2))
    right, _ = ops.label_bits(labels, want_wrong=False)
    assert torch.equal(bits2, ops.resize_nearest_bits(right, h, w, H2, W2))
    s = np.arange(n_pair_sets + n_obj)
    owner = np.where(s < n_pair_sets, (s // 2) % n_obj, s - n_pair_sets)
    assert torch.equal(host(set_bias), host(obj_bias)[torch.from_numpy(owner)])
    assert torch.equal(dst_a, src_a) and torch.equal(dst_b, src_b)


@pytest.mark.parametrize("C", [100, 128, 36, 64])
def test_local_window_match_pair_equals_two_calls(aoc, C):
    """C 100 / 128: both maps as grid.z = 2 of the register kernel; C 36 / 64: two launches.  Either way == two single calls."""
    ops = aoc.ops
    rng = np.random.RandomState(C)
    H, W, n_obj, radii = 13, 21, 3, (2, 4, 6)
    s = 0.5 / math.sqrt(C)                        # squared distances O(1): the transformed outputs stay off their saturation at 1
    q = dev((s * rng.standard_normal((H, W, C))).astype(np.float32))
    a = dev((s * rng.standard_normal((H, W, C))).astype(np.float32))
    b = dev((s * rng.standard_normal((H, W, C))).astype(np.float32))
    labels = np.zeros((H * W, n_obj), dtype=np.float32)
    labels[np.arange(H * W), rng.randint(0, n_obj, H * W)] = 1.0
    right, _ = ops.label_bits(dev(labels), want_wrong=False)
    bias = dev(rng.standard_normal(n_obj).astype(np.float32))
    pair = ops.local_window_match_pair(q, a, b, right, radii, bias, n_obj)
    assert torch.equal(pair[0], ops.local_window_match(q, a, right, radii, bias, n_obj))
    assert torch.equal(pair[1], ops.local_window_match(q, b, right, radii, bias, n_obj))
    assert not torch.equal(pair[0], pair[1]) and float((pair < 0.99).float().mean()) > 0.5


# ------------------------------------------------------------------------------------------ 5. proto_finish / fg2bg_min
def _fg2bg_channels(om, x):
    """x [O, n, hw] -> the background map of every channel on its own (oracle foreground2background per channel)."""
    return torch.cat([om.foreground2background(x[:, k:k + 1], x.shape[0]) for k in range(x.shape[1])], dim=1)


_OFF = [None, "local", "global", "prev", "head"]


@pytest.mark.parametrize("n_obj", [1, 2, 5, 30])
@pytest.mark.parametrize("off", _OFF)
def test_proto_finish(aoc, n_obj, off):
    """aoc_proto_finish against oracle.matching.foreground2background and plain indexing, exact: ties for the minimum, +inf entries,
    an object stride longer than the channels (the gap must stay untouched), each part switched off in turn."""
    from oracle import matching as om
    rng = np.random.RandomState(n_obj * 7 + _OFF.index(off))
    hw, n_local, C = 301, 6, 100
    ch_local, ch_local_bg, ch_global, ch_global_bg, ch_prev = 0, n_local, 2 * n_local, 2 * n_local + 1, 2 * n_local + 2
    n_ch = 2 * n_local + 3
    obj_stride = n_ch * hw + 37
    feat = (rng.randint(0, 4, (n_obj, obj_stride)) * 0.5).astype(np.float32)      # quantised: ties for the minimum
    feat[rng.rand(n_obj, obj_stride) < 0.1] = np.inf
    feat[:, n_ch * hw:] = np.nan                                                    # the gap between objects
    prev_labels = rng.uniform(0, 1, (hw, n_obj)).astype(np.float32)
    heads = [rng.standard_normal((n_obj, C)).astype(np.float32) for _ in range(4)]
    g = dev(feat)
    head = aoc.ops.proto_finish(g, hw, obj_stride, ch_local, n_local, -1 if off == "local" else ch_local_bg, ch_global,
                                -1 if off == "global" else ch_global_bg, -1 if off == "prev" else ch_prev,
                                None if off == "prev" else dev(prev_labels), *([None] * 4 if off == "head" else [dev(t) for t in heads]))
    want = torch.from_numpy(feat.copy())
    ch = want[:, :n_ch * hw].view(n_obj, n_ch, hw)
    if off != "local":
        ch[:, ch_local_bg:ch_local_bg + n_local] = _fg2bg_channels(om, ch[:, ch_local:ch_local + n_local].clone())
    if off != "global":
        ch[:, ch_global_bg:ch_global_bg + 1] = om.foreground2background(ch[:, ch_global:ch_global + 1].clone(), n_obj)
    if off != "prev":
        ch[:, ch_prev] = torch.from_numpy(prev_labels).t()
    np.testing.assert_array_equal(host(g).numpy(), want.numpy())
    if off == "head":
        assert head is None
    else:
        assert torch.equal(host(head), torch.from_numpy(np.concatenate(heads, axis=1)))


@pytest.mark.parametrize("n_obj,n_ch", [(2, 1), (3, 4), (30, 2)])
def test_fg2bg_min_strided(aoc, n_obj, n_ch):
    """aoc_fg2bg_min: min over the OTHER objects and over the channels, strided input and output, ties and +inf, exact."""
    from oracle import matching as om
    rng = np.random.RandomState(n_obj + n_ch)
    inner = 517
    dis_stride, out_stride = n_ch * inner + 13, inner + 5
    dis = (rng.randint(0, 3, (n_obj, dis_stride)) * 0.25).astype(np.float32)
    dis[rng.rand(n_obj, dis_stride) < 0.2] = np.inf
    out = torch.full((n_obj, out_stride), float("nan"), device="cuda")
    aoc.ops.fg2bg_min(dev(dis), n_obj, out=out, dis_obj_stride=dis_stride, out_obj_stride=out_stride, n_ch=n_ch, inner=inner)
    want = om.foreground2background(torch.from_numpy(dis[:, :n_ch * inner].reshape(n_obj, n_ch, inner)), n_obj)[:, 0]
    o = host(out)
    assert torch.equal(o[:, :inner], want)
    assert torch.isnan(o[:, inner:]).all()


# ------------------------------------------------------------------------------------------ 6. small dense calls
@pytest.mark.parametrize("n_obj,D,channels", [(1, 100, 7), (5, 400, 33), (7, 129, 256), (30, 63, 5)])
def test_film_gain(aoc, n_obj, D, channels):
    """gain = 1 + tanh(head . W[c] + b[c]); D not a multiple of 64, n_obj not a multiple of 4 (the object loop steps by 4).  Bound: the
    dot product's ceil(D / 64) lane additions, 6 wave-sum levels and the bias, times sum |h w| + |b| (tanh' <= 1); then tanhf within
    2 ulp and the final addition: 4 U."""
    from oracle import calibration as ocal
    rng = np.random.RandomState(D + n_obj)
    head = (0.3 * rng.standard_normal((n_obj, D)) / math.sqrt(D)).astype(np.float32)
    weight = rng.standard_normal((channels, D)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(channels)).astype(np.float32)
    got = host(aoc.ops.film_gain(dev(head), dev(weight), dev(bias)))
    h64, w64, b64 = (torch.from_numpy(a).double() for a in (head, weight, bias))
    want = ocal.film_gain(h64, w64, b64)
    tol = gamma(-(-D // 64) + 7) * (h64.abs() @ w64.abs().t() + b64.abs()) + 4 * U
    slip = ocal.film_gain(h64[:, :-1], w64[:, :-1], b64)          # the last head dimension dropped
    _check_bound(got, want, tol, slip, f"film_gain O={n_obj} D={D}")


@pytest.mark.parametrize("n,n_obj,C", [(1, 1, 1), (257, 3, 100), (1000, 30, 7), (33, 16, 129)])
def test_label_mix(aoc, n, n_obj, C):
    """out[p] = sum_o labels[p, o] rows[o]: n_obj sequential products and additions."""
    rng = np.random.RandomState(n + C)
    lab = rng.uniform(0, 1, (n, n_obj)).astype(np.float32)
    rows = rng.standard_normal((n_obj, C)).astype(np.float32)
    got = host(aoc.ops.label_mix(dev(lab), dev(rows)))
    l64, r64 = torch.from_numpy(lab).double(), torch.from_numpy(rows).double()
    want = l64 @ r64
    tol = gamma(n_obj + 1) * (l64.abs() @ r64.abs())
    slip = l64[:, :-1] @ r64[:-1]                                  # the last object dropped
    _check_bound(got, want, tol, slip, f"label_mix n={n} O={n_obj} C={C}")


@pytest.mark.parametrize("N,Cc,hw", [(1, 1, 5), (3, 5, 17), (2, 7, 16 * 61 + 1), (5, 3, 3)])
def test_channel_scale_misaligned(aoc, N, Cc, hw):
    """y = gain * x, one rounding; x and y views that start one float into their allocations (head / body / tail of the float4 stream)."""
    rng = np.random.RandomState(N * Cc + hw)
    x = rng.standard_normal((N, Cc, hw)).astype(np.float32)
    gain = rng.uniform(0.5, 2, (N, Cc)).astype(np.float32)
    xb = torch.empty(x.size + 1, device="cuda")
    xv = xb[1:].view(N, Cc, hw)
    xv.copy_(dev(x))
    yb = torch.full((x.size + 1,), float("nan"), device="cuda")
    yv = yb[1:].view(N, Cc, hw)
    aoc.ops.channel_scale(xv, dev(gain), out=yv)
    x64, g64 = torch.from_numpy(x).double(), torch.from_numpy(gain).double()
    want = g64[:, :, None] * x64
    slip = g64[:, :, None] * x64.roll(1, dims=2)                   # every pixel read one place off
    _check_bound(host(yv), want, U * want.abs(), slip, f"channel_scale {N}x{Cc}x{hw}")
    assert torch.isnan(host(yb)[0])


@pytest.mark.parametrize("N,in_dim,out_dim", [(1, 1, 1), (5, 67, 3), (9, 129, 31), (30, 300, 65)])
def test_linear(aoc, N, in_dim, out_dim):
    """y = x W^T + b: ceil(in / 64) lane additions, 6 wave-sum levels and the bias."""
    rng = np.random.RandomState(N + in_dim)
    x = rng.standard_normal((N, in_dim)).astype(np.float32)
    wt = rng.standard_normal((out_dim, in_dim)).astype(np.float32)
    b = rng.standard_normal(out_dim).astype(np.float32)
    got = host(aoc.ops.linear(dev(x), dev(wt), dev(b)))
    x64, w64, b64 = (torch.from_numpy(a).double() for a in (x, wt, b))
    want = x64 @ w64.t() + b64
    tol = gamma(-(-in_dim // 64) + 7) * (x64.abs() @ w64.abs().t() + b64.abs())
    slip = x64[:, :-1] @ w64[:, :-1].t() + b64                     # the last input dropped
    _check_bound(got, want, tol, slip, f"linear N={N} in={in_dim} out={out_dim}")
