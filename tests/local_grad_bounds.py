"""Float64 references, derived bounds, cases and inputs for the training-time local matching: aoc_local_window_match_argmin and
aoc_local_match_grad (csrc/local_grad.hip), and aoc_amd.local_train end to end.  Shared by test_local_grad_host.py (no GPU) and
test_gpu_local_grad.py.  Pure numpy; the library is not imported here.  U and gamma are those of float64_bounds.py, the per-pair
distance bound, the rings, the object planes and the transform those of local_match_bounds.py, the gate and the term those of
match_grad_bounds.py.

Forward.  forward_ref is local_match_bounds.local_window_ref's reference (nested_min over the pairs that count, then
local_transform_ref) that also returns the minimiser: the previous-frame PIXEL of the first minimum in ascending pixel order (which is
row-major window order), -1 where no pair counts (the value is then the padding and T exactly 1), the float64 gap to the runner-up and
the forward distance bound of the winner, per (object, channel, pixel).  Channel order is the kernel's: [largest, r_0, r_1, ...].

Backward, read off local_grad.hip (every product, sum and difference rounds once: -ffp-contract=off):
  g      lg_gate = mg_gate: match_grad_bounds.gate_ref
  term   fl(fl(2 g^) * fl(x - y)): match_grad_bounds._term_err.  Where the operands themselves are off by dx (end to end: the rounding of
         torch's interpolate) the difference is off by dx more: + 2 (|g| + e_g) dx (1 + 2 U)
  sums   a sum of terms each of which passes through at most k additions is off by sum e_term + gamma(k) sum (|term| + e_term), with k:
           grad_query   n_obj n_radii           lg_query_kernel: `acc +=` over (o, ch), ascending
           grad_prev    the row's pairs         lg_prev_kernel: one thread adds a row's matches one after the other
           grad_bias    min(m, 256) n_radii + ceil(m / 256)      lg_bias_partial_kernel, lg_bias_final_kernel
No measured number goes into a bound.  The gradients depend on arg discontinuously, so the tests demand arg == the float64 argmin, and
the host test demands that no (object, channel, pixel) with a candidate, outside the planted duplicates, has a best / runner-up gap under
GAP_FACTOR x the forward distance bound of its winner.

Inputs (case_inputs).  Embeddings s randn with s = 1 / sqrt(C): |q - p|^2 is about 2, the window minima lie around 1 and, under biases
N(0, 0.3^2), T stays inside (0.05, 0.95); at C = 4 the nearest of a window's candidates lies at about 0.1 and the biases are drawn
around 0.6 instead, which puts T near 0.3.  Labels are one-hot owners with about 15 % of the pixels unlabelled; a tenth of the pixels
carry bit 31 and one bit at or above n_obj, which the entry must ignore.  Query pixels that fail the gap condition are drawn again from
the same distribution until none is left.  The planted case (PLANTED) has by construction: object 1 with a single labelled pixel,
object 2 with two bit-equal labelled pixels and nothing else, object 3 absent."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import local_match_bounds as lmb
import match_grad_bounds as mgb
from float64_bounds import U, gamma

f32 = np.float32
PAD = lmb.PAD
GAP_FACTOR = 100.0
LG_BIAS_PIX = 256
ARG_SLIPS = ("ties_highest", "largest_everywhere", "ring_only")


# ------------------------------------------------------------------------------------------ forward with argmin
def forward_ref(query, prev, bits, radii, rate, n_obj, bias, slip=None, dup=(), dq=None, dp=None):
    """query, prev [H, W, C] (float32 values); bits [H * W] uint32; bias [n_obj] float32 or None.
    -> dict(T, tol_T, raw, tol_raw, gap, e_best [O, n_radii, H, W] float64; arg [O, n_radii, H, W] int64), kernel channel order.
    dup: pairs (lo, hi) of bit-equal previous-frame pixels: column hi of D is column lo's (BLAS need not give equal columns equal bits).
    dq, dp [H * W, C]: what the operands are off by (end to end) -> the distance is off by 2 sum_c |q_c - p_c| (dq_c + dp_c) +
    sum_c (dq_c + dp_c)^2 more.
    slip: one of ARG_SLIPS, the same reference with one deliberate mistake in arg:
      ties_highest         the last of several equal minima instead of the first;
      largest_everywhere   the largest window's position in every channel;
      ring_only            the minimiser among the pairs of a channel's own ring (radius above the next smaller one), without the prefix."""
    assert slip is None or slip in ARG_SLIPS, slip
    H, W, C = query.shape
    m = H * W
    radii = [int(r) for r in radii]
    nr = len(radii)
    D, E = lmb.pair_distances(query, prev)
    if dq is not None:
        q, p = np.asarray(query, np.float64).reshape(m, C), np.asarray(prev, np.float64).reshape(m, C)
        for i in range(m):                                   # row by row: [m, m, C] would not fit for the larger maps
            s = dq[i][None, :] + dp
            E[i] = (E[i] + 2.0 * (np.abs(q[i][None, :] - p) * s).sum(1) + (s * s).sum(1)) * (1.0 + 1e-6)
    for lo, hi in dup:
        D[:, hi], E[:, hi] = D[:, lo], E[:, lo]
    ring = lmb.pair_rings(H, W, rate)
    planes = lmb.object_planes(bits, n_obj)
    raw, tol = lmb.nested_min(D, E, ring, planes, radii, rate, PAD)              # plain radius order [O, nr, m]
    arg = np.full((n_obj, nr, m), -1, np.int64)
    gap = np.full((n_obj, nr, m), np.inf)
    e_best = np.zeros((n_obj, nr, m))
    ar = np.arange(m)
    for o in range(n_obj):
        cols = np.nonzero(planes[o])[0]
        if cols.size == 0:
            continue
        d, e, r = D[:, cols], E[:, cols], ring[:, cols]
        for i, rad in enumerate(radii):
            ra = rad // rate
            on = r <= ra
            if slip == "ring_only" and i > 0:
                on = on & (r > radii[i - 1] // rate)
            A = np.where(on, d, np.inf)
            if slip == "ties_highest":
                j = A.shape[1] - 1 - A[:, ::-1].argmin(1)
            else:
                j = A.argmin(1)
            any_on = on.any(1)
            arg[o, i] = np.where(any_on, cols[j], -1)
            e_best[o, i] = np.where(any_on, e[ar, j], 0.0)
            if slip is None and A.shape[1] > 1:
                part = np.partition(A, 1, axis=1)
                with np.errstate(invalid="ignore"):                              # inf - inf where no pair counts: any_on is False there
                    gap[o, i] = np.where(any_on, part[:, 1] - part[:, 0], np.inf)
    if slip == "largest_everywhere":
        arg[:] = arg[:, -1:, :]
    shape = (n_obj, nr, H, W)
    raw, tol, arg, gap, e_best = (lmb.kernel_order(a).reshape(shape) for a in (raw, tol, arg, gap, e_best))
    T, tol_T = lmb.local_transform_ref(raw, tol, bias)
    T = np.where(arg < 0, 1.0, T) if slip is None else T                          # 2 sigmoid(5e4 + b) - 1 is 1 exactly, in float32 and float64
    return dict(T=T, tol_T=tol_T, raw=raw, tol_raw=tol, arg=arg, gap=gap, e_best=e_best)


# ------------------------------------------------------------------------------------------ gradients and their bounds
def grad_ref(go, T, tol_T, arg, query, prev, e_go=0.0, no_gate=False, dq=None, dp=None, k_prev=None):
    """go, T, tol_T, arg [O, n_radii, H, W]; query, prev [H, W, C].  -> dict(grad_query, tol_query, grad_prev, tol_prev [H * W, C];
    grad_bias, tol_bias [O]; g, e_g [O, n_radii, H, W]; counts [H * W]: pairs per previous-frame pixel; e_prev, mag_prev [H * W, C]: the
    two sums behind tol_prev = e_prev + gamma(k) mag_prev).
    no_gate: the slip of a gate without its 1 - T^2 factor (g = grad_out / 2).  dq, dp: see forward_ref.  k_prev: the additions a term of
    grad_prev passes through at most, where the rows' own pair counts may not be used (bit-equal previous-frame pixels: which of them
    collects the pairs is decided by a tie)."""
    n_obj, nr, H, W = T.shape
    m = H * W
    C = query.shape[-1]
    q, p = np.asarray(query, np.float64).reshape(m, C), np.asarray(prev, np.float64).reshape(m, C)
    g, e_g = mgb.gate_ref(go, T, tol_T, e_go)
    if no_gate:
        g = 0.5 * np.asarray(go, np.float64)
    live = arg >= 0
    g, e_g = np.where(live, g, 0.0), np.where(live, e_g, 0.0)
    gq, tq, mag_q = np.zeros((m, C)), np.zeros((m, C)), np.zeros((m, C))
    gp, tp, mag_p = np.zeros((m, C)), np.zeros((m, C)), np.zeros((m, C))
    counts = np.zeros(m, np.int64)
    for o in range(n_obj):
        for ch in range(nr):
            a = arg[o, ch].reshape(m)
            idx = np.nonzero(a >= 0)[0]
            if idx.size == 0:
                continue
            rows = a[idx]
            gg, ee = g[o, ch].reshape(m)[idx, None], e_g[o, ch].reshape(m)[idx, None]
            diff = q[idx] - p[rows]
            term = 2.0 * gg * diff
            e = mgb._term_err(gg, ee, np.abs(diff))
            if dq is not None:
                e = e + 2.0 * (np.abs(gg) + ee) * (dq[idx] + dp[rows]) * (1.0 + 2.0 * U)
            gq[idx] += term
            tq[idx] += e
            mag_q[idx] += np.abs(term) + e
            np.add.at(gp, rows, -term)
            np.add.at(tp, rows, e)
            np.add.at(mag_p, rows, np.abs(term) + e)
            counts += np.bincount(rows, minlength=m)
    tq = tq + gamma(n_obj * nr) * mag_q
    k_rows = np.maximum(counts, 1).astype(np.float64) if k_prev is None else np.full(m, float(k_prev))
    tp = tp + gamma(k_rows)[:, None] * mag_p
    k_b = min(m, LG_BIAS_PIX) * nr + -(-m // LG_BIAS_PIX)
    gb = g.sum((1, 2, 3))
    tb = e_g.sum((1, 2, 3)) + gamma(k_b) * (np.abs(g) + e_g).sum((1, 2, 3))
    return dict(grad_query=gq, tol_query=tq, grad_prev=gp, tol_prev=tp, grad_bias=gb, tol_bias=tb, g=g, e_g=e_g, counts=counts,
                e_prev=tp - gamma(k_rows)[:, None] * mag_p, mag_prev=mag_p)


ratio, check = mgb.ratio, mgb.check


def check_conditions(name, fwd, exempt=None, share=0.5):
    """The conditions on the inputs (float64 only): no (object, channel, pixel) with a candidate, outside `exempt` (bool, arg's shape: the
    planted duplicates), has a best / runner-up gap under GAP_FACTOR x the forward distance bound of its winner; at least `share` of the
    live outputs have T in (0.05, 0.95)."""
    live = fwd["arg"] >= 0
    if not live.any():
        return
    sel = live if exempt is None else live & ~exempt
    margin = fwd["gap"][sel] / np.maximum(fwd["e_best"][sel], 1e-300)
    assert margin.min() >= GAP_FACTOR, f"{name}: a best / runner-up gap is only {margin.min():.1f} x the forward bound"
    T = fwd["T"][live]
    ok = ((T > 0.05) & (T < 0.95)).mean()
    assert ok >= share, f"{name}: only {ok:.2f} of the live outputs are unsaturated"


# ------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "name C H W radii rate n_obj kind")
REAL = (2, 4, 6, 8, 10, 12)
R8 = (1, 2, 3, 4, 5, 6, 7, 8)


def _c(name, C, H, W, radii, rate=1, n_obj=3, kind="random"):
    return Case(name, C, H, W, tuple(radii), rate, n_obj, kind)


# maps 1 x 1, 3 x 5 (smaller than the 2 x 8 query tile), 2 x 8, 3 x 9, 15 x 17 (interior pixels at R = 6), 27 x 29 with the real radii;
# every C with every class of object and radius count at least once; atrous rates 2 and 3
CASES = [
    _c("C100_1x1_r1", 100, 1, 1, (3,), n_obj=1),
    _c("C36_1x1_r8", 36, 1, 1, R8, n_obj=3),
    _c("C100_3x5_r6_O17", 100, 3, 5, REAL, n_obj=17),
    _c("C4_3x5_r1_O30", 4, 3, 5, (2,), n_obj=30),
    _c("C128_2x8_r8_O3", 128, 2, 8, R8, n_obj=3),
    _c("C36_2x8_r6_O1", 36, 2, 8, REAL, n_obj=1),
    _c("C100_3x9_r8_O30", 100, 3, 9, R8, n_obj=30),
    _c("C4_3x9_r6_O17", 4, 3, 9, REAL, n_obj=17),
    _c("C100_15x17_r3", 100, 15, 17, (2, 4, 6), n_obj=3),
    _c("C128_15x17_r3_O17", 128, 15, 17, (2, 4, 6), n_obj=17),
    _c("C36_15x17_r3", 36, 15, 17, (2, 4, 6), n_obj=3),
    _c("C4_15x17_r1", 4, 15, 17, (5,), n_obj=3),
    _c("C100_27x29_real", 100, 27, 29, REAL, n_obj=4),
    _c("C36_27x29_real", 36, 27, 29, REAL, n_obj=3),
    _c("C100_15x17_rate2", 100, 15, 17, (3, 4, 9), rate=2, n_obj=3),
    _c("C36_15x17_rate2", 36, 15, 17, (3, 4, 9), rate=2, n_obj=3),
    _c("C128_15x17_rate3", 128, 15, 17, (3, 7, 12), rate=3, n_obj=3),
    _c("C4_15x17_rate3", 4, 15, 17, (3, 7, 12), rate=3, n_obj=3),
]
PLANTED = _c("planted_C100_15x17", 100, 15, 17, (2, 4, 6), n_obj=4, kind="planted")
PLANTED_LDS = _c("planted_C36_15x17", 36, 15, 17, (2, 4, 6), n_obj=4, kind="planted")
MEMORY = _c("memory_C100_31x33", 100, 31, 33, REAL, n_obj=4)
BY_NAME = {c.name: c for c in CASES + [PLANTED, PLANTED_LDS, MEMORY]}
SINGLE, DUP_LO, DUP_HI, DUP_QUERY = (7, 8), (3, 12), (7, 12), (8, 12)      # planted case: (row, column) on the 15 x 17 map


def window(case):
    return case.rate * (case.radii[-1] // case.rate)


def _labels(rng, case):
    """-> bits [H * W] uint32 and the planted duplicates [(lo, hi)] (pixel indices)."""
    H, W, n_obj = case.H, case.W, case.n_obj
    m = H * W
    if case.kind == "planted":
        bits = np.where(rng.random_sample(m) < 0.5, 1, 0).astype(np.int64)           # object 0 scattered, object 3 absent
        px = lambda rc: rc[0] * W + rc[1]
        bits[px(SINGLE)] |= 1 << 1
        bits[px(DUP_LO)] |= 1 << 2
        bits[px(DUP_HI)] |= 1 << 2
        dup = [(px(DUP_LO), px(DUP_HI))]
    else:
        owner = rng.randint(0, n_obj, m)
        owner[rng.random_sample(m) < 0.15] = -1
        if m > 1:
            owner[rng.randint(0, m)] = 0
        bits = np.where(owner >= 0, 1 << np.maximum(owner, 0), 0).astype(np.int64)
        dup = []
    high = rng.random_sample(m) < 0.1
    high[0] = True
    extra = (1 << 31) | (1 << min(n_obj, 30)) if n_obj < 30 else (1 << 31) | (1 << 30)
    bits[high] |= extra
    return (bits & 0xFFFFFFFF).astype(np.uint32), dup


def case_inputs(case):
    """-> dict(query, prev [H, W, C] float32, bits [H * W] uint32, bias [O] float32, grad_out [O, n_radii, H, W] float32, dup)."""
    C, H, W, n_obj = case.C, case.H, case.W, case.n_obj
    rng = np.random.RandomState(zlib.crc32(("local_grad/" + case.name).encode()) & 0x7FFFFFFF)
    s = 1.0 / np.sqrt(C)
    query, prev = (s * rng.standard_normal((H, W, C))).astype(f32), (s * rng.standard_normal((H, W, C))).astype(f32)
    bits, dup = _labels(rng, case)
    if case.kind == "planted":
        prev.reshape(-1, C)[dup[0][1]] = prev.reshape(-1, C)[dup[0][0]]
    bias = ((0.6 if C == 4 else 0.0) + 0.3 * rng.standard_normal(n_obj)).astype(f32)
    grad_out = rng.standard_normal((n_obj, len(case.radii), H, W)).astype(f32)
    exempt = planted_exempt(case)
    for _ in range(200):
        fwd = forward_ref(query, prev, bits, case.radii, case.rate, n_obj, bias, dup=dup)
        near = (fwd["gap"] < 1.2 * GAP_FACTOR * fwd["e_best"]) & (fwd["arg"] >= 0)
        if exempt is not None:
            near &= ~exempt
        near = near.any((0, 1))
        if not near.any():
            break
        query[near] = (s * rng.standard_normal((int(near.sum()), C))).astype(f32)
    else:
        raise AssertionError(f"{case.name}: the gap condition was not met after 200 rounds of redrawing")
    return dict(query=query, prev=prev, bits=bits, bias=bias, grad_out=grad_out, dup=dup)


def planted_exempt(case):
    """bool [O, n_radii, H, W]: the entries of the planted duplicates' object (their gap is zero on purpose); None for other cases."""
    if case.kind != "planted":
        return None
    ex = np.zeros((case.n_obj, len(case.radii), case.H, case.W), bool)
    ex[2] = True
    return ex


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """-> (inputs, forward reference, gradient reference) of a case, computed once.  Treat as read-only."""
    case = BY_NAME[name]
    inp = case_inputs(case)
    fwd = forward_ref(inp["query"], inp["prev"], inp["bits"], case.radii, case.rate, case.n_obj, inp["bias"], dup=inp["dup"])
    grad = grad_ref(inp["grad_out"], fwd["T"], fwd["tol_T"], fwd["arg"], inp["query"], inp["prev"])
    return inp, fwd, grad


# ------------------------------------------------------------------------------------------ end to end: the resizes around the entries
FIXTURES = ("local_grad_down_O3", "local_grad_nodown_O3", "local_grad_down_orisize_C100", "local_grad_atrous2", "local_grad_absent")
FIXTURE_UNLABELLED = "local_grad_unlabelled"


def interp_matrix(n_in, n_out):
    """[n_out, n_in] float64: torch's bilinear resize with align_corners=True along one axis."""
    M = np.zeros((n_out, n_in))
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for i in range(n_out):
        src = scale * i
        i0 = min(int(np.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        lam = src - i0
        M[i, i0] += 1.0 - lam
        M[i, i1] += lam
    return M


def resize_matrix(h, w, H, W):
    """[H * W, h * w]: the 2-D resize as one matrix on row-major pixels."""
    return np.kron(interp_matrix(h, H), interp_matrix(w, W))


def nearest_index(n_in, n_out):
    """torch 'nearest': source index floor(dst * in / out) per destination index."""
    return np.minimum(np.floor(np.arange(n_out) * (n_in / n_out)).astype(np.int64), n_in - 1)


def labels_to_bits(labels):
    """aoc_label_bits on [h, w, O] labels -> [h, w] uint32: bit o where the label is above 0.9, bit 31 where the labels sum above 0.9."""
    lab = np.asarray(labels, np.float64)
    bits = np.zeros(lab.shape[:2], np.int64)
    for o in range(lab.shape[2]):
        bits |= (lab[:, :, o] > 0.9).astype(np.int64) << o
    bits |= (lab.sum(2) > 0.9).astype(np.int64) << 31
    return (bits & 0xFFFFFFFF).astype(np.uint32)


def fixture_args(fx):
    radii = [int(r) for r in fx["multi_local_distance"]]
    ori = None if int(fx["ori_size"][0]) == 0 else (int(fx["ori_size"][0]), int(fx["ori_size"][1]))
    return radii, ori, int(fx["atrous_rate"]), bool(fx["allow_downsample"])


def fixture_ref(fx, bias=None, weight=None):
    """The numpy reference of local_train.local_matching on a recorded fixture, with its bounds for float32 operands run through torch's
    float32 interpolate.  -> dict(out, tol_out [1, Ho, Wo, O, nr]; grad_query, tol_query, grad_prev, tol_prev [h, w, C]; grad_bias,
    tol_bias [O]; fwd, grad: the references at matching resolution; Wd, Wo: the resize matrices or None).

    What the interpolation adds (module docstring of test_gpu_local_grad.py): a resized value is a sum of at most four products with
    weights that are themselves products of two factors: at most 6 roundings, so the operands are off by dq = gamma(6) Wd |x|; the output is
    off by Wo tol_T + gamma(6) Wo (|T| + tol_T); the incoming gradient by e_go = gamma(k + 3) |Wo|^T |weight| and the outgoing ones by
    gamma(k + 3) |Wd|^T |grad| + |Wd|^T tol, k the most non-zeros in a column of the matrix (that many atomically added terms, each a product
    of the gradient and two weight factors)."""
    radii, ori, rate, down = fixture_args(fx)
    x_p, x_q = fx["in_prev"].astype(np.float64), fx["in_query"].astype(np.float64)
    h, w, C = x_q.shape
    n_obj = fx["in_labels"].shape[2]
    nr = len(radii)
    bias = fx["in_bias"] if bias is None else bias
    weight = fx["weight"] if weight is None else weight
    ori = (h, w) if ori is None else ori
    if down:
        H, W = h // 2 + 1, w // 2 + 1
        Wd = resize_matrix(h, w, H, W)
        q, p = Wd @ x_q.reshape(-1, C), Wd @ x_p.reshape(-1, C)
        dq, dp = gamma(6) * (Wd @ np.abs(x_q.reshape(-1, C))), gamma(6) * (Wd @ np.abs(x_p.reshape(-1, C)))
        assert (q.astype(f32) == q).all() and (p.astype(f32) == p).all(), "the fixture's resized operands are float32 values (weights 0 / 1)"
    else:
        H, W, Wd = h, w, None
        q, p, dq, dp = x_q.reshape(-1, C), x_p.reshape(-1, C), None, None
    bits = labels_to_bits(fx["in_labels"])
    if (H, W) != ori:
        bits = bits[nearest_index(h, H)][:, nearest_index(w, W)]
    fwd = forward_ref(q.reshape(H, W, C).astype(f32), p.reshape(H, W, C).astype(f32), bits.reshape(-1), radii, rate, n_obj, bias, dq=dq, dp=dp)
    wgt = np.asarray(weight, np.float64).reshape(ori[0] * ori[1], n_obj * nr)                   # [pixels, (o, ch)]
    T_flat = fwd["T"].reshape(n_obj * nr, H * W).T                                             # [HW, (o, ch)]
    tol_flat = fwd["tol_T"].reshape(n_obj * nr, H * W).T
    if (H, W) != ori:
        Wo = resize_matrix(H, W, ori[0], ori[1])
        out = Wo @ T_flat
        tol_out = Wo @ tol_flat + gamma(6) * (Wo @ (np.abs(T_flat) + tol_flat))
        k = int((Wo != 0).sum(0).max())
        go, e_go = Wo.T @ wgt, gamma(k + 3) * (Wo.T @ np.abs(wgt))
    else:
        Wo, out, tol_out, go, e_go = None, T_flat, tol_flat, wgt, np.zeros_like(wgt)
    to_planes = lambda a: a.T.reshape(n_obj, nr, H, W)
    grad = grad_ref(to_planes(go), fwd["T"], fwd["tol_T"], fwd["arg"], q.reshape(H, W, C), p.reshape(H, W, C), e_go=to_planes(e_go), dq=dq, dp=dp)
    res = dict(fwd=fwd, grad=grad, Wd=Wd, Wo=Wo, grad_bias=grad["grad_bias"], tol_bias=grad["tol_bias"],
               out=out.reshape(1, ori[0], ori[1], n_obj, nr), tol_out=tol_out.reshape(1, ori[0], ori[1], n_obj, nr))
    for key, src in (("query", "query"), ("prev", "prev")):
        gv, tv = grad["grad_" + src], grad["tol_" + src]
        if Wd is not None:
            k = int((Wd != 0).sum(0).max())
            tv = gamma(k + 3) * (np.abs(Wd).T @ np.abs(gv)) + np.abs(Wd).T @ tv
            gv = Wd.T @ gv
        res["grad_" + key], res["tol_" + key] = gv.reshape(h, w, C), tv.reshape(h, w, C)
    return res
