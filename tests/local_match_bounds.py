"""Float64 reference, bound, slips and inputs for the window kernels of csrc/local_match.hip (aoc_local_window_match_ex /
aoc_local_window_match_pair), shared by test_local_match_host.py (no GPU) and test_gpu_local_match.py.  Pure numpy; the library is not
imported here.  U, gamma and the (want, tol) / slip convention are those of float64_bounds.py.

The kernels: for a query pixel, an object o and nested window radii r_0 < r_1 < ..., the minimum of |q - p|^2 = (|q|^2 + |p|^2) - 2 q.p over
the previous frame's pixels p that carry label bit o and sit at an offset (dy, dx), both multiples of the atrous rate, with
max(|dy|, |dx|) // rate <= r_i // rate; AOC_PAD_DISTANCE where there is none.  C = 100 / 128 take local_window_reg_kernel, every other C
local_window_kernel<32> (the LDS-image kernel).  No constant here is fitted to a kernel's output."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import torch

from float64_bounds import U, _check_bound, gamma

UH = 2.0 ** -11            # unit roundoff of float16
SUBH = 2.0 ** -25          # half the spacing of float16's subnormals: what a rounding to float16 is off by below 2^-14
PAD = 5.0e4                # AOC_PAD_DISTANCE
PAD_H = float(np.float16(PAD))      # 49984: the pad of the float16 mode
KEPT_BIT = 0x80000000      # AOC_ROW_KEPT_BIT
MAX_OBJECTS = 30
_FAR = 1 << 20             # ring of a pair that does not count

f32 = np.float32


def kernel_of(C):
    return "reg" if C in (100, 128) else "lds"


# ------------------------------------------------------------------------------------------ per-pair distances and their bound
def _widen(a, f16):
    a = np.asarray(a, f32)
    if f16:
        a = a.astype(np.float16)
    return a.astype(np.float64)


def pair_distances(query, prev, f16=False, channels=None, e_p2=None):
    """D[i, j] = |q_i - p_j|^2 written as the kernels write it, (|q_i|^2 + |p_j|^2) - 2 q_i.p_j, in float64 over all pairs of pixels, and
    E[i, j], the bound on |kernel's float32 value - D[i, j]|.  query, prev [H, W, C] float32 (rounded to float16 first in f16 mode: the
    value the kernel works on).

    float32 mode.  |q|^2, |p|^2 and q.p are sums of C products.  The register kernel adds them as four fmaf chains per lane, a fold and two
    shuffle adds, the LDS-image kernel one after the other (1 + C / 4 + 2 <= C roundings on the way of a term for the query, C for a
    candidate), the matrix instruction in an order of its own that is not documented: a term goes through at most C roundings in each, so
    every sum is within gamma(C) x (sum of the terms' magnitudes) whatever the order:
        e_q2 = gamma(C) |q|^2,  e_p2 = gamma(C) |p|^2,  e_dot = gamma(C) sum_c |q_c p_c|.
    s = fl(q2^ + p2^):  e_s = e_q2 + e_p2 + U (|q|^2 + |p|^2 + e_q2 + e_p2);  2 acc is exact;  d = fl(s^ - 2 acc^):
        E = pre + U (|D| + pre),  pre = e_s + 2 e_dot.
    float16 mode.  Every aoc_h(x) is one more rounding of a float32 value to float16: x (1 + UH) + SUBH at most (SUBH covers the subnormal
    range, squares below 2^-14).  The squares are rounded (aoc_h(v v), the float32 product of two float16 values is exact), added in float32
    (gamma(C) as above) and the sum is rounded; the accumulator of the matrix instruction is rounded once; aoc_h(q2 + y2) is a float32
    addition and a rounding; so is the final aoc_h(. - 2 aoc_h(acc)).  Magnitudes are O(1), far from 65504.
    e_p2 [pixels of prev]: the error of the candidates' norms where the kernel does not compute them itself (a caller-supplied float32 norm:
    global_match_bounds.py); it replaces the derived one."""
    q = _widen(query, f16).reshape(-1, query.shape[-1])
    p = _widen(prev, f16).reshape(-1, prev.shape[-1])
    if channels is not None:
        q, p = q[:, :channels], p[:, :channels]
    C = q.shape[1]
    g = gamma(max(C, 1))
    q2, p2 = (q * q).sum(1), (p * p).sum(1)
    dot, adot = q @ p.T, np.abs(q) @ np.abs(p).T
    S = q2[:, None] + p2[None, :]
    D = S - 2.0 * dot

    def norm_err(n2):
        if not f16:
            return g * n2
        e = UH * n2 + C * SUBH                       # the rounded squares
        e = e + g * (n2 + e)                         # their float32 sum
        return e + UH * (n2 + e) + SUBH              # aoc_h of the sum

    e_q2, e_p2 = norm_err(q2), norm_err(p2) if e_p2 is None else np.asarray(e_p2, np.float64)
    e_dot = g * adot
    if f16:
        e_dot = e_dot + UH * (np.abs(dot) + e_dot) + SUBH
    e_s = e_q2[:, None] + e_p2[None, :]
    e_s = e_s + U * (S + e_s)
    if f16:
        e_s = e_s + UH * (S + e_s) + SUBH
    pre = e_s + 2.0 * e_dot
    E = pre + U * (np.abs(D) + pre)
    if f16:
        E = E + UH * (np.abs(D) + E) + SUBH
    return D, E


# ------------------------------------------------------------------------------------------ which pair counts for which radius
def pair_rings(H, W, rate, all_offsets=False, clamped_border=False):
    """ring[i, j] = max(|dy|, |dx|) // rate of query pixel i and candidate pixel j where both offsets are multiples of the rate, _FAR where
    they are not.  all_offsets: the slip that counts every offset.  clamped_border: the slip of a candidate column outside the map read at
    the clamped column (features and label of column 0 or W - 1): a border-column candidate then also appears at every |dx| beyond its
    own, of which the smallest multiple of the rate is the one that matters for nested windows."""
    ys, xs = np.divmod(np.arange(H * W), W)
    dy = np.abs(ys[:, None] - ys[None, :])
    dx = np.abs(xs[:, None] - xs[None, :])
    cheb = np.maximum(dy, dx) // rate
    if all_offsets:
        return cheb
    ring = np.where((dy % rate == 0) & (dx % rate == 0), cheb, _FAR)
    if clamped_border:
        qx, px = xs[:, None], xs[None, :]
        left = np.where(px == 0, rate * (qx // rate + 1), _FAR)
        right = np.where(px == W - 1, rate * ((W - 1 - qx) // rate + 1), _FAR)
        alt_dx = np.minimum(left, right)
        alt = np.where((dy % rate == 0) & (alt_dx < _FAR), np.maximum(dy, alt_dx) // rate, _FAR)
        ring = np.minimum(ring, alt)
    return ring


def object_planes(bits, n_obj, high_bits=False):
    """[n_obj, HW] bool: pixel carries bit o, for o < n_obj only, the kept bit masked off.  high_bits: the slip in which object o also takes
    the pixels of bit o + n_obj (bit 31 included) where that bit exists."""
    bits = np.asarray(bits).astype(np.int64) & 0xFFFFFFFF
    planes = np.stack([(bits >> o) & 1 for o in range(n_obj)]).astype(bool)
    if high_bits:
        for o in range(n_obj):
            if o + n_obj <= 31:
                planes[o] |= ((bits >> (o + n_obj)) & 1).astype(bool)
    return planes


def kernel_order(x):
    """[.., n_radii, ..] in plain order r_0 .. r_last on axis 1 -> the kernel's channel order [largest, r_0, r_1, ...]."""
    return np.concatenate([x[:, -1:], x[:, :-1]], axis=1)


def nested_min(D, E, ring, planes, radii, rate, pad, open_rim=False):
    """min of D over the pairs that count, per object and radius: -> (want, tol) [n_obj, n_radii, HW] in plain radius order.  tol is the
    largest E among the pairs that count (a minimum of perturbed values is off by at most the largest perturbation); pad outputs have
    tol 0."""
    n_obj, n_r, n = planes.shape[0], len(radii), D.shape[0]
    want = np.full((n_obj, n_r, n), pad, np.float64)
    tol = np.zeros((n_obj, n_r, n), np.float64)
    for o in range(n_obj):
        cols = np.nonzero(planes[o])[0]
        if cols.size == 0:
            continue
        d, e, r = D[:, cols], E[:, cols], ring[:, cols]
        for i, rad in enumerate(radii):
            ra = rad // rate
            on = (r < ra) if open_rim else (r <= ra)
            any_on = on.any(1)
            want[o, i] = np.where(any_on, np.where(on, d, np.inf).min(1), pad)
            tol[o, i] = np.where(on, e, 0.0).max(1)
    return want, tol


SLIPS = ("open_rim", "clamped_border", "all_offsets", "tail_channels", "high_bits", "shifted_channels")


def local_window_ref(query, prev, bits, radii, rate, n_obj, f16=False, slip=None):
    """-> (want_raw, tol_raw) [n_obj, n_radii, H, W] float64 in the kernel's channel order.  slip: one of SLIPS, the same reference with one
    deliberate mistake:
    open_rim          < instead of <= at every radius;
    clamped_border    candidate columns outside the map take the clamped column's pixel instead of none (local_window_reg_kernel's
                      branch-free load without its `ok` select);
    all_offsets       offsets that are not multiples of the rate count;
    tail_channels     channels 16 (C // 16) onwards dropped (the register kernel's one-channel-per-lane tail at C = 100);
    high_bits         object o also takes the candidates of bit o + n_obj (bits at or above n_obj, the kept bit, treated as objects);
    shifted_channels  nested-window channels in plain order [r_0, ..., largest] instead of [largest, r_0, ...]."""
    assert slip is None or slip in SLIPS, slip
    H, W, C = query.shape
    D, E = pair_distances(query, prev, f16, channels=16 * (C // 16) if slip == "tail_channels" else None)
    ring = pair_rings(H, W, rate, all_offsets=slip == "all_offsets", clamped_border=slip == "clamped_border")
    planes = object_planes(bits, n_obj, high_bits=slip == "high_bits")
    want, tol = nested_min(D, E, ring, planes, list(radii), rate, PAD_H if f16 else PAD, open_rim=slip == "open_rim")
    if slip != "shifted_channels":
        want, tol = kernel_order(want), kernel_order(tol)
    return want.reshape(n_obj, len(radii), H, W), tol.reshape(n_obj, len(radii), H, W)


# ------------------------------------------------------------------------------------------ aoc_proto_transform
def _f(t):
    return 2.0 / (1.0 + np.exp(-t)) - 1.0


def local_transform_ref(want_raw, tol_raw, bias):
    """aoc_proto_transform of the raw reference: want = 2 sigmoid(d + b) - 1, bias [n_obj] (float32 values) or None.

    t^ = fl(d^ + b) is off by e_t = tol_raw + U (|t| + tol_raw).  f(t) = 2 sigmoid(t) - 1 is increasing with slope 2 s (1 - s) <= 1 / 2: what
    e_t does to it is max(f(t + e_t) - f(t), f(t) - f(t - e_t)), evaluated, not linearised (as _rstd_err does).  Then the kernel's own
    roundings at t^, with s^ up to sigmoid(t + e_t) and 1 - s^ up to 1 - sigmoid(t - e_t): expf within 2 ulp (relative 4 U, the convention
    of tanhf in float64_bounds.py), so 1 + expf is off by relative 4 U (1 - s) + U (1 + 4 U); the division passes that on and rounds once;
    s - 0.5 and the doubling round once each (both are in fact exact for s in [1 / 4, 1]; counted all the same)."""
    want_raw, tol_raw = np.asarray(want_raw, np.float64), np.asarray(tol_raw, np.float64)
    b = np.zeros(want_raw.shape[0]) if bias is None else np.asarray(bias, f32).astype(np.float64)
    t = want_raw + b.reshape(-1, 1, 1, 1)
    e_t = tol_raw + U * (np.abs(t) + tol_raw)
    want = _f(t)
    df = np.maximum(_f(t + e_t) - want, want - _f(t - e_t))
    s_hi = 1.0 / (1.0 + np.exp(-(t + e_t)))
    one_minus_s = 1.0 - 1.0 / (1.0 + np.exp(-(t - e_t)))
    rd = 4.0 * U * one_minus_s + U * (1.0 + 4.0 * U)
    rs = rd / (1.0 - rd)
    rs = rs + U * (1.0 + rs)
    e_s = s_hi * rs
    half = np.abs(s_hi - 0.5) + e_s
    e_out = 2.0 * (e_s + U * half)
    e_out = e_out + U * (np.abs(want) + df + e_out)
    return want, df + e_out


# ------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "name C H W radii rate n_obj f16 pair transformed")


def _case(name, C, H, W, radii, rate=1, n_obj=7, f16=False, pair=False, transformed=False):
    return Case(name, C, H, W, tuple(radii), rate, n_obj, f16, pair, transformed)


R8 = (1, 2, 3, 5, 8, 13, 21, 31)


def _cases():
    c = []
    # the register kernel (C = 100 / 128)
    c.append(_case("reg_model_C100", 100, 23, 37, (2, 4, 6, 8, 10, 12), n_obj=4, transformed=True))
    c.append(_case("reg_model_C128", 128, 23, 37, (2, 4, 6, 8, 10, 12), n_obj=4))
    c.append(_case("reg_max_radii_objects_R31", 100, 23, 37, R8, n_obj=30))
    c.append(_case("reg_four_groups_R22", 128, 9, 41, (22,)))
    c.append(_case("reg_radius0_R28", 128, 9, 41, (0, 28)))
    for H, W in ((1, 1), (1, 9), (2, 7), (3, 8), (5, 17)):
        for radii in ((1, 3), (4, 12)):
            c.append(_case(f"reg_map_{H}x{W}_r{radii[0]}_{radii[1]}", 100, H, W, radii))
    c.append(_case("reg_rate2_r3_4_9", 100, 11, 19, (3, 4, 9), rate=2, transformed=True))
    c.append(_case("reg_rate2_collapse_r2_3", 100, 11, 19, (2, 3), rate=2))
    c.append(_case("reg_rate3_r3_7_12", 128, 13, 21, (3, 7, 12), rate=3))
    c.append(_case("reg_f16_C100_rate1", 100, 11, 19, (2, 5, 9), f16=True, transformed=True))
    c.append(_case("reg_f16_C100_rate2", 100, 11, 19, (3, 4, 9), rate=2, f16=True))
    c.append(_case("reg_f16_C128_rate1", 128, 11, 19, (2, 5, 9), f16=True))
    c.append(_case("reg_f16_C128_rate2", 128, 11, 19, (3, 4, 9), rate=2, f16=True))
    # the LDS-image kernel (every other C)
    for C in (36, 64, 4, 124):
        c.append(_case(f"lds_C{C}_13x21", C, 13, 21, (2, 4, 6), transformed=C == 36))
        for r in (8, 9, 16, 17, 25):
            c.append(_case(f"lds_C{C}_7x18_R{r}", C, 7, 18, (r,)))
        for H, W in ((1, 1), (3, 17), (5, 16)):
            c.append(_case(f"lds_C{C}_map_{H}x{W}", C, H, W, (2, 5)))
    c.append(_case("lds_max_radii_objects_C4", 4, 5, 16, (1, 2, 3, 4, 5, 6, 7, 8), n_obj=30))
    c.append(_case("lds_rate2_C36", 36, 13, 21, (3, 4, 9), rate=2))
    c.append(_case("lds_f16_C64", 64, 13, 21, (2, 4, 6), f16=True, transformed=True))
    # the pair entry: one launch with grid z = 2 at C = 100, two launches at C = 36
    c.append(_case("pair_C100", 100, 9, 21, (2, 5, 9), pair=True, transformed=True))
    c.append(_case("pair_C36", 36, 9, 21, (2, 5, 9), pair=True))
    return c


LOCAL_CASES = _cases()
# the LDS-image kernel above 64 KB of dynamic LDS: 66 560 and 104 448 bytes
LOCAL_LDS_CASES = [_case("lds_66KB_C36_O24", 36, 5, 18, R8, n_obj=24), _case("lds_102KB_C124_O30", 124, 5, 18, R8, n_obj=30)]
CASE_BY_NAME = {c.name: c for c in LOCAL_CASES + LOCAL_LDS_CASES}


def lds_image_bytes(C, radii, rate, n_obj):
    """local_window_match_impl's dynamic LDS request for local_window_kernel."""
    R = radii[-1] // rate * rate
    rs = 4 * ((C // 4 + 3) // 4 * 4) + 4
    ng = (16 + 2 * R + 15) // 16
    return ng * 16 * rs * 4 + ng * 16 * 8 + 32 * 4 + 4 * 16 * len(radii) * n_obj * 4


# ------------------------------------------------------------------------------------------ inputs
V_LINE, H_LINE, BORDER, ODD = 1, 2, 3, 4


def absent_objects(n_obj):
    """Objects that no pixel carries: 6, 11, 16, ...  (Four-object cases have none: objects 0 to 3 all have a role.)"""
    return [o for o in range(6, n_obj) if o % 5 == 1]


def local_inputs(case):
    """-> dict(query, prev[, prev_b], bits, bias).  Features s randn with s = 0.5 / sqrt(C): |q - p|^2 is O(1) and the transformed outputs stay
    off saturation.  Labels, by construction rather than luck:
      object 1   a vertical line at one column c0, object 2 a horizontal line at one row r0, placed so that where the map allows it a query
                 sits exactly rate (r_0 // rate) columns / rows away and sees the line on the rim of its smallest window only (open_rim);
      object 3   the outermost ring of pixels of the map only (clamped_border);
      object 4   where rate > 1: only pixels with y % rate == x % rate == 1, at offsets that are no multiples of the rate from every query
                 with y % rate == x % rate == 0 (all_offsets);
      the other objects but the absent ones (absent_objects) are scattered: every pixel carries each with probability rho (0.08, more on
                 tiny maps), so small windows are neither all empty nor all full;
      a tenth of the pixels, pixel 0 among them, carry bit 31 and one bit n_obj + k (<= 30), k an absent object where there is one: the
                 entry must ignore them (high_bits)."""
    C, H, W, n_obj, rate = case.C, case.H, case.W, case.n_obj, case.rate
    rng = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7FFFFFFF)
    s = 0.5 / np.sqrt(C)
    out = {"query": (s * rng.standard_normal((H, W, C))).astype(f32), "prev": (s * rng.standard_normal((H, W, C))).astype(f32)}
    if case.pair:
        out["prev_b"] = (s * rng.standard_normal((H, W, C))).astype(f32)
    ys, xs = np.divmod(np.arange(H * W), W)
    bits = np.zeros(H * W, np.int64)
    e0 = case.radii[0] // rate * rate
    c0 = min(W // 2, max(0, W - 1 - e0))
    r0 = min(H // 2, max(0, H - 1 - e0))
    bits[xs == c0] |= 1 << V_LINE
    bits[ys == r0] |= 1 << H_LINE
    bits[(ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)] |= 1 << BORDER
    roles = {V_LINE, H_LINE, BORDER}
    if rate > 1 and n_obj > ODD:
        roles.add(ODD)
        bits[(ys % rate == 1) & (xs % rate == 1)] |= 1 << ODD
    absent = absent_objects(n_obj)
    rho = min(0.5, max(0.08, 3.0 / (H * W)))
    for o in range(n_obj):
        if o in roles or o in absent:
            continue
        bits[rng.random_sample(H * W) < rho] |= 1 << o
    bits[0] |= 1
    high = rng.random_sample(H * W) < 0.1
    high[0] = True
    k_max = min(n_obj - 1, 30 - n_obj)
    ks = [k for k in absent if k <= k_max] or list(range(k_max + 1))
    k = np.asarray(ks)[rng.randint(0, len(ks), H * W)]
    bits[high] |= (1 << 31) | (1 << (n_obj + k[high]))
    out["bits"] = bits.astype(np.uint32)
    b = rng.uniform(0.25, 1.0, n_obj) * np.where(np.arange(n_obj) % 2 == 0, 1.0, -1.0)
    out["bias"] = b.astype(f32)
    return out


def local_slips(case):
    """Which slips a case uses (each must leave the bound there; the host test proves it):
    high_bits         every case (pixel 0 always carries high bits);
    open_rim          where a rim can be reached: some window's radius in pixels fits inside the map's larger side (a 7 x 18 map has no pixel
                      25 columns away from any other) and the map has more than one pixel, or the first radius is 0;
    clamped_border    where rate > 1 only.  At rate 1 a border pixel read again at a clamped column is the same pixel at a larger offset than
                      its own: nested windows already hold it and no minimum moves, so that slip cannot be seen; at rate > 1 the pixel's own
                      offset may be no multiple of the rate while the clamped one is;
    all_offsets       rate > 1;
    tail_channels     C no multiple of 16;
    shifted_channels  more than one ring after // rate, and a pixel of the map beyond the smallest window (every channel is the same
                      otherwise);
    other_map         the pair entry (applied by the tests: the second output from the first map)."""
    kinds = ["high_bits"]
    reach = [r // case.rate * case.rate for r in case.radii]
    if reach[0] == 0 or (case.H * case.W > 1 and min(reach) <= max(case.H, case.W) - 1):
        kinds.append("open_rim")
    if case.rate > 1:
        kinds += ["clamped_border", "all_offsets"]
    if case.C % 16:
        kinds.append("tail_channels")
    if len(set(r // case.rate for r in case.radii)) > 1 and reach[0] <= max(case.H, case.W) - 2:
        kinds.append("shifted_channels")
    return kinds


@functools.lru_cache(maxsize=None)
def local_case_ref(name, which="prev"):
    """The reference of a case, computed once: -> (want_raw, tol_raw, {slip: want_raw of the slipped reference}).  Read-only arrays."""
    case = CASE_BY_NAME[name]
    inp = local_inputs(case)
    args = (inp["query"], inp[which], inp["bits"], case.radii, case.rate, case.n_obj, case.f16)
    want, tol = local_window_ref(*args)
    slips = {kind: local_window_ref(*args, slip=kind)[0] for kind in local_slips(case)}
    for a in (want, tol, *slips.values()):
        a.setflags(write=False)
    return want, tol, slips


def check_bound(got, want, tol, slip, what):
    """_check_bound on numpy arrays (copied: the cached references stay read-only)."""
    _check_bound(*(torch.from_numpy(np.array(a, dtype=np.float64)) for a in (got, want, tol, slip)), what)


def check_conditions(case, want_raw, want_t=None):
    """The conditions on the float64 reference alone (never on a kernel's output): on maps larger than 2 x 2 at least a quarter of the raw
    outputs are distances and at least one is pad; more than half of the transformed non-pad outputs are below 0.99."""
    pad = PAD_H if case.f16 else PAD
    is_pad = want_raw == pad
    if case.H * case.W > 4:
        assert (~is_pad).mean() >= 0.25, f"{case.name}: only {(~is_pad).mean():.3f} of the raw outputs are distances"
        assert is_pad.any(), f"{case.name}: no pad output"
    if want_t is not None:
        live = want_t[~is_pad]
        assert live.size and (live < 0.99).mean() > 0.5, f"{case.name}: transformed outputs saturate"
