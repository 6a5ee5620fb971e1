"""Float64 references and elementwise bounds for the kernels of csrc/decoder_tail.hip, in the manner of float64_bounds.py (U, gamma,
_check_bound and the film-gain / head-delta / plane-mean pieces come from there).  No constant is fitted to output: every bound follows from
the kernel's float32 expressions, which the library compiles with -ffp-contract=off (one rounding per operation; the explicit fmaf of the tap
sums one rounding per step).

Bicubic reference.  PyTorch's upsample_bicubic2d, align_corners=True: output index o reads the source coordinate o (in - 1) / (out - 1)
(0 when out = 1), i0 = its floor, t = its fraction, four taps at i0 - 1 .. i0 + 2 clamped to the map with the weights
    w0 = c2(t + 1), w1 = c1(t), w2 = c1(1 - t), w3 = c2(2 - t),
    c1(x) = ((A + 2) x - (A + 3)) x x + 1,   c2(x) = ((A x - 5 A) x + 8 A) x - 4 A,   A = -0.75.
Here the coordinate is split with Python integers (i0 and t exact), the weights are float64, and the taps are accumulated into the
[out, in] matrix of the 1-D interpolation (a clamped tap adds to the border column): the 2-D resize is My x Mx^T.

Weight error of the kernel (bicubic_taps).  t^ = fl(float(rem) / float(out - 1)): one rounding, |t^ - t| <= U t (+ dt_extra, what a reference
that forms the coordinate another way is itself off by).  The arguments x0 = fl(t^ + 1), u = fl(1 - t^), x3 = fl(u + 1) add one rounding
each.  A perturbed argument moves a weight by at most max |dw/dx| over its piece:
    c1'(x) = 3 (A + 2) x^2 - 2 (A + 3) x on [0, 1]: extreme at x = (A + 3) / (3 (A + 2)) = 0.6, |c1'| <= 1.35;
    c2'(x) = 3 A x^2 - 10 A x + 8 A on [1, 2]: -0.75 at 1, 0 at 2, 0.25 at x = 5/3, |c2'| <= 0.75.
The polynomial itself is evaluated in 5 (c1) or 6 (c2) rounded operations; its rounding error is carried step by step with the magnitudes
of the intermediate values (_c1_rounding, _c2_rounding), because the outer weights cancel to 0 at t = 0 and a relative count would not hold.

Tap sums.  fma(w3, x3, fma(w2, x2, fma(w1, x1, w0 x0))): every term goes through at most 4 roundings: gamma(4) sum |w^| |x|.  The kernel
runs the vertical pass first (v = My x, error EV), then the horizontal one on v^, then one multiplication by the gain."""
import numpy as np
import torch

from float64_bounds import U, _cdiv, _wave_dot_tol, gamma, head_delta_ref, plane_mean_ref, t64

A = -0.75
C1_SLOPE = 1.35
C2_SLOPE = 0.75


def _c1(x, a=A):
    return ((a + 2) * x - (a + 3)) * x * x + 1


def _c2(x, a=A):
    return ((a * x - 5 * a) * x + 8 * a) * x - 4 * a


def _step(val, err):
    """One rounded operation whose exact result is val (known to err before the rounding)."""
    return err + U * (np.abs(val) + err)


def _c1_rounding(x, dx):
    """Rounding error of ((1.25 x - 2.25) x) x + 1 evaluated in float32 at an argument of magnitude <= |x| + dx."""
    xa = np.abs(x) + dx
    p = 1.25 * x
    e = _step(p, 0.0)
    q = p - 2.25
    e = _step(q, e)
    r = q * x
    e = _step(r, e * xa)
    s = r * x
    e = _step(s, e * xa)
    return _step(s + 1, e)


def _c2_rounding(x, dx):
    """Rounding error of ((A x - 5 A) x + 8 A) x - 4 A evaluated in float32 (5 A, 8 A, 4 A are exact constants)."""
    xa = np.abs(x) + dx
    a = A * x
    e = _step(a, 0.0)
    b = a - 5 * A
    e = _step(b, e)
    c = b * x
    e = _step(c, e * xa)
    d = c + 8 * A
    e = _step(d, e)
    f = d * x
    e = _step(f, e * xa)
    return _step(f - 4 * A, e)


def bicubic_taps(n_in, n_out, dt_extra=0.0, a=A, align_corners=True):
    """-> idx [out, 4] (unclamped tap indices), w [out, 4] float64 weights, ew [out, 4] bound on the kernel's weight error."""
    o = np.arange(n_out, dtype=np.int64)
    if align_corners:
        if n_out > 1:
            num = o * (n_in - 1)
            i0 = num // (n_out - 1)
            t = (num - i0 * (n_out - 1)).astype(np.float64) / (n_out - 1)
        else:
            i0, t = np.zeros(1, np.int64), np.zeros(1)
    else:                                                     # the slip: half-pixel centres
        src = (o + 0.5) * (n_in / n_out) - 0.5
        i0 = np.floor(src).astype(np.int64)
        t = src - i0
    x0, u = t + 1, 1 - t
    x3 = u + 1
    w = np.stack([_c2(x0, a), _c1(t, a), _c1(u, a), _c2(x3, a)], 1)
    dt = U * t + dt_extra
    dx0, du = dt + U * x0, dt + U * u
    dx3 = du + U * x3
    ew = np.stack([C2_SLOPE * dx0 + _c2_rounding(x0, dx0), C1_SLOPE * dt + _c1_rounding(t, dt), C1_SLOPE * du + _c1_rounding(u, du),
                   C2_SLOPE * dx3 + _c2_rounding(x3, dx3)], 1)
    idx = i0[:, None] + np.arange(-1, 3)[None, :]
    return idx, w, ew


def bicubic_matrix(n_in, n_out, dt_extra=0.0, a=A, align_corners=True, zero_pad=False):
    """The [out, in] matrix M of the 1-D resize, the same with |w| (AM), the accumulated weight-error bound (E) and the number of taps that
    land in each entry (CNT), as float64 tensors.  zero_pad (a slip): taps outside the map are dropped instead of clamped."""
    idx, w, ew = bicubic_taps(n_in, n_out, dt_extra, a, align_corners)
    rows = np.repeat(np.arange(n_out), 4)
    cols = idx.reshape(-1)
    keep = np.ones_like(cols, bool)
    if zero_pad:
        keep = (cols >= 0) & (cols < n_in)
    cols = np.clip(cols, 0, n_in - 1)
    out = []
    for vals in (w.reshape(-1), np.abs(w).reshape(-1), ew.reshape(-1), np.ones(cols.size)):
        m = np.zeros((n_out, n_in))
        np.add.at(m, (rows[keep], cols[keep]), vals[keep])
        out.append(torch.from_numpy(m))
    return out


def bicubic_resize(x, H, W, **slip):
    """x [..., h, w] float64 -> [..., H, W]; slip: keyword arguments of bicubic_matrix (a=-0.5, align_corners=False, zero_pad=True)."""
    My = bicubic_matrix(x.shape[-2], H, **slip)[0]
    Mx = bicubic_matrix(x.shape[-1], W, **slip)[0]
    return torch.einsum("ih,...hw,jw->...ij", My, x, Mx)


def _scatter(idx, w, n_in):
    m = np.zeros((idx.shape[0], n_in))
    np.add.at(m, (np.repeat(np.arange(idx.shape[0]), 4), np.clip(idx, 0, n_in - 1).reshape(-1)), w.reshape(-1))
    return torch.from_numpy(m)


def bicubic_resize_swapped(x, H, W):
    """The slip 'h / w weights swapped': row i takes the weights of column i mod W and column j those of row j mod H (tap indices kept)."""
    h, w = x.shape[-2:]
    iy, wy, _ = bicubic_taps(h, H)
    ix, wx, _ = bicubic_taps(w, W)
    return torch.einsum("ih,...hw,jw->...ij", _scatter(iy, wx[np.arange(H) % W], h), x, _scatter(ix, wy[np.arange(W) % H], w))


def cat_scale_ref(x, low, gain, H, W, dgain=None, dt_extra=0.0):
    """aoc_bicubic_cat_scale.  x [N, Ce, h, w], low [N, Cr, H, W] or None, gain [N, Ce + Cr] or None (float64) -> (want, tol), both
    [N, Ce + Cr, H, W].  dgain: what the gain itself is already off by (the shortcut stage).

    Vertical pass: |v^ - v| <= EV = (Ey + gamma(4) (AMy + Ey)) |x|.  Horizontal pass on v^:
        ES = Ex |v| + (AMx + Ex) EV + gamma(4) (AMx + Ex) (|v| + EV).
    Gain: |g^ s^ - g s| <= dg |s| + (|g| + dg) ES, then one rounding of the product; gain = NULL multiplies by 1 exactly.  The shortcut
    planes are one product: U |g low| (+ dg |low|).  dt_extra: see bicubic_taps; one value or (rows, columns)."""
    N, Ce, h, w = x.shape
    dty, dtx = dt_extra if isinstance(dt_extra, tuple) else (dt_extra, dt_extra)
    My, AMy, Ey, _ = bicubic_matrix(h, H, dty)
    Mx, AMx, Ex, _ = bicubic_matrix(w, W, dtx)
    V = torch.einsum("ih,nchw->nciw", My, x)
    EV = torch.einsum("ih,nchw->nciw", Ey + gamma(4) * (AMy + Ey), x.abs())
    S = torch.einsum("nciw,jw->ncij", V, Mx)
    ES = (torch.einsum("nciw,jw->ncij", V.abs(), Ex) + torch.einsum("nciw,jw->ncij", EV, AMx + Ex)
          + gamma(4) * torch.einsum("nciw,jw->ncij", V.abs() + EV, AMx + Ex))
    full, dfull = S, ES
    if low is not None:
        full, dfull = torch.cat([S, low], 1), torch.cat([ES, torch.zeros_like(low)], 1)
    if gain is None:
        return full, dfull
    g = gain.view(N, -1, 1, 1)
    dg = torch.zeros_like(g) if dgain is None else dgain.view(N, -1, 1, 1)
    want = g * full
    tol = dg * full.abs() + (g.abs() + dg) * dfull
    return want, tol + U * (want.abs() + tol)


def column_sums(n_in, n_out, **slip):
    """c[s] = sum of the taps that land on source index s, and the bound on the kernel's c^: the weight errors of those taps plus their
    cnt[s] sequential additions (bicubic_plane_mean_kernel adds them in output order)."""
    M, AM, E, CNT = bicubic_matrix(n_in, n_out, **slip)
    cnt = CNT.sum(0)
    return M.sum(0), E.sum(0) + torch.tensor([gamma(int(k)) for k in cnt]) * (AM + E).sum(0)


def bicubic_plane_mean_ref(x, H, W, **slip):
    """aoc_bicubic_plane_mean.  x [P, h, w] -> (want [P], tol [P]); want equals the mean of the float64 upsample (linear and separable).
    A term fl(fl(cy cx) x) is two roundings, then at most ceil(hw / 256) additions in its thread, 6 wave-sum levels, 3 cross-wave additions,
    the division and the rounding of float(H W): depth = 2 + ceil(hw / 256) + 6 + 3 + 2."""
    P, h, w = x.shape
    cy, ecy = column_sums(h, H, **slip)
    cx, ecx = column_sums(w, W, **slip)
    want = torch.einsum("h,phw,w->p", cy, x, cx) / (H * W)
    ew = ecy.view(h, 1) * cx.abs().view(1, w) + (cy.abs() + ecy).view(h, 1) * ecx.view(1, w)
    wa = (cy.abs() + ecy).view(h, 1) * (cx.abs() + ecx).view(1, w)
    depth = 2 + _cdiv(h * w, 256) + 6 + 3 + 2
    tol = torch.einsum("hw,phw->p", ew + gamma(depth) * wa, x.abs()) / (H * W)
    return want, tol


def shortcut_stage_ref(x, low, head, weight, bias, slip=None, torch_f32=False):
    """aoc_shortcut_stage_enqueue -> dict(px, dpx, head, dhead, gain, dgain, out, dout).
    px = [mean of the upsample | mean of low] with the bounds of bicubic_plane_mean_ref and float64_bounds.plane_mean_ref; the extended head
    = [IA_head | sum_o px - px] with head_delta_ref's bound evaluated on |px| + dpx, plus what px is off by (sum_o dpx + dpx); the gain through
    the wave dot product of _wave_dot_tol with that as dx, tanh' <= 1 and 4 U for tanhf and the final addition; the output through
    cat_scale_ref with dgain.    slip: 'concat_reversed' (low first), 'no_minus' (px1_delta without - px1), or a dict of bicubic_matrix
    keywords / 'swapped' for the resize.
    torch_f32: the bounds for the reference's own float32 run of the same lines instead of the kernels' (the golden fixtures): the resize with
    torch_coordinate_error, avg_pool2d as a float32 sum of H W terms in any order (gamma(H W) on the mean of |.|, on top of what the
    pooled tensor is off by), nn.Linear as a dot product of D + Ce + Cr terms in any order (gamma of that + 1 for the bias)."""
    N, Ce, h, w = x.shape
    Cr, H, W = low.shape[1:]
    D = head.shape[1]
    dt_extra = (torch_coordinate_error(h), torch_coordinate_error(w)) if torch_f32 else 0.0
    bm, dbm = bicubic_plane_mean_ref(x.reshape(N * Ce, h, w), H, W)
    lm, dlm = plane_mean_ref(low.reshape(N * Cr, H * W))
    if torch_f32:
        up, dup = cat_scale_ref(x, None, None, H, W, None, dt_extra)
        dbm = (dup.mean((2, 3)) + gamma(H * W) * (up.abs() + dup).mean((2, 3))).reshape(-1)
        dlm = gamma(H * W) * low.abs().mean((2, 3)).reshape(-1)
    px = torch.cat([bm.view(N, Ce), lm.view(N, Cr)], 1)
    dpx = torch.cat([dbm.view(N, Ce), dlm.view(N, Cr)], 1)
    if isinstance(slip, dict):
        bm = bicubic_resize(x, H, W, **slip).mean((2, 3))
        px = torch.cat([bm, lm.view(N, Cr)], 1)
    elif slip == "swapped":
        px = torch.cat([bicubic_resize_swapped(x, H, W).mean((2, 3)), lm.view(N, Cr)], 1)
    elif slip == "concat_reversed":
        px = torch.cat([lm.view(N, Cr), bm.view(N, Ce)], 1)
    delta, _ = head_delta_ref(px, slip == "no_minus")
    _, ddelta = head_delta_ref(px.abs() + dpx)
    ddelta = ddelta + dpx.sum(0, keepdim=True) + dpx
    hx = torch.cat([head, delta], 1)
    dhx = torch.cat([torch.zeros_like(head), ddelta], 1)
    arg = hx @ weight.t() + bias
    gain = 1.0 + torch.tanh(arg)
    dgain = _wave_dot_tol(hx.abs(), dhx, weight.abs(), bias.abs(), D + Ce + Cr) + 4 * U
    if torch_f32:
        dgain = dhx @ weight.abs().t() + gamma(D + Ce + Cr + 1) * ((hx.abs() + dhx) @ weight.abs().t() + bias.abs()) + 4 * U
    if isinstance(slip, dict):
        up = bicubic_resize(x, H, W, **slip)
    elif slip == "swapped":
        up = bicubic_resize_swapped(x, H, W)
    else:
        up = None
    if slip == "concat_reversed":
        out, dout = gain.view(N, -1, 1, 1) * torch.cat([low, bicubic_resize(x, H, W)], 1), None
    elif up is not None:
        out, dout = gain.view(N, -1, 1, 1) * torch.cat([up, low], 1), None
    else:
        out, dout = cat_scale_ref(x, low, gain, H, W, dgain, dt_extra)
    return dict(px=px, dpx=dpx, head=hx, dhead=dhx, gain=gain, dgain=dgain, out=out, dout=dout)


def logit_head_ref(x, wb_fg, wb_bg, slip=None, dwb_fg=None, dwb_bg=None):
    """aoc_logit_head.  x [N, C, hw], wb_* [N, C + 1] -> (pred [N, hw], tol).  Each head is object_logit_kernel's sum: C products, C
    sequential additions and the bias, gamma(C + 1) (sum |w x| + |b|).  The min over the objects n >= 1 of values each known to tol_bg[n] is
    known to max_n tol_bg[n]; object 0 takes one more addition.
    slip: 'min_all' (the min includes object 0), 'add_all' (the augmentation added to every object), 'max' (max for min).
    dwb_*: what the rows [w | b] themselves are off by (a float32 nn.Linear in front): sum dw |x| + db, and |w| + dw in the rounding term."""
    N, C, hw = x.shape

    def head(wb, dwb):
        wa, ba = wb[:, :C].abs(), wb[:, C].abs()
        tol = 0.0
        if dwb is not None:
            tol = torch.einsum("nc,ncp->np", dwb[:, :C], x.abs()) + dwb[:, C].view(N, 1)
            wa, ba = wa + dwb[:, :C], ba + dwb[:, C]
        return (torch.einsum("nc,ncp->np", wb[:, :C], x) + wb[:, C].view(N, 1),
                tol + gamma(C + 1) * (torch.einsum("nc,ncp->np", wa, x.abs()) + ba.view(N, 1)))
    fg, dfg = head(wb_fg, dwb_fg)
    if N == 1:
        return fg, dfg
    bg, dbg = head(wb_bg, dwb_bg)
    first = 0 if slip == "min_all" else 1
    m = bg[first:].max(0)[0] if slip == "max" else bg[first:].min(0)[0]
    dm = dbg[1:].max(0)[0]
    pred, tol = fg.clone(), dfg.clone()
    if slip == "add_all":
        return pred + m.view(1, hw), tol
    pred[0] = fg[0] + m
    tol[0] = dfg[0] + dm
    tol[0] = tol[0] + U * (pred[0].abs() + tol[0])
    return pred, tol


def torch_coordinate_error(n_in):
    """What PyTorch's own source coordinate is off by per axis: it rounds the scale (in - 1) / (out - 1) and the product o * scale, each
    relative U of a coordinate below in - 1, and the subtraction of the floor is exact: dt <= 2 U (in - 1) + U."""
    return 2 * U * (n_in - 1) + U


# ------------------------------------------------------------------------------------------ inputs and slip choices shared by the host and GPU tests
f32 = np.float32
RESIZE_SLIPS = {"align_corners_false": dict(align_corners=False), "a_minus_half": dict(a=-0.5), "zero_pad": dict(zero_pad=True), "swapped": "swapped"}


def resize_slip(kind, x, H, W):
    return bicubic_resize_swapped(x, H, W) if kind == "swapped" else bicubic_resize(x, H, W, **RESIZE_SLIPS[kind])


LOGIT_SLIPS = ["min_all", "add_all", "max"]


def resize_inputs(rng, N, Ce, Cr, h, w, H, W):
    x = rng.standard_normal((N, Ce, h, w)).astype(f32)
    low = np.maximum(rng.standard_normal((N, Cr, H, W)), 0).astype(f32) if Cr else None           # the shortcut branch comes out of a ReLU
    gain = (1 + np.tanh(rng.standard_normal((N, Ce + Cr)))).astype(f32)
    return x, low, gain


def live_resize_slips(x, H, W, want):
    """The resize slips that change the result at this geometry (at the identity size, for one source pixel and for a single output
    pixel some of them coincide with the reference); decided between float64 references only."""
    out = {}
    for kind in RESIZE_SLIPS:
        s = resize_slip(kind, x, H, W)
        if float((s - want).abs().max()) > 1e-3 * float(want.abs().max()):
            out[kind] = s
    return out


def logit_inputs_random(rng, N, C, hw):
    x = rng.standard_normal((N, C, hw)).astype(f32)
    wb_fg = (rng.standard_normal((N, C + 1)) / np.sqrt(C)).astype(f32)
    wb_bg = (rng.standard_normal((N, C + 1)) / np.sqrt(C)).astype(f32)
    return x, wb_fg, wb_bg


