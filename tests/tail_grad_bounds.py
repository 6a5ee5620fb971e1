"""References and bounds for the training-time decoder tail (csrc/tail_grad.hip, aoc_amd.tail_train), shared by tests/test_tail_grad_host.py
and tests/test_gpu_tail_grad.py.

Every *_ref is a pure function of the tensors an entry point receives, widened to float64; it returns the float64 results and, for each, an
elementwise bound on |kernel - reference|: a running error analysis of the kernel's own float32 expressions (``gates_grad_bounds.E``;
-ffp-contract=off, one rounding per operation, U = 2^-24), with the geometry of tests/decoder_tail_bounds.py (``bicubic_matrix`` gives the 1-D
interpolation matrix M, |M|, the bound E on the kernel's weight errors and the number of taps CNT per entry; the adjoint kernel uses the
forward's weights bit for bit, so E is the adjoint's weight error too).  No constant is fitted to output.  The summation depths:

    adjoint          u[I, j]: the cnt_x[j] taps that land on column j, one product rounding each and at most cnt_x[j] additions: gamma(cnt_x[j] + 1);
                     t[i, j] likewise over the rows with cnt_y[i]
    <x, t>           one product rounding, then at most ceil(h w / 256) additions in the thread, 6 butterfly levels, 3 wave sums and one addition
                     per band (at most h bands): gamma(ceil(h w / 256) + 10 + h)
    plane sums       gates_grad_bounds.dot_depth(hw) (aoc_channel_scale_grad's order)
    delta pull-back  N - 1 sequential additions and the subtraction (torch, float32)

Every reference has slipped twins (its ``slip`` argument) which the tests demand to leave the bound.  Called with float64 tensors that are NOT
float32-representable (the host tests do, to compare with float64 autograd) the values are plain float64 mathematics; the bounds then mean
nothing and are ignored."""
import numpy as np
import torch

import decoder_tail_bounds as dtb
import gates_grad_bounds as ggb
from float64_bounds import _cdiv, gamma
from gates_grad_bounds import E, check, dot_depth, rng, t64  # noqa: F401

f32, f64 = np.float32, np.float64
ADJOINT_SLIPS = {"no_clamped_duplicates": dict(zero_pad=True), "align_corners_false": dict(align_corners=False), "a_minus_half": dict(a=-0.5)}


def _gam(cnt):
    return torch.tensor([gamma(int(k) + 1) for k in cnt], dtype=torch.float64)


# ------------------------------------------------------------------------------------------ 1 the shortcut stage
def upsample64(x, H, W, **slip):
    return dtb.bicubic_resize(t64(x), H, W, **slip)


def adjoint_ref(g, h, w, **slip):
    """g [..., H, W] -> (t [..., h, w] = My^T g Mx, tol).  slip: keyword arguments of bicubic_matrix for the VALUE only."""
    g = t64(g)
    H, W = g.shape[-2:]
    My, AMy, Ey, Cy = dtb.bicubic_matrix(h, H)
    Mx, AMx, Ex, Cx = dtb.bicubic_matrix(w, W)
    gx, gy = _gam(Cx.sum(0)), _gam(Cy.sum(0))
    u = torch.einsum("...ij,jw->...iw", g, Mx)
    eu = torch.einsum("...ij,jw->...iw", g.abs(), Ex) + gx * torch.einsum("...ij,jw->...iw", g.abs(), AMx + Ex)
    t = torch.einsum("ih,...iw->...hw", My, u)
    et = (torch.einsum("ih,...iw->...hw", Ey, u.abs()) + torch.einsum("ih,...iw->...hw", AMy + Ey, eu)
          + gy.view(h, 1) * torch.einsum("ih,...iw->...hw", AMy + Ey, u.abs() + eu))
    if slip:
        t = torch.einsum("ih,...ij,jw->...hw", dtb.bicubic_matrix(h, H, **slip)[0], g, dtb.bicubic_matrix(w, W, **slip)[0])
    return t, et


def stage_dots_ref(grad_out, x, low, slip=None):
    """aoc_shortcut_stage_grad_dots.  grad_out [N, Ce + Cr, H, W], x [N, Ce, h, w], low [N, Cr, H, W] or None -> ((t, tol), (dgain, tol))."""
    go, xx = t64(grad_out), t64(x)
    N, Ce, h, w = xx.shape
    H, W = go.shape[2:]
    t, et = adjoint_ref(go[:, :Ce], h, w, **(ADJOINT_SLIPS[slip] if slip else {}))
    prod = E(xx) * E(t, et)
    dg = prod.sum((2, 3), _cdiv(h * w, 256) + 10 + h)
    dgv, dge = dg.v, dg.e
    if low is not None and go.shape[1] > Ce:
        Cr = go.shape[1] - Ce
        (_, _), (lv, le) = ggb.channel_scale_grad_ref(go[:, Ce:].reshape(N * Cr, H * W), t64(low).reshape(N * Cr, H * W), torch.ones(N * Cr))
        dgv, dge = torch.cat([dgv, lv.view(N, Cr)], 1), torch.cat([dge, le.view(N, Cr)], 1)
    return (t, et), (dgv, dge)


def delta_pullback_ref(dd, slip=None):
    """dpx[n] = sum_m dd[m] - dd[n] (ascending m) -> (want, tol).  slip 'no_sum': - dd[n] alone."""
    d = E(t64(dd))
    N = d.v.shape[0]
    tot = d.sum(0, max(N - 1, 1), keepdim=True)
    if slip == "no_sum":
        tot = E(torch.zeros_like(tot.v))
    r = E(tot.v.expand_as(d.v), tot.e.expand_as(d.v)) - d
    return r.v, r.e


def _shift(dpx, hw):
    """dpx / (float)hw as E"""
    hwf = float(f32(hw))
    return E(t64(dpx)) / E(torch.full_like(t64(dpx), hwf), torch.full_like(t64(dpx), abs(hwf - hw)))


def _coef(n_in, n_out, **slip):
    c, ec = dtb.column_sums(n_in, n_out, **slip)
    return E(c, ec)


def stage_apply_ref(grad_out, t, gain, dpx, Ce, slip=None):
    """aoc_shortcut_stage_grad_apply.  grad_out [N, Ce + Cr, H, W], t [N, Ce, h, w] (the tensor pass A left), gain, dpx [N, Ce + Cr] or None ->
    ((grad_x, tol), (grad_low, tol) or None).  slip: 'no_feedback' (the plane-mean term dropped), 'coarse_hw' (the shift divided by h w)."""
    go, tt = t64(grad_out), t64(t)
    N, Ct, H, W = go.shape
    h, w = tt.shape[2:]
    g = E(t64(gain).view(N, Ct, 1, 1)) if gain is not None else None
    gx = E(tt) * E(g.v[:, :Ce]) if g is not None else E(tt)
    gl = None
    if Ct > Ce:
        gl = E(go[:, Ce:]) * E(g.v[:, Ce:]) if g is not None else E(go[:, Ce:])
    if dpx is not None and slip != "no_feedback":
        s = _shift(t64(dpx).view(N, Ct, 1, 1), h * w if slip == "coarse_hw" else H * W)
        cy, cx = _coef(h, H), _coef(w, W)
        cc = E(cy.v.view(h, 1), cy.e.view(h, 1)) * E(cx.v.view(1, w), cx.e.view(1, w))
        fb = E(cc.v.view(1, 1, h, w), cc.e.view(1, 1, h, w)) * E(s.v[:, :Ce], s.e[:, :Ce])
        gx = gx + fb
        if gl is not None:
            gl = gl + E(s.v[:, Ce:].expand_as(gl.v), s.e[:, Ce:].expand_as(gl.v))
    return (gx.v, gx.e), ((gl.v, gl.e) if gl is not None else None)


def delta_apply_ref(grad_y, gain, dpx, slip=None):
    """aoc_delta_gate_grad_apply.  grad_y [N, C, hw], gain, dpx [N, C] -> (grad_x, tol).  slip 'no_feedback'."""
    gy = t64(grad_y)
    N, C, hw = gy.shape
    r = E(gy) * E(t64(gain).view(N, C, 1))
    if dpx is not None and slip != "no_feedback":
        s = _shift(t64(dpx).view(N, C, 1), hw)
        r = r + E(s.v.expand_as(gy), s.e.expand_as(gy))
    return r.v, r.e


def shortcut_stage_backward64(x, low, head, weight, bias, grad_out, slip=None):
    """The whole backward of the shortcut stage in float64 from the formulas above (values only) -> dict(grad_x, grad_low, grad_head,
    grad_weight, grad_bias).  slip: an ADJOINT_SLIPS key, 'no_feedback', 'no_sum', 'coarse_hw'."""
    x, low, head, weight, bias, grad_out = (t64(a) for a in (x, low, head, weight, bias, grad_out))
    N, Ce = x.shape[:2]
    D = head.shape[1]
    H, W = grad_out.shape[2:]
    px = torch.cat([upsample64(x, H, W).mean((2, 3)), low.mean((2, 3))], 1)
    hx = torch.cat([head, px.sum(0, keepdim=True) - px], 1)
    gain = 1.0 + torch.tanh(hx @ weight.t() + bias)
    (t, _), (dgain, _) = stage_dots_ref(grad_out, x, low, slip if slip in ADJOINT_SLIPS else None)
    (gh, _), (gw, _), (gb, _) = ggb.film_gain_grad_ref(dgain, gain, hx, weight)
    dpx, _ = delta_pullback_ref(gh[:, D:], slip if slip == "no_sum" else None)
    (gx, _), (gl, _) = stage_apply_ref(grad_out, t, gain, dpx, Ce, slip if slip in ("no_feedback", "coarse_hw") else None)
    return dict(grad_x=gx, grad_low=gl, grad_head=gh[:, :D], grad_weight=gw, grad_bias=gb, gain=gain, px=px)


def delta_gate_backward64(x, head, weight, bias, grad_y, slip=None):
    """IA(x, cat([head, delta(mean(x))])) backwards in float64 (values only)."""
    x, head, weight, bias, grad_y = (t64(a) for a in (x, head, weight, bias, grad_y))
    N, C = x.shape[:2]
    D = head.shape[1]
    x3, g3 = x.reshape(N, C, -1), grad_y.reshape(N, C, -1)
    px = x3.mean(2)
    hx = torch.cat([head, px.sum(0, keepdim=True) - px], 1)
    gain = 1.0 + torch.tanh(hx @ weight.t() + bias)
    dgain = (g3 * x3).sum(2)
    (gh, _), (gw, _), (gb, _) = ggb.film_gain_grad_ref(dgain, gain, hx, weight)
    dpx, _ = delta_pullback_ref(gh[:, D:], slip if slip == "no_sum" else None)
    gx, _ = delta_apply_ref(g3, gain, dpx, slip if slip == "no_feedback" else None)
    return dict(grad_x=gx.reshape(x.shape), grad_head=gh[:, :D], grad_weight=gw, grad_bias=gb)


# ------------------------------------------------------------------------------------------ 2 the logit head
RULES = ("lowest", "highest", "all")


def bg_logits64(x, wb_bg):
    x, wb = t64(x), t64(wb_bg)
    C = x.shape[1]
    return torch.einsum("nc,ncp->np", wb[:, :C], x) + wb[:, C].view(-1, 1)


def select(bg, rule="lowest"):
    """bg [N, hw] float64 -> sel [N, hw] (0 / 1): who receives the gradient of pred[0].  'lowest' / 'highest' index among the objects n >= 1 that
    attain the minimum, 'all' of them; 'bg_to_all_objects' every n >= 1; 'bg0_in_min' the lowest index with object 0 taking part.  NaN never
    attains it; no finite or -inf value: nobody."""
    N, hw = bg.shape
    sel = torch.zeros(N, hw, dtype=torch.float64)
    if N == 1:
        return sel
    first = 0 if rule == "bg0_in_min" else 1
    if rule == "bg_to_all_objects":
        sel[1:] = 1.0
        return sel
    b = torch.where(torch.isnan(bg[first:]), torch.full_like(bg[first:], float("inf")), bg[first:])
    m = b.min(0)[0]
    tie = (b == m.view(1, hw)) & (m.view(1, hw) < float("inf"))
    if rule == "all":
        sel[first:] = tie.double()
        return sel
    idx = torch.arange(N - first).view(-1, 1).expand(N - first, hw)
    if rule == "highest":
        pick = torch.where(tie, idx, torch.full_like(idx, -1)).max(0)[0]
    else:
        pick = torch.where(tie, idx, torch.full_like(idx, N)).min(0)[0]
    ok = tie.any(0)
    sel[first:][pick.clamp(0, N - first - 1)[ok], torch.arange(hw)[ok]] = 1.0
    return sel


def arg_of(sel):
    """the kernel's arg [hw] for a one-hot selection: the selected object, 0 for nobody"""
    return (sel * torch.arange(sel.shape[0], dtype=torch.float64).view(-1, 1)).sum(0).to(torch.int32)


def logit_head_grad_ref(g, sel, x, wb_fg, wb_bg):
    """aoc_logit_head_grad with the selection as a 0 / 1 matrix [N, hw].  g [N, hw], x [N, C, hw], wb_* [N, C + 1] ->
    ((grad_x, tol), (grad_wb_fg, tol), (grad_wb_bg, tol))."""
    g, x, wf = t64(g), t64(x), t64(wb_fg)
    N, C, hw = x.shape
    wb = t64(wb_bg) if wb_bg is not None else torch.zeros_like(wf)
    b = E(sel * g[0:1])                                          # g[0] where selected, 0.0 elsewhere: exact
    gx = E(g.view(N, 1, hw)) * E(wf[:, :C].reshape(N, C, 1))
    extra = E(b.v.view(N, 1, hw)) * E(wb[:, :C].reshape(N, C, 1))
    hit = sel.view(N, 1, hw).expand(N, C, hw) > 0
    both = gx + extra
    gx = E(torch.where(hit, both.v, gx.v), torch.where(hit, both.e, gx.e))
    x1 = torch.cat([x, torch.ones(N, 1, hw, dtype=torch.float64)], 1)
    depth = dot_depth(hw)
    gf = (E(g.view(N, 1, hw)) * E(x1)).sum(2, depth)
    gb = (E(b.v.view(N, 1, hw)) * E(x1)).sum(2, depth)
    return (gx.v, gx.e), (gf.v, gf.e), (gb.v, gb.e)


def head_linear_grad_ref(g, head, weight):
    """the three float32 products of tail_train._HeadLinear in any summation order: gamma(terms) on the sum of magnitudes"""
    g, head, weight = t64(g), t64(head), t64(weight)
    N, K = g.shape
    return ((g @ weight, gamma(K) * (g.abs() @ weight.abs())), (g.t() @ head, gamma(N) * (g.abs().t() @ head.abs())), (g.sum(0), gamma(N) * g.abs().sum(0)))


def background_merge_ref(fg, bg, rule="lowest"):
    """fg, bg [N, hw] float64 -> (pred [N, hw], sel [N, hw])"""
    fg, bg = t64(fg), t64(bg)
    sel = select(bg, rule)
    pred = fg.clone()
    if fg.shape[0] > 1:
        first = 0 if rule == "bg0_in_min" else 1
        pred[0] = fg[0] + bg[first:].min(0)[0]
    return pred, sel


def background_merge_grad_ref(g, sel):
    g = t64(g)
    return g.clone(), sel * g[0:1]


def logit_head_backward64(x, head, fg_w, fg_b, bg_w, bg_b, grad_pred, rule="lowest"):
    """predict() backwards in float64 (values only): both linear layers, the head and the merge."""
    x, head, fg_w, fg_b, bg_w, bg_b, g = (t64(a) for a in (x, head, fg_w, fg_b, bg_w, bg_b, grad_pred))
    N, C = x.shape[:2]
    x3, g2 = x.reshape(N, C, -1), g.reshape(N, -1)
    wf, wb = head @ fg_w.t() + fg_b, head @ bg_w.t() + bg_b
    sel = select(bg_logits64(x3, wb), rule)
    (gx, _), (gf, _), (gb, _) = logit_head_grad_ref(g2, sel, x3, wf, wb)
    out = dict(grad_x=gx.reshape(x.shape), sel=sel)
    (hf, _), (out["grad_fg_weight"], _), (out["grad_fg_bias"], _) = head_linear_grad_ref(gf, head, fg_w)
    (hb, _), (out["grad_bg_weight"], _), (out["grad_bg_bias"], _) = head_linear_grad_ref(gb, head, bg_w)
    out["grad_head"] = hf + hb
    return out


def undecided_pixels(x, wb_fg, wb_bg):
    """pixels whose float64 gap between the smallest and the second-smallest bg logit (objects n >= 1) is not above twice the forward bound"""
    x, wb_fg, wb_bg = t64(x), t64(wb_fg), t64(wb_bg)
    N, C, hw = x.shape
    if N < 3:
        return torch.zeros(hw, dtype=torch.bool)
    bg = bg_logits64(x, wb_bg)[1:]
    tol = gamma(C + 1) * (torch.einsum("nc,ncp->np", wb_bg[1:, :C].abs(), x[1:].abs()) + wb_bg[1:, C].abs().view(-1, 1))
    two = torch.topk(bg, 2, dim=0, largest=False)[0]
    return (two[1] - two[0]) <= 2 * tol.max(0)[0]


# ------------------------------------------------------------------------------------------ cases shared by the host and GPU tests
STAGE_GEOMETRIES = ((2, 3, 2, 5, 7, 9, 14), (1, 1, 0, 1, 1, 4, 6), (2, 2, 1, 3, 4, 1, 1), (1, 2, 1, 7, 9, 7, 9), (2, 2, 2, 2, 2, 33, 65), (3, 5, 3, 9, 6, 4, 5),
                    (1, 2, 1, 4, 9, 3, 255), (1, 2, 1, 4, 9, 3, 256), (1, 2, 1, 4, 9, 3, 257), (30, 4, 3, 3, 4, 6, 7))
MAP_GEOMETRY = (3, 8, 4, 61, 107, 121, 213)
DELTA_CASES = tuple((N, hw) for hw in (1, 35, 1023, 1024, 1025) for N in (1, 3, 30))
HEAD_CASES = ((1, 128, 300), (2, 8, 1), (4, 128, 257), (3, 13, 1025), (30, 16, 513))
HEAD_SEEDS = {(1, 128, 300): 0, (2, 8, 1): 0, (4, 128, 257): 0, (3, 13, 1025): 0, (30, 16, 513): 0}      # test_tail_grad_host asserts: no undecided pixel
MERGE_HW = (1, 255, 257)
FIXTURES = ("tail_grad_O3", "tail_grad_O1", "tail_grad_O4_odd")


def stage_case(N, Ce, Cr, h, w, H, W, D=5):
    rs = rng(N, Ce, Cr, h, w, H, W)
    x, low, _ = dtb.resize_inputs(rs, N, Ce, Cr, h, w, H, W)
    Ct = Ce + Cr
    return dict(x=x, low=low, head=rs.standard_normal((N, D)).astype(f32), weight=(rs.standard_normal((Ct, D + Ct)) / np.sqrt(D + Ct)).astype(f32),
                bias=(0.1 * rs.standard_normal(Ct)).astype(f32), grad_out=rs.standard_normal((N, Ct, H, W)).astype(f32),
                gain=(1 + np.tanh(rs.standard_normal((N, Ct)))).astype(f32), dpx=rs.standard_normal((N, Ct)).astype(f32))


def head_case(N, C, hw, seed=None):
    rs = rng(N, C, hw, HEAD_SEEDS.get((N, C, hw), 0) if seed is None else seed)
    x, wb_fg, wb_bg = dtb.logit_inputs_random(rs, N, C, hw)
    return dict(x=x, wb_fg=wb_fg, wb_bg=wb_bg, g=rs.standard_normal((N, hw)).astype(f32))


def planted_ties():
    """small integers, exact in float32: x [4, 2, 6], rows so that bg[n, p] = x[n, 0, p] (weights (1, 0), bias 0).  Pixels: 0 a two-way tie of
    objects 1 and 2; 1 a three-way tie; 2 a tie of objects 2 and N - 1 = 3; 3 a tie of 1 and 3; 4 no tie (object 2); 5 object 0 below everyone."""
    N, C, hw = 4, 2, 6
    x = np.zeros((N, C, hw), f32)
    x[:, 0] = np.array([[9, 9, 9, 9, 9, -5], [1, 2, 7, 0, 5, 3], [1, 2, 3, 4, 2, 6], [4, 2, 3, 0, 8, 7]], f32)
    x[:, 1] = np.arange(N * hw, dtype=f32).reshape(N, hw) % 5 - 2
    wb_bg = np.tile(np.array([[1, 0, 0]], f32), (N, 1))
    wb_fg = np.array([[1, -1, 2], [2, 1, 0], [-1, 3, 1], [0, 2, -2]], f32)
    g = np.array([[1, -2, 3, 4, -1, 2], [2, 1, -1, 3, 1, -2], [1, 1, 2, -3, 2, 1], [-1, 2, 1, 1, -2, 3]], f32)
    return dict(x=x, wb_fg=wb_fg, wb_bg=wb_bg, g=g)


# ------------------------------------------------------------------------------------------ the recorded decoder (fixtures tail_grad_*.npz)
FIXTURE_DIMS = dict(Ce=64, Cr=8, D=12, Cl=16)
SMALL = ("GCT_sc", "bn_sc", "IA10", "bn1", "IA11", "bn2", "IA_final_fg", "IA_final_bg")          # the modules whose parameters a fixture stores


def _h16(a):
    return np.asarray(a, f32).astype(np.float16).astype(f64)


def build_decoder(dec, gct_cls, gate_cls, seed, Ce=64, Cr=8, D=12, Cl=16):
    """decoding_module.py:74-89 at small widths on `dec` (any module: the reference's ``__new__`` holder, a mirror's or a twin's carrier), the
    convolutions from numpy's seed (He-scaled) and every small parameter drawn away from its constructor value, all rounded to float16."""
    from torch import nn
    dec.GCT_sc = gct_cls(Cl)
    dec.conv_sc = nn.Conv2d(Cl, Cr, 1, bias=False)
    dec.bn_sc = nn.GroupNorm(int(Cr / 4), Cr)
    dec.relu = nn.ReLU(inplace=True)
    dec.IA10 = gate_cls(D + Ce + Cr, Ce + Cr)
    dec.conv1 = nn.Conv2d(Ce + Cr, int(Ce / 2), kernel_size=3, padding=1, bias=False)
    dec.bn1 = nn.GroupNorm(32, int(Ce / 2))
    dec.IA11 = gate_cls(D + int(Ce / 2), int(Ce / 2))
    dec.conv2 = nn.Conv2d(int(Ce / 2), int(Ce / 2), kernel_size=3, padding=1, bias=False)
    dec.bn2 = nn.GroupNorm(32, int(Ce / 2))
    dec.IA_final_fg = nn.Linear(D, int(Ce / 2) + 1)
    dec.IA_final_bg = nn.Linear(D, int(Ce / 2) + 1)
    rs = np.random.RandomState([int(seed), 78])
    with torch.no_grad():
        for name, m in dec.named_modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.weight.shape[0] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.from_numpy(_h16(rs.standard_normal(tuple(m.weight.shape)) * np.sqrt(2.0 / fan_out))).to(m.weight.dtype))
        for name, p in small_parameters(dec):
            leaf = name.split(".")[-1]
            if name.startswith("bn") and leaf == "weight" or leaf == "alpha":
                a = rs.uniform(0.5, 1.5, tuple(p.shape))
            elif name.startswith("bn") or leaf in ("gamma", "beta"):
                a = 0.5 * rs.standard_normal(tuple(p.shape))
            else:
                a = p.detach().numpy() * (3.0 if leaf == "weight" else 1.0)           # the linear layers as constructed, the gates a little wider
            p.copy_(torch.from_numpy(_h16(a)).to(p.dtype).reshape(p.shape))
    return dec


def small_parameters(dec):
    return [(f"{m}.{k}", p) for m in SMALL for k, p in getattr(dec, m).named_parameters()]


def load_small(dec, fx):
    with torch.no_grad():
        for name, p in small_parameters(dec):
            p.copy_(torch.from_numpy(fx["w_" + name.replace(".", "__")].astype(f32)).to(p.dtype).reshape(p.shape))
