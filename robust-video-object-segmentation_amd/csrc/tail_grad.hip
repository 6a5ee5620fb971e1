// Training-time decoder tail: the backward of the shortcut stage of decoder_final (decoding_module.py:163, 170-176), the apply pass of a
// "delta gate" (:126-130, :181-185: an IA_gate whose head carries the inter-object code of its own input's plane means), the prediction
// head with the index of the background minimum (:144-160, 213-225) and their gradients.  Eight entry points (include/aoc_hip.h);
// aoc_amd.tail_train wires them into autograd.  The bicubic weights are bicubic.h's, the forward's own; the head with its argmin is a
// kernel of its own whose pred keeps aoc_logit_head's bits.
//
// No float atomics.  Every sum runs in an order fixed by the shapes and by the 16-byte alignment of the planes:
//   bicubic adjoint  gather form.  u[I, j] = sum over the output columns J in ascending order, the taps k = 0..3 of each in turn, of
//                    wx[J][k] g[I, J] where clamp(ix(J) + k - 1) == j; then t[i, j] = the same over the output rows I with wy and u.  Every
//                    product is rounded, then added (-ffp-contract=off), from 0.0f; clamped taps that meet on a border pixel are all added.
//   <x, t>           a workgroup owns a band of coarse rows of one plane: thread t of 256 adds the band's elements t, t + 256, ... (row-major),
//                    the xor butterfly of aoc_wave_sum, the four wave sums in ascending order; then the bands in ascending order from 0.0f.
//   plane sums       aoc_channel_scale_grad's order: thread t of T adds its front scalar, its float4 t, t + T, ... (.x .y .z .w in turn), its
//                    back scalar, each product rounded first; the butterfly; the wave sums in ascending order.  T = 256 for planes of at most
//                    2 048 float4, else 1 024.  The shortcut planes' dots ARE aoc_channel_scale_grad (called per object).
// A streamed plane that is written is cut (plane_stream.h) by the alignment of the written plane; the head's gradient cuts every plane by x's alignment
// (by grad_pred's for the bias column), whatever is written, so each output has the same bits alone as with the others.
#include "bicubic.h"
#include "plane_stream.h"

namespace {

constexpr size_t TG_LDS_MAX = 64 * 1024;         // dynamic LDS a launch may ask for without an attribute

// a compare-and-select; decoder_tail.hip clamps with min(max()), which compiles to other instructions in these kernels, so each file keeps its own
__host__ __device__ __forceinline__ int tg_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the first output index whose second tap floor(o (in - 1) / (out - 1)) is >= s (out when there is none)
__host__ __device__ __forceinline__ int tg_first_out(int s, int in, int out) {
    if (s <= 0) return 0;
    if (in <= 1 || out <= 1) return out;
    const int64_t o = ((int64_t)s * (out - 1) + in - 2) / (in - 1);
    return o < out ? (int)o : out;
}

// acc += the taps of output o (weights wt, second tap i0) that land on source index s, k = 0..3 in turn
__device__ __forceinline__ float tg_gather(float acc, const f32x4 wt, int i0, int s, int hi, float v) {
    if (tg_clampi(i0 - 1, hi) == s) acc += wt.x * v;
    if (tg_clampi(i0, hi) == s) acc += wt.y * v;
    if (tg_clampi(i0 + 1, hi) == s) acc += wt.z * v;
    if (tg_clampi(i0 + 2, hi) == s) acc += wt.w * v;
    return acc;
}

// ------------------------------------------------------------------------------------------ 1: t = U^T grad_out, <x, t>
// grid (N * Ce planes, bands): a workgroup owns R coarse rows [r0, r1) of one plane and walks the fine rows whose taps can reach them
// (first_out(r0 - 2) .. first_out(r1 + 1)) in chunks of RB rows:
//   a. the chunk of grad_out -> LDS, one contiguous run (lane = consecutive float);
//   b. the horizontal adjoint u[rr][j] of the chunk -> LDS (thread = one (row, coarse column), its columns J in ascending order);
//   c. the vertical adjoint into the band's accumulators in LDS (thread = one coarse pixel, the chunk's rows in ascending order).
// Neighbouring bands read the same fine rows at their seam (at most four coarse rows' worth); the upsample itself is never formed.
struct DotsLds { size_t tw, ti, cj, ri, g, u, acc, wsum, total; };
__host__ __device__ inline DotsLds dots_lds(int w, int H, int W, int R, int RB) {
    DotsLds L;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t r = off; off += (bytes + 15) / 16 * 16; return r; };
    L.tw = take((size_t)(H + W) * 16);            // tap weights: rows, then columns
    L.ti = take((size_t)(H + W) * 4);             // second-tap indices
    L.cj = take((size_t)2 * w * 4);               // per coarse column: first and one-past-last output column that can reach it
    L.ri = take((size_t)2 * R * 4);               // per coarse row of the band: the same for output rows
    L.g = take((size_t)RB * W * 4);
    L.u = take((size_t)RB * w * 4);
    L.acc = take((size_t)R * w * 4);
    L.wsum = take(16);
    L.total = off;
    return L;
}

__global__ __launch_bounds__(256) void bicubic_adjoint_kernel(const float *__restrict__ gout, const float *__restrict__ x, int Ce, int Ctot, int h, int w, int H,
                                                              int W, int R, int RB, float *__restrict__ t_out, float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tg_lds[];
    const DotsLds L = dots_lds(w, H, W, R, RB);
    f32x4 *tw = reinterpret_cast<f32x4 *>(tg_lds + L.tw);
    int *ti = reinterpret_cast<int *>(tg_lds + L.ti);
    int *cj = reinterpret_cast<int *>(tg_lds + L.cj);
    int *ri = reinterpret_cast<int *>(tg_lds + L.ri);
    float *gb = reinterpret_cast<float *>(tg_lds + L.g);
    float *ub = reinterpret_cast<float *>(tg_lds + L.u);
    float *acc = reinterpret_cast<float *>(tg_lds + L.acc);
    float *wsum = reinterpret_cast<float *>(tg_lds + L.wsum);
    const int64_t plane = blockIdx.x;
    const int64_t n = plane / Ce;
    const int c = (int)(plane - n * Ce);
    const int r0 = blockIdx.y * R, r1 = min(r0 + R, h), nr = r1 - r0;
    const int tid = threadIdx.x;
    const float *gp = gout + ((size_t)n * Ctot + c) * H * W;
    for (int i = tid; i < H + W; i += 256) {
        int i0;
        tw[i] = i < H ? bicubic_taps(i, h, H, i0) : bicubic_taps(i - H, w, W, i0);
        ti[i] = i0;
    }
    for (int i = tid; i < w + nr; i += 256) {
        if (i < w) {
            cj[2 * i] = tg_first_out(i - 2, w, W);
            cj[2 * i + 1] = tg_first_out(i + 2, w, W);
        } else {
            const int s = r0 + i - w;
            ri[2 * (i - w)] = tg_first_out(s - 2, h, H);
            ri[2 * (i - w) + 1] = tg_first_out(s + 2, h, H);
        }
    }
    for (int f = tid; f < nr * w; f += 256) acc[f] = 0.0f;
    const int I_lo = tg_first_out(r0 - 2, h, H), I_end = tg_first_out(r1 + 1, h, H);
    __syncthreads();
    for (int I0 = I_lo; I0 < I_end; I0 += RB) {
        const int nb = min(RB, I_end - I0);
        const float *gc = gp + (size_t)I0 * W;
        for (int f = tid; f < nb * W; f += 256) gb[f] = gc[f];
        __syncthreads();
        for (int f = tid; f < nb * w; f += 256) {
            const int rr = f / w, j = f - rr * w;
            const float *grow = gb + rr * W;
            const int J1 = cj[2 * j + 1];
            float a = 0.0f;
            for (int J = cj[2 * j]; J < J1; ++J) a = tg_gather(a, tw[H + J], ti[H + J], j, w - 1, grow[J]);
            ub[f] = a;
        }
        __syncthreads();
        for (int f = tid; f < nr * w; f += 256) {
            const int rr = f / w, j = f - rr * w;
            const int Ia = max(ri[2 * rr], I0), Ib = min(ri[2 * rr + 1], I0 + nb);
            float a = acc[f];
            for (int I = Ia; I < Ib; ++I) a = tg_gather(a, tw[I], ti[I], r0 + rr, h - 1, ub[(I - I0) * w + j]);
            acc[f] = a;
        }
        __syncthreads();
    }
    float *tp = t_out + (size_t)plane * h * w + (size_t)r0 * w;
    const float *xp = x ? x + (size_t)plane * h * w + (size_t)r0 * w : nullptr;
    float dot = 0.0f;
    for (int f = tid; f < nr * w; f += 256) {
        const float v = acc[f];
        tp[f] = v;
        if (xp) dot += xp[f] * v;
    }
    if (partial) {
        dot = aoc_wave_sum(dot);
        if (aoc_lane() == 0) wsum[tid >> 6] = dot;
        __syncthreads();
        if (tid == 0) partial[plane * gridDim.y + blockIdx.y] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// dgain[n, c < Ce] = the bands' partial dots in ascending order from 0.0f
__global__ __launch_bounds__(256) void band_sum_kernel(const float *__restrict__ partial, int64_t planes, int bands, int Ce, int Ctot, float *__restrict__ dgain) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= planes) return;
    float s = 0.0f;
    for (int b = 0; b < bands; ++b) s += partial[p * bands + b];
    const int64_t n = p / Ce;
    dgain[n * Ctot + (p - n * Ce)] = s;
}

struct DotsPlan { int R, RB, bands; size_t lds; };
// bands so that about 1 024 workgroups exist where the map has the rows for it, not fewer than 4 coarse rows each (the seam rows are read twice);
// the band and the chunk are halved until the workgroup's LDS fits.  First choices, not tuned.  R == 0: not even one row fits.
DotsPlan dots_plan(int64_t planes, int h, int w, int H, int W) {
    DotsPlan p;
    const int64_t want = (1024 + planes - 1) / planes;
    int R = (int)((h + want - 1) / want);
    if (R < 4) R = 4;
    if (R > h) R = h;
    int RB = 8;
    if (RB > H) RB = H;
    while (R > 1 && (size_t)R * w * 4 > 24 * 1024) R = (R + 1) / 2;
    while (RB > 1 && dots_lds(w, H, W, R, RB).total > TG_LDS_MAX) RB = (RB + 1) / 2;
    while (R > 1 && dots_lds(w, H, W, R, RB).total > TG_LDS_MAX) R = (R + 1) / 2;
    p.lds = dots_lds(w, H, W, R, RB).total;
    p.R = p.lds <= TG_LDS_MAX ? R : 0;
    p.RB = RB;
    p.bands = p.R ? (h + p.R - 1) / p.R : 0;
    return p;
}

bool tg_sizes_ok(int h, int w, int H, int W) {
    return h >= 1 && w >= 1 && H >= 1 && W >= 1 && (int64_t)h * w < (1ll << 31) && (int64_t)H * W < (1ll << 31);
}

struct StageGradWs { size_t t, partial, total; };
StageGradWs stage_grad_ws(int N, int Ce, int h, int w, int bands) {
    StageGradWs s;
    s.t = 0;
    s.partial = aoc_align_up((size_t)N * Ce * h * w * sizeof(float), 256);
    s.total = s.partial + aoc_align_up((size_t)N * Ce * (size_t)(bands > 0 ? bands : 1) * sizeof(float), 256);
    return s;
}

// ------------------------------------------------------------------------------------------ 2: the apply passes
// grad_x[n, c] = gain t + (cy[i] cx[j]) (dpx / (float)(H W)) in place over t: one workgroup per coarse plane; cy, cx are formed exactly as
// bicubic_plane_mean_kernel forms them (output order), so the pull-back uses the forward's own coefficients
size_t coef_lds(int h, int w, int H, int W) { return (size_t)(H + W) * 20 + (size_t)(h + w) * sizeof(float); }

__global__ __launch_bounds__(256) void bicubic_apply_kernel(const float *__restrict__ gain, const float *__restrict__ dpx, int Ce, int Ctot, int h, int w, int H,
                                                            int W, float *__restrict__ grad_x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tg_lds[];
    f32x4 *tw = reinterpret_cast<f32x4 *>(tg_lds);          // [H + W]: rows, then columns
    int *ti = reinterpret_cast<int *>(tw + H + W);          // [H + W]
    float *cs = reinterpret_cast<float *>(ti + H + W);      // [h + w]: cy, then cx
    const int64_t plane = blockIdx.x;
    const int64_t n = plane / Ce;
    const int64_t k = n * Ctot + (plane - n * Ce);
    const float g = gain ? gain[k] : 1.0f;
    float *tp = grad_x + (size_t)plane * h * w;
    const int total = h * w;
    if (!dpx) {
        for (int f = threadIdx.x; f < total; f += 256) tp[f] = g * tp[f];
        return;
    }
    const float s = dpx[k] / (float)((int64_t)H * W);
    for (int i = threadIdx.x; i < H + W; i += 256) {
        int i0;
        tw[i] = i < H ? bicubic_taps(i, h, H, i0) : bicubic_taps(i - H, w, W, i0);
        ti[i] = i0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < h + w; i += 256) {
        const bool rows = i < h;
        const int src = rows ? i : i - h, in = rows ? h : w, on = rows ? H : W, base = rows ? 0 : H;
        const int o1 = tg_first_out(src + 2, in, on);
        float a = 0.0f;
        for (int o = tg_first_out(src - 2, in, on); o < o1; ++o) {
            const f32x4 wt = tw[base + o];
            const int i0 = ti[base + o];
            if (tg_clampi(i0 - 1, in - 1) == src) a += wt.x;
            if (tg_clampi(i0, in - 1) == src) a += wt.y;
            if (tg_clampi(i0 + 1, in - 1) == src) a += wt.z;
            if (tg_clampi(i0 + 2, in - 1) == src) a += wt.w;
        }
        cs[i] = a;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < total; f += 256) {
        const int r = f / w, j = f - r * w;
        tp[f] = g * tp[f] + (cs[r] * cs[h + j]) * s;
    }
}

// out[n, c] = gain[k] src[n, c0 + c] + dpx[k] / (float)hw, k = n * src_ctot + c0 + c.  grid (N * C planes, slices); the plane is cut by
// the alignment of the plane it writes, the source is read 16 bytes per lane at 4-byte alignment
__global__ __launch_bounds__(256) void scale_shift_kernel(const float *__restrict__ src, const float *__restrict__ gain, const float *__restrict__ dpx, int C,
                                                          int src_ctot, int c0, int64_t hw, float *__restrict__ out) {
    const int64_t plane = blockIdx.x;
    const int64_t n = plane / C;
    const int64_t k = n * src_ctot + c0 + (plane - n * C);
    const float g = gain ? gain[k] : 1.0f;
    const float s = dpx ? dpx[k] / (float)hw : 0.0f;
    const float *sp = src + k * hw;
    float *op = out + plane * hw;
    const int64_t front = aoc_front(op, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nthreads = (int64_t)gridDim.y * 256;
    if (tid < front) op[tid] = g * sp[tid] + s;
    for (int64_t i = tid; i < body4; i += nthreads) {
        const int64_t e = front + 4 * i;
        const f32x4 v = aoc_load4(sp + e);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = g * v[q] + s;
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(op + e));
    }
    if (tid < hw - back0) op[back0 + tid] = g * sp[back0 + tid] + s;
}

// ------------------------------------------------------------------------------------------ 3: the prediction head with its argmin
// decoder_tail.hip's logit_head_kernel with an index beside every minimum; the channel sums keep that kernel's order (sequential over c,
// bias last), so pred has aoc_logit_head's bits (tested).  The strict `<` keeps the lowest object of a tie within a wave (it walks its objects upwards); across the waves
// the lower index wins an equal value.  0 = no object (N == 1 writes nothing; every bg logit NaN or +inf selects none).
constexpr int LH_MAXW = 4;
__global__ __launch_bounds__(64 * LH_MAXW) void logit_head_argmin_kernel(const float *__restrict__ x, const float *__restrict__ wb_fg,
                                                                         const float *__restrict__ wb_bg, int64_t stride, int N, int C, int64_t hw,
                                                                         float *__restrict__ pred, int32_t *__restrict__ arg) {
    __shared__ float lmin[LH_MAXW][64];
    __shared__ int lidx[LH_MAXW][64];
    __shared__ float lfg0[64];
    const int lane = threadIdx.x, q = __builtin_amdgcn_readfirstlane(threadIdx.y), nw = blockDim.y;      // a wave has one q
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;
    const bool live = p < hw;
    const int64_t pc = live ? p : hw - 1;                 // clamped: dead lanes load a valid address and store nothing
    float mn = INFINITY;
    int mi = 0;
    for (int n = q; n < N; n += nw) {
        const float *xp = x + (size_t)n * C * hw + pc;
        const float *wf = wb_fg + (size_t)n * stride, *wg = wb_bg + (size_t)n * stride;
        const bool bg = n > 0;
        float sf = 0.0f, sb = 0.0f;
        int c = 0;
        for (; c + 16 <= C; c += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = xp[(size_t)(c + u) * hw];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                sf += wf[c + u] * v[u];
                if (bg) sb += wg[c + u] * v[u];
            }
        }
        for (; c + 8 <= C; c += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = xp[(size_t)(c + u) * hw];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                sf += wf[c + u] * v[u];
                if (bg) sb += wg[c + u] * v[u];
            }
        }
        for (; c < C; ++c) {
            const float xv = xp[(size_t)c * hw];
            sf += wf[c] * xv;
            if (bg) sb += wg[c] * xv;
        }
        sf += wf[C];
        if (bg) {
            sb += wg[C];
            if (sb < mn) { mn = sb; mi = n; }
            if (live) pred[(size_t)n * hw + p] = sf;
        } else {
            lfg0[lane] = sf;
        }
    }
    lmin[q][lane] = mn;
    lidx[q][lane] = mi;
    __syncthreads();
    if (q == 0 && live) {
        float s = lfg0[lane];
        if (N > 1) {
            float m = lmin[0][lane];
            int a = lidx[0][lane];
            for (int k = 1; k < nw; ++k) {
                const float v = lmin[k][lane];
                const int b = lidx[k][lane];
                if (v < m || (v == m && b != 0 && (a == 0 || b < a))) { m = v; a = b; }
            }
            s += m;
            arg[p] = a;
        }
        pred[p] = s;
    }
}

// One workgroup per column (n, c) of the heads' rows, c == C the bias: reads grad_pred[n], grad_pred[0], arg and the plane x[n, c] once, writes
// the plane grad_x[n, c] once, leaves the two plane sums.  Pixels another object won add +0.0f to the bg sum.
template <int T>
__global__ __launch_bounds__(T) void logit_head_grad_kernel(const float *__restrict__ g, const int32_t *__restrict__ arg, const float *__restrict__ x,
                                                            const float *__restrict__ wb_fg, const float *__restrict__ wb_bg, int64_t stride, int N, int C,
                                                            int64_t hw, float *__restrict__ grad_x, float *__restrict__ gfg, float *__restrict__ gbg) {
    __shared__ float wsum[2][T / 64];
    const int64_t col = blockIdx.x;
    const int n = (int)(col / (C + 1)), c = (int)(col - (int64_t)n * (C + 1));
    const int t = threadIdx.x;
    const bool bias = c == C, sel = n > 0 && N > 1, sums = gfg || gbg;
    if (bias && !sums) return;
    const float *gn = g + (size_t)n * hw;
    const float *xp = bias ? nullptr : x + ((size_t)n * C + c) * hw;
    float *op = (grad_x && !bias) ? grad_x + ((size_t)n * C + c) * hw : nullptr;
    const float wf = op ? wb_fg[(size_t)n * stride + c] : 0.0f, wg = (op && sel) ? wb_bg[(size_t)n * stride + c] : 0.0f;
    const int64_t front = aoc_front(bias ? (const void *)gn : (const void *)xp, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    const bool op16 = op && ((reinterpret_cast<uintptr_t>(op + front) & 15) == 0);
    float af = 0.0f, ab = 0.0f;
    auto one = [&](int64_t p) {
        const float a = gn[p];
        const bool hit = sel && arg[p] == n;
        const float b = hit ? g[p] : 0.0f;
        if (sums) {
            const float xv = bias ? 1.0f : xp[p];
            af += a * xv;
            ab += hit ? b * xv : 0.0f;
        }
        if (op) op[p] = hit ? a * wf + b * wg : a * wf;
    };
    if (t < front) one(t);
    for (int64_t i = t; i < body4; i += T) {
        const int64_t e = front + 4 * i;
        const f32x4 a4 = aoc_load4(gn + e);
        f32x4 b4 = {0.0f, 0.0f, 0.0f, 0.0f}, x4 = {1.0f, 1.0f, 1.0f, 1.0f}, o4;
        bool hit[4] = {false, false, false, false};
        if (sel) {
            const i32x4 r4 = aoc_load4i(arg + e);
            const f32x4 g04 = aoc_load4(g + e);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                hit[q] = r4[q] == n;
                b4[q] = hit[q] ? g04[q] : 0.0f;
            }
        }
        if (!bias && sums) x4 = aoc_load4(xp + e);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (sums) { af += a4[q] * x4[q]; ab += hit[q] ? b4[q] * x4[q] : 0.0f; }
            o4[q] = hit[q] ? a4[q] * wf + b4[q] * wg : a4[q] * wf;
        }
        if (op) aoc_store4(op + e, o4, op16);
    }
    if (t < hw - back0) one(back0 + t);
    if (!sums) return;
    af = aoc_wave_sum(af);
    ab = aoc_wave_sum(ab);
    if (aoc_lane() == 0) { wsum[0][t >> 6] = af; wsum[1][t >> 6] = ab; }
    __syncthreads();
    if (t == 0) {
        float sf = 0.0f, sb = 0.0f;
        for (int k = 0; k < T / 64; ++k) { sf += wsum[0][k]; sb += wsum[1][k]; }
        if (gfg) gfg[col] = sf;
        if (gbg) gbg[col] = sel ? sb : 0.0f;
    }
}

// augment_background_logit with the index of the minimum (ascending n, strict `<`: the lowest object of a tie; 0 = none)
__global__ __launch_bounds__(256) void background_merge_argmin_kernel(const float *__restrict__ fg, const float *__restrict__ bg, int N, int64_t hw,
                                                                      float *__restrict__ pred, int32_t *__restrict__ arg) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    float m = INFINITY;
    int a = 0;
    for (int n = 1; n < N; ++n) {
        const float b = bg[(size_t)n * hw + p];
        if (b < m) { m = b; a = n; }
        pred[(size_t)n * hw + p] = fg[(size_t)n * hw + p];
    }
    pred[p] = N > 1 ? fg[p] + m : fg[p];
    if (N > 1) arg[p] = a;
}

__global__ __launch_bounds__(256) void background_merge_grad_kernel(const float *__restrict__ g, const int32_t *__restrict__ arg, int N, int64_t hw,
                                                                    float *__restrict__ grad_fg, float *__restrict__ grad_bg) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const float g0 = g[p];
    const int a = N > 1 ? arg[p] : 0;
    if (grad_fg) grad_fg[p] = g0;
    if (grad_bg) grad_bg[p] = 0.0f;
    for (int n = 1; n < N; ++n) {
        if (grad_fg) grad_fg[(size_t)n * hw + p] = g[(size_t)n * hw + p];
        if (grad_bg) grad_bg[(size_t)n * hw + p] = n == a ? g0 : 0.0f;
    }
}

int stage_grad_check(int N, int Ce, int Cr, int h, int w, int H, int W) {
    if (N < 1 || Ce < 1 || Cr < 0 || !tg_sizes_ok(h, w, H, W)) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (int64_t)N * Ce > 0x7fffffffLL || (int64_t)N * ((int64_t)Ce + Cr) > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    return AOC_OK;
}

}  // namespace

extern "C" {

size_t aoc_shortcut_stage_grad_workspace_bytes(int N, int Ce, int h, int w, int H, int W) {
    if (stage_grad_check(N, Ce, 0, h, w, H, W) != AOC_OK) return 0;
    const DotsPlan p = dots_plan((int64_t)N * Ce, h, w, H, W);
    if (p.R == 0) return 0;
    return stage_grad_ws(N, Ce, h, w, p.bands).total;
}

int aoc_shortcut_stage_grad_dots(const float *grad_out, const float *x, const float *low, int N, int Ce, int Cr, int h, int w, int H, int W, float *t_out,
                                 float *dgain, void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_out) return AOC_ERR_INVALID_ARG;
    int rc = stage_grad_check(N, Ce, Cr, h, w, H, W);
    if (rc != AOC_OK) return rc;
    if (dgain && (!x || (Cr > 0 && !low))) return AOC_ERR_INVALID_ARG;
    const DotsPlan p = dots_plan((int64_t)N * Ce, h, w, H, W);
    if (p.R == 0 || p.bands > 65535) return AOC_ERR_UNSUPPORTED;
    if (!t_out && !dgain) return AOC_OK;
    const StageGradWs s = stage_grad_ws(N, Ce, h, w, p.bands);
    if ((!t_out || dgain) && (!workspace || workspace_bytes < s.total)) return AOC_ERR_WORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *t = t_out ? t_out : reinterpret_cast<float *>(ws + s.t);
    float *partial = dgain ? reinterpret_cast<float *>(ws + s.partial) : nullptr;
    hipStream_t st = aoc_hip_stream(stream);
    const int Ctot = Ce + Cr;
    const int64_t planes = (int64_t)N * Ce;
    // the shortcut planes' dots first: aoc_channel_scale_grad validates its own arguments (all of them checked above already), and a
    // rejection there must come back before anything of this call has been enqueued
    const int64_t HW = (int64_t)H * W;
    for (int n = 0; dgain && n < N && Cr > 0; ++n)
        if ((rc = aoc_channel_scale_grad(grad_out + ((size_t)n * Ctot + Ce) * HW, low + (size_t)n * Cr * HW, nullptr, Cr, HW, nullptr,
                                         dgain + (size_t)n * Ctot + Ce, stream)) != AOC_OK)
            return rc;
    hipLaunchKernelGGL(bicubic_adjoint_kernel, dim3((unsigned)planes, (unsigned)p.bands), dim3(256), p.lds, st, grad_out, dgain ? x : (const float *)nullptr, Ce,
                       Ctot, h, w, H, W, p.R, p.RB, t, partial);
    AOC_RETURN_IF_LAUNCH_FAILED();
    if (dgain) {
        hipLaunchKernelGGL(band_sum_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, st, partial, planes, p.bands, Ce, Ctot, dgain);
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    return AOC_OK;
}

int aoc_shortcut_stage_grad_apply(const float *grad_out, const float *gain, const float *dpx, int N, int Ce, int Cr, int h, int w, int H, int W, float *grad_x,
                                  float *grad_low, aoc_stream_t stream) {
    const int rc = stage_grad_check(N, Ce, Cr, h, w, H, W);
    if (rc != AOC_OK) return rc;
    if (grad_low && (!grad_out || Cr < 1)) return AOC_ERR_INVALID_ARG;
    if (grad_x && dpx && coef_lds(h, w, H, W) > TG_LDS_MAX) return AOC_ERR_UNSUPPORTED;
    hipStream_t st = aoc_hip_stream(stream);
    const int Ctot = Ce + Cr;
    if (grad_x && (gain || dpx)) {
        hipLaunchKernelGGL(bicubic_apply_kernel, dim3((unsigned)((int64_t)N * Ce)), dim3(256), dpx ? coef_lds(h, w, H, W) : 0, st, gain, dpx, Ce, Ctot, h, w, H, W,
                           grad_x);
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    if (grad_low) {
        const int64_t HW = (int64_t)H * W;
        hipLaunchKernelGGL(scale_shift_kernel, dim3((unsigned)((int64_t)N * Cr), aoc_plane_slices(HW)), dim3(256), 0, st, grad_out, gain, dpx, Cr, Ctot, Ce, HW,
                           grad_low);
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    return AOC_OK;
}

int aoc_delta_gate_grad_apply(const float *grad_y, const float *gain, const float *dpx, int N, int C, int64_t hw, float *grad_x, aoc_stream_t stream) {
    if (!grad_y || !gain || !grad_x || N < 1 || C < 1 || hw < 1) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (int64_t)N * C > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(scale_shift_kernel, dim3((unsigned)((int64_t)N * C), aoc_plane_slices(hw)), dim3(256), 0, aoc_hip_stream(stream), grad_y, gain, dpx, C, C, 0, hw,
                       grad_x);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_logit_head_argmin(const float *x, const float *wb_fg, const float *wb_bg, int64_t stride, int N, int C, int64_t hw, float *pred, int32_t *arg,
                          aoc_stream_t stream) {
    if (!x || !wb_fg || !pred || N < 1 || C < 1 || hw < 1 || stride < C + 1 || (N > 1 && (!wb_bg || !arg))) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (hw + 63) / 64 > 0x7fffffff) return AOC_ERR_UNSUPPORTED;
    const int nw = N < LH_MAXW ? N : LH_MAXW;
    hipLaunchKernelGGL(logit_head_argmin_kernel, dim3((unsigned)((hw + 63) / 64)), dim3(64, nw), 0, aoc_hip_stream(stream), x, wb_fg, wb_bg ? wb_bg : wb_fg,
                       stride, N, C, hw, pred, arg);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_logit_head_grad(const float *grad_pred, const int32_t *arg, const float *x, const float *wb_fg, const float *wb_bg, int64_t stride, int N, int C,
                        int64_t hw, float *grad_x, float *grad_wb_fg, float *grad_wb_bg, aoc_stream_t stream) {
    if (!grad_pred || !x || N < 1 || C < 1 || hw < 1 || stride < C + 1 || (N > 1 && !arg)) return AOC_ERR_INVALID_ARG;
    if (grad_x && (!wb_fg || (N > 1 && !wb_bg))) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (int64_t)N * ((int64_t)C + 1) > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    if (!grad_x && !grad_wb_fg && !grad_wb_bg) return AOC_OK;
    const unsigned cols = (unsigned)((int64_t)N * (C + 1));
    hipStream_t st = aoc_hip_stream(stream);
    if (hw / 4 <= 2048)
        hipLaunchKernelGGL(logit_head_grad_kernel<256>, dim3(cols), dim3(256), 0, st, grad_pred, arg, x, wb_fg, wb_bg, stride, N, C, hw, grad_x, grad_wb_fg,
                           grad_wb_bg);
    else
        hipLaunchKernelGGL(logit_head_grad_kernel<1024>, dim3(cols), dim3(1024), 0, st, grad_pred, arg, x, wb_fg, wb_bg, stride, N, C, hw, grad_x, grad_wb_fg,
                           grad_wb_bg);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_background_merge_argmin(const float *fg, const float *bg, int N, int64_t hw, float *pred, int32_t *arg, aoc_stream_t stream) {
    if (!fg || !pred || N < 1 || hw < 1 || (N > 1 && (!bg || !arg))) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (hw + 255) / 256 > 0x7fffffff) return AOC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(background_merge_argmin_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, aoc_hip_stream(stream), fg, bg, N, hw, pred, arg);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_background_merge_grad(const float *grad_pred, const int32_t *arg, int N, int64_t hw, float *grad_fg, float *grad_bg, aoc_stream_t stream) {
    if (!grad_pred || N < 1 || hw < 1 || (N > 1 && !arg)) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (hw + 255) / 256 > 0x7fffffff) return AOC_ERR_UNSUPPORTED;
    if (!grad_fg && !grad_bg) return AOC_OK;
    hipLaunchKernelGGL(background_merge_grad_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, aoc_hip_stream(stream), grad_pred, arg, N, hw, grad_fg,
                       grad_bg);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
