// Training-time ASPP (networks/layers/aspp.py:7-78): the backward of the forward's multi-set kernels.  Four entry points and two
// workspace-size functions (include/aoc_hip.h); aoc_amd.aspp_train wires them into autograd.
//
//   front   v_k = x * gate_k(sum x^2) for the branches' GCTs and mean = sum x / hw for the pooled branch (aspp.py:19 four times, :46):
//           aoc_plane_dot_multi (x read once for every set's plane dot), aoc_gct_gate_multi_grad (one workgroup per set) and
//           aoc_channel_scale_multi_grad_apply (one pass writes grad_x from every set's gradient, the summed dsum and the mean's cotangent).
//   back    out = GCT_640(cat), cat = [relu(GN(u_k) gamma_k + beta_k) ..., relu(tail) broadcast] (aspp.py:21-23 four times, :61-65):
//           aoc_groupnorm_cat_relu_grad = a plane pass (five sums per source plane, one per tail plane), two small launches and an apply pass.
//           z, its ReLU mask and cat are recomputed with gn_cat_apply_kernel's own float expression (x a + b, a = rstd gamma, b = beta -
//           mean a); neither the ungated concatenation nor its gradient is ever stored.
//
// A streamed plane is cut (plane_stream.h) by the alignment of the plane the pass WRITES, or of the gradient plane it reads where nothing is
// written.
//
// No float atomics.  Every sum runs in an order fixed by the shapes and by that alignment cut:
//   plane sums     aoc_channel_scale_grad's order: thread t of T adds its front scalar, its float4 t, t + T, ... (components .x .y .z .w in
//                  turn), its back scalar, each product rounded before it is added (-ffp-contract=off); then the xor butterfly of
//                  aoc_wave_sum; then the wave sums in ascending wave order.  T = 256 for planes of at most 2 048 float4, else 1 024.
//   small kernels  one thread per output, a serial loop in ascending index of the summed dimension, from 0.0f; the GCT sums over c are
//                  gct_gate_grad_body's (gct_gate_grad.h).
// The thread counts, the loads in flight and the slices per plane are first choices, not tuned ones.
#include <stdlib.h>

#include "gct_gate_grad.h"

namespace {

// ------------------------------------------------------------------------------------------ front 1: dots[k, p] = <g_k[p], x[p]>
// One workgroup per plane.  Set k's plane is cut by g_k's own alignment (channel_scale_grad_kernel<T, false, true> cuts by grad_y), so set k
// carries the bits of aoc_channel_scale_grad(g_k, x).  Where every set shares one cut (tensors of one allocator and one shape do) each
// float4 of x is loaded once and feeds every set's accumulator; otherwise the sets are walked one after the other and x comes from the cache.
template <int T>
__device__ __forceinline__ float ag_plane_dot_one(const float *__restrict__ gp, const float *__restrict__ xp, int64_t hw, int t) {
    const int64_t front = aoc_front(gp, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    float acc = 0.0f;
    if (t < front) acc += gp[t] * xp[t];
    for (int64_t i = t; i < body4; i += T) acc = aoc_dot4(acc, aoc_load4(gp + front + 4 * i), aoc_load4(xp + front + 4 * i));
    if (t < hw - back0) acc += gp[back0 + t] * xp[back0 + t];
    return acc;
}

template <int T>
__global__ __launch_bounds__(T) void plane_dot_multi_kernel(const float *__restrict__ x, AocSrcList g, int n_set, int64_t planes, int64_t hw,
                                                             float *__restrict__ dots) {
    __shared__ float wsum[AOC_PTR_LIST][T / 64];
    const int64_t plane = blockIdx.x;
    const int t = threadIdx.x;
    const float *xp = x + plane * hw;
    float acc[AOC_PTR_LIST];
#pragma unroll
    for (int k = 0; k < AOC_PTR_LIST; ++k) acc[k] = 0.0f;
    const int64_t front = aoc_front(g.p[0] + plane * hw, hw);
    bool same = true;
#pragma unroll
    for (int k = 1; k < AOC_PTR_LIST; ++k)
        if (k < n_set) same = same && aoc_front(g.p[k] + plane * hw, hw) == front;
    if (same) {
        const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
        if (t < front) {
            const float xv = xp[t];
#pragma unroll
            for (int k = 0; k < AOC_PTR_LIST; ++k)
                if (k < n_set) acc[k] += g.p[k][plane * hw + t] * xv;
        }
        for (int64_t i = t; i < body4; i += T) {                       // 1 + n_set 16-byte loads in flight per thread
            const int64_t e = plane * hw + front + 4 * i;
            const f32x4 xv = aoc_load4(x + e);
#pragma unroll
            for (int k = 0; k < AOC_PTR_LIST; ++k)
                if (k < n_set) acc[k] = aoc_dot4(acc[k], aoc_load4(g.p[k] + e), xv);
        }
        if (t < hw - back0) {
            const float xv = xp[back0 + t];
#pragma unroll
            for (int k = 0; k < AOC_PTR_LIST; ++k)
                if (k < n_set) acc[k] += g.p[k][plane * hw + back0 + t] * xv;
        }
    } else {
#pragma unroll
        for (int k = 0; k < AOC_PTR_LIST; ++k)
            if (k < n_set) acc[k] = ag_plane_dot_one<T>(g.p[k] + plane * hw, xp, hw, t);
    }
#pragma unroll
    for (int k = 0; k < AOC_PTR_LIST; ++k) {
        if (k < n_set) {
            const float v = aoc_wave_sum(acc[k]);
            if (aoc_lane() == 0) wsum[k][t >> 6] = v;
        }
    }
    __syncthreads();
    if (t < n_set) {
        float s = 0.0f;
        for (int w = 0; w < T / 64; ++w) s += wsum[t][w];
        dots[(int64_t)t * planes + plane] = s;
    }
}

// ------------------------------------------------------------------------------------------ front 2: through gct_gate_kernel's expressions
// grid (n_set); workgroup k is aoc_gct_gate_grad (gct_gate_grad_body) on row k of the parameters and on dgate[k], gate[k]; all sets read one plane_sums
__global__ __launch_bounds__(256) void gct_gate_multi_grad_kernel(const float *__restrict__ dgate, const float *__restrict__ gate, const float *__restrict__ s,
                                                                  const float *__restrict__ alpha, const float *__restrict__ gamma, int N, int C, float eps,
                                                                  int l1, float *__restrict__ dsum, float *__restrict__ grad_alpha,
                                                                  float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    __shared__ float wsum[4];
    const size_t k = blockIdx.x, nc = (size_t)N * C;
    gct_gate_grad_body(dgate + k * nc, gate + k * nc, s, alpha + k * C, gamma + k * C, N, C, eps, l1, dsum ? dsum + k * nc : nullptr,
                          grad_alpha ? grad_alpha + k * C : nullptr, grad_gamma ? grad_gamma + k * C : nullptr, grad_beta ? grad_beta + k * C : nullptr,
                          wsum);
}

// dsum_total[i] = sum_k dsum[k, i], ascending k from 0.0f
__global__ __launch_bounds__(256) void set_sum_kernel(const float *__restrict__ dsum, int n_set, int64_t n, float *__restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int k = 0; k < n_set; ++k) s += dsum[(int64_t)k * n + i];
    total[i] = s;
}

// ------------------------------------------------------------------------------------------ front 3: the apply pass
// grad_x[p, i] = ((sum_k g_k[p, i] gate_k[p]) + (2 dsum_total[p]) x[p, i]) + dmean[p] / (float)hw: the sum over k starts from the product of
// set 0 and adds the sets in ascending order; dmean == NULL drops the last addition.  grid (planes, slices), the plane cut by grad_x.
__device__ __forceinline__ float ag_front_apply1(const float (&gv)[AOC_PTR_LIST], const float (&gt)[AOC_PTR_LIST], int n_set, float xv, float ds2, float c,
                                                 bool has_c) {
    float s = gv[0] * gt[0];
#pragma unroll
    for (int k = 1; k < AOC_PTR_LIST; ++k)
        if (k < n_set) s += gv[k] * gt[k];
    s = s + ds2 * xv;
    return has_c ? s + c : s;
}

__global__ __launch_bounds__(256) void channel_scale_multi_grad_apply_kernel(AocSrcList g, const float *__restrict__ gates, const float *__restrict__ x,
                                                                             const float *__restrict__ dsum_total, const float *__restrict__ dmean,
                                                                             int n_set, int64_t planes, int64_t hw, float *__restrict__ grad_x) {
    const int64_t plane = blockIdx.x;                        // planes on x (up to 2^31 - 1), the slices of a plane on y
    const int64_t base = plane * hw;
    float gt[AOC_PTR_LIST];
#pragma unroll
    for (int k = 0; k < AOC_PTR_LIST; ++k) gt[k] = k < n_set ? gates[(int64_t)k * planes + plane] : 0.0f;
    const float ds2 = 2.0f * dsum_total[plane];
    const bool has_c = dmean != nullptr;
    const float c = has_c ? dmean[plane] / (float)hw : 0.0f;
    float *op = grad_x + base;
    const int64_t front = aoc_front(op, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nthreads = (int64_t)gridDim.y * 256;
    if (tid < front || tid < hw - back0) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int64_t e = side ? back0 + tid : tid;
            if (side ? tid < hw - back0 : tid < front) {
                float gv[AOC_PTR_LIST];
#pragma unroll
                for (int k = 0; k < AOC_PTR_LIST; ++k) gv[k] = k < n_set ? g.p[k][base + e] : 0.0f;
                op[e] = ag_front_apply1(gv, gt, n_set, x[base + e], ds2, c, has_c);
            }
        }
    }
    for (int64_t i = tid; i < body4; i += nthreads) {
        const int64_t e = base + front + 4 * i;
        f32x4 g4[AOC_PTR_LIST];
#pragma unroll
        for (int k = 0; k < AOC_PTR_LIST; ++k)
            if (k < n_set) g4[k] = aoc_load4(g.p[k] + e);
        const f32x4 x4 = aoc_load4(x + e);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gv[AOC_PTR_LIST];
#pragma unroll
            for (int k = 0; k < AOC_PTR_LIST; ++k) gv[k] = k < n_set ? g4[k][j] : 0.0f;
            o[j] = ag_front_apply1(gv, gt, n_set, x4[j], ds2, c, has_c);
        }
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(grad_x + e));
    }
}

// ------------------------------------------------------------------------------------------ back: GroupNorm x n_src -> cat -> GCT
// what a source plane's elements need of the forward: z = x a + b (gn_cat_apply_kernel's expression), xhat = (x - mean) rstd
struct AgPlane { float mean, rstd, gam, a, b; };
__device__ __forceinline__ AgPlane ag_plane(const float *__restrict__ stats, const float *__restrict__ gamma, const float *__restrict__ beta, int k, int n,
                                            int c, int N, int C_src, int group_channels) {
    AgPlane P;
    const int64_t gi = ((int64_t)k * N + n) * (C_src / group_channels) + c / group_channels;
    const int cc = k * C_src + c;
    P.mean = stats[2 * gi];
    P.rstd = stats[2 * gi + 1];
    P.gam = gamma ? gamma[cc] : 1.0f;
    P.a = P.rstd * P.gam;
    P.b = (beta ? beta[cc] : 0.0f) - P.mean * P.a;
    return P;
}

struct AgAcc { float p1, p2, p3, p4, p5; };
__device__ __forceinline__ void ag_add1(const AgPlane &P, AgAcc &acc, float gy, float x) {
    const float z = x * P.a + P.b;
    const bool m = z > 0.0f;                                  // the mask of the forward's fmaxf(z, 0), torch's `> 0`
    const float cat = fmaxf(z, 0.0f);
    const float xhat = (x - P.mean) * P.rstd;
    acc.p1 += gy * cat;
    acc.p2 += m ? gy : 0.0f;
    acc.p3 += m ? gy * xhat : 0.0f;
    acc.p4 += cat;
    acc.p5 += cat * xhat;
}

// back 1: grid (N * C_total).  A source plane leaves P1 .. P5; a tail plane leaves sum g in P2's slot and P1 = relu(tail) * sum g.  The plane
// is cut by g's alignment (nothing is written).  P [5][N * C_total].
template <int T>
__global__ __launch_bounds__(T) void gn_cat_grad_plane_kernel(const float *__restrict__ g, AocSrcList u, int n_src, int N, int C_src, int group_channels,
                                                               int64_t hw, const float *__restrict__ stats, const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, const float *__restrict__ tail, int C_tail,
                                                               float *__restrict__ P) {
    __shared__ float wsum[5][T / 64];
    const int C_total = n_src * C_src + C_tail;
    const int64_t plane = blockIdx.x, planes = (int64_t)N * C_total;
    const int n = (int)(plane / C_total), cc = (int)(plane - (int64_t)n * C_total);
    const int t = threadIdx.x;
    const float *gp = g + plane * hw;
    const int64_t front = aoc_front(gp, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    const bool is_src = cc < n_src * C_src;
    AgAcc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (is_src) {
        const int k = cc / C_src, c = cc - k * C_src;
        const AgPlane Pl = ag_plane(stats, gamma, beta, k, n, c, N, C_src, group_channels);
        const float *xp = aoc_pick(u, k) + ((int64_t)n * C_src + c) * hw;
        if (t < front) ag_add1(Pl, acc, gp[t], xp[t]);
        int64_t i = t;
        for (; i + (int64_t)T < body4; i += 2 * (int64_t)T) {             // four 16-byte loads in flight per thread
            f32x4 g4[2], x4[2];
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                g4[v] = aoc_load4(gp + front + 4 * (i + v * (int64_t)T));
                x4[v] = aoc_load4(xp + front + 4 * (i + v * (int64_t)T));
            }
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int j = 0; j < 4; ++j) ag_add1(Pl, acc, g4[v][j], x4[v][j]);
        }
        for (; i < body4; i += T) {
            const f32x4 g4 = aoc_load4(gp + front + 4 * i), x4 = aoc_load4(xp + front + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) ag_add1(Pl, acc, g4[j], x4[j]);
        }
        if (t < hw - back0) ag_add1(Pl, acc, gp[back0 + t], xp[back0 + t]);
    } else {
        if (t < front) acc.p2 += gp[t];
        for (int64_t i = t; i < body4; i += T) {
            const f32x4 g4 = aoc_load4(gp + front + 4 * i);
            acc.p2 += g4[0]; acc.p2 += g4[1]; acc.p2 += g4[2]; acc.p2 += g4[3];
        }
        if (t < hw - back0) acc.p2 += gp[back0 + t];
    }
    acc.p1 = aoc_wave_sum(acc.p1);
    acc.p2 = aoc_wave_sum(acc.p2);
    acc.p3 = aoc_wave_sum(acc.p3);
    acc.p4 = aoc_wave_sum(acc.p4);
    acc.p5 = aoc_wave_sum(acc.p5);
    if (aoc_lane() == 0) {
        wsum[0][t >> 6] = acc.p1; wsum[1][t >> 6] = acc.p2; wsum[2][t >> 6] = acc.p3; wsum[3][t >> 6] = acc.p4; wsum[4][t >> 6] = acc.p5;
    }
    __syncthreads();
    if (t == 0) {
        float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int w = 0; w < T / 64; ++w)
#pragma unroll
            for (int q = 0; q < 5; ++q) s[q] += wsum[q][w];
        if (!is_src) s[0] = fmaxf(tail[(int64_t)n * C_tail + (cc - n_src * C_src)], 0.0f) * s[1];
#pragma unroll
        for (int q = 0; q < 5; ++q) P[q * planes + plane] = s[q];
    }
}

// back 2: one workgroup, aoc_gct_gate_grad's arithmetic with dgate = P1 on the concatenation's GCT (l2 mode)
__global__ __launch_bounds__(256) void gn_cat_grad_gate_kernel(const float *__restrict__ P1, const float *__restrict__ gate, const float *__restrict__ s,
                                                               const float *__restrict__ alpha, const float *__restrict__ gamma, int N, int C, float eps,
                                                               float *__restrict__ ds, float *__restrict__ grad_alpha, float *__restrict__ grad_gamma,
                                                               float *__restrict__ grad_beta) {
    __shared__ float wsum[4];
    gct_gate_grad_body(P1, gate, s, alpha, gamma, N, C, eps, 0, ds, grad_alpha, grad_gamma, grad_beta, wsum);
}

// A[n, cc] = G P2 + (2 ds) P4 and B[n, cc] = G P3 + (2 ds) P5: the same instructions wherever they are needed
__device__ __forceinline__ void ag_AB(const float *__restrict__ P, const float *__restrict__ G, const float *__restrict__ ds, int64_t planes, int64_t plane,
                                      float &A, float &B) {
    const float gg = G[plane], d2 = 2.0f * ds[plane];
    A = gg * P[1 * planes + plane] + d2 * P[3 * planes + plane];
    B = gg * P[2 * planes + plane] + d2 * P[4 * planes + plane];
}

// back 3: thread i < n_src N groups: coef[i] = (s1 / M, s2 / M) over the group's channels in ascending c; the next n_src C_src threads:
// grad_gamma[cc] = sum_n B, grad_beta[cc] = sum_n A in ascending n; the last N C_tail threads: grad_tail
__global__ __launch_bounds__(256) void gn_cat_grad_small_kernel(const float *__restrict__ P, const float *__restrict__ G, const float *__restrict__ ds,
                                                                const float *__restrict__ gamma, const float *__restrict__ tail, int n_src, int N, int C_src,
                                                                int C_tail, int group_channels, float Mf, float hwf, float *__restrict__ coef,
                                                                float *__restrict__ grad_gamma, float *__restrict__ grad_beta, float *__restrict__ grad_tail) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int groups = C_src / group_channels;
    const int C_total = n_src * C_src + C_tail;
    const int64_t planes = (int64_t)N * C_total;
    const int64_t n_coef = (int64_t)n_src * N * groups, n_aff = (int64_t)n_src * C_src;
    if (i < n_coef) {
        if (!coef) return;
        const int gq = (int)(i % groups);
        const int n = (int)((i / groups) % N), k = (int)(i / ((int64_t)groups * N));
        float s1 = 0.0f, s2 = 0.0f;
        for (int j = 0; j < group_channels; ++j) {
            const int cc = k * C_src + gq * group_channels + j;
            const float gm = gamma ? gamma[cc] : 1.0f;
            float A, B;
            ag_AB(P, G, ds, planes, (int64_t)n * C_total + cc, A, B);
            s1 += gm * A;
            s2 += gm * B;
        }
        coef[2 * i] = s1 / Mf;
        coef[2 * i + 1] = s2 / Mf;
        return;
    }
    if (i < n_coef + n_aff) {
        if (!grad_gamma && !grad_beta) return;
        const int cc = (int)(i - n_coef);
        float sa = 0.0f, sb = 0.0f;
        for (int n = 0; n < N; ++n) {
            float A, B;
            ag_AB(P, G, ds, planes, (int64_t)n * C_total + cc, A, B);
            sa += A;
            sb += B;
        }
        if (grad_gamma) grad_gamma[cc] = sb;
        if (grad_beta) grad_beta[cc] = sa;
        return;
    }
    const int64_t j = i - n_coef - n_aff;
    if (!grad_tail || j >= (int64_t)N * C_tail) return;
    const int n = (int)(j / C_tail), c = (int)(j % C_tail);
    const int64_t plane = (int64_t)n * C_total + n_src * C_src + c;
    const float tv = tail[j];
    grad_tail[j] = tv > 0.0f ? G[plane] * P[1 * planes + plane] + ((2.0f * ds[plane]) * hwf) * tv : 0.0f;
}

// back 4: grid (n_src N C_src, slices): dz = m (g G + (2 ds) cat), grad_u = rstd ((gamma dz - s1 / M) - xhat (s2 / M)); the plane is cut by
// grad_u's alignment; a source whose pointer is NULL is skipped
__device__ __forceinline__ float ag_back_apply1(const AgPlane &P, float gg, float d2, float c1, float c2, float gy, float x) {
    const float z = x * P.a + P.b;
    const float cat = fmaxf(z, 0.0f);
    const float dz = z > 0.0f ? gy * gg + d2 * cat : 0.0f;
    const float xhat = (x - P.mean) * P.rstd;
    return P.rstd * ((P.gam * dz - c1) - xhat * c2);
}

__global__ __launch_bounds__(256) void gn_cat_grad_apply_kernel(const float *__restrict__ g, AocSrcList u, int n_src, int N, int C_src, int C_tail,
                                                                int group_channels, int64_t hw, const float *__restrict__ stats,
                                                                const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ G,
                                                                const float *__restrict__ ds, const float *__restrict__ coef, AocDstList grad_u) {
    const int64_t sp = blockIdx.x;                           // (k, n, c)
    const int c = (int)(sp % C_src), n = (int)((sp / C_src) % N), k = (int)(sp / ((int64_t)C_src * N));
    float *ob = aoc_pick(grad_u, k);
    if (!ob) return;
    const int C_total = n_src * C_src + C_tail;
    const int64_t plane = (int64_t)n * C_total + (int64_t)k * C_src + c;
    const AgPlane Pl = ag_plane(stats, gamma, beta, k, n, c, N, C_src, group_channels);
    const int64_t gi = ((int64_t)k * N + n) * (C_src / group_channels) + c / group_channels;
    const float c1 = coef[2 * gi], c2 = coef[2 * gi + 1];
    const float gg = G[plane], d2 = 2.0f * ds[plane];
    const float *gp = g + plane * hw;
    const float *xp = aoc_pick(u, k) + ((int64_t)n * C_src + c) * hw;
    float *op = ob + ((int64_t)n * C_src + c) * hw;
    const int64_t front = aoc_front(op, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nthreads = (int64_t)gridDim.y * 256;
    if (tid < front) op[tid] = ag_back_apply1(Pl, gg, d2, c1, c2, gp[tid], xp[tid]);
    for (int64_t i = tid; i < body4; i += nthreads) {
        const int64_t e = front + 4 * i;
        const f32x4 g4 = aoc_load4(gp + e), x4 = aoc_load4(xp + e);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ag_back_apply1(Pl, gg, d2, c1, c2, g4[j], x4[j]);
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(op + e));
    }
    if (tid < hw - back0) op[back0 + tid] = ag_back_apply1(Pl, gg, d2, c1, c2, gp[back0 + tid], xp[back0 + tid]);
}

struct AgWs {
    float *P, *ds, *coef;
    size_t total;
};
inline AgWs ag_carve(void *base, int n_src, int N, int C_src, int C_tail, int groups) {
    AgWs w;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *r = p ? p + off : nullptr; off += aoc_align_up(bytes, 256); return reinterpret_cast<float *>(r); };
    const size_t planes = (size_t)N * ((size_t)n_src * C_src + C_tail);
    w.P = take(5 * planes * sizeof(float));
    w.ds = take(planes * sizeof(float));
    w.coef = take((size_t)n_src * N * groups * 2 * sizeof(float));
    w.total = off;
    return w;
}

// [a, a + na) and [b, b + nb) floats share an element (NULL shares nothing)
inline bool ag_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    if (!a || !b || na < 1 || nb < 1) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}
struct AgRange { const void *p; int64_t n; };
// every output is disjoint from every input and from every other output
inline bool ag_outputs_clash(const AgRange *in, int n_in, const AgRange *out, int n_out) {
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < n_in; ++j)
            if (ag_overlap(out[i].p, out[i].n, in[j].p, in[j].n)) return true;
        for (int j = 0; j < i; ++j)
            if (ag_overlap(out[i].p, out[i].n, out[j].p, out[j].n)) return true;
    }
    return false;
}

}  // namespace

extern "C" {

int aoc_plane_dot_multi(const float *x, const float *const *g_ptrs, int n_set, int64_t planes, int64_t hw, float *dots, aoc_stream_t stream) {
    if (!x || !g_ptrs || !dots || n_set < 1 || n_set > AOC_PTR_LIST || planes < 1 || hw < 1) return AOC_ERR_INVALID_ARG;
    if (planes > 0x7fffffffLL || hw > INT64_MAX / 4 / planes) return AOC_ERR_UNSUPPORTED;
    const int64_t n = planes * hw;
    AocSrcList g = {};
    for (int k = 0; k < n_set; ++k) {
        if (!g_ptrs[k]) return AOC_ERR_INVALID_ARG;
        if (ag_overlap(dots, (int64_t)n_set * planes, g_ptrs[k], n)) return AOC_ERR_INVALID_ARG;
        g.p[k] = g_ptrs[k];
    }
    if (ag_overlap(dots, (int64_t)n_set * planes, x, n)) return AOC_ERR_INVALID_ARG;
    hipStream_t st = aoc_hip_stream(stream);
    if (hw / 4 <= 2048) hipLaunchKernelGGL(plane_dot_multi_kernel<256>, dim3((unsigned)planes), dim3(256), 0, st, x, g, n_set, planes, hw, dots);
    else hipLaunchKernelGGL(plane_dot_multi_kernel<1024>, dim3((unsigned)planes), dim3(1024), 0, st, x, g, n_set, planes, hw, dots);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

size_t aoc_gct_gate_multi_grad_workspace_bytes(int n_set, int N, int C) {
    return n_set < 1 || N < 1 || C < 1 ? 0 : aoc_align_up((size_t)n_set * N * C * sizeof(float), 256);
}

int aoc_gct_gate_multi_grad(const float *dgate, const float *gate, const float *plane_sums, const float *alpha, const float *gamma, const float *beta,
                            int n_set, int N, int C, float eps, int l1_mode, float *dsum_total, float *dsum, float *grad_alpha, float *grad_gamma,
                            float *grad_beta, void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    (void)beta;                            // the saved gates carry beta's effect; kept in the signature beside aoc_gct_gate_multi's
    if (!dgate || !gate || !plane_sums || !alpha || !gamma || n_set < 1 || n_set > AOC_PTR_LIST || N < 1 || C < 1) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS) return AOC_ERR_UNSUPPORTED;
    if (!dsum_total && !dsum && !grad_alpha && !grad_gamma && !grad_beta) return AOC_OK;
    const int64_t nc = (int64_t)N * C, snc = (int64_t)n_set * nc, sc = (int64_t)n_set * C;
    float *per_set = dsum;
    if (dsum_total && !dsum) {
        if (!workspace || workspace_bytes < aoc_gct_gate_multi_grad_workspace_bytes(n_set, N, C)) return AOC_ERR_WORKSPACE;
        per_set = static_cast<float *>(workspace);
    }
    const AgRange in[] = {{dgate, snc}, {gate, snc}, {plane_sums, nc}, {alpha, sc}, {gamma, sc}};
    const AgRange out[] = {{dsum_total, nc}, {per_set, snc}, {grad_alpha, sc}, {grad_gamma, sc}, {grad_beta, sc}};
    if (ag_outputs_clash(in, 5, out, 5)) return AOC_ERR_INVALID_ARG;
    hipStream_t st = aoc_hip_stream(stream);
    hipLaunchKernelGGL(gct_gate_multi_grad_kernel, dim3((unsigned)n_set), dim3(256), 0, st, dgate, gate, plane_sums, alpha, gamma, N, C, eps, l1_mode, per_set,
                       grad_alpha, grad_gamma, grad_beta);
    if (dsum_total)
        hipLaunchKernelGGL(set_sum_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, (const float *)per_set, n_set, nc, dsum_total);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_channel_scale_multi_grad_apply(const float *const *g_ptrs, const float *gates, const float *x, const float *dsum_total, const float *dmean,
                                       int n_set, int64_t planes, int64_t hw, float *grad_x, aoc_stream_t stream) {
    if (!g_ptrs || !gates || !x || !dsum_total || !grad_x || n_set < 1 || n_set > AOC_PTR_LIST || planes < 1 || hw < 1) return AOC_ERR_INVALID_ARG;
    if (planes > 0x7fffffffLL || hw > INT64_MAX / 4 / planes) return AOC_ERR_UNSUPPORTED;
    const int64_t n = planes * hw;
    AocSrcList g = {};
    AgRange in[AOC_PTR_LIST + 4];
    int n_in = 0;
    for (int k = 0; k < n_set; ++k) {
        if (!g_ptrs[k]) return AOC_ERR_INVALID_ARG;
        g.p[k] = g_ptrs[k];
        in[n_in++] = {g_ptrs[k], n};
    }
    in[n_in++] = {gates, (int64_t)n_set * planes};
    in[n_in++] = {x, n};
    in[n_in++] = {dsum_total, planes};
    in[n_in++] = {dmean, planes};
    const AgRange out[] = {{grad_x, n}};
    if (ag_outputs_clash(in, n_in, out, 1)) return AOC_ERR_INVALID_ARG;
    hipLaunchKernelGGL(channel_scale_multi_grad_apply_kernel, dim3((unsigned)planes, aoc_plane_slices(hw)), dim3(256), 0, aoc_hip_stream(stream), g, gates, x,
                       dsum_total, dmean, n_set, planes, hw, grad_x);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

size_t aoc_groupnorm_cat_relu_grad_workspace_bytes(int n_src, int N, int C_src, int C_tail, int groups) {
    if (n_src < 1 || n_src > AOC_PTR_LIST || N < 1 || C_src < 1 || C_tail < 0 || groups < 1 || C_src % groups) return 0;
    return ag_carve(nullptr, n_src, N, C_src, C_tail, groups).total;
}

int aoc_groupnorm_cat_relu_grad(const float *grad_out, const float *const *u_ptrs, int n_src, int N, int C_src, int64_t hw, int groups, const float *stats,
                                const float *gamma, const float *beta, const float *tail, int C_tail, const float *plane_sumsq, const float *gate,
                                const float *gct_alpha, const float *gct_gamma, float gct_eps, float *const *grad_u_ptrs, float *grad_gamma,
                                float *grad_beta, float *grad_tail, float *grad_gct_alpha, float *grad_gct_gamma, float *grad_gct_beta, void *workspace,
                                size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_out || !u_ptrs || !stats || !plane_sumsq || !gate || !gct_alpha || !gct_gamma || n_src < 1 || n_src > AOC_PTR_LIST || N < 1 || C_src < 1 ||
        hw < 1 || groups < 1 || C_tail < 0)
        return AOC_ERR_INVALID_ARG;
    if (C_src % groups) return AOC_ERR_INVALID_ARG;
    if (C_tail > 0 && !tail) return AOC_ERR_INVALID_ARG;
    if (grad_tail && C_tail < 1) return AOC_ERR_INVALID_ARG;
    const int64_t C_total = (int64_t)n_src * C_src + C_tail;
    if (N > AOC_MAX_OBJECTS || (int64_t)N * C_total > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    if (hw > INT64_MAX / 4 / ((int64_t)N * C_total)) return AOC_ERR_UNSUPPORTED;
    const int64_t planes = (int64_t)N * C_total, ny = planes * hw, nx = (int64_t)N * C_src * hw, n_aff = (int64_t)n_src * C_src;
    const int64_t n_stats = (int64_t)n_src * N * groups * 2;
    AocSrcList u = {};
    AocDstList gu = {};
    AgRange in[AOC_PTR_LIST + 10], out[AOC_PTR_LIST + 8];
    int n_in = 0, n_out = 0;
    bool any_u = false;
    for (int k = 0; k < n_src; ++k) {
        if (!u_ptrs[k]) return AOC_ERR_INVALID_ARG;
        u.p[k] = u_ptrs[k];
        in[n_in++] = {u_ptrs[k], nx};
        if (grad_u_ptrs && grad_u_ptrs[k]) {
            gu.p[k] = grad_u_ptrs[k];
            out[n_out++] = {grad_u_ptrs[k], nx};
            any_u = true;
        }
    }
    if (!any_u && !grad_gamma && !grad_beta && !grad_tail && !grad_gct_alpha && !grad_gct_gamma && !grad_gct_beta) return AOC_OK;
    if (!workspace || workspace_bytes < aoc_groupnorm_cat_relu_grad_workspace_bytes(n_src, N, C_src, C_tail, groups)) return AOC_ERR_WORKSPACE;
    in[n_in++] = {grad_out, ny};
    in[n_in++] = {stats, n_stats};
    in[n_in++] = {gamma, n_aff};
    in[n_in++] = {beta, n_aff};
    in[n_in++] = {tail, (int64_t)N * C_tail};
    in[n_in++] = {plane_sumsq, planes};
    in[n_in++] = {gate, planes};
    in[n_in++] = {gct_alpha, C_total};
    in[n_in++] = {gct_gamma, C_total};
    out[n_out++] = {grad_gamma, n_aff};
    out[n_out++] = {grad_beta, n_aff};
    out[n_out++] = {grad_tail, (int64_t)N * C_tail};
    out[n_out++] = {grad_gct_alpha, C_total};
    out[n_out++] = {grad_gct_gamma, C_total};
    out[n_out++] = {grad_gct_beta, C_total};
    out[n_out++] = {workspace, (int64_t)(aoc_groupnorm_cat_relu_grad_workspace_bytes(n_src, N, C_src, C_tail, groups) / sizeof(float))};
    if (ag_outputs_clash(in, n_in, out, n_out)) return AOC_ERR_INVALID_ARG;
    hipStream_t st = aoc_hip_stream(stream);
    const AgWs w = ag_carve(workspace, n_src, N, C_src, C_tail, groups);
    const int gc = C_src / groups;
    if (hw / 4 <= 2048)
        hipLaunchKernelGGL(gn_cat_grad_plane_kernel<256>, dim3((unsigned)planes), dim3(256), 0, st, grad_out, u, n_src, N, C_src, gc, hw, stats, gamma, beta, tail,
                           C_tail, w.P);
    else
        hipLaunchKernelGGL(gn_cat_grad_plane_kernel<1024>, dim3((unsigned)planes), dim3(1024), 0, st, grad_out, u, n_src, N, C_src, gc, hw, stats, gamma, beta,
                           tail, C_tail, w.P);
    const bool need_ds = any_u || grad_gamma || grad_beta || grad_tail;
    hipLaunchKernelGGL(gn_cat_grad_gate_kernel, dim3(1), dim3(256), 0, st, (const float *)w.P, gate, plane_sumsq, gct_alpha, gct_gamma, N, (int)C_total, gct_eps,
                       need_ds ? w.ds : (float *)nullptr, grad_gct_alpha, grad_gct_gamma, grad_gct_beta);
    if (need_ds) {
        const int64_t threads = (int64_t)n_src * N * groups + n_aff + (int64_t)N * C_tail;
        hipLaunchKernelGGL(gn_cat_grad_small_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const float *)w.P, gate, (const float *)w.ds,
                           gamma, tail, n_src, N, C_src, C_tail, gc, (float)((int64_t)gc * hw), (float)hw, any_u ? w.coef : (float *)nullptr, grad_gamma,
                           grad_beta, grad_tail);
    }
    if (any_u)
        hipLaunchKernelGGL(gn_cat_grad_apply_kernel, dim3((unsigned)((int64_t)n_src * N * C_src), aoc_plane_slices(hw)), dim3(256), 0, st, grad_out, u, n_src, N,
                           C_src, C_tail, gc, hw, stats, gamma, beta, gate, (const float *)w.ds, (const float *)w.coef, gu);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
