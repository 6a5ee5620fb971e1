// Training-time decoder forms: the backward of aoc_groupnorm_relu / aoc_groupnorm_relu_scale (the four normalisations of a Bottleneck,
// gct.py:69-90, the last one with the IA_gate of decoding_module.py:196,198 / :206,208 folded in) and of aoc_cat_film_scale
// (decoding_module.py:193-194, 203-204).  Two entry points (include/aoc_hip.h); aoc_amd.decoder_train wires them into autograd.
//
// The GroupNorm backward is three launches: a plane pass (one workgroup per (n, c) plane reads grad_y, x and the residual once and leaves
// A = sum dz, B = sum dz xhat and dgain = sum grad_y a), one small launch (the group sums s1 / M, s2 / M, grad_gamma, grad_beta) and an
// apply pass (the same three streams again, grad_x and grad_residual written once).  z is recomputed with the forward's expression
// (x a + b, then + residual, with gn_apply_kernel's a and b), so the mask z > 0 is the one the forward's fmaxf applied; no xhat, mask,
// grad_y a product or ungated activation is ever stored.  A streamed plane is cut (plane_stream.h) by the alignment of the plane the
// pass WRITES (grad_x, else grad_residual; of grad_y where nothing is written); sources, and a second destination, are accessed 16 bytes
// per lane at 4-byte alignment.
//
// No float atomics.  Every sum runs in an order fixed by the shapes and by that alignment cut:
//   plane sums     aoc_channel_scale_grad's order: thread t of T adds its front scalar, its float4 t, t + T, ... (components .x .y .z .w in
//                  turn), its back scalar, each product rounded before it is added (-ffp-contract=off); then the xor butterfly of
//                  aoc_wave_sum; then the wave sums in ascending wave order.  T = 256 for planes of at most 2 048 float4, else 1 024.
//   small kernel   one thread per output, a serial loop in ascending index of the summed dimension, from 0.0f.
#include "plane_stream.h"

namespace {

// what a plane's elements need of the forward: z = x a + b [+ r] (gn_apply_kernel's expression), xhat = (x - mean) rstd
struct NgPlane {
    float mean, rstd, gam, a, b, g;
    int relu, has_gain;
};
__device__ __forceinline__ NgPlane ng_plane(const float *__restrict__ stats, const float *__restrict__ gamma, const float *__restrict__ beta,
                                            const float *__restrict__ gain, int64_t plane, int C, int group_channels, int relu) {
    NgPlane P;
    const int c = (int)(plane % C);
    const int64_t n = plane / C;
    const int64_t gi = n * (C / group_channels) + c / group_channels;
    P.mean = stats[2 * gi];
    P.rstd = stats[2 * gi + 1];
    P.gam = gamma ? gamma[c] : 1.0f;
    P.a = P.rstd * P.gam;
    P.b = (beta ? beta[c] : 0.0f) - P.mean * P.a;
    P.has_gain = gain != nullptr;
    P.g = gain ? gain[plane] : 1.0f;
    P.relu = relu;
    return P;
}
__device__ __forceinline__ float ng_z(const NgPlane &P, float x, float r, bool has_r) {
    float v = x * P.a + P.b;
    if (has_r) v += r;
    return v;
}
// dz = da (z > 0), da = gain grad_y: the mask of the forward's fmaxf(z, 0), torch's `> 0`
__device__ __forceinline__ float ng_dz(const NgPlane &P, float gy, float z) {
    const float da = P.has_gain ? P.g * gy : gy;
    return (P.relu && !(z > 0.0f)) ? 0.0f : da;
}

struct NgAcc { float A, B, G; };
__device__ __forceinline__ void ng_add1(const NgPlane &P, NgAcc &acc, float gy, float x, float r, bool has_r) {
    const float z = ng_z(P, x, r, has_r);
    const float dz = ng_dz(P, gy, z);
    const float xhat = (x - P.mean) * P.rstd;
    acc.A += dz;
    acc.B += dz * xhat;
    acc.G += gy * (P.relu ? fmaxf(z, 0.0f) : z);
}

// ------------------------------------------------------------------------------------------ 1: the plane pass
// grid (N * C): A[plane], B[plane] (workspace) and dgain[plane] (optional) from one read of grad_y, x and the residual
template <int T>
__global__ __launch_bounds__(T) void gn_grad_plane_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ res,
                                                           const float *__restrict__ stats, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const float *__restrict__ gain, int C, int group_channels,
                                                           int64_t hw, int relu, float *__restrict__ A, float *__restrict__ B, float *__restrict__ dgain) {
    __shared__ float wsum[3][T / 64];
    const int64_t plane = blockIdx.x;
    const int t = threadIdx.x;
    const NgPlane P = ng_plane(stats, gamma, beta, gain, plane, C, group_channels, relu);
    const float *gp = gy + plane * hw;
    const float *xp = x + plane * hw;
    const bool has_r = res != nullptr;
    const float *rp = has_r ? res + plane * hw : nullptr;
    const int64_t front = aoc_front(gp, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    NgAcc acc = {0.0f, 0.0f, 0.0f};
    if (t < front) ng_add1(P, acc, gp[t], xp[t], has_r ? rp[t] : 0.0f, has_r);
    int64_t i = t;
    for (; i + (int64_t)T < body4; i += 2 * (int64_t)T) {             // six 16-byte loads in flight per thread
        f32x4 g4[2], x4[2], r4[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            g4[u] = aoc_load4(gp + front + 4 * (i + u * (int64_t)T));
            x4[u] = aoc_load4(xp + front + 4 * (i + u * (int64_t)T));
            if (has_r) r4[u] = aoc_load4(rp + front + 4 * (i + u * (int64_t)T));
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) ng_add1(P, acc, g4[u][k], x4[u][k], has_r ? r4[u][k] : 0.0f, has_r);
    }
    for (; i < body4; i += T) {
        const f32x4 g4 = aoc_load4(gp + front + 4 * i), x4 = aoc_load4(xp + front + 4 * i);
        f32x4 r4 = {0.0f, 0.0f, 0.0f, 0.0f};
        if (has_r) r4 = aoc_load4(rp + front + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) ng_add1(P, acc, g4[k], x4[k], r4[k], has_r);
    }
    if (t < hw - back0) ng_add1(P, acc, gp[back0 + t], xp[back0 + t], has_r ? rp[back0 + t] : 0.0f, has_r);
    acc.A = aoc_wave_sum(acc.A);
    acc.B = aoc_wave_sum(acc.B);
    acc.G = aoc_wave_sum(acc.G);
    if (aoc_lane() == 0) { wsum[0][t >> 6] = acc.A; wsum[1][t >> 6] = acc.B; wsum[2][t >> 6] = acc.G; }
    __syncthreads();
    if (t == 0) {
        float a = 0.0f, b = 0.0f, g = 0.0f;
        for (int w = 0; w < T / 64; ++w) { a += wsum[0][w]; b += wsum[1][w]; g += wsum[2][w]; }
        if (A) { A[plane] = a; B[plane] = b; }
        if (dgain) dgain[plane] = g;
    }
}

// ------------------------------------------------------------------------------------------ 2: the small sums
// thread i < N * groups: coef[i] = (s1 / M, s2 / M), s1 = sum_{c in g} gamma_c A[n, c], s2 = sum_{c in g} gamma_c B[n, c] over ascending c;
// thread N * groups + c: grad_gamma[c] = sum_n B[n, c], grad_beta[c] = sum_n A[n, c] over ascending n
__global__ __launch_bounds__(256) void gn_grad_small_kernel(const float *__restrict__ A, const float *__restrict__ B, const float *__restrict__ gamma, int N,
                                                            int C, int group_channels, float Mf, float *__restrict__ coef,
                                                            float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int groups = C / group_channels;
    const int64_t ng = (int64_t)N * groups;
    if (i < ng) {
        if (!coef) return;
        const int g = (int)(i % groups);
        const int64_t row = (i / groups) * C + (int64_t)g * group_channels;
        float s1 = 0.0f, s2 = 0.0f;
        for (int k = 0; k < group_channels; ++k) {
            const float gm = gamma ? gamma[g * group_channels + k] : 1.0f;
            s1 += gm * A[row + k];
            s2 += gm * B[row + k];
        }
        coef[2 * i] = s1 / Mf;
        coef[2 * i + 1] = s2 / Mf;
        return;
    }
    const int64_t c = i - ng;
    if (c >= C) return;
    if (grad_gamma) {
        float acc = 0.0f;
        for (int n = 0; n < N; ++n) acc += B[(int64_t)n * C + c];
        grad_gamma[c] = acc;
    }
    if (grad_beta) {
        float acc = 0.0f;
        for (int n = 0; n < N; ++n) acc += A[(int64_t)n * C + c];
        grad_beta[c] = acc;
    }
}

// ------------------------------------------------------------------------------------------ 3: the apply pass
// grid (N * C, slices): grad_residual = dz, grad_x = rstd ((gamma_c dz - s1 / M) - xhat s2 / M)
__device__ __forceinline__ void ng_apply1(const NgPlane &P, float c1, float c2, float gy, float x, float r, bool has_r, float &gx, float &gr) {
    const float dz = ng_dz(P, gy, ng_z(P, x, r, has_r));
    const float xhat = (x - P.mean) * P.rstd;
    gr = dz;
    gx = P.rstd * ((P.gam * dz - c1) - xhat * c2);
}

__global__ __launch_bounds__(256) void gn_grad_apply_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ res,
                                                            const float *__restrict__ stats, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const float *__restrict__ gain,
                                                            const float *__restrict__ coef, int C, int group_channels, int64_t hw, int relu,
                                                            float *__restrict__ grad_x, float *__restrict__ grad_res) {
    const int64_t plane = blockIdx.x;                        // planes on x (up to 2^31 - 1), the slices of a plane on y
    const NgPlane P = ng_plane(stats, gamma, beta, gain, plane, C, group_channels, relu);
    const int64_t gi = (plane / C) * (C / group_channels) + (plane % C) / group_channels;
    const float c1 = grad_x ? coef[2 * gi] : 0.0f, c2 = grad_x ? coef[2 * gi + 1] : 0.0f;
    const float *gp = gy + plane * hw;
    const float *xp = x + plane * hw;
    const bool has_r = res != nullptr;
    const float *rp = has_r ? res + plane * hw : nullptr;
    float *ox = grad_x ? grad_x + plane * hw : nullptr;
    float *orr = grad_res ? grad_res + plane * hw : nullptr;
    const int64_t front = aoc_front(ox ? ox : orr, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nthreads = (int64_t)gridDim.y * 256;
    if (tid < front) {
        float vx, vr;
        ng_apply1(P, c1, c2, gp[tid], xp[tid], has_r ? rp[tid] : 0.0f, has_r, vx, vr);
        if (ox) ox[tid] = vx;
        if (orr) orr[tid] = vr;
    }
    for (int64_t i = tid; i < body4; i += nthreads) {
        const int64_t e = front + 4 * i;
        const f32x4 g4 = aoc_load4(gp + e), x4 = aoc_load4(xp + e);
        f32x4 r4 = {0.0f, 0.0f, 0.0f, 0.0f}, vx, vr;
        if (has_r) r4 = aoc_load4(rp + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float a, b;
            ng_apply1(P, c1, c2, g4[k], x4[k], r4[k], has_r, a, b);
            vx[k] = a;
            vr[k] = b;
        }
        if (ox) {
            __builtin_nontemporal_store(vx, reinterpret_cast<f32x4 *>(ox + e));
            if (orr) aoc_store4_a4(orr + e, vr);              // the second destination may sit at another misalignment
        } else {
            __builtin_nontemporal_store(vr, reinterpret_cast<f32x4 *>(orr + e));
        }
    }
    if (tid < hw - back0) {
        const int64_t e = back0 + tid;
        float vx, vr;
        ng_apply1(P, c1, c2, gp[e], xp[e], has_r ? rp[e] : 0.0f, has_r, vx, vr);
        if (ox) ox[e] = vx;
        if (orr) orr[e] = vr;
    }
}

struct NgWs {
    float *A, *B, *coef;
    size_t total;
};
inline NgWs ng_carve(void *base, int N, int C, int groups) {
    NgWs w;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *r = p ? p + off : nullptr; off += aoc_align_up(bytes, 256); return reinterpret_cast<float *>(r); };
    w.A = take((size_t)N * C * sizeof(float));
    w.B = take((size_t)N * C * sizeof(float));
    w.coef = take((size_t)N * groups * 2 * sizeof(float));
    w.total = off;
    return w;
}

// ------------------------------------------------------------------------------------------ the concatenation's gate
// One workgroup per plane (o, c) of grad_y [O, Cx + Cm, hw]: the source plane is x[o, c] for c < Cx, else mem[o, c - Cx]; the gradient plane
// grad_x[o, c] / grad_mem[o, c - Cx] = gain grad_y (skipped where its pointer is NULL), dgain = <grad_y, source>.  The plane is cut by
// grad_y's alignment whatever is written (x, mem and the two gradients sit at other misalignments whenever hw is odd), so the order of the
// dot, and with it dgain's bits, is the same with and without the gradient planes.
template <int T>
__global__ __launch_bounds__(T) void cat_scale_grad_kernel(const float *__restrict__ gy, const float *x, const float *mem, const float *__restrict__ gain,
                                                           int Cx, int Cm, int64_t hw, float *__restrict__ grad_x, float *__restrict__ grad_mem,
                                                           float *__restrict__ dgain) {
    __shared__ float wsum[T / 64];
    const int64_t plane = blockIdx.x;
    const int t = threadIdx.x;
    const int Ct = Cx + Cm;
    const int c = (int)(plane % Ct);
    const int64_t o = plane / Ct;
    const float *gp = gy + plane * hw;
    const float *sp = c < Cx ? x + (o * Cx + c) * hw : mem + (o * Cm + (c - Cx)) * hw;
    float *op = c < Cx ? (grad_x ? grad_x + (o * Cx + c) * hw : nullptr) : (grad_mem ? grad_mem + (o * Cm + (c - Cx)) * hw : nullptr);
    const bool dot = dgain != nullptr;
    const float g = op ? gain[plane] : 0.0f;
    const int64_t front = aoc_front(gp, hw);                   // always grad_y's cut: dgain's bits do not depend on what else is written
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    const bool op16 = op && ((reinterpret_cast<uintptr_t>(op + front) & 15) == 0);
    float acc = 0.0f;
    if (t < front) {
        const float v = gp[t];
        if (dot) acc += v * sp[t];
        if (op) op[t] = g * v;
    }
    int64_t i = t;
    for (; i + 3 * (int64_t)T < body4; i += 4 * (int64_t)T) {       // eight 16-byte loads in flight per thread
        f32x4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = aoc_load4(gp + front + 4 * (i + u * (int64_t)T));
            if (dot) b[u] = aoc_load4(sp + front + 4 * (i + u * (int64_t)T));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (dot) { acc += a[u][0] * b[u][0]; acc += a[u][1] * b[u][1]; acc += a[u][2] * b[u][2]; acc += a[u][3] * b[u][3]; }
            if (op) aoc_store4(op + front + 4 * (i + u * (int64_t)T), a[u] * g, op16);
        }
    }
    for (; i < body4; i += T) {
        const f32x4 a = aoc_load4(gp + front + 4 * i);
        if (dot) {
            const f32x4 b = aoc_load4(sp + front + 4 * i);
            acc += a[0] * b[0]; acc += a[1] * b[1]; acc += a[2] * b[2]; acc += a[3] * b[3];
        }
        if (op) aoc_store4(op + front + 4 * i, a * g, op16);
    }
    if (t < hw - back0) {
        const float v = gp[back0 + t];
        if (dot) acc += v * sp[back0 + t];
        if (op) op[back0 + t] = g * v;
    }
    if (dot) {
        acc = aoc_wave_sum(acc);
        if (aoc_lane() == 0) wsum[t >> 6] = acc;
        __syncthreads();
        if (t == 0) {
            float s = 0.0f;
            for (int w = 0; w < T / 64; ++w) s += wsum[w];
            dgain[plane] = s;
        }
    }
}

}  // namespace

extern "C" {

size_t aoc_groupnorm_relu_grad_workspace_bytes(int N, int C, int groups) {
    if (N < 1 || C < 1 || groups < 1 || C % groups) return 0;
    return ng_carve(nullptr, N, C, groups).total;
}

int aoc_groupnorm_relu_grad(const float *grad_y, const float *x, const float *residual, const float *stats, const float *gamma, const float *beta,
                            const float *gain, int N, int C, int64_t hw, int groups, int relu, float *grad_x, float *grad_residual, float *grad_gamma,
                            float *grad_beta, float *dgain, void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_y || !x || !stats || N < 1 || C < 1 || hw < 1 || groups < 1) return AOC_ERR_INVALID_ARG;
    if (C % groups) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (int64_t)N * C > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    if (!grad_x && !grad_residual && !grad_gamma && !grad_beta && !dgain) return AOC_OK;
    const bool sums = grad_x || grad_gamma || grad_beta;       // A and B are wanted
    if (sums && (!workspace || workspace_bytes < aoc_groupnorm_relu_grad_workspace_bytes(N, C, groups))) return AOC_ERR_WORKSPACE;
    hipStream_t st = aoc_hip_stream(stream);
    const NgWs w = ng_carve(sums ? workspace : nullptr, N, C, groups);
    const int gc = C / groups;
    const unsigned planes = (unsigned)((int64_t)N * C);
    if (sums || dgain) {
        if (hw / 4 <= 2048)
            hipLaunchKernelGGL(gn_grad_plane_kernel<256>, dim3(planes), dim3(256), 0, st, grad_y, x, residual, stats, gamma, beta, gain, C, gc, hw, relu, w.A, w.B,
                               dgain);
        else
            hipLaunchKernelGGL(gn_grad_plane_kernel<1024>, dim3(planes), dim3(1024), 0, st, grad_y, x, residual, stats, gamma, beta, gain, C, gc, hw, relu, w.A,
                               w.B, dgain);
    }
    if (sums) {
        const int64_t threads = (int64_t)N * groups + C;
        hipLaunchKernelGGL(gn_grad_small_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, w.A, w.B, gamma, N, C, gc,
                           (float)((int64_t)gc * hw), grad_x ? w.coef : (float *)nullptr, grad_gamma, grad_beta);
    }
    if (grad_x || grad_residual)
        hipLaunchKernelGGL(gn_grad_apply_kernel, dim3(planes, aoc_plane_slices(hw)), dim3(256), 0, st, grad_y, x, residual, stats, gamma, beta, gain, w.coef, C, gc,
                           hw, relu, grad_x, grad_residual);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_cat_film_scale_grad(const float *grad_y, const float *x, const float *mem, const float *gain, int n_obj, int Cx, int Cm, int64_t hw, float *grad_x,
                            float *grad_mem, float *dgain, aoc_stream_t stream) {
    if (!grad_y || n_obj < 1 || Cx < 1 || Cm < 0 || hw < 1) return AOC_ERR_INVALID_ARG;
    if (((grad_x || grad_mem) && !gain) || (dgain && (!x || (Cm > 0 && !mem))) || (grad_mem && Cm < 1)) return AOC_ERR_INVALID_ARG;
    const int64_t planes = (int64_t)n_obj * ((int64_t)Cx + Cm);
    if (n_obj > AOC_MAX_OBJECTS || planes > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    if (!grad_x && !grad_mem && !dgain) return AOC_OK;
    hipStream_t st = aoc_hip_stream(stream);
    if (hw / 4 <= 2048)
        hipLaunchKernelGGL(cat_scale_grad_kernel<256>, dim3((unsigned)planes), dim3(256), 0, st, grad_y, x, mem, gain, Cx, Cm, hw, grad_x, grad_mem, dgain);
    else
        hipLaunchKernelGGL(cat_scale_grad_kernel<1024>, dim3((unsigned)planes), dim3(1024), 0, st, grad_y, x, mem, gain, Cx, Cm, hw, grad_x, grad_mem, dgain);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
