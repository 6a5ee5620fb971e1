// Training-time DynamicPreHead: the backward of aoc_prehead (decoding_module.py:228-240, 1x1 conv -> GroupNorm -> ReLU, with the concatenation
// of aocnet.py:360-362).  One entry point (include/aoc_hip.h, which states every expression and summation order); aoc_amd.prehead_train wires
// it into autograd.
//
// The forward never stores the convolution output: it recomputes y = W x + b from the n_in-channel input in both of its passes.  So does the
// backward, in five launches:
//   plane pass   per (chunk of 256 pixels, object), like prehead_stats_kernel: y, xhat, v with the forward's instructions (the same <24>, <26>,
//                <28> and generic instantiations, the same fmaf order, the float32 mean / rstd of the forward's workspace), so v > 0 is the
//                forward output's own mask; per channel the chunk's sums of dz and dz xhat, in double: the float32 terms of 16 channels go
//                through LDS, eight threads per (channel, sum) add 32 pixels each, then a butterfly over the eight
//   small        (c1, c2) per (object, group), grad_gamma, grad_beta
//   apply pass   y and dy again; grad_feat in n_in registers, one write per plane; the workgroup's x tile and a tile of PG_CT channels of dy go
//                through LDS, where thread q owns the pair (c, k) = (q / (n_in + 1), q mod (n_in + 1)) and walks the chunk's pixels serially
//                (column n_in of the x tile is 1.0f: the bias)
//   reduce       the chunks' partials -> grad_weight, grad_bias
//   embedding    grad_out[:, :C] read along p, the objects added in ascending order, transposed through LDS, stored along the channels
// No mask, y, xhat or dy tensor leaves the chip; no float atomics; nothing depends on a pointer's alignment or on which outputs are wanted.
#include "aoc_common.h"

namespace {

constexpr int PG_MAX_IN = 32, PG_MAX_OUT = 128, PG_PIX = 256, PG_CT = 8;
constexpr int PG_ROW = PG_PIX + 4;          // floats per LDS tile row: 16-byte aligned rows, consecutive rows four banks apart
constexpr int PG_PT = 16, PG_PROW = PG_PIX + 32;          // the plane pass: channels per tile (2 x 16 rows of 8 threads = 256), floats per row

template <int N_IN>
struct PgDims {
    static constexpr int NK = N_IN > 0 ? N_IN : PG_MAX_IN;
};

__device__ __forceinline__ void pg_stage_weights(float *lw, const float *__restrict__ w, const float *__restrict__ b, int n_out, int n_in) {
    for (int i = threadIdx.x; i < n_out * n_in; i += PG_PIX) lw[i] = w[i];
    for (int i = threadIdx.x; i < n_out; i += PG_PIX) lw[n_out * n_in + i] = b[i];
    __syncthreads();
}

// prehead_stats_kernel's / prehead_apply_kernel's chain: bias first, k ascending, one fmaf per step
template <int N_IN>
__device__ __forceinline__ float pg_conv(const float *lw, const float (&x)[PgDims<N_IN>::NK], int c, int n_in, int n_out) {
    float y = lw[n_out * n_in + c];
#pragma unroll
    for (int k = 0; k < PgDims<N_IN>::NK; ++k)
        if (N_IN > 0 || k < n_in) y = __builtin_fmaf(lw[c * n_in + k], x[k], y);
    return y;
}

// ------------------------------------------------------------------------------------------ 1: the plane pass
// grid (n_chunks, n_obj): partial[o][c][chunk] = (sum dz, sum dz xhat) over the chunk's pixels, in double
template <int N_IN>
__global__ __launch_bounds__(PG_PIX) void prehead_grad_plane_kernel(const float *__restrict__ go, const float *__restrict__ feat,
                                                                     const float *__restrict__ stats, const float *__restrict__ w,
                                                                     const float *__restrict__ b, const float *__restrict__ gamma,
                                                                     const float *__restrict__ beta, int n_in_rt, int n_out, int group_size, int64_t hw,
                                                                     int C, int n_chunks, double *__restrict__ partial) {
    constexpr int NK = PgDims<N_IN>::NK;
    __shared__ float lw[PG_MAX_OUT * NK + PG_MAX_OUT];
    __shared__ __attribute__((aligned(16))) float terms[2 * PG_PT * PG_PROW];       // row 2 cc: dz, row 2 cc + 1: dz xhat of the tile's channel cc
    const int n_in = N_IN > 0 ? N_IN : n_in_rt;
    const int o = blockIdx.y, t = threadIdx.x;
    pg_stage_weights(lw, w, b, n_out, n_in);
    const int64_t p = (int64_t)blockIdx.x * PG_PIX + t;
    const bool live = p < hw;
    float x[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) x[k] = (k < n_in && live) ? feat[((size_t)o * n_in + k) * hw + p] : 0.0f;
    const int n_groups = n_out / group_size;
    const size_t gbase = ((size_t)o * (C + n_out) + C) * hw;
    const int row = t >> 3, j = t & 7;                       // the sums: eight threads per row
    for (int c0 = 0; c0 < n_out; c0 += PG_PT) {
        const int ct = min(PG_PT, n_out - c0);
        for (int cc = 0; cc < ct; ++cc) {
            const int c = c0 + cc;
            const float y = pg_conv<N_IN>(lw, x, c, n_in, n_out);
            const int g = c / group_size;
            const float mean = stats[((size_t)o * n_groups + g) * 2], rstd = stats[((size_t)o * n_groups + g) * 2 + 1];
            const float xhat = (y - mean) * rstd;
            const float v = xhat * gamma[c] + beta[c];
            const float gy = live ? go[gbase + (size_t)c * hw + p] : 0.0f;
            const float dz = (live && v > 0.0f) ? gy : 0.0f;
            terms[(2 * cc) * PG_PROW + t] = dz;
            terms[(2 * cc + 1) * PG_PROW + t] = dz * xhat;
        }
        __syncthreads();
        double acc = 0.0;
        if (row < 2 * ct) {
            const f32x4 *r4 = reinterpret_cast<const f32x4 *>(terms + row * PG_PROW);
#pragma unroll
            for (int m = 0; m < PG_PIX / 32; ++m) {
                const f32x4 q = r4[j + 8 * m];
                acc += (double)q[0]; acc += (double)q[1]; acc += (double)q[2]; acc += (double)q[3];
            }
        }
        acc += __shfl_xor(acc, 4);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 1);
        if (j == 0 && row < 2 * ct) partial[(((size_t)o * n_out + c0 + (row >> 1)) * n_chunks + blockIdx.x) * 2 + (row & 1)] = acc;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ 2: the small sums
// one wave per output.  Workgroup i < n_obj * n_groups: coef[i] = (c1, c2); workgroup n_obj * n_groups + c: grad_beta[c], grad_gamma[c].  Double:
// the summed (object, chunk) pairs q = 0, 1, ... are dealt to the 64 lanes (lane l adds q = l, l + 64, ... in ascending order), the lanes by xor
// butterfly (32 .. 1); a group's channels ascending.
__device__ __forceinline__ void pg_wave_sum2(double &a, double &b) {
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
}
__global__ __launch_bounds__(64) void prehead_grad_small_kernel(const double *__restrict__ partial, const float *__restrict__ gamma, int n_obj, int n_out,
                                                                int group_size, int n_chunks, double M, float *__restrict__ coef,
                                                                float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int n_groups = n_out / group_size;
    const int ng = n_obj * n_groups;
    if (i < ng) {
        const int g = i % n_groups, o = i / n_groups;
        double A = 0.0, B = 0.0;
        for (int c = g * group_size; c < (g + 1) * group_size; ++c) {
            const double *src = partial + ((size_t)o * n_out + c) * n_chunks * 2;
            double a = 0.0, bb = 0.0;
            for (int ch = lane; ch < n_chunks; ch += 64) { a += src[2 * ch]; bb += src[2 * ch + 1]; }
            pg_wave_sum2(a, bb);
            A += (double)gamma[c] * a;
            B += (double)gamma[c] * bb;
        }
        if (lane == 0) {
            coef[2 * (size_t)i] = (float)(A / M);
            coef[2 * (size_t)i + 1] = (float)(B / M);
        }
        return;
    }
    const int c = i - ng;
    if (c >= n_out) return;
    double a = 0.0, bb = 0.0;
    const int64_t pairs = (int64_t)n_obj * n_chunks;
    for (int64_t q = lane; q < pairs; q += 64) {
        const int64_t o = q / n_chunks, ch = q - o * n_chunks;
        const double *src = partial + (((size_t)o * n_out + c) * n_chunks + ch) * 2;
        a += src[0];
        bb += src[1];
    }
    pg_wave_sum2(a, bb);
    if (lane == 0) {
        if (grad_beta) grad_beta[c] = (float)a;
        if (grad_gamma) grad_gamma[c] = (float)bb;
    }
}

// ------------------------------------------------------------------------------------------ 3: the apply pass
// grid (n_chunks, n_obj): grad_feat (optional) and wpart[o][chunk][c][n_in + 1] (optional)
template <int N_IN>
__global__ __launch_bounds__(PG_PIX) void prehead_grad_apply_kernel(const float *__restrict__ go, const float *__restrict__ feat,
                                                                     const float *__restrict__ stats, const float *__restrict__ w,
                                                                     const float *__restrict__ b, const float *__restrict__ gamma,
                                                                     const float *__restrict__ beta, const float *__restrict__ coef, int n_in_rt, int n_out,
                                                                     int group_size, int64_t hw, int C, int n_chunks, float *__restrict__ grad_feat,
                                                                     float *__restrict__ wpart) {
    constexpr int NK = PgDims<N_IN>::NK;
    __shared__ float lw[PG_MAX_OUT * NK + PG_MAX_OUT];
    __shared__ __attribute__((aligned(16))) float xs[(NK + 1) * PG_ROW];          // [k][pixel]; row n_in holds 1.0f (0.0f past the plane's end)
    __shared__ __attribute__((aligned(16))) float dys[PG_CT * PG_ROW];            // [channel of the tile][pixel]
    const int n_in = N_IN > 0 ? N_IN : n_in_rt;
    const int o = blockIdx.y, t = threadIdx.x;
    pg_stage_weights(lw, w, b, n_out, n_in);
    const int64_t p = (int64_t)blockIdx.x * PG_PIX + t;
    const bool live = p < hw;
    float x[NK], gf[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        x[k] = (k < n_in && live) ? feat[((size_t)o * n_in + k) * hw + p] : 0.0f;
        gf[k] = 0.0f;
    }
    const bool sums = wpart != nullptr;
    if (sums) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (N_IN > 0 || k < n_in) xs[k * PG_ROW + t] = x[k];
        xs[n_in * PG_ROW + t] = live ? 1.0f : 0.0f;
    }
    const int n_groups = n_out / group_size;
    const int xcols = n_in + 1;
    const size_t gbase = ((size_t)o * (C + n_out) + C) * hw;
    for (int c0 = 0; c0 < n_out; c0 += PG_CT) {
        const int ct = min(PG_CT, n_out - c0);
        for (int cc = 0; cc < ct; ++cc) {
            const int c = c0 + cc;
            const float y = pg_conv<N_IN>(lw, x, c, n_in, n_out);
            const int g = c / group_size;
            const float mean = stats[((size_t)o * n_groups + g) * 2], rstd = stats[((size_t)o * n_groups + g) * 2 + 1];
            const float c1 = coef[((size_t)o * n_groups + g) * 2], c2 = coef[((size_t)o * n_groups + g) * 2 + 1];
            const float xhat = (y - mean) * rstd;
            const float gam = gamma[c];
            const float v = xhat * gam + beta[c];
            const float gy = live ? go[gbase + (size_t)c * hw + p] : 0.0f;
            const float dz = (live && v > 0.0f) ? gy : 0.0f;
            const float dy = live ? rstd * ((gam * dz - c1) - xhat * c2) : 0.0f;
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (N_IN > 0 || k < n_in) gf[k] = __builtin_fmaf(lw[c * n_in + k], dy, gf[k]);
            if (sums) dys[cc * PG_ROW + t] = dy;
        }
        if (sums) {                                   // uniform over the workgroup
            __syncthreads();
            for (int q = t; q < ct * xcols; q += PG_PIX) {
                const int cc = q / xcols, k = q - cc * xcols;
                const f32x4 *d4 = reinterpret_cast<const f32x4 *>(dys + cc * PG_ROW);
                const f32x4 *x4 = reinterpret_cast<const f32x4 *>(xs + k * PG_ROW);
                float acc = 0.0f;
#pragma unroll 4
                for (int i = 0; i < PG_PIX / 4; ++i) {
                    const f32x4 d = d4[i], xv = x4[i];
                    acc = __builtin_fmaf(d[0], xv[0], acc);
                    acc = __builtin_fmaf(d[1], xv[1], acc);
                    acc = __builtin_fmaf(d[2], xv[2], acc);
                    acc = __builtin_fmaf(d[3], xv[3], acc);
                }
                wpart[(((size_t)o * n_chunks + blockIdx.x) * n_out + c0 + cc) * xcols + k] = acc;
            }
            __syncthreads();
        }
    }
    if (grad_feat && live) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (N_IN > 0 || k < n_in) grad_feat[((size_t)o * n_in + k) * hw + p] = gf[k];
    }
}

// ------------------------------------------------------------------------------------------ 4: the partials' reduction
// 64 outputs per workgroup; wave s adds the parts s, s + 4, ... in double, then ((s0 + s1) + s2) + s3
__global__ __launch_bounds__(256) void prehead_grad_reduce_kernel(const float *__restrict__ wpart, int64_t n_parts, int n_out, int xcols,
                                                                  float *__restrict__ grad_weight, float *__restrict__ grad_bias) {
    __shared__ double sl[4][64];
    const int j = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int64_t total = (int64_t)n_out * xcols, idx = (int64_t)blockIdx.x * 64 + j;
    double acc = 0.0;
    if (idx < total)
        for (int64_t i = s; i < n_parts; i += 4) acc += (double)wpart[(size_t)i * total + idx];
    sl[s][j] = acc;
    __syncthreads();
    if (s == 0 && idx < total) {
        const double v = ((sl[0][j] + sl[1][j]) + sl[2][j]) + sl[3][j];
        const int c = (int)(idx / xcols), k = (int)(idx % xcols);
        if (k < xcols - 1) {
            if (grad_weight) grad_weight[(size_t)c * (xcols - 1) + k] = (float)v;
        } else if (grad_bias) {
            grad_bias[c] = (float)v;
        }
    }
}

// ------------------------------------------------------------------------------------------ 5: the embedding's gradient
// grid (ceil(hw / 64), ceil(C / 32)): a tile of 64 pixels x 32 channels; reads along p, stores along the channels
__global__ __launch_bounds__(256) void prehead_grad_emb_kernel(const float *__restrict__ go, int n_obj, int C, int n_out, int64_t hw,
                                                               float *__restrict__ grad_emb) {
    __shared__ float tile[32][65];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int k0 = blockIdx.y * 32;
    {
        const int pp = t & 63;
        const int64_t p = p0 + pp;
        for (int kk = t >> 6; kk < 32; kk += 4) {
            const int k = k0 + kk;
            float s = 0.0f;
            if (p < hw && k < C)
                for (int o = 0; o < n_obj; ++o) s += go[((size_t)o * (C + n_out) + k) * hw + p];
            tile[kk][pp] = s;
        }
    }
    __syncthreads();
    {
        const int kk = t & 31, k = k0 + kk;
        for (int pp = t >> 5; pp < 64; pp += 8) {
            const int64_t p = p0 + pp;
            if (p < hw && k < C) grad_emb[(size_t)p * C + k] = tile[kk][pp];
        }
    }
}

struct PgWs {
    double *partial;
    float *coef, *wpart;
    size_t total;
};
inline PgWs pg_carve(void *base, int n_obj, int n_in, int n_out, int n_groups, size_t n_chunks) {
    PgWs w;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *r = p ? p + off : nullptr; off += aoc_align_up(bytes, 256); return r; };
    w.partial = reinterpret_cast<double *>(take((size_t)n_obj * n_out * n_chunks * 2 * sizeof(double)));
    w.coef = reinterpret_cast<float *>(take((size_t)n_obj * n_groups * 2 * sizeof(float)));
    w.wpart = reinterpret_cast<float *>(take((size_t)n_obj * n_chunks * n_out * (n_in + 1) * sizeof(float)));
    w.total = off;
    return w;
}

}  // namespace

extern "C" {

size_t aoc_prehead_grad_workspace_bytes(int n_obj, int n_in, int n_out, int n_groups, int64_t hw) {
    if (n_obj < 1 || n_in < 1 || n_out < 1 || n_groups < 1 || hw < 1 || n_out % n_groups) return 0;
    return pg_carve(nullptr, n_obj, n_in, n_out, n_groups, (size_t)((hw + PG_PIX - 1) / PG_PIX)).total;
}

int aoc_prehead_grad(const float *grad_out, const float *feat, const float *stats, const float *weight, const float *bias, const float *gamma,
                     const float *beta, int n_obj, int n_in, int n_out, int n_groups, int64_t hw, int C, float *grad_feat, float *grad_weight,
                     float *grad_bias, float *grad_gamma, float *grad_beta, float *grad_emb_hwc, void *workspace, size_t workspace_bytes,
                     aoc_stream_t stream) {
    if (!grad_out || !feat || !stats || !weight || !bias || !gamma || !beta || n_obj < 1 || n_in < 1 || n_out < 1 || n_groups < 1 || hw < 1 || C < 0)
        return AOC_ERR_INVALID_ARG;
    if (n_in > PG_MAX_IN || n_out > PG_MAX_OUT || n_out % n_groups != 0 || n_obj > 65535 || (grad_emb_hwc != nullptr && C == 0)) return AOC_ERR_UNSUPPORTED;
    const int64_t chunks64 = (hw + PG_PIX - 1) / PG_PIX;
    if (chunks64 > 0x1fffffffLL || C > 65535 * 32) return AOC_ERR_UNSUPPORTED;          // the grids: hw / 64 and C / 32 workgroups
    const bool params = grad_weight || grad_bias;
    const bool apply = grad_feat || params;
    const bool plane = apply || grad_gamma || grad_beta;
    if (!plane && !grad_emb_hwc) return AOC_OK;
    if (plane && (!workspace || workspace_bytes < aoc_prehead_grad_workspace_bytes(n_obj, n_in, n_out, n_groups, hw))) return AOC_ERR_WORKSPACE;
    hipStream_t st = aoc_hip_stream(stream);
    const int n_chunks = (int)chunks64, group_size = n_out / n_groups;
    const PgWs ws = pg_carve(plane ? workspace : nullptr, n_obj, n_in, n_out, n_groups, (size_t)n_chunks);
    float *wpart = params ? ws.wpart : nullptr;
#define AOC_PG(NI)                                                                                                                                        \
    do {                                                                                                                                                  \
        hipLaunchKernelGGL(prehead_grad_plane_kernel<NI>, dim3(n_chunks, n_obj), dim3(PG_PIX), 0, st, grad_out, feat, stats, weight, bias, gamma, beta, n_in, \
                           n_out, group_size, hw, C, n_chunks, ws.partial);                                                                               \
        hipLaunchKernelGGL(prehead_grad_small_kernel, dim3((unsigned)(n_obj * n_groups + n_out)), dim3(64), 0, st, ws.partial, gamma,                      \
                           n_obj, n_out, group_size, n_chunks, (double)group_size * (double)hw, ws.coef, grad_gamma, grad_beta);                         \
        if (apply)                                                                                                                                        \
            hipLaunchKernelGGL(prehead_grad_apply_kernel<NI>, dim3(n_chunks, n_obj), dim3(PG_PIX), 0, st, grad_out, feat, stats, weight, bias, gamma, beta,  \
                               ws.coef, n_in, n_out, group_size, hw, C, n_chunks, grad_feat, wpart);                                                     \
    } while (0)
    if (plane) {
        if (n_in == 24) AOC_PG(24); else if (n_in == 26) AOC_PG(26); else if (n_in == 28) AOC_PG(28); else AOC_PG(0);
    }
#undef AOC_PG
    if (params) {
        const int64_t total = (int64_t)n_out * (n_in + 1);
        hipLaunchKernelGGL(prehead_grad_reduce_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, ws.wpart, (int64_t)n_obj * n_chunks, n_out,
                           n_in + 1, grad_weight, grad_bias);
    }
    if (grad_emb_hwc)
        hipLaunchKernelGGL(prehead_grad_emb_kernel, dim3((unsigned)((hw + 63) / 64), (unsigned)((C + 31) / 32)), dim3(256), 0, st, grad_out, n_obj, C, n_out, hw,
                           grad_emb_hwc);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
