// Training-time calibration gates: the backward of IA_gate (ATT:7-17), of GCT (gct.py:17-36) and of conditioning_layer / conditioning_block
// (CLB:24-86).  Six entry points (include/aoc_hip.h); aoc_amd.gates_train wires them into autograd.
//
// Three of them stream activation-sized tensors (channel_scale_grad, gct_scale_grad, cond_scale_grad); the other three work on the small
// [N, C] / [C, D] operands.  A streamed plane is cut (plane_stream.h) by the alignment of the plane it WRITES, or, for the plane dot that
// writes nothing, of grad_y; a source plane may sit at another misalignment than the destination (scores [N, hw] against the planes
// [N, C, hw] with odd hw) without falling back to a scalar plane.
//
// No float atomics.  Every sum runs in an order fixed by the shapes and by that alignment cut:
//   plane dot      thread t of T adds its front scalar, its float4 t, t + T, ... (components .x .y .z .w in turn), its back scalar, each
//                  product rounded before it is added (-ffp-contract=off); then the xor butterfly of aoc_wave_sum; then the wave sums in
//                  ascending wave order.  T = 256 for planes of at most 2 048 float4, else 1 024.
//   small kernels  one thread per output, a serial loop in ascending index of the summed dimension, from 0.0f.
#include <stdlib.h>

#include "gct_gate_grad.h"

namespace {

// ------------------------------------------------------------------------------------------ 1: grad_x = gain * grad_y, dgain = <grad_y, x>
// One workgroup per plane; grad_y and x are read once, grad_x written once.  WRITE / DOT select the halves at compile time.
template <int T, bool WRITE, bool DOT>
__global__ __launch_bounds__(T) void channel_scale_grad_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ gain,
                                                                int64_t hw, float *__restrict__ gx, float *__restrict__ dgain) {
    __shared__ float wsum[T / 64];
    const int64_t plane = blockIdx.x;
    const int t = threadIdx.x;
    const float *gp = gy + plane * hw;
    const float *xp = DOT ? x + plane * hw : nullptr;
    float *op = WRITE ? gx + plane * hw : nullptr;
    const float g = WRITE ? gain[plane] : 0.0f;
    const int64_t front = aoc_front(WRITE ? (const void *)op : (const void *)gp, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    float acc = 0.0f;
    if (t < front) {
        const float v = gp[t];
        if (DOT) acc += v * xp[t];
        if (WRITE) op[t] = g * v;
    }
    const float *gb = gp + front;
    const float *xb = DOT ? xp + front : nullptr;
    int64_t i = t;
    for (; i + 3 * (int64_t)T < body4; i += 4 * (int64_t)T) {       // eight 16-byte loads in flight per thread
        f32x4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = aoc_load4(gb + 4 * (i + u * (int64_t)T));
            if (DOT) b[u] = aoc_load4(xb + 4 * (i + u * (int64_t)T));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (DOT) acc = aoc_dot4(acc, a[u], b[u]);
            if (WRITE) __builtin_nontemporal_store(a[u] * g, reinterpret_cast<f32x4 *>(op + front) + (i + u * (int64_t)T));
        }
    }
    for (; i < body4; i += T) {
        const f32x4 a = aoc_load4(gb + 4 * i);
        if (DOT) acc = aoc_dot4(acc, a, aoc_load4(xb + 4 * i));
        if (WRITE) __builtin_nontemporal_store(a * g, reinterpret_cast<f32x4 *>(op + front) + i);
    }
    if (t < hw - back0) {
        const float v = gp[back0 + t];
        if (DOT) acc += v * xp[back0 + t];
        if (WRITE) op[back0 + t] = g * v;
    }
    if (DOT) {
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

template <int T>
void launch_channel_scale_grad(const float *gy, const float *x, const float *gain, int64_t planes, int64_t hw, float *gx, float *dgain, hipStream_t s) {
    const dim3 grid((unsigned)planes), block(T);
    if (gx && dgain) hipLaunchKernelGGL((channel_scale_grad_kernel<T, true, true>), grid, block, 0, s, gy, x, gain, hw, gx, dgain);
    else if (gx) hipLaunchKernelGGL((channel_scale_grad_kernel<T, true, false>), grid, block, 0, s, gy, x, gain, hw, gx, dgain);
    else hipLaunchKernelGGL((channel_scale_grad_kernel<T, false, true>), grid, block, 0, s, gy, x, gain, hw, gx, dgain);
}

// ------------------------------------------------------------------------------------------ 2: through gain = 1 + tanh(head W^T + b)
__device__ __forceinline__ float gg_da(const float *__restrict__ dgain, const float *__restrict__ gain, size_t i) {
    const float t = gain[i] - 1.0f;
    return dgain[i] * (1.0f - t * t);
}

// acc += a[i] * w[i * ld] for i = 0 .. n - 1 in that order; the loads of eight steps are issued together, the additions stay in sequence (a
// long serial sum otherwise pays one memory round trip per step)
__device__ __forceinline__ float gg_serial_dot(const float *a, const float *__restrict__ w, int n, size_t ld, float acc) {
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        float wv[8], av[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { wv[u] = w[(size_t)(i + u) * ld]; av[u] = a[i + u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += av[u] * wv[u];
    }
    for (; i < n; ++i) acc += a[i] * w[(size_t)i * ld];
    return acc;
}

// rows [0, n_obj): grad_head[o, d] over ascending c (da of 256 channels at a time through LDS); rows [n_obj, n_obj + channels):
// grad_weight[c, d] (and grad_bias[c]) over ascending o
__global__ __launch_bounds__(256) void film_gain_grad_kernel(const float *__restrict__ dgain, const float *__restrict__ gain, const float *__restrict__ head,
                                                             const float *__restrict__ weight, int n_obj, int D, int channels,
                                                             float *__restrict__ grad_head, float *__restrict__ grad_weight, float *__restrict__ grad_bias) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    const int row = blockIdx.y;
    if (row < n_obj) {
        __shared__ float sda[256];
        if (!grad_head) return;
        const int dd = d < D ? d : D - 1;                       // every thread walks the loop (barriers); the store is guarded
        float acc = 0.0f;
        for (int c0 = 0; c0 < channels; c0 += 256) {
            __syncthreads();
            if (c0 + (int)threadIdx.x < channels) sda[threadIdx.x] = gg_da(dgain, gain, (size_t)row * channels + c0 + threadIdx.x);
            __syncthreads();
            acc = gg_serial_dot(sda, weight + (size_t)c0 * D + dd, min(256, channels - c0), D, acc);
        }
        if (d < D) grad_head[(size_t)row * D + d] = acc;
        return;
    }
    const int c = row - n_obj;
    if (grad_weight && d < D) {
        float acc = 0.0f;
        for (int o = 0; o < n_obj; ++o) acc += gg_da(dgain, gain, (size_t)o * channels + c) * head[(size_t)o * D + d];
        grad_weight[(size_t)c * D + d] = acc;
    }
    if (grad_bias && d == 0) {
        float acc = 0.0f;
        for (int o = 0; o < n_obj; ++o) acc += gg_da(dgain, gain, (size_t)o * channels + c);
        grad_bias[c] = acc;
    }
}

// ------------------------------------------------------------------------------------------ 3: through gct_gate_kernel's expressions
// one workgroup: gct_gate_grad_body (gct_gate_grad.h)
__global__ __launch_bounds__(256) void gct_gate_grad_kernel(const float *__restrict__ dgate, const float *__restrict__ gate, const float *__restrict__ s,
                                                            const float *__restrict__ alpha, const float *__restrict__ gamma, int N, int C, float eps, int l1,
                                                            float *__restrict__ dsum, float *__restrict__ grad_alpha, float *__restrict__ grad_gamma,
                                                            float *__restrict__ grad_beta) {
    __shared__ float wsum[4];
    gct_gate_grad_body(dgate, gate, s, alpha, gamma, N, C, eps, l1, dsum, grad_alpha, grad_gamma, grad_beta, wsum);
}

// ------------------------------------------------------------------------------------------ 4, 6: the apply passes
// KIND 0 (GCT):          out = gy * a[plane] + b[plane] * f'(x),  f' by `mode` (aoc_plane_reduce's: 0 -> 1, 1 -> 2 x, 2 -> sign x)
// KIND 1 (conditioning): out = (gy * a[plane] + (scores[n, p] > thr[n] ? b[plane] / hw : 0)) + c[plane] / hw;  gy == NULL drops the first term
template <int KIND>
__device__ __forceinline__ float gg_apply1(float gyv, float sv, float a, float b, float c, float thr, int mode, bool has_gy) {
    if (KIND == 0) return gyv * a + b * (mode == 1 ? 2.0f * sv : (mode == 2 ? aoc_sign(sv) : 1.0f));
    const float m = sv > thr ? b : 0.0f;
    return (has_gy ? gyv * a + m : m) + c;
}

template <int KIND>
__global__ __launch_bounds__(256) void gate_apply_kernel(const float *__restrict__ gy, const float *__restrict__ src, int64_t src_planes_per_row,
                                                         const float *__restrict__ pa, const float *__restrict__ pb, const float *__restrict__ pc,
                                                         const float *__restrict__ thr_all, float div, int mode, int64_t hw, float *__restrict__ out) {
    const int64_t plane = blockIdx.x;                        // planes on x (up to 2^31 - 1), the slices of a plane on y
    const int64_t srow = plane / src_planes_per_row;         // KIND 0: src = x, one row per plane; KIND 1: src = scores, one row per sample
    const float *gp = gy ? gy + plane * hw : nullptr;
    const float *sp = src + srow * hw;
    float *op = out + plane * hw;
    const bool has_gy = gy != nullptr;
    const float a = (KIND == 0 || has_gy) ? pa[plane] : 0.0f;
    const float b = pb ? pb[plane] / div : 0.0f;
    const float c = (KIND == 1 && pc) ? pc[plane] / div : 0.0f;
    const float thr = KIND == 1 ? thr_all[srow] : 0.0f;
    const int64_t front = aoc_front(op, hw);
    const int64_t body4 = (hw - front) / 4, back0 = front + body4 * 4;
    const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nthreads = (int64_t)gridDim.y * 256;
    if (tid < front) op[tid] = gg_apply1<KIND>(has_gy ? gp[tid] : 0.0f, sp[tid], a, b, c, thr, mode, has_gy);
    for (int64_t i = tid; i < body4; i += nthreads) {
        const f32x4 sv = aoc_load4(sp + front + 4 * i);
        f32x4 gv = {0.0f, 0.0f, 0.0f, 0.0f}, o;
        if (has_gy) gv = aoc_load4(gp + front + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = gg_apply1<KIND>(gv[k], sv[k], a, b, c, thr, mode, has_gy);
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(op + front) + i);
    }
    if (tid < hw - back0) op[back0 + tid] = gg_apply1<KIND>(has_gy ? gp[back0 + tid] : 0.0f, sp[back0 + tid], a, b, c, thr, mode, has_gy);
}

// ------------------------------------------------------------------------------------------ 5: through cond_codes_kernel
// dd[m, j] = sum_i dcode[m, C + i] W2[i, j] in ascending i, the same instructions wherever it is needed
__device__ __forceinline__ float gg_dd(const float *__restrict__ dcode, const float *__restrict__ w2, int m, int j, int C, int ld) {
    return gg_serial_dot(dcode + (size_t)m * ld + C, w2 + j, C, C, 0.0f);
}

// rows [0, N): the input gradients of sample n, column j;  rows [N, N + 2C + D): the parameter gradients of code entry o (row o of W1, row
// o - C of W2, row o - 2C of W3), column j, over ascending n
__global__ __launch_bounds__(256) void cond_codes_grad_kernel(const float *__restrict__ dcode, const float *__restrict__ gap, const float *__restrict__ px,
                                                              const float *__restrict__ head, const float *__restrict__ w1, const float *__restrict__ w2,
                                                              const float *__restrict__ w3, int N, int C, int D, float *__restrict__ dgap,
                                                              float *__restrict__ dpx, float *__restrict__ grad_head, float *__restrict__ grad_w1,
                                                              float *__restrict__ grad_b1, float *__restrict__ grad_w2, float *__restrict__ grad_b2,
                                                              float *__restrict__ grad_w3, float *__restrict__ grad_b3) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int row = blockIdx.y;
    const int ld = 2 * C + D;
    if (row < N) {
        const int n = row;
        if (dgap && j < C) dgap[(size_t)n * C + j] = gg_serial_dot(dcode + (size_t)n * ld, w1 + j, C, C, 0.0f);
        if (dpx && j < C) {                                   // CLB:69 backwards: delta[m] = sum_k px[k] - px[m]  =>  dpx[n] = sum_m dd[m] - dd[n]
            float tot = 0.0f;
            for (int m = 0; m < N; ++m) tot += gg_dd(dcode, w2, m, j, C, ld);
            dpx[(size_t)n * C + j] = tot - gg_dd(dcode, w2, n, j, C, ld);
        }
        if (grad_head && j < D) grad_head[(size_t)n * D + j] = gg_serial_dot(dcode + (size_t)n * ld + 2 * C, w3 + j, D, D, 0.0f);
        return;
    }
    const int o = row - N;
    float bsum = 0.0f;
    for (int n = 0; n < N; ++n) bsum += dcode[(size_t)n * ld + o];
    if (o < C) {
        if (grad_w1 && j < C) {
            float acc = 0.0f;
            for (int n = 0; n < N; ++n) acc += dcode[(size_t)n * ld + o] * gap[(size_t)n * C + j];
            grad_w1[(size_t)o * C + j] = acc;
        }
        if (grad_b1 && j == 0) grad_b1[o] = bsum;
    } else if (o < 2 * C) {
        if (grad_w2 && j < C) {
            float tot = 0.0f;
            for (int m = 0; m < N; ++m) tot += px[(size_t)m * C + j];               // the forward's delta, cond_codes_kernel
            float acc = 0.0f;
            for (int n = 0; n < N; ++n) acc += dcode[(size_t)n * ld + o] * (tot - px[(size_t)n * C + j]);
            grad_w2[(size_t)(o - C) * C + j] = acc;
        }
        if (grad_b2 && j == 0) grad_b2[o - C] = bsum;
    } else {
        if (grad_w3 && j < D) {
            float acc = 0.0f;
            for (int n = 0; n < N; ++n) acc += dcode[(size_t)n * ld + o] * head[(size_t)n * D + j];
            grad_w3[(size_t)(o - 2 * C) * D + j] = acc;
        }
        if (grad_b3 && j == 0) grad_b3[o - 2 * C] = bsum;
    }
}

}  // namespace

extern "C" {

int aoc_channel_scale_grad(const float *grad_y, const float *x, const float *gain, int64_t planes, int64_t hw, float *grad_x, float *dgain,
                           aoc_stream_t stream) {
    if (!grad_y || planes < 1 || hw < 1 || (grad_x && !gain) || (dgain && !x)) return AOC_ERR_INVALID_ARG;
    if (planes > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    if (!grad_x && !dgain) return AOC_OK;
    if (hw / 4 <= 2048) launch_channel_scale_grad<256>(grad_y, x, gain, planes, hw, grad_x, dgain, aoc_hip_stream(stream));
    else launch_channel_scale_grad<1024>(grad_y, x, gain, planes, hw, grad_x, dgain, aoc_hip_stream(stream));
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_film_gain_grad(const float *dgain, const float *gain, const float *head, const float *weight, int n_obj, int head_dim, int channels,
                       float *grad_head, float *grad_weight, float *grad_bias, aoc_stream_t stream) {
    if (!dgain || !gain || n_obj < 1 || head_dim < 1 || channels < 1 || (grad_head && !weight) || (grad_weight && !head)) return AOC_ERR_INVALID_ARG;
    if (n_obj > AOC_MAX_OBJECTS || n_obj + channels > 65535) return AOC_ERR_UNSUPPORTED;
    if (!grad_head && !grad_weight && !grad_bias) return AOC_OK;
    const unsigned rows = (grad_weight || grad_bias) ? n_obj + channels : n_obj;
    hipLaunchKernelGGL(film_gain_grad_kernel, dim3((head_dim + 255) / 256, rows), dim3(256), 0, aoc_hip_stream(stream), dgain, gain, head, weight, n_obj,
                       head_dim, channels, grad_head, grad_weight, grad_bias);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_gct_gate_grad(const float *dgate, const float *gate, const float *plane_sums, const float *alpha, const float *gamma, const float *beta, int N,
                      int C, float eps, int l1_mode, float *dsum, float *grad_alpha, float *grad_gamma, float *grad_beta, aoc_stream_t stream) {
    (void)beta;                            // the saved gate carries beta's effect; kept in the signature beside aoc_gct_gate's
    if (!dgate || !gate || !plane_sums || !alpha || !gamma || N < 1 || C < 1) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS) return AOC_ERR_UNSUPPORTED;
    if (!dsum && !grad_alpha && !grad_gamma && !grad_beta) return AOC_OK;
    hipLaunchKernelGGL(gct_gate_grad_kernel, dim3(1), dim3(256), 0, aoc_hip_stream(stream), dgate, gate, plane_sums, alpha, gamma, N, C, eps, l1_mode,
                       dsum, grad_alpha, grad_gamma, grad_beta);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_gct_scale_grad(const float *grad_y, const float *x, const float *gate, const float *dsum, int mode, int64_t planes, int64_t hw, float *grad_x,
                       aoc_stream_t stream) {
    if (!grad_y || !x || !gate || !dsum || !grad_x || planes < 1 || hw < 1 || mode < 0 || mode > 2) return AOC_ERR_INVALID_ARG;
    if (planes > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gate_apply_kernel<0>, dim3((unsigned)planes, aoc_plane_slices(hw)), dim3(256), 0, aoc_hip_stream(stream), grad_y, x, (int64_t)1, gate,
                       dsum, (const float *)nullptr, (const float *)nullptr, 1.0f, mode, hw, grad_x);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_cond_codes_grad(const float *dcode, const float *gap, const float *plane_means, const float *head, const float *w1, const float *w2,
                        const float *w3, int N, int C, int D, float *dgap, float *dpx, float *grad_head, float *grad_w1, float *grad_b1, float *grad_w2,
                        float *grad_b2, float *grad_w3, float *grad_b3, aoc_stream_t stream) {
    if (!dcode || N < 1 || C < 0 || D < 0 || C + D < 1) return AOC_ERR_INVALID_ARG;
    if ((dgap && !w1) || (dpx && !w2) || (grad_head && !w3) || (grad_w1 && !gap) || (grad_w2 && !plane_means) || (grad_w3 && !head))
        return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (int64_t)N + 2 * (int64_t)C + D > 65535) return AOC_ERR_UNSUPPORTED;
    const bool params = grad_w1 || grad_b1 || grad_w2 || grad_b2 || grad_w3 || grad_b3;
    if (!params && !dgap && !dpx && !grad_head) return AOC_OK;
    const unsigned rows = params ? N + 2 * C + D : N;
    hipLaunchKernelGGL(cond_codes_grad_kernel, dim3((std::max(C, D) + 255) / 256, rows), dim3(256), 0, aoc_hip_stream(stream), dcode, gap, plane_means, head,
                       w1, w2, w3, N, C, D, dgap, dpx, grad_head, grad_w1, grad_b1, grad_w2, grad_b2, grad_w3, grad_b3);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_cond_scale_grad(const float *grad_y, const float *gain, const float *scores, const float *threshold, const float *dgap, const float *dpx, int N,
                        int C, int64_t hw, float *grad_x, aoc_stream_t stream) {
    if (!scores || !threshold || !grad_x || N < 1 || C < 1 || hw < 1 || (grad_y && !gain)) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (int64_t)N * C > 0x7fffffffLL) return AOC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gate_apply_kernel<1>, dim3((unsigned)((int64_t)N * C), aoc_plane_slices(hw)), dim3(256), 0, aoc_hip_stream(stream), grad_y, scores, (int64_t)C,
                       gain, dgap, dpx, threshold, (float)hw, 0, hw, grad_x);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
