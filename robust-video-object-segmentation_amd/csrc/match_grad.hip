// Training-time global matching: the argmin forward and the gradient kernels of the dense path (global_matching, AEM:616-685 over
// AEM:178-227, 61-89) and of the k = 1 proxy path (global_matching_proxy, AEM:336-402 over AEM:112-175).
//
// With d = |q|^2 + |r|^2 - 2 q.r and T = 2 sigmoid(d + b) - 1:  dT/dd = dT/db = (1 - T^2) / 2,  dd/dq = 2 (q - r*),  dd/dr* = 2 (r* - q),
// r* the row torch.min picks (the lowest row on ties).  The reference keeps the [m, O, n] distance tensor for autograd; here the backward
// needs the winning row per (pixel, object), the saved T and the operands.
//
//   g[i, o]       = (grad_out[i, o] * 0.5f) * (1.0f - T * T)                           one product, one difference, one product
//   grad_query[i] = sum over o, ascending, of (2 g) * (q_i - r_arg)                    a gather: no atomics
//   grad_pool[r]  = sum over the pairs (i, o) with arg = r, ascending i then o, of (2 g) * (r - q_i)
//   grad_bias[o]  = sum over i of g[i, o]
//
// Determinism: no float atomic anywhere.  The pairs of a pool row are found through an inverse list (integer atomics count and slot them, so
// the ORDER inside a list is arbitrary); a workgroup then ranks its list by pair id before it adds, so the order of summation never
// depends on the slotting.  A row with more than MG_LIST pairs ("hot": one row can win every pixel of every object) is not listed at all:
// MG_NSEG workgroups each scan a fixed range of pair ids for it, add their matches in ascending order, and a last kernel adds the
// MG_NSEG partial rows in ascending order.  Every sum is therefore a fixed tree of the buffers' contents alone.
#include "aoc_common.h"

namespace {

constexpr int MG_LIST = 256;    // longest list one workgroup ranks and adds by itself (= its thread count)
constexpr int MG_NSEG = 32;     // fixed pair-id ranges per hot row
constexpr int MG_CHUNK = 64;    // pairs a hot-row workgroup looks at per step (one ballot of a wave); most query rows staged in LDS at once
// query rows staged per step: 64 up to C = 128, 32 above, so that the dynamic LDS stays at 32 KiB for every C <= AOC_MAX_CHANNELS
inline __host__ __device__ int mg_stage_rows(int C) { return C > 128 ? MG_CHUNK / 2 : MG_CHUNK; }
constexpr int MG_BIAS_PIX = 256;   // pixels per first-stage block of the bias sum
constexpr int PG_PIX = 64;         // pixels per first-stage block of the proxy sums

// One wave per pixel: g and a bounds-checked dense copy of arg for the later kernels, the pairs counted per pool row, grad_query.
__global__ __launch_bounds__(64) void mg_pairs_kernel(const float *__restrict__ grad_out, const float *__restrict__ T, const int32_t *__restrict__ arg,
                                                      int64_t pstride, int64_t ostride, const float *__restrict__ query,
                                                      const float *__restrict__ pool, int64_t m, int64_t n, int C, int n_obj,
                                                      float *__restrict__ gbuf, int32_t *__restrict__ abuf, int32_t *__restrict__ count,
                                                      float *__restrict__ grad_query) {
    __shared__ float lg[AOC_MAX_OBJECTS + 2];
    __shared__ int32_t la[AOC_MAX_OBJECTS + 2];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    if (lane < n_obj) {
        const int64_t at = i * pstride + lane * ostride;
        const float g = aoc_transform_gate(grad_out[at], T[at]);
        int32_t a = arg[at];
        if (a < 0 || a >= n) a = -1;
        gbuf[i * n_obj + lane] = g;
        abuf[i * n_obj + lane] = a;
        lg[lane] = g;
        la[lane] = a;
        if (count && a >= 0) atomicAdd(&count[a], 1);
    }
    __syncthreads();
    if (!grad_query) return;
    for (int c = lane; c < C; c += 64) {
        const float q = query[i * C + c];
        float acc = 0.0f;
        for (int o = 0; o < n_obj; ++o) {
            const int32_t a = la[o];
            if (a >= 0) acc += (2.0f * lg[o]) * (q - pool[(int64_t)a * C + c]);
        }
        grad_query[i * C + c] = acc;
    }
}

// A listed row's place in the list buffer.  Where it lands depends on the order of the atomics; nothing that is summed does.
__global__ __launch_bounds__(256) void mg_alloc_kernel(const int32_t *__restrict__ count, int64_t n, int32_t *__restrict__ base, int32_t *__restrict__ total) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t c = count[r];
    base[r] = (c > 0 && c <= MG_LIST) ? atomicAdd(total, c) : 0;
}

__global__ __launch_bounds__(256) void mg_fill_kernel(const int32_t *__restrict__ abuf, int64_t n_pairs, const int32_t *__restrict__ count,
                                                      const int32_t *__restrict__ base, int32_t *__restrict__ cursor, int32_t *__restrict__ list) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int32_t a = abuf[p];
    if (a < 0 || count[a] > MG_LIST) return;
    list[base[a] + atomicAdd(&cursor[a], 1)] = (int32_t)p;
}

// acc += (2 g) * (r_c - q_i[c]) over the `np` pairs lpid[0 .. np), in that order; their query rows pass through LDS mg_stage_rows(C) at a time.
// Thread c < C owns channel c.  Every thread of the workgroup calls it.
__device__ __forceinline__ void mg_add_pairs(const int32_t *lpid, int np, const float *__restrict__ query, const float *__restrict__ gbuf, int C, int n_obj,
                                             float rc, float *lq, float *lg2, float &acc) {
    const int rows = mg_stage_rows(C);
    for (int k0 = 0; k0 < np; k0 += rows) {
        const int nk = min(rows, np - k0);
        for (int idx = threadIdx.x; idx < nk * C; idx += blockDim.x) {
            const int k = idx / C, c = idx - k * C;
            lq[idx] = query[(int64_t)(lpid[k0 + k] / n_obj) * C + c];
        }
        if ((int)threadIdx.x < nk) lg2[threadIdx.x] = 2.0f * gbuf[lpid[k0 + threadIdx.x]];
        __syncthreads();
        if ((int)threadIdx.x < C)
            for (int k = 0; k < nk; ++k) acc += lg2[k] * (rc - lq[k * C + threadIdx.x]);
        __syncthreads();
    }
}

// One workgroup per pool row: zeros for a row nobody chose (unkept rows among them), the ranked list's sum for a listed row; a hot row is
// queued for mg_hot_kernel.
__global__ __launch_bounds__(MG_LIST) void mg_rows_kernel(const float *__restrict__ query, const float *__restrict__ pool, const float *__restrict__ gbuf,
                                                          int C, int n_obj, const int32_t *__restrict__ count, const int32_t *__restrict__ base,
                                                          const int32_t *__restrict__ list, int32_t *__restrict__ n_hot, int32_t *__restrict__ hot_rows,
                                                          float *__restrict__ grad_pool) {
    extern __shared__ __attribute__((aligned(16))) float lq[];       // [mg_stage_rows(C)][C]
    __shared__ int32_t lraw[MG_LIST], lpid[MG_LIST];
    __shared__ float lg2[MG_CHUNK];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t cnt = count[r];
    if (cnt == 0) {
        if (tid < C) grad_pool[r * C + tid] = 0.0f;
        return;
    }
    if (cnt > MG_LIST) {
        if (tid == 0) hot_rows[atomicAdd(n_hot, 1)] = (int32_t)r;
        return;
    }
    if (tid < cnt) lraw[tid] = list[base[r] + tid];
    __syncthreads();
    if (tid < cnt) {            // pair ids are distinct: the rank is the number of smaller ones
        const int32_t e = lraw[tid];
        int rank = 0;
        for (int k = 0; k < cnt; ++k) rank += lraw[k] < e;
        lpid[rank] = e;
    }
    __syncthreads();
    const float rc = tid < C ? pool[r * C + tid] : 0.0f;
    float acc = 0.0f;
    mg_add_pairs(lpid, cnt, query, gbuf, C, n_obj, rc, lq, lg2, acc);
    if (tid < C) grad_pool[r * C + tid] = acc;
}

// Hot rows: workgroup (h, s) adds the matches of hot row h among the pair ids [s seg, (s + 1) seg), ascending.
__global__ __launch_bounds__(256) void mg_hot_kernel(const float *__restrict__ query, const float *__restrict__ pool, const float *__restrict__ gbuf,
                                                     const int32_t *__restrict__ abuf, int64_t n_pairs, int64_t seg, int C, int n_obj,
                                                     const int32_t *__restrict__ n_hot, const int32_t *__restrict__ hot_rows, float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lq[];
    __shared__ int32_t lpid[MG_CHUNK];
    __shared__ float lg2[MG_CHUNK];
    const int h = blockIdx.x;
    if (h >= *n_hot) return;
    const int32_t r = hot_rows[h];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t beg = (int64_t)blockIdx.y * seg, end = min(n_pairs, beg + seg);
    const float rc = tid < C ? pool[(int64_t)r * C + tid] : 0.0f;
    float acc = 0.0f;
    for (int64_t p0 = beg; p0 < end; p0 += MG_CHUNK) {
        const int64_t p = p0 + lane;
        const bool hit = p < end && abuf[p] == r;
        const unsigned long long mask = __ballot(hit);          // the same 64 pairs in every wave
        const int np = __popcll(mask);
        if (np == 0) continue;                                   // uniform over the workgroup
        if (tid < 64 && hit) lpid[__popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)p;
        __syncthreads();
        mg_add_pairs(lpid, np, query, gbuf, C, n_obj, rc, lq, lg2, acc);
    }
    if (tid < C) partial[((int64_t)h * MG_NSEG + blockIdx.y) * C + tid] = acc;
}

__global__ __launch_bounds__(256) void mg_hot_final_kernel(const float *__restrict__ partial, int C, const int32_t *__restrict__ n_hot,
                                                           const int32_t *__restrict__ hot_rows, float *__restrict__ grad_pool) {
    const int h = blockIdx.x;
    if (h >= *n_hot) return;
    const int tid = threadIdx.x;
    if (tid >= C) return;
    float acc = 0.0f;
    for (int s = 0; s < MG_NSEG; ++s) acc += partial[((int64_t)h * MG_NSEG + s) * C + tid];
    grad_pool[(int64_t)hot_rows[h] * C + tid] = acc;
}

// sum over the pixels of g[i, o]: MG_BIAS_PIX pixels per first-stage thread, ascending, then the blocks, ascending
__global__ __launch_bounds__(32) void mg_bias_partial_kernel(const float *__restrict__ gbuf, int64_t m, int n_obj, float *__restrict__ part) {
    const int o = threadIdx.x;
    if (o >= n_obj) return;
    const int64_t beg = (int64_t)blockIdx.x * MG_BIAS_PIX, end = min(m, beg + MG_BIAS_PIX);
    float acc = 0.0f;
    for (int64_t i = beg; i < end; ++i) acc += gbuf[i * n_obj + o];
    part[(int64_t)blockIdx.x * n_obj + o] = acc;
}
__global__ __launch_bounds__(32) void mg_bias_final_kernel(const float *__restrict__ part, int n_blocks, int n_obj, float *__restrict__ grad_bias) {
    const int o = threadIdx.x;
    if (o >= n_obj) return;
    float acc = 0.0f;
    for (int b = 0; b < n_blocks; ++b) acc += part[(int64_t)b * n_obj + o];
    grad_bias[o] = acc;
}

// ---- k = 1 proxies
__global__ __launch_bounds__(64) void pg_pairs_kernel(const float *__restrict__ grad_out, const float *__restrict__ T, int64_t pstride, int64_t ostride,
                                                      const float *__restrict__ query, const float *__restrict__ proxies, int C, int n_obj,
                                                      float *__restrict__ gbuf, float *__restrict__ grad_query) {
    __shared__ float lg[AOC_MAX_OBJECTS + 2];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    if (lane < n_obj) {
        const int64_t at = i * pstride + lane * ostride;
        const float g = aoc_transform_gate(grad_out[at], T[at]);
        gbuf[i * n_obj + lane] = g;
        lg[lane] = g;
    }
    __syncthreads();
    if (!grad_query) return;
    for (int c = lane; c < C; c += 64) {
        const float q = query[i * C + c];
        float acc = 0.0f;
        for (int o = 0; o < n_obj; ++o) acc += (2.0f * lg[o]) * (q - proxies[o * C + c]);
        grad_query[i * C + c] = acc;
    }
}
// part[b, o, c] = sum over the block's pixels, ascending, of g[i, o] q_i[c]; part[b, o, C] = the same sum of g[i, o]
__global__ __launch_bounds__(256) void pg_partial_kernel(const float *__restrict__ gbuf, const float *__restrict__ query, int64_t m, int C, int n_obj,
                                                         float *__restrict__ part) {
    const int o = blockIdx.y, c = threadIdx.x;
    const int64_t beg = (int64_t)blockIdx.x * PG_PIX, end = min(m, beg + PG_PIX);
    float s = 0.0f, gs = 0.0f;
    for (int64_t i = beg; i < end; ++i) {
        const float g = gbuf[i * n_obj + o];
        gs += g;
        if (c < C) s += g * query[i * C + c];
    }
    float *dst = part + ((int64_t)blockIdx.x * n_obj + o) * (C + 1);
    if (c < C) dst[c] = s;
    if (c == 0) dst[C] = gs;
}
__global__ __launch_bounds__(256) void pg_final_kernel(const float *__restrict__ part, int n_blocks, const float *__restrict__ proxies, int C, int n_obj,
                                                       float *__restrict__ grad_proxies, float *__restrict__ grad_bias) {
    const int o = blockIdx.x, c = threadIdx.x;
    float s = 0.0f, gs = 0.0f;
    for (int b = 0; b < n_blocks; ++b) {
        const float *src = part + ((int64_t)b * n_obj + o) * (C + 1);
        gs += src[C];
        if (c < C) s += src[c];
    }
    if (grad_proxies && c < C) grad_proxies[o * C + c] = 2.0f * (proxies[o * C + c] * gs - s);
    if (grad_bias && c == 0) grad_bias[o] = gs;
}

struct MgLayout {
    size_t gbuf, abuf, ints, base, list, hot_rows, partial, bias_part, total;
    int64_t h_max;
    int bias_blocks;
};
MgLayout mg_layout(int64_t m, int64_t n, int C, int n_obj) {
    MgLayout l;
    const size_t pairs = (size_t)m * n_obj;
    l.h_max = (int64_t)(pairs / (MG_LIST + 1));
    l.bias_blocks = (int)((m + MG_BIAS_PIX - 1) / MG_BIAS_PIX);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += aoc_align_up(bytes, 256); return here; };
    l.gbuf = take(pairs * sizeof(float));
    l.abuf = take(pairs * sizeof(int32_t));
    l.ints = take(((size_t)2 * n + 2) * sizeof(int32_t));         // count [n], cursor [n], list total, hot rows: zeroed per call
    l.base = take((size_t)n * sizeof(int32_t));
    l.list = take(pairs * sizeof(int32_t));
    l.hot_rows = take((size_t)(l.h_max + 1) * sizeof(int32_t));
    l.partial = take((size_t)(l.h_max + 1) * MG_NSEG * C * sizeof(float));
    l.bias_part = take((size_t)l.bias_blocks * n_obj * sizeof(float));
    l.total = at;
    return l;
}

// 0 = fine; the sizes every entry point shares
int mg_check_sizes(int64_t m, int C, int n_obj) {
    if (m < 1 || C < 1 || n_obj < 1) return AOC_ERR_INVALID_ARG;
    if (C > AOC_MAX_CHANNELS || n_obj > AOC_MAX_OBJECTS || m >= (1ll << 31) / AOC_MAX_OBJECTS) return AOC_ERR_UNSUPPORTED;
    return AOC_OK;
}

}  // namespace

extern "C" {

size_t aoc_dense_match_argmin_workspace_bytes(int64_t m, int64_t n_fg_capacity, int n_obj) {
    if (m < 1 || n_fg_capacity < 0 || n_obj < 1) return 0;
    return aoc_dense_argmin_workspace_bytes_impl(m, n_fg_capacity, n_obj);
}

int aoc_dense_match_argmin(const float *query, int64_t m, int C, const float *pool, const int32_t *fg_rows, const int32_t *n_fg,
                           int64_t n_fg_capacity, const uint32_t *wrong_bits, const float *obj_bias, int n_obj,
                           float *out, int32_t *arg, int64_t out_pixel_stride, int64_t out_obj_stride, int transform,
                           void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!query || !pool || !fg_rows || !n_fg || !wrong_bits || !out || !arg || !workspace) return AOC_ERR_INVALID_ARG;
    if (aoc_off16(pool)) return AOC_ERR_INVALID_ARG;                       // dense_match_partial_kernel reads the pool rows as float4
    if (m < 1 || C < 4 || n_obj < 1 || n_fg_capacity < 1 || n_fg_capacity >= (1ll << 31)) return AOC_ERR_INVALID_ARG;
    if ((C & 3) || C > 128 || n_obj > AOC_MAX_OBJECTS) return AOC_ERR_UNSUPPORTED;      // the widths of aoc_dense_match_min
    if (workspace_bytes < aoc_dense_match_argmin_workspace_bytes(m, n_fg_capacity, n_obj)) return AOC_ERR_WORKSPACE;
    return aoc_dense_match_argmin_impl(query, m, C, pool, fg_rows, n_fg, n_fg_capacity, wrong_bits, obj_bias, n_obj, out, arg, out_pixel_stride,
                                       out_obj_stride, transform, workspace, stream);
}

size_t aoc_dense_match_grad_workspace_bytes(int64_t m, int64_t n, int C, int n_obj) {
    if (n < 1 || n >= (1ll << 31) || mg_check_sizes(m, C, n_obj) != AOC_OK) return 0;
    return mg_layout(m, n, C, n_obj).total;
}

int aoc_dense_match_grad(const float *grad_out, const float *T, const int32_t *arg, int64_t pixel_stride, int64_t obj_stride,
                         const float *query, int64_t m, int C, const float *pool, int64_t n, int n_obj,
                         float *grad_query, float *grad_pool, float *grad_bias,
                         void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_out || !T || !arg || !query || !pool || !workspace) return AOC_ERR_INVALID_ARG;
    if (n < 1 || n >= (1ll << 31)) return AOC_ERR_INVALID_ARG;
    if (int rc = mg_check_sizes(m, C, n_obj)) return rc;
    const MgLayout l = mg_layout(m, n, C, n_obj);
    if (workspace_bytes < l.total) return AOC_ERR_WORKSPACE;
    hipStream_t st = aoc_hip_stream(stream);
    char *ws = static_cast<char *>(workspace);
    float *gbuf = reinterpret_cast<float *>(ws + l.gbuf);
    int32_t *abuf = reinterpret_cast<int32_t *>(ws + l.abuf);
    int32_t *count = reinterpret_cast<int32_t *>(ws + l.ints), *cursor = count + n, *total = cursor + n, *n_hot = total + 1;
    int32_t *base = reinterpret_cast<int32_t *>(ws + l.base), *list = reinterpret_cast<int32_t *>(ws + l.list);
    int32_t *hot_rows = reinterpret_cast<int32_t *>(ws + l.hot_rows);
    float *partial = reinterpret_cast<float *>(ws + l.partial), *bias_part = reinterpret_cast<float *>(ws + l.bias_part);
    const int64_t n_pairs = m * n_obj;

    if (grad_pool && hipMemsetAsync(count, 0, ((size_t)2 * n + 2) * sizeof(int32_t), st) != hipSuccess) return AOC_ERR_LAUNCH;
    hipLaunchKernelGGL(mg_pairs_kernel, dim3((unsigned)m), dim3(64), 0, st, grad_out, T, arg, pixel_stride, obj_stride, query, pool, m, n, C, n_obj,
                       gbuf, abuf, grad_pool ? count : nullptr, grad_query);
    if (grad_pool) {
        const size_t lds = (size_t)mg_stage_rows(C) * C * sizeof(float);
        hipLaunchKernelGGL(mg_alloc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, count, n, base, total);
        hipLaunchKernelGGL(mg_fill_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, abuf, n_pairs, count, base, cursor, list);
        hipLaunchKernelGGL(mg_rows_kernel, dim3((unsigned)n), dim3(MG_LIST), lds, st, query, pool, gbuf, C, n_obj, count, base, list, n_hot, hot_rows,
                           grad_pool);
        if (l.h_max > 0) {
            const int64_t seg = ((n_pairs + MG_NSEG - 1) / MG_NSEG + MG_CHUNK - 1) / MG_CHUNK * MG_CHUNK;
            hipLaunchKernelGGL(mg_hot_kernel, dim3((unsigned)l.h_max, MG_NSEG), dim3(256), lds, st, query, pool, gbuf, abuf, n_pairs, seg, C, n_obj,
                               n_hot, hot_rows, partial);
            hipLaunchKernelGGL(mg_hot_final_kernel, dim3((unsigned)l.h_max), dim3(256), 0, st, partial, C, n_hot, hot_rows, grad_pool);
        }
    }
    if (grad_bias) {
        hipLaunchKernelGGL(mg_bias_partial_kernel, dim3(l.bias_blocks), dim3(32), 0, st, gbuf, m, n_obj, bias_part);
        hipLaunchKernelGGL(mg_bias_final_kernel, dim3(1), dim3(32), 0, st, bias_part, l.bias_blocks, n_obj, grad_bias);
    }
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

size_t aoc_proxy_match_grad_workspace_bytes(int64_t m, int C, int n_obj) {
    if (mg_check_sizes(m, C, n_obj) != AOC_OK) return 0;
    const size_t blocks = (size_t)((m + PG_PIX - 1) / PG_PIX);
    return aoc_align_up((size_t)m * n_obj * sizeof(float), 256) + aoc_align_up(blocks * n_obj * (C + 1) * sizeof(float), 256);
}

int aoc_proxy_match_grad(const float *grad_out, const float *T, int64_t pixel_stride, int64_t obj_stride,
                         const float *query, int64_t m, int C, const float *proxies, int n_obj,
                         float *grad_query, float *grad_proxies, float *grad_bias,
                         void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_out || !T || !query || !proxies || !workspace) return AOC_ERR_INVALID_ARG;
    if (int rc = mg_check_sizes(m, C, n_obj)) return rc;
    if (workspace_bytes < aoc_proxy_match_grad_workspace_bytes(m, C, n_obj)) return AOC_ERR_WORKSPACE;
    hipStream_t st = aoc_hip_stream(stream);
    float *gbuf = static_cast<float *>(workspace);
    float *part = reinterpret_cast<float *>(static_cast<char *>(workspace) + aoc_align_up((size_t)m * n_obj * sizeof(float), 256));
    const int blocks = (int)((m + PG_PIX - 1) / PG_PIX);
    hipLaunchKernelGGL(pg_pairs_kernel, dim3((unsigned)m), dim3(64), 0, st, grad_out, T, pixel_stride, obj_stride, query, proxies, C, n_obj, gbuf,
                       grad_query);
    if (grad_proxies || grad_bias) {
        hipLaunchKernelGGL(pg_partial_kernel, dim3(blocks, n_obj), dim3(256), 0, st, gbuf, query, m, C, n_obj, part);
        hipLaunchKernelGGL(pg_final_kernel, dim3(n_obj), dim3(256), 0, st, part, blocks, proxies, C, n_obj, grad_proxies, grad_bias);
    }
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
