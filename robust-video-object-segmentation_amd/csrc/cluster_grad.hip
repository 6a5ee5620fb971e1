// Training-time cluster matching (AEM:405-478 over AEM:231-332): the set minimum of aoc_proxy_corr_min with the winner's slot, the
// backward of that minimum and the pull-back of the gradient through centroid_avg (AEM:280) to the reference embeddings.
//
// The forward keeps proxy_corr_min_kernel's arithmetic (correlation.hip: the same v_mfma_f32_16x16x4_f32 sequence over the channels
// 4t + kq, |q|^2 as four strided partial sums folded by two lane exchanges, |p|^2 as given or summed stream after stream,
// d = (|q|^2 + |p|^2) - 2 q.p), so its values equal aoc_proxy_corr_min's bit for bit (tested); the proxies are read from global memory (a
// few KB that stay in cache) and a slot index rides beside each lane's running minimum.
//
// The backward is the inverse of the dense case: few rows, every one of them hot.  Stage 1 cuts the pixels into a fixed number of
// contiguous chunks; a workgroup owns (chunk, set, group of 32 slots), walks its pixels in order and adds g q_i into the LDS row of the
// winning slot, one thread per channel (no two threads share an address, no atomics).  Stage 2 is one workgroup per proxy row that adds
// the chunks' partial sums in ascending (set, chunk) order.  grad_query is a gather per pixel.  First choices, not tuned (STATUS.md).
#include <stdlib.h>

#include "aoc_common.h"

namespace {

constexpr int CG_SETS = 64;     // sets per launch (kernel-argument table); a call with more runs several launches in set order
constexpr int CG_SLOTS = 32;    // slots of a set one stage-1 workgroup accumulates in LDS
constexpr int CG_MAX_CHUNKS = 128;
constexpr int CG_CHUNK_MIN = 32;

struct CgSets {
    int64_t off[CG_SETS];       // output offset of the set
    int32_t begin[CG_SETS], size[CG_SETS];
    int32_t bias[CG_SETS];      // forward: index into set_bias (the set's own number); backward: set_bias_index
    int32_t sbase[CG_SETS];     // first slot of the set in the launch's slot list
    int32_t n, n_slot;
};

inline int cg_chunks(int64_t m) {
    const int64_t c = (m + CG_CHUNK_MIN - 1) / CG_CHUNK_MIN;
    return (int)(c < 1 ? 1 : (c > CG_MAX_CHUNKS ? CG_MAX_CHUNKS : c));
}

// ------------------------------------------------------------------------------------------ forward
// the A fragment (16 query rows) and the rows' squared norms in fp32; correlation.hip's load_a_fragment carries the float16 rounding as well
template <int TMAX>
__device__ __forceinline__ void cg_load_a(const float *__restrict__ query, int64_t m, int C, int64_t row0, float (&a)[TMAX], float &q2) {
    const int lane = aoc_lane();
    const int i = lane & 15, kq = lane >> 4, T = C >> 2;
    int64_t row = row0 + i;
    if (row > m - 1) row = m - 1;
    const float *src = query + row * C + kq;
    float part = 0.0f;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        a[t] = (t < T) ? src[4 * t] : 0.0f;
        part += a[t] * a[t];
    }
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    q2 = part;
}

template <int TMAX>
__global__ __launch_bounds__(256) void cg_set_argmin_kernel(const float *__restrict__ query, int64_t m, int C, const float *__restrict__ proxies,
                                                            const float *__restrict__ proxy_sqnorm, CgSets sets, const float *__restrict__ set_bias,
                                                            float *__restrict__ out, int32_t *__restrict__ arg, int64_t pstride, int transform) {
    const int lane = aoc_lane(), wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4, T = C >> 2;
    const int64_t n_row_tiles = (m + 15) / 16;
    for (int64_t rt = (int64_t)blockIdx.x * 4 + wave; rt < n_row_tiles; rt += (int64_t)gridDim.x * 4) {
        const int64_t row0 = rt * 16;
        float a[TMAX], q2;
        cg_load_a<TMAX>(query, m, C, row0, a, q2);
        float q2r[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) q2r[r] = __shfl(q2, g * 4 + r);
        for (int s = 0; s < sets.n; ++s) {
            const int begin = sets.begin[s], size = sets.size[s];
            float best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
            int slot[4] = {-1, -1, -1, -1};
            for (int c0 = 0; c0 < size; c0 += 16) {
                const int col = c0 + j;
                const bool valid = col < size;
                const float *prow = proxies + (size_t)(begin + (valid ? col : 0)) * C;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < TMAX; ++t) {
                    const float b = (valid && t < T) ? prow[4 * t + g] : 0.0f;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b, acc, 0, 0, 0);
                }
                float p2 = INFINITY;
                if (valid) {
                    if (proxy_sqnorm) {
                        p2 = proxy_sqnorm[begin + col];
                    } else {   // |p|^2 in the order of the staged image: stream kq = 0, then 1, 2, 3 (AEM:150)
                        p2 = 0.0f;
                        for (int kq = 0; kq < 4; ++kq)
                            for (int t = 0; t < T; ++t) p2 += prow[4 * t + kq] * prow[4 * t + kq];
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = (q2r[r] + p2) - 2.0f * acc[r];        // AEM:43
                    if (d < best[r]) { best[r] = d; slot[r] = col; }      // ascending slots: the first minimum stays
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int x = 1; x < 16; x <<= 1) {
                    const float ov = __shfl_xor(best[r], x);
                    const int os = __shfl_xor(slot[r], x);
                    if (ov < best[r] || (ov == best[r] && os < slot[r])) { best[r] = ov; slot[r] = os; }
                }
            }
            // every lane of a row group holds the four results: lane j < 4 stores row g * 4 + j
            float v = best[0];
            int w = slot[0];
#pragma unroll
            for (int r = 1; r < 4; ++r)
                if (j == r) { v = best[r]; w = slot[r]; }
            const int64_t row = row0 + g * 4 + j;
            if (j < 4 && row < m) {
                if (v == INFINITY) { v = AOC_PAD_DISTANCE; w = -1; }       // empty / all-ignored set: AEM:310-313
                const float b = set_bias ? set_bias[sets.bias[s]] : 0.0f;
                const int64_t at = row * pstride + sets.off[s];
                out[at] = transform ? aoc_proto_transform(v, b) : v;
                arg[at] = w;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ backward of the set minimum
// one wave per pixel; lane handles channels lane, lane + 64, ...
__global__ __launch_bounds__(256) void cg_query_grad_kernel(const float *__restrict__ grad_out, const float *__restrict__ T, const int32_t *__restrict__ arg,
                                                            int64_t pstride, const float *__restrict__ query, int64_t m, int C,
                                                            const float *__restrict__ proxies, CgSets sets, float *__restrict__ grad_query, int first) {
    const int lane = aoc_lane();
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    float q[4], acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        q[k] = c < C ? query[i * C + c] : 0.0f;
        acc[k] = (first || c >= C) ? 0.0f : grad_query[i * C + c];
    }
    for (int s = 0; s < sets.n; ++s) {
        const int64_t at = i * pstride + sets.off[s];
        const int a = arg[at];
        if (a < 0 || a >= sets.size[s]) continue;
        const float g2 = 2.0f * aoc_transform_gate(grad_out[at], T[at]);
        const float *p = proxies + (size_t)(sets.begin[s] + a) * C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c < C) acc[k] += g2 * (q[k] - p[c]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < C) grad_query[i * C + c] = acc[k];
    }
}

// stage 1: workgroup (chunk, set, slot group); part [n_slot][n_chunk][C + 1], element C = sum of g
__global__ __launch_bounds__(256) void cg_partial_kernel(const float *__restrict__ grad_out, const float *__restrict__ T, const int32_t *__restrict__ arg,
                                                         int64_t pstride, const float *__restrict__ query, int64_t m, int C, CgSets sets, int n_chunk,
                                                         int64_t per, float *__restrict__ part) {
    extern __shared__ float cg_lds[];     // [CG_SLOTS][C] then [CG_SLOTS]
    const int ch = blockIdx.x, si = blockIdx.y, slot0 = blockIdx.z * CG_SLOTS;
    const int size = sets.size[si];
    if (slot0 >= size) return;
    const int ns = size - slot0 < CG_SLOTS ? size - slot0 : CG_SLOTS;
    const int c = threadIdx.x;
    float *sumg = cg_lds + CG_SLOTS * C;
    if (c < C)
        for (int k = 0; k < ns; ++k) cg_lds[k * C + c] = 0.0f;
    if (c == 0)
        for (int k = 0; k < ns; ++k) sumg[k] = 0.0f;
    const int64_t i0 = ch * per, i1 = (i0 + per < m) ? i0 + per : m;
    const int64_t off = sets.off[si];
    for (int64_t i = i0; i < i1; ++i) {      // thread c owns column c of every LDS row and thread 0 the sums: no barrier is needed
        const int64_t at = i * pstride + off;
        const int a = arg[at] - slot0;
        if (a < 0 || a >= ns) continue;
        const float g = aoc_transform_gate(grad_out[at], T[at]);
        if (c < C) cg_lds[a * C + c] += g * query[i * C + c];
        if (c == 0) sumg[a] += g;
    }
    for (int k = 0; k < ns; ++k) {
        float *dst = part + ((size_t)(sets.sbase[si] + slot0 + k) * n_chunk + ch) * (C + 1);
        if (c < C) dst[c] = cg_lds[k * C + c];
        if (c == 0) dst[C] = sumg[k];
    }
}

// stage 2: one workgroup per proxy row; slot_sum [n_slot] = sum of g of the (set, slot)
__global__ __launch_bounds__(256) void cg_rows_kernel(const float *__restrict__ part, int n_chunk, int C, const float *__restrict__ proxies, CgSets sets,
                                                      float *__restrict__ grad_proxies, float *__restrict__ slot_sum, int first) {
    const int r = blockIdx.x, c = threadIdx.x;
    float sq = 0.0f, sg = 0.0f;
    for (int si = 0; si < sets.n; ++si) {
        const int k = r - sets.begin[si];
        if (k < 0 || k >= sets.size[si]) continue;
        const float *src = part + (size_t)(sets.sbase[si] + k) * n_chunk * (C + 1);
        float g1 = 0.0f;
        for (int ch = 0; ch < n_chunk; ++ch) {
            if (c < C) sq += src[(size_t)ch * (C + 1) + c];
            g1 += src[(size_t)ch * (C + 1) + C];
        }
        sg += g1;
        if (c == 0) slot_sum[sets.sbase[si] + k] = g1;
    }
    if (grad_proxies && c < C) {
        const size_t at = (size_t)r * C + c;
        const float v = 2.0f * (proxies[at] * sg - sq);
        grad_proxies[at] = first ? v : grad_proxies[at] + v;
    }
}

__global__ __launch_bounds__(64) void cg_bias_kernel(const float *__restrict__ slot_sum, CgSets sets, int n_bias, float *__restrict__ grad_bias, int first) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n_bias) return;
    float acc = 0.0f;
    for (int si = 0; si < sets.n; ++si) {
        if (sets.bias[si] != b) continue;
        for (int k = 0; k < sets.size[si]; ++k) acc += slot_sum[sets.sbase[si] + k];
    }
    grad_bias[b] = first ? acc : grad_bias[b] + acc;
}

// ------------------------------------------------------------------------------------------ backward of centroid_avg
__global__ __launch_bounds__(256) void cg_count_kernel(const int32_t *__restrict__ seg_offsets, const int32_t *__restrict__ labels, int kmax,
                                                       int64_t rows_capacity, int32_t *__restrict__ counts) {
    const int s = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t o0 = seg_offsets[s], len = (int64_t)seg_offsets[s + 1] - o0;
    if (p >= len || o0 < 0 || o0 + p >= rows_capacity) return;
    const int j = labels[o0 + p];
    if (j >= 0 && j < kmax) atomicAdd(&counts[s * kmax + j], 1);     // integer: the order does not matter
}

// one wave per kept position p; row fg_rows[p] is written by this wave alone
__global__ __launch_bounds__(256) void cg_avg_gather_kernel(const float *__restrict__ grad_proxies, int C, const int32_t *__restrict__ fg_rows,
                                                            const int32_t *__restrict__ n_fg, const int32_t *__restrict__ seg_offsets,
                                                            const int32_t *__restrict__ seg_k, const int32_t *__restrict__ labels, int n_seg, int kmax,
                                                            int64_t rows_capacity, const int32_t *__restrict__ counts, float *__restrict__ grad_pool,
                                                            int64_t pool_rows) {
    const int lane = aoc_lane();
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= pool_rows || p >= *n_fg) return;
    const int64_t row = fg_rows[p];
    if (row < 0 || row >= pool_rows) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < n_seg; ++s) {
        const int64_t o0 = seg_offsets[s], len = (int64_t)seg_offsets[s + 1] - o0;
        if (p >= len || o0 < 0 || o0 + p >= rows_capacity) continue;
        const int j = labels[o0 + p];
        if (j < 0 || j >= kmax || j >= seg_k[s]) continue;
        const int cnt = counts[s * kmax + j];
        if (cnt < 1) continue;
        const float *src = grad_proxies + ((size_t)(s * 2 + 1) * kmax + j) * C;
        const float n = (float)cnt;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = lane + 64 * k;
            if (c < C) acc[k] += src[c] / n;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < C) grad_pool[row * C + c] = acc[k];
    }
}

// sets [s0, s0 + n) of the host arrays -> a launch table; the arguments were validated before
CgSets cg_table(int s0, int n, const int32_t *begin, const int32_t *size, const int64_t *off, const int32_t *bias_index) {
    CgSets t;
    t.n = n;
    int base = 0;
    for (int k = 0; k < CG_SETS; ++k) {
        const bool in = k < n;
        t.begin[k] = in ? begin[s0 + k] : 0;
        t.size[k] = in ? size[s0 + k] : 0;
        t.off[k] = in ? off[s0 + k] : 0;
        t.bias[k] = in ? (bias_index ? bias_index[s0 + k] : s0 + k) : 0;
        t.sbase[k] = base;
        base += t.size[k];
    }
    t.n_slot = base;
    return t;
}

int cg_check_sets(int C, int n_proxy, int n_set, const int32_t *begin, const int32_t *size, const int64_t *off) {
    if (!begin || !size || !off) return AOC_ERR_INVALID_ARG;
    if (C < 4 || n_set < 1 || n_proxy < 0) return AOC_ERR_INVALID_ARG;
    if ((C & 3) || C > AOC_MAX_CHANNELS) return AOC_ERR_UNSUPPORTED;
    for (int s = 0; s < n_set; ++s) {
        if (size[s] < 0 || begin[s] < 0 || begin[s] + size[s] > n_proxy || off[s] < 0) return AOC_ERR_INVALID_ARG;
        if (size[s] > AOC_MAX_CLUSTERS) return AOC_ERR_UNSUPPORTED;
    }
    return AOC_OK;
}

}  // namespace

extern "C" {

int aoc_proxy_set_match_argmin(const float *query, int64_t m, int C, const float *proxies, const float *proxy_sqnorm, int n_proxy, int n_set,
                               const int32_t *set_begin_host, const int32_t *set_size_host, const int64_t *set_out_offset_host,
                               const float *set_bias, float *out, int32_t *arg, int64_t out_pixel_stride, int transform, aoc_stream_t stream) {
    if (!query || !proxies || !out || !arg) return AOC_ERR_INVALID_ARG;
    if (m < 1 || out_pixel_stride < 1) return AOC_ERR_INVALID_ARG;
    const int rc = cg_check_sets(C, n_proxy, n_set, set_begin_host, set_size_host, set_out_offset_host);
    if (rc) return rc;
    hipStream_t st = aoc_hip_stream(stream);
    const int64_t n_row_tiles = (m + 15) / 16;
    int64_t grid = (n_row_tiles + 3) / 4;
    if (grid > 2048) grid = 2048;
    for (int s0 = 0; s0 < n_set; s0 += CG_SETS) {
        const CgSets tab = cg_table(s0, n_set - s0 < CG_SETS ? n_set - s0 : CG_SETS, set_begin_host, set_size_host, set_out_offset_host, nullptr);
#define AOC_CG(TM) hipLaunchKernelGGL((cg_set_argmin_kernel<TM>), dim3((unsigned)grid), dim3(256), 0, st, query, m, C, proxies, proxy_sqnorm, tab, set_bias, out, arg, out_pixel_stride, transform)
        if (C == 100) AOC_CG(25); else if (C <= 128) AOC_CG(32); else AOC_CG(64);
#undef AOC_CG
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    return AOC_OK;
}

size_t aoc_proxy_set_match_grad_workspace_bytes(int64_t m, int C, int64_t n_slot) {
    if (m < 1 || C < 1 || n_slot < 0) return 0;
    return aoc_align_up((size_t)n_slot * cg_chunks(m) * (C + 1) * sizeof(float) + 16, 256) + aoc_align_up((size_t)n_slot * sizeof(float) + 16, 256);
}

int aoc_proxy_set_match_grad(const float *grad_out, const float *T, const int32_t *arg, int64_t pixel_stride, const float *query, int64_t m, int C,
                             const float *proxies, int n_proxy, int n_set, const int32_t *set_begin_host, const int32_t *set_size_host,
                             const int64_t *set_out_offset_host, const int32_t *set_bias_index_host, int n_bias, float *grad_query,
                             float *grad_proxies, float *grad_bias, void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_out || !T || !arg || !query || !proxies) return AOC_ERR_INVALID_ARG;
    if (m < 1 || pixel_stride < 1 || n_bias < 0) return AOC_ERR_INVALID_ARG;
    const int rc = cg_check_sets(C, n_proxy, n_set, set_begin_host, set_size_host, set_out_offset_host);
    if (rc) return rc;
    if (grad_bias && (!set_bias_index_host || n_bias < 1)) return AOC_ERR_INVALID_ARG;
    int64_t n_slot = 0;
    for (int s = 0; s < n_set; ++s) {
        if (set_bias_index_host && (set_bias_index_host[s] < 0 || set_bias_index_host[s] >= n_bias)) return AOC_ERR_INVALID_ARG;
        n_slot += set_size_host[s];
    }
    const bool reduce = grad_proxies || grad_bias;
    if (reduce && (!workspace || workspace_bytes < aoc_proxy_set_match_grad_workspace_bytes(m, C, n_slot))) return AOC_ERR_WORKSPACE;
    hipStream_t st = aoc_hip_stream(stream);
    const int n_chunk = cg_chunks(m);
    const int64_t per = (m + n_chunk - 1) / n_chunk;
    float *part = static_cast<float *>(workspace);
    float *slot_sum = reduce ? reinterpret_cast<float *>(static_cast<char *>(workspace) +
                                                         aoc_align_up((size_t)n_slot * n_chunk * (C + 1) * sizeof(float) + 16, 256)) : nullptr;
    const size_t lds = (size_t)CG_SLOTS * (C + 1) * sizeof(float);
    for (int s0 = 0; s0 < n_set; s0 += CG_SETS) {
        // a launch's slots start at 0 of the workspace again: launches on one stream run in order
        const CgSets tab = cg_table(s0, n_set - s0 < CG_SETS ? n_set - s0 : CG_SETS, set_begin_host, set_size_host, set_out_offset_host, set_bias_index_host);
        const int first = s0 == 0;
        if (grad_query)
            hipLaunchKernelGGL(cg_query_grad_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, grad_out, T, arg, pixel_stride, query, m, C, proxies, tab,
                               grad_query, first);
        if (reduce) {
            int smax = 0;
            for (int k = 0; k < tab.n; ++k) smax = tab.size[k] > smax ? tab.size[k] : smax;
            if (smax > 0)
                hipLaunchKernelGGL(cg_partial_kernel, dim3((unsigned)n_chunk, (unsigned)tab.n, (unsigned)((smax + CG_SLOTS - 1) / CG_SLOTS)), dim3(256), lds, st,
                                   grad_out, T, arg, pixel_stride, query, m, C, tab, n_chunk, per, part);
            if (n_proxy > 0 && (grad_proxies || smax > 0))
                hipLaunchKernelGGL(cg_rows_kernel, dim3((unsigned)n_proxy), dim3(256), 0, st, part, n_chunk, C, proxies, tab, grad_proxies, slot_sum, first);
            if (grad_bias)
                hipLaunchKernelGGL(cg_bias_kernel, dim3((unsigned)((n_bias + 63) / 64)), dim3(64), 0, st, slot_sum, tab, n_bias, grad_bias, first);
        }
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    return AOC_OK;
}

size_t aoc_centroid_avg_grad_workspace_bytes(int n_seg, int kmax) {
    if (n_seg < 1 || kmax < 1) return 0;
    return aoc_align_up((size_t)n_seg * kmax * sizeof(int32_t) + 16, 256);
}

int aoc_centroid_avg_grad(const float *grad_proxies, int C, const int32_t *fg_rows, const int32_t *n_fg, const int32_t *seg_offsets,
                          const int32_t *seg_k, const int32_t *labels, int n_seg, int kmax, int64_t rows_capacity, float *grad_pool,
                          int64_t pool_rows, void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_proxies || !fg_rows || !n_fg || !seg_offsets || !seg_k || !labels || !grad_pool) return AOC_ERR_INVALID_ARG;
    if (C < 1 || n_seg < 1 || kmax < 1 || rows_capacity < 1 || pool_rows < 1) return AOC_ERR_INVALID_ARG;
    if (C > AOC_MAX_CHANNELS || kmax > AOC_MAX_CLUSTERS || n_seg > 65535) return AOC_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < aoc_centroid_avg_grad_workspace_bytes(n_seg, kmax)) return AOC_ERR_WORKSPACE;
    hipStream_t st = aoc_hip_stream(stream);
    int32_t *counts = static_cast<int32_t *>(workspace);
    if (hipMemsetAsync(counts, 0, (size_t)n_seg * kmax * sizeof(int32_t), st) != hipSuccess) return AOC_ERR_LAUNCH;
    if (hipMemsetAsync(grad_pool, 0, (size_t)pool_rows * C * sizeof(float), st) != hipSuccess) return AOC_ERR_LAUNCH;
    const int64_t span = rows_capacity < pool_rows ? rows_capacity : pool_rows;      // a segment is no longer than the kept rows
    // the counts cover every packed label (a segment may be as long as the label array); the gather only the positions that can be kept rows
    hipLaunchKernelGGL(cg_count_kernel, dim3((unsigned)((rows_capacity + 255) / 256), (unsigned)n_seg), dim3(256), 0, st, seg_offsets, labels, kmax, rows_capacity,
                       counts);
    hipLaunchKernelGGL(cg_avg_gather_kernel, dim3((unsigned)((span + 3) / 4)), dim3(256), 0, st, grad_proxies, C, fg_rows, n_fg, seg_offsets, seg_k, labels,
                       n_seg, kmax, rows_capacity, counts, grad_pool, pool_rows);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
