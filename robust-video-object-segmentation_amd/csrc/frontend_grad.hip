// Training-time front end of the proto-mask tensor (aocnet.py:270-358): the backward of the masked mean pooling behind the attention
// heads (ATT:134-153), the backward of foreground2background (AEM:9-23), and the aggregation of the five matching outputs into the
// proto-mask tensor with its background channels (aocnet.py:341-358), forward and backward.
//
// All four are streaming kernels: lanes run along hw, every big operand is read once in coalesced rows, the small [O, C] head gradients
// sit in LDS.  One exception: pixel-major labels [hw, n_obj] of the pooling gradient are read as lab[p * n_obj + o], 4 bytes per lane with
// a stride of n_obj floats between lanes -- not coalesced; they are the small operand (O hw floats per 32-channel tile against C hw written)
// and stay in cache across the objects of a pixel.  A thread moves 16 bytes (four consecutive pixels) per access when every row it touches starts on a 16-byte boundary (the
// row length and every stride a multiple of four floats, the base pointers 16-byte aligned); otherwise the same kernel is instantiated with
// one pixel per thread and 4-byte accesses, still coalesced.  Which one runs depends on the shapes and pointers alone and changes no bit.
//
// Every sum runs in a fixed order (ascending object index) without float atomics: the same buffers give the same bits.  Every argmin
// takes the lowest (object, channel) among equal minima, the order of the reference's concatenation (AEM:13-19).  Block sizes and the
// channel tile are first choices, not tuned (STATUS.md).
#include <stdlib.h>

#include "aoc_common.h"

namespace {

constexpr int FG_THREADS = 256;
constexpr int FG_CT = 32;        // channels of grad_emb one pooling-gradient workgroup writes (its [O, FG_CT] weights sit in LDS)
constexpr int FG_OMAX = 32;      // objects the pooling gradient keeps in registers (AOC's limit is 30)

template <int V>
__device__ __forceinline__ void fg_load(const float *__restrict__ p, float (&v)[V]) {
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        v[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void fg_store(float *__restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4) {
        f32x4 t = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4 *>(p) = t;
    } else {
        *p = v[0];
    }
}

inline bool fg_aligned16(const void *p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline unsigned fg_blocks(int64_t n, int v) { return (unsigned)((n + (int64_t)FG_THREADS * v - 1) / ((int64_t)FG_THREADS * v)); }

// The lowest and the second-lowest object of a column, "second" = the lowest among the objects other than the first; among equal values
// the lower object index.  o2 stays -1 for a single object.  +inf columns resolve like any other (object 0, then object 1).
struct FgTwo {
    float m1, m2;
    int o1, o2;
    __device__ __forceinline__ void first(float v) { m1 = v; o1 = 0; m2 = INFINITY; o2 = -1; }
    __device__ __forceinline__ bool add(float v, int o) {       // true: v became the lowest
        if (v < m1) { m2 = m1; o2 = o1; m1 = v; o1 = o; return true; }
        if (v < m2 || o2 < 0) { m2 = v; o2 = o; }
        return false;
    }
};

// ------------------------------------------------------------------------------------------ pooling gradient
// cnt[o] = sum_p l[o,p], cnt[n_obj + o] = sum_p (1 - l[o,p]): thread t adds the pixels t, t + 256, ... in ascending order, then a binary
// tree over the 256 partial sums.  One workgroup per object.
__global__ __launch_bounds__(FG_THREADS) void pool_count_kernel(const float *__restrict__ lab, int64_t hw, int n_obj, int pixel_major,
                                                                 float *__restrict__ cnt) {
    __shared__ float sp[FG_THREADS], sn[FG_THREADS];
    const int o = blockIdx.x, t = threadIdx.x;
    float p = 0.0f, n = 0.0f;
    for (int64_t i = t; i < hw; i += FG_THREADS) {
        const float l = pixel_major ? lab[(size_t)i * n_obj + o] : lab[(size_t)o * hw + i];
        p += l;
        n += 1.0f - l;
    }
    sp[t] = p;
    sn[t] = n;
    __syncthreads();
    for (int s = FG_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) { sp[t] += sp[t + s]; sn[t] += sn[t + s]; }
        __syncthreads();
    }
    if (t == 0) { cnt[o] = sp[0]; cnt[n_obj + o] = sn[0]; }
}

// grad_emb[c, p] = sum_o ( wp[o,c] l[o,p] + wn[o,c] (1 - l[o,p]) ),  wp = gpos / (Np + eps), wn = gneg / (Nn + eps), added in ascending o,
// the positive term of an object before its negative one.  Workgroup = 256 x V pixels times FG_CT channels; the labels of a thread's
// pixels stay in registers over the channel loop.  OM: compile-time bound of the object loop (4, 8 or FG_OMAX).
template <int OM, int V>
__global__ __launch_bounds__(FG_THREADS) void pool_grad_kernel(const float *__restrict__ gpos, const float *__restrict__ gneg,
                                                                const float *__restrict__ lab, const float *__restrict__ cnt, int64_t hw, int C,
                                                                int n_obj, int pixel_major, float eps, float *__restrict__ grad_emb) {
    __shared__ float wp[OM * FG_CT], wn[OM * FG_CT];
    const int c0 = blockIdx.y * FG_CT;
    for (int idx = threadIdx.x; idx < OM * FG_CT; idx += FG_THREADS) {
        const int o = idx / FG_CT, c = idx - o * FG_CT;
        float a = 0.0f, b = 0.0f;
        if (o < n_obj && c0 + c < C) {
            a = gpos[(size_t)o * C + c0 + c] / (cnt[o] + eps);
            if (gneg) b = gneg[(size_t)o * C + c0 + c] / (cnt[n_obj + o] + eps);
        }
        wp[idx] = a;
        wn[idx] = b;
    }
    __syncthreads();
    const int64_t x = ((int64_t)blockIdx.x * FG_THREADS + threadIdx.x) * V;
    if (x >= hw) return;
    float l[OM][V];
#pragma unroll
    for (int o = 0; o < OM; ++o) {
#pragma unroll
        for (int k = 0; k < V; ++k) l[o][k] = 0.0f;
        if (o < n_obj) {
            if (pixel_major) {
#pragma unroll
                for (int k = 0; k < V; ++k) l[o][k] = lab[(size_t)(x + k) * n_obj + o];
            } else {
                fg_load<V>(lab + (size_t)o * hw + x, l[o]);
            }
        }
    }
    const int nc = C - c0 < FG_CT ? C - c0 : FG_CT;
    for (int c = 0; c < nc; ++c) {
        float acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.0f;
#pragma unroll
        for (int o = 0; o < OM; ++o) {
            if (o < n_obj) {
                const float a = wp[o * FG_CT + c], b = wn[o * FG_CT + c];
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    acc[k] += a * l[o][k];
                    if (gneg) acc[k] += b * (1.0f - l[o][k]);
                }
            }
        }
        fg_store<V>(grad_emb + (size_t)(c0 + c) * hw + x, acc);
    }
}

// ------------------------------------------------------------------------------------------ foreground2background gradient
// Per x: the winner over all (o', c) and the winner over the entries of the other objects, recomputed from dis; object o's gradient goes
// to the first unless the first is its own, then to the second.  Every element of grad_dis [n_obj, n_ch, inner] is written (zeros too).
template <int V>
__global__ __launch_bounds__(FG_THREADS) void fg2bg_grad_kernel(const float *__restrict__ grad_out, int64_t gout_stride, const float *__restrict__ dis,
                                                                 int n_obj, int n_ch, int64_t inner, int64_t dis_stride, float *__restrict__ grad_dis,
                                                                 int64_t gdis_stride) {
    const int64_t x = ((int64_t)blockIdx.x * FG_THREADS + threadIdx.x) * V;
    if (x >= inner) return;
    FgTwo two[V];
    int c1[V], c2[V];
    for (int o = 0; o < n_obj; ++o) {
        float v[V], t[V];
        int cv[V];
        for (int c = 0; c < n_ch; ++c) {
            fg_load<V>(dis + (size_t)o * dis_stride + (size_t)c * inner + x, t);
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (c == 0 || t[k] < v[k]) { v[k] = t[k]; cv[k] = c; }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (o == 0) {
                two[k].first(v[k]);
                c1[k] = cv[k];
                c2[k] = 0;
            } else {
                const int was = two[k].o2;
                const int c1_before = c1[k];
                if (two[k].add(v[k], o)) { c2[k] = c1_before; c1[k] = cv[k]; }
                else if (two[k].o2 != was) { c2[k] = cv[k]; }
            }
        }
    }
    float others[V], own[V];      // sum of grad_out over the objects other than o1 (ascending); grad_out of o1
#pragma unroll
    for (int k = 0; k < V; ++k) { others[k] = 0.0f; own[k] = 0.0f; }
    for (int o = 0; o < n_obj; ++o) {
        float g[V];
        fg_load<V>(grad_out + (size_t)o * gout_stride + x, g);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (o == two[k].o1) own[k] = g[k];
            else others[k] += g[k];
        }
    }
    for (int o = 0; o < n_obj; ++o)
        for (int c = 0; c < n_ch; ++c) {
            float r[V];
#pragma unroll
            for (int k = 0; k < V; ++k)
                r[k] = (o == two[k].o1 && c == c1[k]) ? others[k] : (o == two[k].o2 && c == c2[k]) ? own[k] : 0.0f;
            fg_store<V>(grad_dis + (size_t)o * gdis_stride + (size_t)c * inner + x, r);
        }
}

// ------------------------------------------------------------------------------------------ aggregation
// The columns of the proto-mask tensor, aocnet.py:355-358: source s (0 global, 1 cluster, 2 proxy, 3 local, 4 local proxy) holds
// [n_obj, k[s], hw]; its channel j is channel begin[s] + j of feat [n_obj, n_ch, hw]; then the previous-frame mask; then (background on)
// the local background channels and the global background channel.  blockIdx.y = the column: sum k[s] source columns, then the mask.
struct PaCols {
    const float *src[5];
    float *grad[5];          // backward only; NULL = not wanted
    int32_t k[5], begin[5];
    int32_t ch_mask, ch_local_bg, ch_global_bg;     // -1 = background off
    int32_t n_src_cols;
};

__device__ __forceinline__ void pa_column(const PaCols &a, int col, int &s, int &j, int &bg) {
    s = 0;
    j = col;
    while (s < 4 && j >= a.k[s]) { j -= a.k[s]; ++s; }
    bg = s == 0 ? a.ch_global_bg : (s == 3 && a.ch_local_bg >= 0) ? a.ch_local_bg + j : -1;
}

template <int V>
__global__ __launch_bounds__(FG_THREADS) void proto_aggregate_kernel(PaCols a, const float *__restrict__ prev_label, float *__restrict__ feat, int n_obj,
                                                                      int64_t hw, int n_ch) {
    const int64_t x = ((int64_t)blockIdx.x * FG_THREADS + threadIdx.x) * V;
    if (x >= hw) return;
    const int col = blockIdx.y;
    const size_t fstride = (size_t)n_ch * hw;
    float v[V];
    if (col == a.n_src_cols) {                                   // aocnet.py:155: the previous-frame mask
        for (int o = 0; o < n_obj; ++o) {
            fg_load<V>(prev_label + (size_t)o * hw + x, v);
            fg_store<V>(feat + o * fstride + (size_t)a.ch_mask * hw + x, v);
        }
        return;
    }
    int s, j, bg;
    pa_column(a, col, s, j, bg);
    const float *src = a.src[s] + (size_t)j * hw + x;
    const size_t sstride = (size_t)a.k[s] * hw;
    float *dst = feat + (size_t)(a.begin[s] + j) * hw + x;
    if (bg < 0 || n_obj == 1) {
        for (int o = 0; o < n_obj; ++o) {
            fg_load<V>(src + o * sstride, v);
            fg_store<V>(dst + o * fstride, v);
            if (bg >= 0) fg_store<V>(feat + o * fstride + (size_t)bg * hw + x, v);      // AEM:10-11: one object keeps its own map
        }
        return;
    }
    // the arithmetic of fg2bg_kernel / proto_finish_kernel (calibration.hip), term by term
    float m1[V], m2[V];
    int arg[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { m1[k] = INFINITY; m2[k] = INFINITY; arg[k] = -1; }
    for (int o = 0; o < n_obj; ++o) {
        fg_load<V>(src + o * sstride, v);
        fg_store<V>(dst + o * fstride, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float t = fminf(INFINITY, v[k]);
            if (t < m1[k]) { m2[k] = m1[k]; m1[k] = t; arg[k] = o; }
            else if (t < m2[k]) { m2[k] = t; }
        }
    }
    for (int o = 0; o < n_obj; ++o) {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (o == arg[k]) ? m2[k] : m1[k];
        fg_store<V>(feat + o * fstride + (size_t)bg * hw + x, v);
    }
}

template <int V>
__global__ __launch_bounds__(FG_THREADS) void proto_aggregate_grad_kernel(PaCols a, const float *__restrict__ gfeat, const float *__restrict__ feat,
                                                                           int n_obj, int64_t hw, int n_ch) {
    const int64_t x = ((int64_t)blockIdx.x * FG_THREADS + threadIdx.x) * V;
    if (x >= hw) return;
    int s, j, bg;
    pa_column(a, blockIdx.y, s, j, bg);
    if (!a.grad[s]) return;
    const size_t fstride = (size_t)n_ch * hw, sstride = (size_t)a.k[s] * hw;
    const size_t fg_at = (size_t)(a.begin[s] + j) * hw + x;
    float *dst = a.grad[s] + (size_t)j * hw + x;
    float g[V], r[V];
    if (bg < 0 || n_obj == 1) {
        for (int o = 0; o < n_obj; ++o) {
            fg_load<V>(gfeat + o * fstride + fg_at, g);
            if (bg >= 0) {
                fg_load<V>(gfeat + o * fstride + (size_t)bg * hw + x, r);
#pragma unroll
                for (int k = 0; k < V; ++k) g[k] += r[k];
            }
            fg_store<V>(dst + o * sstride, g);
        }
        return;
    }
    const size_t bg_at = (size_t)bg * hw + x;
    FgTwo two[V];
    for (int o = 0; o < n_obj; ++o) {
        fg_load<V>(feat + o * fstride + fg_at, g);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (o == 0) two[k].first(g[k]);
            else two[k].add(g[k], o);
        }
    }
    // o1 receives its own foreground gradient, then the background gradients of all the others in ascending order; o2 the one of o1
    float acc[V], own[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        acc[k] = gfeat[two[k].o1 * fstride + fg_at + k];
        own[k] = gfeat[two[k].o1 * fstride + bg_at + k];
    }
    for (int o = 0; o < n_obj; ++o) {
        fg_load<V>(gfeat + o * fstride + bg_at, g);
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (o != two[k].o1) acc[k] += g[k];
    }
    for (int o = 0; o < n_obj; ++o) {
        fg_load<V>(gfeat + o * fstride + fg_at, g);
#pragma unroll
        for (int k = 0; k < V; ++k) r[k] = (o == two[k].o1) ? acc[k] : (o == two[k].o2) ? g[k] + own[k] : g[k];
        fg_store<V>(dst + o * sstride, r);
    }
}

bool pa_fill(PaCols &a, const float *const *src, float *const *grad, const int *k, int background) {
    int at = 0;
    for (int s = 0; s < 5; ++s) {
        if (k[s] < 1 || k[s] > 4096) return false;
        a.src[s] = src ? src[s] : nullptr;
        a.grad[s] = grad ? grad[s] : nullptr;
        a.k[s] = k[s];
        a.begin[s] = at;
        at += k[s];
    }
    if (k[0] != 1 || k[2] != 1 || k[3] != k[4]) return false;        // AEM:675-681, 393-399 give one channel; both local calls share the radii
    a.n_src_cols = at;
    a.ch_mask = at;
    a.ch_local_bg = background ? at + 1 : -1;
    a.ch_global_bg = background ? at + 1 + k[3] : -1;
    return true;
}

}  // namespace

extern "C" {

size_t aoc_masked_mean_pool_grad_workspace_bytes(int n_obj) { return n_obj < 1 ? 0 : aoc_align_up((size_t)2 * n_obj * sizeof(float), 256); }

int aoc_masked_mean_pool_grad(const float *grad_pos, const float *grad_neg, const float *labels, int64_t hw, int C, int n_obj, int labels_pixel_major,
                              float epsilon, float *grad_emb, void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_pos || !labels || !grad_emb || hw < 1 || C < 1 || n_obj < 1) return AOC_ERR_INVALID_ARG;
    if (n_obj > FG_OMAX) return AOC_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < aoc_masked_mean_pool_grad_workspace_bytes(n_obj)) return AOC_ERR_WORKSPACE;
    float *cnt = static_cast<float *>(workspace);
    hipStream_t st = aoc_hip_stream(stream);
    hipLaunchKernelGGL(pool_count_kernel, dim3(n_obj), dim3(FG_THREADS), 0, st, labels, hw, n_obj, labels_pixel_major, cnt);
    AOC_RETURN_IF_LAUNCH_FAILED();
    const bool vec = hw % 4 == 0 && fg_aligned16(grad_emb) && (labels_pixel_major || fg_aligned16(labels));
    const dim3 grid(fg_blocks(hw, vec ? 4 : 1), (unsigned)((C + FG_CT - 1) / FG_CT));
#define FG_POOL(OM, V)                                                                                                                          \
    hipLaunchKernelGGL((pool_grad_kernel<OM, V>), grid, dim3(FG_THREADS), 0, st, grad_pos, grad_neg, labels, cnt, hw, C, n_obj, labels_pixel_major, \
                       epsilon, grad_emb)
    if (vec) {
        if (n_obj <= 4) FG_POOL(4, 4); else if (n_obj <= 8) FG_POOL(8, 4); else FG_POOL(FG_OMAX, 4);
    } else {
        if (n_obj <= 4) FG_POOL(4, 1); else if (n_obj <= 8) FG_POOL(8, 1); else FG_POOL(FG_OMAX, 1);
    }
#undef FG_POOL
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_fg2bg_grad(const float *grad_out, int64_t grad_out_obj_stride, const float *dis, int n_obj, int n_ch, int64_t inner, int64_t dis_obj_stride,
                   float *grad_dis, int64_t grad_dis_obj_stride, aoc_stream_t stream) {
    if (!grad_out || !dis || !grad_dis || n_obj < 2 || n_ch < 1 || inner < 1 || dis_obj_stride < n_ch * inner || grad_dis_obj_stride < n_ch * inner ||
        grad_out_obj_stride < inner)
        return AOC_ERR_INVALID_ARG;
    const bool vec = inner % 4 == 0 && dis_obj_stride % 4 == 0 && grad_dis_obj_stride % 4 == 0 && grad_out_obj_stride % 4 == 0 && fg_aligned16(grad_out) &&
                     fg_aligned16(dis) && fg_aligned16(grad_dis);
    if (vec)
        hipLaunchKernelGGL((fg2bg_grad_kernel<4>), dim3(fg_blocks(inner, 4)), dim3(FG_THREADS), 0, aoc_hip_stream(stream), grad_out, grad_out_obj_stride, dis,
                           n_obj, n_ch, inner, dis_obj_stride, grad_dis, grad_dis_obj_stride);
    else
        hipLaunchKernelGGL((fg2bg_grad_kernel<1>), dim3(fg_blocks(inner, 1)), dim3(FG_THREADS), 0, aoc_hip_stream(stream), grad_out, grad_out_obj_stride, dis,
                           n_obj, n_ch, inner, dis_obj_stride, grad_dis, grad_dis_obj_stride);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_proto_aggregate_channels(int n_cluster, int n_local, int background) {
    if (n_cluster < 1 || n_local < 1) return AOC_ERR_INVALID_ARG;
    return 1 + n_cluster + 1 + 2 * n_local + 1 + (background ? n_local + 1 : 0);
}

int aoc_proto_aggregate(const float *global_fg, const float *cluster_fg, const float *proxy_fg, const float *local_fg, const float *local_proxy_fg,
                        const float *prev_label, int n_obj, int64_t hw, int n_cluster, int n_local, int background, float *feat, aoc_stream_t stream) {
    if (!global_fg || !cluster_fg || !proxy_fg || !local_fg || !local_proxy_fg || !prev_label || !feat || n_obj < 1 || hw < 1)
        return AOC_ERR_INVALID_ARG;
    const float *src[5] = {global_fg, cluster_fg, proxy_fg, local_fg, local_proxy_fg};
    const int k[5] = {1, n_cluster, 1, n_local, n_local};
    PaCols a;
    if (!pa_fill(a, src, nullptr, k, background)) return AOC_ERR_INVALID_ARG;
    const int n_ch = aoc_proto_aggregate_channels(n_cluster, n_local, background);
    bool vec = hw % 4 == 0 && fg_aligned16(feat) && fg_aligned16(prev_label);
    for (int s = 0; s < 5; ++s) vec = vec && fg_aligned16(src[s]);
    const dim3 grid(fg_blocks(hw, vec ? 4 : 1), (unsigned)(a.n_src_cols + 1));
    if (vec)
        hipLaunchKernelGGL((proto_aggregate_kernel<4>), grid, dim3(FG_THREADS), 0, aoc_hip_stream(stream), a, prev_label, feat, n_obj, hw, n_ch);
    else
        hipLaunchKernelGGL((proto_aggregate_kernel<1>), grid, dim3(FG_THREADS), 0, aoc_hip_stream(stream), a, prev_label, feat, n_obj, hw, n_ch);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_proto_aggregate_grad(const float *grad_feat, const float *feat, int n_obj, int64_t hw, int n_cluster, int n_local, int background,
                             float *grad_global, float *grad_cluster, float *grad_proxy, float *grad_local, float *grad_local_proxy,
                             aoc_stream_t stream) {
    if (!grad_feat || !feat || n_obj < 1 || hw < 1) return AOC_ERR_INVALID_ARG;
    float *grad[5] = {grad_global, grad_cluster, grad_proxy, grad_local, grad_local_proxy};
    const int k[5] = {1, n_cluster, 1, n_local, n_local};
    PaCols a;
    if (!pa_fill(a, nullptr, grad, k, background)) return AOC_ERR_INVALID_ARG;
    const int n_ch = aoc_proto_aggregate_channels(n_cluster, n_local, background);
    bool vec = hw % 4 == 0 && fg_aligned16(grad_feat) && fg_aligned16(feat);
    for (int s = 0; s < 5; ++s) vec = vec && fg_aligned16(grad[s]);
    const dim3 grid(fg_blocks(hw, vec ? 4 : 1), (unsigned)a.n_src_cols);
    if (vec)
        hipLaunchKernelGGL((proto_aggregate_grad_kernel<4>), grid, dim3(FG_THREADS), 0, aoc_hip_stream(stream), a, grad_feat, feat, n_obj, hw, n_ch);
    else
        hipLaunchKernelGGL((proto_aggregate_grad_kernel<1>), grid, dim3(FG_THREADS), 0, aoc_hip_stream(stream), a, grad_feat, feat, n_obj, hw, n_ch);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
