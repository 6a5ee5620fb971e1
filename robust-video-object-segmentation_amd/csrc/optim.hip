// The training update: what train_manager_mm.py:283-284 does between loss.backward() and the next forward --
// torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.TRAIN_CLIP_GRAD_NORM) and optim.SGD(momentum=0.9, nesterov=True).step()
// (train_manager_mm.py:68-72) -- over a TABLE of tensors (include/aoc_hip.h: aoc_mt_tensor).  Six entry points; aoc_amd.optim_train wires them
// into a torch.optim.Optimizer.
//
// The reference puts every parameter into a group of its own (utils/learning.py:24-34), so torch runs its single-tensor path: several small
// launches per tensor over several hundred tensors, about fifteen parameter-sized streams.  Here a step is three launches for the whole model:
//
//   sums     one workgroup of 256 threads per CHUNK of AOC_MT_CHUNK floats of one tensor (the workgroup finds its tensor by a binary search
//            over chunk_begin: the table is read through uniform addresses).  Reads g once.
//   finish   one workgroup: the chunk sums in double, total_norm and the clip coefficient, both left on the device.
//   step     per chunk: reads g (non-temporal: its last use), p and the momentum buffer, writes p and the buffer -- five streams -- and zeroes g
//            in the same pass where asked.  The coefficient is read from device memory: nothing synchronises.
//   (mark    once, after the first step with a momentum: a launch of n_tensors threads sets bit 0 of the records whose buffer now holds a value)
//
// Every pointer is class 4: 16 bytes per lane through the 4-byte-aligned vector types of plane_stream.h, cut from the tensor's FIRST ELEMENT,
// never from the 16-byte grid -- a parameter that is a view at an odd float offset is legal and no summation order depends on an address.
// No float atomics.  The orders:
//   chunk sum   thread t of 256 owns the floats 1024 j + 4 t .. + 3 of the chunk (j = 0 .. 3) and adds their squares in ascending address, each
//               square rounded before it is added (-ffp-contract=off), from 0.0f; the xor butterfly of aoc_wave_sum (32 .. 1); the four wave
//               sums ascending, ((w0 + w1) + w2) + w3; stored as a double
//   finish      thread t adds partial[t], partial[t + 256], ... ascending in double from 0.0; the xor butterfly (32 .. 1) in double; the four
//               wave sums ascending
#include "plane_stream.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_VEC = AOC_MT_CHUNK / (4 * MT_THREADS);          // float4s per thread and stream
static_assert(AOC_MT_CHUNK % (4 * MT_THREADS) == 0, "a chunk is a whole number of float4 rows of the workgroup");

// the tensor that owns chunk c: the LAST record with chunk_begin <= c (an empty tensor shares its chunk_begin with its successor, so the last
// one is never empty for c < n_chunks).  c is uniform over the workgroup, and so is every address read here.
__device__ __forceinline__ int mt_find(const aoc_mt_tensor *__restrict__ table, int n_tensors, int64_t c) {
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk_begin <= c) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct MtSpan { int tensor; int64_t base; int64_t n; };           // the chunk's first float inside its tensor and the tensor's size

__device__ __forceinline__ MtSpan mt_span(const aoc_mt_tensor *__restrict__ table, int n_tensors) {
    const int64_t c = blockIdx.x;
    MtSpan s;
    s.tensor = mt_find(table, n_tensors, c);
    s.base = (c - table[s.tensor].chunk_begin) * AOC_MT_CHUNK;
    s.n = table[s.tensor].n;
    return s;
}

// 16 bytes when the four floats at p + o lie inside [0, n), else the ones that do (the rest are `fill`)
__device__ __forceinline__ f32x4 mt_load(const float *p, int64_t o, int64_t n, bool stream, float fill = 0.0f) {
    if (o + 4 <= n) return stream ? aoc_stream_load4(p + o) : aoc_load4(p + o);
    f32x4 v = {fill, fill, fill, fill};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (o + k < n) v[k] = stream ? __builtin_nontemporal_load(p + o + k) : p[o + k];
    return v;
}
__device__ __forceinline__ void mt_store(float *p, int64_t o, int64_t n, const f32x4 v) {
    if (o + 4 <= n) { aoc_store4_a4(p + o, v); return; }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (o + k < n) p[o + k] = v[k];
}

// ------------------------------------------------------------------------------------------ 1: sum of squares per chunk
__global__ __launch_bounds__(MT_THREADS) void mt_sumsq_kernel(const aoc_mt_tensor *__restrict__ table, int n_tensors, double *__restrict__ partial) {
    __shared__ float wsum[4];
    const MtSpan s = mt_span(table, n_tensors);
    const float *g = table[s.tensor].grad;
    float acc = 0.0f;
    if (g) {                                                      // uniform
        f32x4 v[MT_VEC];
#pragma unroll
        for (int j = 0; j < MT_VEC; ++j) v[j] = mt_load(g, s.base + j * (4 * MT_THREADS) + 4 * threadIdx.x, s.n, false);
#pragma unroll
        for (int j = 0; j < MT_VEC; ++j) acc = aoc_dot4(acc, v[j], v[j]);     // the floats past the tensor's end are 0: adding +0.0f changes nothing
    }
    acc = aoc_wave_sum(acc);
    if (aoc_lane() == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (double)(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
}

// ------------------------------------------------------------------------------------------ 2: the norm and the coefficient
__global__ __launch_bounds__(MT_THREADS) void mt_finish_kernel(const double *__restrict__ partial, int64_t n_chunks, float max_norm,
                                                               float *__restrict__ total_norm, float *__restrict__ coef) {
    __shared__ double wsum[4];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_chunks; i += MT_THREADS) acc += partial[i];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (aoc_lane() == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        const float norm = (float)sqrt(sum);
        const float c = max_norm / (norm + 1e-6f);
        if (total_norm) total_norm[0] = norm;
        if (coef) coef[0] = c > 1.0f ? 1.0f : c;                  // torch.clamp(max=1.0): a NaN stays a NaN
    }
}

// ------------------------------------------------------------------------------------------ 3: g *= coef
__global__ __launch_bounds__(MT_THREADS) void mt_scale_kernel(const aoc_mt_tensor *__restrict__ table, int n_tensors, const float *__restrict__ coef) {
    const MtSpan s = mt_span(table, n_tensors);
    float *g = table[s.tensor].grad;
    if (!g) return;
    const float c = coef[0];
    f32x4 v[MT_VEC];
#pragma unroll
    for (int j = 0; j < MT_VEC; ++j) v[j] = mt_load(g, s.base + j * (4 * MT_THREADS) + 4 * threadIdx.x, s.n, false);
#pragma unroll
    for (int j = 0; j < MT_VEC; ++j) mt_store(g, s.base + j * (4 * MT_THREADS) + 4 * threadIdx.x, s.n, v[j] * c);
}

// g = 0 (zero_grad(set_to_none=False) as one launch)
__global__ __launch_bounds__(MT_THREADS) void mt_zero_kernel(const aoc_mt_tensor *__restrict__ table, int n_tensors) {
    const MtSpan s = mt_span(table, n_tensors);
    float *g = table[s.tensor].grad;
    if (!g) return;
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < MT_VEC; ++j) mt_store(g, s.base + j * (4 * MT_THREADS) + 4 * threadIdx.x, s.n, z);
}

// ------------------------------------------------------------------------------------------ 4: the update
struct MtStep { float lr, momentum, one_minus_dampening; int nesterov, zero_grad; };

// torch's _single_tensor_sgd behind clip_grad_norm_, one rounding per operation (-ffp-contract=off; the vector operators are element-wise)
template <bool MOMENTUM>
__global__ __launch_bounds__(MT_THREADS) void mt_sgd_kernel(const aoc_mt_tensor *__restrict__ table, int n_tensors, const float *__restrict__ coef,
                                                            const float *__restrict__ lr_dev, const MtStep a) {
    const MtSpan s = mt_span(table, n_tensors);
    const aoc_mt_tensor &T = table[s.tensor];
    float *g = T.grad;
    if (!g) return;                                               // no gradient: parameter and buffer stay as they are
    float *p = T.param, *b = T.momentum;
    const float c = coef ? coef[0] : 1.0f;
    const float wd = T.weight_decay;
    const float neg_lr = -(lr_dev ? lr_dev[s.tensor] : a.lr);
    const bool has_b = MOMENTUM && (T.flags & AOC_MT_HAS_MOMENTUM) != 0;
    f32x4 gv[MT_VEC], pv[MT_VEC], bv[MT_VEC];
#pragma unroll
    for (int j = 0; j < MT_VEC; ++j) {
        const int64_t o = s.base + j * (4 * MT_THREADS) + 4 * threadIdx.x;
        gv[j] = mt_load(g, o, s.n, true);
        pv[j] = mt_load(p, o, s.n, false);
        if (has_b) bv[j] = mt_load(b, o, s.n, false);
    }
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < MT_VEC; ++j) {
        const int64_t o = s.base + j * (4 * MT_THREADS) + 4 * threadIdx.x;
        f32x4 d = gv[j] * c;
        if (wd != 0.0f) d = d + pv[j] * wd;
        f32x4 v = d;
        if (MOMENTUM) {
            const f32x4 nb = has_b ? bv[j] * a.momentum + d * a.one_minus_dampening : d;
            v = a.nesterov ? d + nb * a.momentum : nb;
            mt_store(b, o, s.n, nb);
        }
        mt_store(p, o, s.n, pv[j] + v * neg_lr);
        if (a.zero_grad) mt_store(g, o, s.n, z);
    }
}

// bit 0 of every record whose buffer the step has just written
__global__ void mt_mark_kernel(aoc_mt_tensor *__restrict__ table, int n_tensors) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_tensors && table[i].grad && table[i].n > 0) table[i].flags |= AOC_MT_HAS_MOMENTUM;
}

// ------------------------------------------------------------------------------------------ host
constexpr int64_t MT_MAX_CHUNKS = 0x7fffffff;

// the scalars of every entry, then the host mirror where the caller has one: sizes, the prefix, the pointers the kernels will follow
int mt_check(const aoc_mt_tensor *table, const aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, bool need_param, bool need_momentum) {
    if (n_tensors < 0 || n_chunks < 0 || n_chunks > MT_MAX_CHUNKS) return AOC_ERR_INVALID_ARG;
    if ((n_tensors > 0 && !table) || (n_tensors == 0 && n_chunks != 0)) return AOC_ERR_INVALID_ARG;
    if (!table_host) return AOC_OK;
    int64_t at = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const aoc_mt_tensor &t = table_host[i];
        if (t.n < 0 || t.chunk_begin != at) return AOC_ERR_INVALID_ARG;
        at += (t.n + AOC_MT_CHUNK - 1) / AOC_MT_CHUNK;
        if (at > MT_MAX_CHUNKS) return AOC_ERR_INVALID_ARG;
        if (t.n > 0 && t.grad && ((need_param && !t.param) || (need_momentum && !t.momentum))) return AOC_ERR_INVALID_ARG;
    }
    return at == n_chunks ? AOC_OK : AOC_ERR_INVALID_ARG;
}

int sgd_check(float lr, float momentum, float dampening, int nesterov) {
    (void)lr;
    if (!(momentum >= 0.0f)) return AOC_ERR_INVALID_ARG;
    if (nesterov && (momentum == 0.0f || dampening != 0.0f)) return AOC_ERR_INVALID_ARG;      // torch: "Nesterov momentum requires a momentum and zero dampening"
    return AOC_OK;
}

size_t partial_bytes(int64_t n_chunks) { return (size_t)(n_chunks > 0 ? n_chunks : 1) * sizeof(double); }

}  // namespace

extern "C" {

int64_t aoc_mt_chunks(int64_t n) { return n > 0 ? (n + AOC_MT_CHUNK - 1) / AOC_MT_CHUNK : 0; }

int aoc_grad_sumsq_partials(const aoc_mt_tensor *table, const aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, double *partial,
                            aoc_stream_t stream) {
    const int rc = mt_check(table, table_host, n_tensors, n_chunks, false, false);
    if (rc != AOC_OK) return rc;
    if (n_chunks == 0) return AOC_OK;
    if (!partial || (reinterpret_cast<uintptr_t>(partial) & 7)) return AOC_ERR_INVALID_ARG;
    hipLaunchKernelGGL(mt_sumsq_kernel, dim3((unsigned)n_chunks), dim3(MT_THREADS), 0, aoc_hip_stream(stream), table, n_tensors, partial);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_grad_norm_finish(const double *partial, int64_t n_chunks, float max_norm, float *total_norm, float *coef, aoc_stream_t stream) {
    if (n_chunks < 0 || n_chunks > MT_MAX_CHUNKS || (n_chunks > 0 && (!partial || (reinterpret_cast<uintptr_t>(partial) & 7)))) return AOC_ERR_INVALID_ARG;
    if (!total_norm && !coef) return AOC_ERR_INVALID_ARG;
    hipLaunchKernelGGL(mt_finish_kernel, dim3(1), dim3(MT_THREADS), 0, aoc_hip_stream(stream), partial, n_chunks, max_norm, total_norm, coef);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_multi_tensor_scale(const aoc_mt_tensor *table, const aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, const float *coef,
                           aoc_stream_t stream) {
    const int rc = mt_check(table, table_host, n_tensors, n_chunks, false, false);
    if (rc != AOC_OK) return rc;
    if (!coef) return AOC_ERR_INVALID_ARG;
    if (n_chunks == 0) return AOC_OK;
    hipLaunchKernelGGL(mt_scale_kernel, dim3((unsigned)n_chunks), dim3(MT_THREADS), 0, aoc_hip_stream(stream), table, n_tensors, coef);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_multi_tensor_zero(const aoc_mt_tensor *table, const aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, aoc_stream_t stream) {
    const int rc = mt_check(table, table_host, n_tensors, n_chunks, false, false);
    if (rc != AOC_OK) return rc;
    if (n_chunks == 0) return AOC_OK;
    hipLaunchKernelGGL(mt_zero_kernel, dim3((unsigned)n_chunks), dim3(MT_THREADS), 0, aoc_hip_stream(stream), table, n_tensors);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_sgd_step(aoc_mt_tensor *table, aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, const float *coef, float lr, const float *lr_dev,
                 float momentum, float dampening, int nesterov, int zero_grad, aoc_stream_t stream) {
    int rc = sgd_check(lr, momentum, dampening, nesterov);
    if (rc != AOC_OK) return rc;
    const bool mom = momentum != 0.0f;
    if ((rc = mt_check(table, table_host, n_tensors, n_chunks, true, mom)) != AOC_OK) return rc;
    if (n_chunks == 0) return AOC_OK;
    const MtStep a = {lr, momentum, 1.0f - dampening, nesterov != 0, zero_grad != 0};
    if (mom) hipLaunchKernelGGL(mt_sgd_kernel<true>, dim3((unsigned)n_chunks), dim3(MT_THREADS), 0, aoc_hip_stream(stream), table, n_tensors, coef, lr_dev, a);
    else hipLaunchKernelGGL(mt_sgd_kernel<false>, dim3((unsigned)n_chunks), dim3(MT_THREADS), 0, aoc_hip_stream(stream), table, n_tensors, coef, lr_dev, a);
    AOC_RETURN_IF_LAUNCH_FAILED();
    if (!mom) return AOC_OK;
    // The buffers of the tensors that had a gradient hold a value now.  With a host mirror the launch is skipped once every such record says
    // so already (every step but the first), and the mirror is kept equal to the device table.
    bool need_mark = table_host == nullptr;
    for (int i = 0; table_host && i < n_tensors; ++i)
        if (table_host[i].grad && table_host[i].n > 0 && !(table_host[i].flags & AOC_MT_HAS_MOMENTUM)) {
            table_host[i].flags |= AOC_MT_HAS_MOMENTUM;
            need_mark = true;
        }
    if (need_mark) {
        hipLaunchKernelGGL(mt_mark_kernel, dim3((unsigned)((n_tensors + 255) / 256)), dim3(256), 0, aoc_hip_stream(stream), table, n_tensors);
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    return AOC_OK;
}

size_t aoc_clip_sgd_step_workspace_bytes(int64_t n_chunks) { return n_chunks < 0 || n_chunks > MT_MAX_CHUNKS ? 0 : partial_bytes(n_chunks) + 16; }

int aoc_clip_sgd_step(aoc_mt_tensor *table, aoc_mt_tensor *table_host, int n_tensors, int64_t n_chunks, float max_norm, float *total_norm, float lr,
                      const float *lr_dev, float momentum, float dampening, int nesterov, int zero_grad, void *workspace, size_t workspace_bytes,
                      aoc_stream_t stream) {
    int rc = sgd_check(lr, momentum, dampening, nesterov);
    if (rc != AOC_OK) return rc;
    if ((rc = mt_check(table, table_host, n_tensors, n_chunks, true, momentum != 0.0f)) != AOC_OK) return rc;
    if (!total_norm) return AOC_ERR_INVALID_ARG;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7)) return AOC_ERR_INVALID_ARG;
    if (workspace_bytes < aoc_clip_sgd_step_workspace_bytes(n_chunks)) return AOC_ERR_WORKSPACE;
    double *partial = static_cast<double *>(workspace);
    float *coef = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + partial_bytes(n_chunks));
    // every argument is validated above: the calls below can only fail in a launch
    if ((rc = aoc_grad_sumsq_partials(table, table_host, n_tensors, n_chunks, partial, stream)) != AOC_OK) return rc;
    if ((rc = aoc_grad_norm_finish(partial, n_chunks, max_norm, total_norm, coef, stream)) != AOC_OK) return rc;
    return aoc_sgd_step(table, table_host, n_tensors, n_chunks, coef, lr, lr_dev, momentum, dampening, nesterov, zero_grad, stream);
}

}  // extern "C"
