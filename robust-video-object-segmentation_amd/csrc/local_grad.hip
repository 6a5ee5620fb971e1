// Training-time local matching: the argmin forward and the gradient kernels of local_matching / local_matching_proxy (AEM:968-1060 over
// AEM:921-963, the parallel path; the reference's for-loop path shadows both embeddings with its loop variables and is not mirrored).
//
// With d = |q|^2 + |p|^2 - 2 q.p and T = 2 sigmoid(d + b) - 1:  dT/dd = dT/db = (1 - T^2) / 2,  dd/dq = 2 (q - p*),  dd/dp* = 2 (p* - q),
// p* the previous-frame pixel torch.min picks in a channel's window (the first in row-major window order on ties).  The reference unfolds
// the previous frame into [HW, C, (2R+1)^2] and keeps that and the masked distance volume for autograd; here the backward needs the
// winning pixel per (object, channel, query pixel), the saved T and the two maps.
//
//   g[o, ch, i]   = (grad_out * 0.5f) * (1.0f - T * T)                                  aoc_transform_gate (aoc_common.h)
//   grad_query[i] = sum over (o, ch), ascending, of (2 g) * (q_i - p_arg)               a gather
//   grad_prev[j]  = sum over the (i, o, ch) with arg = j, ascending i, then o, then ch, of (2 g) * (p_j - q_i)
//                   also a gather: only query pixels within the window of j can have chosen it, so a workgroup per previous-frame
//                   pixel scans their arg entries in that order and adds the matches as it meets them
//   grad_bias[o]  = sum over i, ascending, (within a pixel over ch, ascending) of g
//
// Determinism: no float atomic anywhere and no integer atomic in the backward; every sum is a fixed sequence of the buffers' contents.
// The forward's LDS atomic is a 64-bit integer minimum, which is order-independent.
//
// Kernel shapes are first choices (one workgroup per previous-frame pixel, one wave per query pixel, consecutive channels that share a
// winner are NOT merged): nothing here has been tuned on a profile yet.
#include "local_window.h"

namespace {

constexpr int LG_MAX_WINDOW = 31;
constexpr int LG_BIAS_PIX = 256;    // pixels per first-stage block of the bias sum

// Monotone uint32 image of a float: a < b  <=>  image(a) < image(b) (distances can round slightly below zero, so the plain bit pattern
// would not do).  Negative floats have all bits flipped, the others the sign bit set.
__device__ __forceinline__ uint32_t lg_image(float d) {
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lg_unimage(uint32_t m) { return __uint_as_float((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m); }
// key = image(distance) << 32 | previous-frame pixel: the 64-bit minimum is the smallest distance and, among equals, the lowest pixel
__device__ __forceinline__ unsigned long long lg_key(float d, uint32_t pix) { return ((unsigned long long)lg_image(d) << 32) | pix; }
__device__ __forceinline__ unsigned long long lg_pad_key() { return lg_key(AOC_PAD_DISTANCE, 0xffffffffu); }

// prefix-min over the rings of one (query pixel, object) -> the nested windows' value and winner; channel order [max, r_0, r_1, ...]
// (AEM:1034-1046).  keys: this pixel's [ring][object] keys.
__device__ __forceinline__ void lg_emit(const unsigned long long *keys, int nr, int n_obj, int o, const float *obj_bias, int transform,
                                        float *out, int32_t *arg, int H, int W, int oy, int ox) {
    const float bias = obj_bias ? obj_bias[o] : 0.0f;
    unsigned long long run = ~0ull;
    for (int cls = 0; cls < nr; ++cls) {
        const unsigned long long v = keys[cls * n_obj + o];
        run = v < run ? v : run;
        const float d = lg_unimage((uint32_t)(run >> 32));
        const int ch = (cls == nr - 1) ? 0 : cls + 1;
        const size_t at = (((size_t)o * nr + ch) * H + oy) * W + ox;
        out[at] = transform ? aoc_proto_transform(d, bias) : d;   // AEM:1049
        arg[at] = d >= AOC_PAD_DISTANCE ? -1 : (int32_t)(uint32_t)run;
    }
}

// local_window_reg_kernel (local_match.hip) in fp32 with a position beside every minimum: the same 2 x 8 query tile, the same register
// operands, the same four fmaf chains and shuffle folds of the norms, the same v_mfma_f32_16x16x4_f32 chain and (q2 + y2) - 2 acc, so the
// values are that kernel's bit for bit.  Its float ds_min into one array per wave is replaced by a 64-bit integer minimum into ONE key
// array per workgroup (LDS atomics are workgroup-wide): 16 queries x n_radii x n_obj x 8 B, 30 KB at most.
template <int TMAX>
__global__ __launch_bounds__(256) void lg_window_reg_argmin_kernel(const float *__restrict__ query, const float *__restrict__ prev,
                                                                    const uint32_t *__restrict__ right_bits, int H, int W, LocalRadii radii,
                                                                    const float *__restrict__ obj_bias, int n_obj, float *__restrict__ out,
                                                                    int32_t *__restrict__ arg, int transform, int rate) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int C = 4 * TMAX;
    constexpr int NP = TMAX / 4;                        // float4 pieces per lane
    constexpr bool TAIL = (TMAX % 4) != 0;              // TMAX = 25: one more channel per lane (16 NP + g)
    static_assert(TMAX % 4 == 0 || TMAX % 4 == 1, "lane g takes pieces g, g + 4, ... and at most one tail channel");
    const int nr = radii.n;
    const int RA = radii.r[nr - 1];                     // window half-size in atrous units
    const int R = RA * rate;
    const int NC = 8 + 2 * R;                           // candidate columns of the block
    const int NG = (NC + 15) / 16;
    const int n_keys = 16 * nr * n_obj;
    const int lane = aoc_lane(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    int32_t *lcls = reinterpret_cast<int32_t *>(lds);                                       // [RA + 1] ring -> class
    unsigned long long *lkey = reinterpret_cast<unsigned long long *>(lds + 32);             // [16 queries][n_radii][n_obj]
    const int x0 = blockIdx.x * 8;
    const int y0 = blockIdx.y * 2;

    for (int i = threadIdx.x; i < n_keys; i += blockDim.x) lkey[i] = lg_pad_key();           // AEM:1032 pad
    if ((int)threadIdx.x <= RA) {            // lw_ring_classes, written out as in local_window_reg_kernel: this kernel stays that one's copy, line by line
        int c = 0;
        while (radii.r[c] < (int)threadIdx.x) ++c;
        lcls[threadIdx.x] = c;
    }

    // this lane's 4 NP (+1) channels of a pixel row
    auto load_row = [&](const float *__restrict__ p, float (&v)[TMAX]) {
        const float4 *p4 = reinterpret_cast<const float4 *>(p) + g;
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const float4 x = p4[4 * u];
            v[4 * u] = x.x; v[4 * u + 1] = x.y; v[4 * u + 2] = x.z; v[4 * u + 3] = x.w;
        }
        if constexpr (TAIL) v[4 * NP] = p[16 * NP + g];
    };
    // sum of squares of the lane's channels, reduced over the four lanes (g) that share a pixel: local_window_reg_kernel's order
    auto sq_norm = [&](const float (&v)[TMAX]) -> float {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int t = 0; t + 3 < TMAX; t += 4) {
            s0 = __builtin_fmaf(v[t], v[t], s0); s1 = __builtin_fmaf(v[t + 1], v[t + 1], s1);
            s2 = __builtin_fmaf(v[t + 2], v[t + 2], s2); s3 = __builtin_fmaf(v[t + 3], v[t + 3], s3);
        }
        if constexpr (TAIL) s0 = __builtin_fmaf(v[TMAX - 1], v[TMAX - 1], s0);
        float s = (s0 + s1) + (s2 + s3);
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        return s;
    };

    // query i = 0..15 is pixel (y0 + i / 8, x0 + i % 8); as an MFMA row, lane (j, g) supplies query j; as an MFMA result, register r of
    // lane (j, g) is query 4 g + r against candidate j: its row y0 + g / 2 is the same for the lane's four results
    float a[TMAX], q2r[4];
    {   // A operand (pixels beyond the map re-read the last row / column; they are never stored)
        load_row(query + ((size_t)min(y0 + (j >> 3), H - 1) * W + min(x0 + (j & 7), W - 1)) * C, a);
        const float q2 = sq_norm(a);
#pragma unroll
        for (int r = 0; r < 4; ++r) q2r[r] = __shfl(q2, g * 4 + r);
    }
    __syncthreads();                                    // lcls, lkey
    const int qy = y0 + (g >> 1);                       // query row of this lane's results
    const int qc0 = 4 * (g & 1);                        // ... and their first column (relative to x0)

    // candidate rows cy in [y0 - R, y0 + 1 + R] (clipped); this wave takes cy_beg + wave, + 4, ...
    const int cy_beg = max(0, y0 - R), cy_end = min(H - 1, y0 + 1 + R);
    const int cy_first = cy_beg + wave;
    const int n_items = cy_first <= cy_end ? ((cy_end - cy_first) / 4 + 1) * NG : 0;

    float b0[TMAX], b1[TMAX];
    uint32_t bits0 = 0u, bits1 = 0u, pix0 = 0u, pix1 = 0u;
    int cy_ld = cy_first, gi_ld = 0;                    // item -> (cy, gi), advanced incrementally (wave-uniform)
    auto issue = [&](float (&b)[TMAX], uint32_t &bits, uint32_t &pixel) {
        const int c = gi_ld * 16 + j, cx = x0 - R + c;
        const bool ok = c < NC && cx >= 0 && cx < W;
        const int cxc = min(max(cx, 0), W - 1);                       // clamped address, selected afterwards: the loads stay branch-free
        const size_t pix = (size_t)cy_ld * W + cxc;
        load_row(prev + pix * C, b);
        const uint32_t raw = right_bits[pix];
        bits = ok ? (raw & ~AOC_ROW_KEPT_BIT) : 0u;                    // AEM:1023-1028 (pad 0)
        pixel = (uint32_t)pix;                                         // used only where ok: the pixel itself then
        if (++gi_ld == NG) { gi_ld = 0; cy_ld += 4; }
    };
    int cy_cur = cy_first, gi_cur = 0;
    auto compute = [&](float (&b)[TMAX], uint32_t bits, uint32_t pixel) {
        const float y2 = sq_norm(b);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TMAX; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], acc, 0, 0, 0);
        int ady = cy_cur - qy;
        ady = ady < 0 ? -ady : ady;
        bool row_on = ady <= R && qy < H;
        int aky = ady;
        if (rate != 1) { aky = ady / rate; row_on = row_on && aky * rate == ady; }
        const int cq = gi_cur * 16 + j - R - qc0;                      // cx - qx for r = 0
        if (bits != 0u && row_on) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int dx = cq - r;
                dx = dx < 0 ? -dx : dx;
                bool on = dx <= R && x0 + qc0 + r < W;
                int akx = dx;
                if (rate != 1) { akx = dx / rate; on = on && akx * rate == dx; }
                if (on) {
                    const float d = (q2r[r] + y2) - 2.0f * acc[r];     // AEM:961
                    const unsigned long long key = lg_key(d, pixel);
                    const int cls = lcls[max(aky, akx)];
                    uint32_t bb = bits;
                    while (bb) {                                        // AEM:1032 where(mask, d, pad)
                        const int o = __builtin_ctz(bb);
                        bb &= bb - 1;
                        if (o < n_obj) atomicMin(&lkey[((g * 4 + r) * nr + cls) * n_obj + o], key);
                    }
                }
            }
        }
        if (++gi_cur == NG) { gi_cur = 0; cy_cur += 4; }
    };

    if (n_items > 0) issue(b0, bits0, pix0);
    for (int it = 0; it < n_items; it += 2) {
        if (it + 1 < n_items) issue(b1, bits1, pix1);
        compute(b0, bits0, pix0);
        if (it + 1 < n_items) {
            if (it + 2 < n_items) issue(b0, bits0, pix0);
            compute(b1, bits1, pix1);
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 16 * n_obj; idx += blockDim.x) {
        const int qi = idx / n_obj, o = idx - qi * n_obj;
        const int oy = y0 + (qi >> 3), ox = x0 + (qi & 7);
        if (ox >= W || oy >= H) continue;
        lg_emit(lkey + (size_t)qi * nr * n_obj, nr, n_obj, o, obj_bias, transform, out, arg, H, W, oy, ox);
    }
}

// Every other width (C % 4 == 0, C <= 128): one workgroup per query pixel, a thread per window position.  Norms and the dot product are
// plain sequential sums (held to the float64 bound, not to aoc_local_window_match_ex's bits).
__global__ __launch_bounds__(256) void lg_window_argmin_kernel(const float *__restrict__ query, const float *__restrict__ prev,
                                                                const uint32_t *__restrict__ right_bits, int H, int W, int C, LocalRadii radii,
                                                                const float *__restrict__ obj_bias, int n_obj, float *__restrict__ out,
                                                                int32_t *__restrict__ arg, int transform, int rate) {
    __shared__ __attribute__((aligned(16))) float lq[128];
    __shared__ int32_t lcls[LG_MAX_WINDOW + 1];
    __shared__ unsigned long long lkey[LW_MAX_RADII * AOC_MAX_OBJECTS];
    const int nr = radii.n;
    const int RA = radii.r[nr - 1];
    const int y = blockIdx.y, x = blockIdx.x;
    const int tid = threadIdx.x;
    for (int i = tid; i < nr * n_obj; i += blockDim.x) lkey[i] = lg_pad_key();               // AEM:1032 pad
    lw_ring_classes(radii, RA, lcls);
    for (int c = tid; c < C; c += blockDim.x) lq[c] = query[((size_t)y * W + x) * C + c];
    __syncthreads();
    float q2 = 0.0f;
    for (int c = 0; c < C; ++c) q2 += lq[c] * lq[c];
    const int side = 2 * RA + 1;
    const uint32_t obj_mask = n_obj >= 32 ? 0xffffffffu : ((1u << n_obj) - 1u);
    for (int pos = tid; pos < side * side; pos += blockDim.x) {
        const int wy = pos / side - RA, wx = pos % side - RA;
        const int cy = y + wy * rate, cx = x + wx * rate;
        if (cy < 0 || cy >= H || cx < 0 || cx >= W) continue;                                // AEM:1023-1028 (pad 0)
        const size_t pix = (size_t)cy * W + cx;
        uint32_t bits = right_bits[pix] & ~AOC_ROW_KEPT_BIT & obj_mask;
        if (bits == 0u) continue;
        const float4 *p4 = reinterpret_cast<const float4 *>(prev + pix * C);
        float p2 = 0.0f, dot = 0.0f;
        for (int t = 0; t < (C >> 2); ++t) {
            const float4 v = p4[t];
            const float4 q = *reinterpret_cast<const float4 *>(lq + 4 * t);
            p2 += v.x * v.x; p2 += v.y * v.y; p2 += v.z * v.z; p2 += v.w * v.w;
            dot += q.x * v.x; dot += q.y * v.y; dot += q.z * v.z; dot += q.w * v.w;
        }
        const float d = (q2 + p2) - 2.0f * dot;                                              // AEM:961
        const unsigned long long key = lg_key(d, (uint32_t)pix);
        const int awy = wy < 0 ? -wy : wy, awx = wx < 0 ? -wx : wx;
        const int cls = lcls[max(awy, awx)];
        while (bits) {                                                                       // AEM:1032 where(mask, d, pad)
            const int o = __builtin_ctz(bits);
            bits &= bits - 1;
            atomicMin(&lkey[cls * n_obj + o], key);
        }
    }
    __syncthreads();
    if (tid < n_obj) lg_emit(lkey, nr, n_obj, tid, obj_bias, transform, out, arg, H, W, y, x);
}

// ------------------------------------------------------------------------------------------ backward
// g and a checked copy of arg, pixel-major [i][o * n_radii + ch] for the two gathers (an arg outside the map or the window becomes -1,
// its g zero)
__global__ __launch_bounds__(256) void lg_gate_kernel(const float *__restrict__ grad_out, const float *__restrict__ T, const int32_t *__restrict__ arg,
                                                       int H, int W, int P, int window, float *__restrict__ gbuf, int32_t *__restrict__ abuf) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t hw = (int64_t)H * W;
    if (idx >= hw * P) return;
    const int p = (int)(idx / hw);
    const int i = (int)(idx - (int64_t)p * hw);
    int32_t a = arg[idx];
    bool ok = a >= 0 && a < hw;
    if (ok) {
        int dy = a / W - i / W, dx = a % W - i % W;
        dy = dy < 0 ? -dy : dy;
        dx = dx < 0 ? -dx : dx;
        ok = dy <= window && dx <= window;
    }
    gbuf[(int64_t)i * P + p] = ok ? aoc_transform_gate(grad_out[idx], T[idx]) : 0.0f;
    abuf[(int64_t)i * P + p] = ok ? a : -1;
}

// One wave per query pixel: acc += (2 g) * (q - p_arg) over (o, ch), ascending.
__global__ __launch_bounds__(64) void lg_query_kernel(const float *__restrict__ gbuf, const int32_t *__restrict__ abuf, const float *__restrict__ query,
                                                      const float *__restrict__ prev, int C, int P, float *__restrict__ grad_query) {
    __shared__ float lg2[LW_MAX_RADII * AOC_MAX_OBJECTS];
    __shared__ int32_t la[LW_MAX_RADII * AOC_MAX_OBJECTS];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    for (int p = lane; p < P; p += 64) {
        lg2[p] = 2.0f * gbuf[i * P + p];
        la[p] = abuf[i * P + p];
    }
    __syncthreads();
    for (int c = lane; c < C; c += 64) {
        const float q = query[i * C + c];
        float acc = 0.0f;
        for (int p = 0; p < P; ++p) {
            const int32_t a = la[p];
            if (a >= 0) acc += lg2[p] * (q - prev[(int64_t)a * C + c]);
        }
        grad_query[i * C + c] = acc;
    }
}

// One workgroup per previous-frame pixel j.  The entries (query pixel i in the window of j, row-major; then o; then ch) are looked at
// 256 at a time; the matches of a step keep their order (ballot ranks inside a wave, the waves in order) and thread c < C adds them one
// after the other: acc += (2 g) * (p_j[c] - q_i[c]).
__global__ __launch_bounds__(256) void lg_prev_kernel(const float *__restrict__ gbuf, const int32_t *__restrict__ abuf, const float *__restrict__ query,
                                                      const float *__restrict__ prev, int H, int W, int C, int P, int window,
                                                      float *__restrict__ grad_prev) {
    __shared__ int32_t lcnt[4];
    __shared__ int32_t lpix[256];
    __shared__ float lg2[256];
    const int j = blockIdx.x;
    const int jy = j / W, jx = j - jy * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y_lo = max(0, jy - window), y_hi = min(H - 1, jy + window);
    const int x_lo = max(0, jx - window), x_hi = min(W - 1, jx + window);
    const int ww = x_hi - x_lo + 1;
    const int n_entries = (y_hi - y_lo + 1) * ww * P;
    const float pc = tid < C ? prev[(int64_t)j * C + tid] : 0.0f;
    float acc = 0.0f;
    for (int base = 0; base < n_entries; base += 256) {
        const int e = base + tid;
        bool hit = false;
        int i = 0, p = 0;
        if (e < n_entries) {
            const int w = e / P;
            p = e - w * P;
            const int wy = w / ww;
            i = (y_lo + wy) * W + x_lo + (w - wy * ww);
            hit = abuf[(int64_t)i * P + p] == j;
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) lcnt[wave] = __popcll(mask);
        __syncthreads();
        int off = 0, total = 0;
        for (int k = 0; k < 4; ++k) {
            const int n = lcnt[k];
            if (k < wave) off += n;
            total += n;
        }
        if (hit) {
            const int k = off + __popcll(mask & ((1ull << lane) - 1ull));
            lpix[k] = i;
            lg2[k] = 2.0f * gbuf[(int64_t)i * P + p];
        }
        __syncthreads();
        if (tid < C)
            for (int k = 0; k < total; ++k) acc += lg2[k] * (pc - query[(int64_t)lpix[k] * C + tid]);
        __syncthreads();
    }
    if (tid < C) grad_prev[(int64_t)j * C + tid] = acc;
}

// sum of g[o, ch, i]: LG_BIAS_PIX pixels per first-stage thread (ascending pixel, within it ascending ch), then the blocks, ascending
__global__ __launch_bounds__(32) void lg_bias_partial_kernel(const float *__restrict__ gbuf, int64_t m, int nr, int n_obj, float *__restrict__ part) {
    const int o = threadIdx.x;
    if (o >= n_obj) return;
    const int64_t beg = (int64_t)blockIdx.x * LG_BIAS_PIX, end = min(m, beg + LG_BIAS_PIX);
    const int P = nr * n_obj;
    float acc = 0.0f;
    for (int64_t i = beg; i < end; ++i)
        for (int ch = 0; ch < nr; ++ch) acc += gbuf[i * P + o * nr + ch];
    part[(int64_t)blockIdx.x * n_obj + o] = acc;
}
__global__ __launch_bounds__(32) void lg_bias_final_kernel(const float *__restrict__ part, int n_blocks, int n_obj, float *__restrict__ grad_bias) {
    const int o = threadIdx.x;
    if (o >= n_obj) return;
    float acc = 0.0f;
    for (int b = 0; b < n_blocks; ++b) acc += part[(int64_t)b * n_obj + o];
    grad_bias[o] = acc;
}

struct LgLayout {
    size_t gbuf, abuf, bias_part, total;
    int bias_blocks;
};
LgLayout lg_layout(int H, int W, int n_radii, int n_obj) {
    LgLayout l;
    const size_t m = (size_t)H * W, pairs = m * n_radii * n_obj;
    l.bias_blocks = (int)((m + LG_BIAS_PIX - 1) / LG_BIAS_PIX);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += aoc_align_up(bytes, 256); return here; };
    l.gbuf = take(pairs * sizeof(float));
    l.abuf = take(pairs * sizeof(int32_t));
    l.bias_part = take((size_t)l.bias_blocks * n_obj * sizeof(float));
    l.total = at;
    return l;
}

// 0 = fine
int lg_check_sizes(int H, int W, int C, int n_radii, int n_obj) {
    if (H < 1 || W < 1 || C < 1 || n_radii < 1 || n_obj < 1) return AOC_ERR_INVALID_ARG;
    if (C > AOC_MAX_CHANNELS || n_radii > LW_MAX_RADII || n_obj > AOC_MAX_OBJECTS) return AOC_ERR_UNSUPPORTED;
    if ((int64_t)H * W >= (1ll << 31) / (LW_MAX_RADII * AOC_MAX_OBJECTS)) return AOC_ERR_UNSUPPORTED;     // int32 pixel and entry indices
    return AOC_OK;
}

}  // namespace

extern "C" {

int aoc_local_window_match_argmin(const float *query, const float *prev, const uint32_t *right_bits, int H, int W, int C,
                                  const int32_t *radii_host, int n_radii, const float *obj_bias, int n_obj,
                                  float *out, int32_t *arg, int transform, int atrous_rate, aoc_stream_t stream) {
    if (!query || !prev || !right_bits || !radii_host || !out || !arg) return AOC_ERR_INVALID_ARG;
    if (aoc_off16(query, prev)) return AOC_ERR_INVALID_ARG;                // float4 pixel rows in both kernels
    if (H < 1 || W < 1 || C < 4 || n_radii < 1 || n_obj < 1 || atrous_rate < 1) return AOC_ERR_INVALID_ARG;
    if ((C & 3) || C > 128 || n_radii > LW_MAX_RADII || n_obj > AOC_MAX_OBJECTS) return AOC_ERR_UNSUPPORTED;
    if ((int64_t)H * W >= (1ll << 31) - 1) return AOC_ERR_UNSUPPORTED;                 // the pixel index is a key's low word, -1 is "none"
    LocalRadii radii;
    if (int rc = lw_radii_from_host(radii_host, n_radii, atrous_rate, radii)) return rc;
    if (radii.r[n_radii - 1] * atrous_rate > LG_MAX_WINDOW) return AOC_ERR_UNSUPPORTED;
    hipStream_t st = aoc_hip_stream(stream);
    if (C == 100 || C == 128) {
        const dim3 grid((W + 7) / 8, (H + 1) / 2);
        const size_t lds = 32 * sizeof(float) + (size_t)16 * n_radii * n_obj * sizeof(unsigned long long);
        if (C == 100)
            hipLaunchKernelGGL(lg_window_reg_argmin_kernel<25>, grid, dim3(256), lds, st, query, prev, right_bits, H, W, radii, obj_bias, n_obj, out, arg,
                               transform, atrous_rate);
        else
            hipLaunchKernelGGL(lg_window_reg_argmin_kernel<32>, grid, dim3(256), lds, st, query, prev, right_bits, H, W, radii, obj_bias, n_obj, out, arg,
                               transform, atrous_rate);
    } else {
        if (H > 65535) return AOC_ERR_UNSUPPORTED;                                     // grid y
        hipLaunchKernelGGL(lg_window_argmin_kernel, dim3(W, H), dim3(256), 0, st, query, prev, right_bits, H, W, C, radii, obj_bias, n_obj, out, arg,
                           transform, atrous_rate);
    }
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

size_t aoc_local_match_grad_workspace_bytes(int H, int W, int C, int n_radii, int n_obj) {
    if (lg_check_sizes(H, W, C, n_radii, n_obj) != AOC_OK) return 0;
    return lg_layout(H, W, n_radii, n_obj).total;
}

int aoc_local_match_grad(const float *grad_out, const float *T, const int32_t *arg,
                         const float *query, const float *prev, int H, int W, int C, int n_radii, int n_obj, int window,
                         float *grad_query, float *grad_prev, float *grad_bias,
                         void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (!grad_out || !T || !arg || !query || !prev || !workspace) return AOC_ERR_INVALID_ARG;
    if (window < 0) return AOC_ERR_INVALID_ARG;
    if (int rc = lg_check_sizes(H, W, C, n_radii, n_obj)) return rc;
    if (window > LG_MAX_WINDOW) return AOC_ERR_UNSUPPORTED;
    const LgLayout l = lg_layout(H, W, n_radii, n_obj);
    if (workspace_bytes < l.total) return AOC_ERR_WORKSPACE;
    hipStream_t st = aoc_hip_stream(stream);
    char *ws = static_cast<char *>(workspace);
    float *gbuf = reinterpret_cast<float *>(ws + l.gbuf);
    int32_t *abuf = reinterpret_cast<int32_t *>(ws + l.abuf);
    float *bias_part = reinterpret_cast<float *>(ws + l.bias_part);
    const int P = n_radii * n_obj;
    const int64_t m = (int64_t)H * W;
    hipLaunchKernelGGL(lg_gate_kernel, dim3((unsigned)((m * P + 255) / 256)), dim3(256), 0, st, grad_out, T, arg, H, W, P, window, gbuf, abuf);
    if (grad_query) hipLaunchKernelGGL(lg_query_kernel, dim3((unsigned)m), dim3(64), 0, st, gbuf, abuf, query, prev, C, P, grad_query);
    if (grad_prev) hipLaunchKernelGGL(lg_prev_kernel, dim3((unsigned)m), dim3(256), 0, st, gbuf, abuf, query, prev, H, W, C, P, window, grad_prev);
    if (grad_bias) {
        hipLaunchKernelGGL(lg_bias_partial_kernel, dim3(l.bias_blocks), dim3(32), 0, st, gbuf, m, n_radii, n_obj, bias_part);
        hipLaunchKernelGGL(lg_bias_final_kernel, dim3(1), dim3(32), 0, st, bias_part, l.bias_blocks, n_obj, grad_bias);
    }
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
