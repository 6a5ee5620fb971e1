// The tail of CalibrationDecoding (networks/aoc/decoding_module.py): the shortcut stage of decoder_final (:163, :170-176: bicubic
// align_corners=True upsample, concatenation with the shortcut branch, full-map average pool, px1_delta, IA10) and the prediction head
// (:144-147: IA_logit for the fg and bg heads + augment_background_logit).  fp32, inference only, caller-owned buffers.
//
// The bicubic tap weights and their semantics are bicubic.h's, shared with the adjoint of tail_grad.hip.
#include "bicubic.h"

namespace {

constexpr size_t BC_LDS_MAX = 64 * 1024;         // dynamic LDS a launch may ask for without an attribute

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// four taps, one rounding each: fma(w3, x3, fma(w2, x2, fma(w1, x1, w0 x0)))
__device__ __forceinline__ float tap_sum(f32x4 wt, float x0, float x1, float x2, float x3) {
    return __builtin_fmaf(wt.w, x3, __builtin_fmaf(wt.z, x2, __builtin_fmaf(wt.y, x1, wt.x * x0)));
}

// out[n, c < Ce] = gain[n, c] * bicubic(x[n, c]).  grid (bands, N * Ce): a workgroup owns R output rows of one plane.
//   1. tap tables of the W output columns and of its R rows -> LDS (weights float4, index of the second tap);
//   2. the vertical pass: v[r][j] = sum_k wy[r][k] x[iy_k][j] -> LDS (reads the coarse plane, which lives in L1 / L2, along its rows);
//   3. the horizontal pass over the band as ONE contiguous run of R * W floats: lane = consecutive float, the run shifted so that every
//      wave-wide store is a 256-byte aligned 256-byte line pair (rows of odd W have no alignment of their own); written once, nontemporal.
__global__ __launch_bounds__(256) void bicubic_scale_kernel(const float *__restrict__ x, const float *__restrict__ gain, int Ce, int Ctot, int h, int w,
                                                            int H, int W, int R, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bc_lds[];
    f32x4 *xw = reinterpret_cast<f32x4 *>(bc_lds);          // [W]
    f32x4 *yw = xw + W;                                     // [R]
    int *xi = reinterpret_cast<int *>(yw + R);              // [W]
    int *yi = xi + W;                                       // [R]
    float *v = reinterpret_cast<float *>(yi + R);           // [R][w]
    const int plane = blockIdx.y, n = plane / Ce, c = plane - n * Ce;
    const int r0 = blockIdx.x * R, nr = min(R, H - r0);
    const float *xp = x + (size_t)plane * h * w;
    float *op = out + ((size_t)n * Ctot + c) * H * W + (size_t)r0 * W;
    const float g = gain ? gain[(size_t)n * Ctot + c] : 1.0f;
    for (int i = threadIdx.x; i < W + nr; i += 256) {
        int i0;
        if (i < W) {
            xw[i] = bicubic_taps(i, w, W, i0);
            xi[i] = i0;
        } else {
            yw[i - W] = bicubic_taps(r0 + i - W, h, H, i0);
            yi[i - W] = i0;
        }
    }
    __syncthreads();
    {
        int r = threadIdx.x / w, j = threadIdx.x - r * w;
        const int dr = 256 / w, dj = 256 - dr * w;
        for (int f = threadIdx.x; f < nr * w; f += 256) {
            const f32x4 wt = yw[r];
            const int i0 = yi[r];
            const float a0 = xp[(size_t)clampi(i0 - 1, h - 1) * w + j], a1 = xp[(size_t)clampi(i0, h - 1) * w + j];
            const float a2 = xp[(size_t)clampi(i0 + 1, h - 1) * w + j], a3 = xp[(size_t)clampi(i0 + 2, h - 1) * w + j];
            v[f] = tap_sum(wt, a0, a1, a2, a3);
            r += dr;
            j += dj;
            if (j >= w) { j -= w; ++r; }
        }
    }
    __syncthreads();
    {
        const int shift = (int)((reinterpret_cast<uintptr_t>(op) >> 2) & 63);          // floats past a 256-byte line
        const int total = nr * W;
        const int dr = 256 / W, dj = 256 - dr * W;
        int f = (int)threadIdx.x - shift;
        if (f < 0) f += 256;                               // the lanes in front of the band take their next turn
        int r = f / W, o = f - r * W;
        for (; f < total; f += 256) {
            const f32x4 wt = xw[o];
            const int i0 = xi[o];
            const float *vr = v + r * w;
            const float s = tap_sum(wt, vr[clampi(i0 - 1, w - 1)], vr[clampi(i0, w - 1)], vr[clampi(i0 + 1, w - 1)], vr[clampi(i0 + 2, w - 1)]);
            __builtin_nontemporal_store(g * s, op + f);
            r += dr;
            o += dj;
            if (o >= W) { o -= W; ++r; }
        }
    }
}

// out[n, Ce + c] = gain[n, Ce + c] * low[n, c]: the stream of channel_scale_kernel with the concatenation's plane offsets.  grid (bx, Cr, N)
__global__ __launch_bounds__(256) void cat_scale_low_kernel(const float *__restrict__ low, const float *__restrict__ gain, int Ce, int Cr, int64_t hw,
                                                            float *__restrict__ out) {
    const int c = blockIdx.y, n = blockIdx.z, Ctot = Ce + Cr;
    const float g = gain ? gain[(size_t)n * Ctot + Ce + c] : 1.0f;
    const float *xp = low + ((size_t)n * Cr + c) * hw;
    float *yp = out + ((size_t)n * Ctot + Ce + c) * hw;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(xp);
    int64_t head = ((16 - (addr & 15)) & 15) / 4;
    if (head > hw) head = hw;
    const bool same_align = ((reinterpret_cast<uintptr_t>(yp) & 15) == (addr & 15));
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    if (same_align) {
        if (tid < head) yp[tid] = g * xp[tid];
        const int64_t body4 = (hw - head) / 4;
        const f32x4 *x4 = reinterpret_cast<const f32x4 *>(xp + head);
        f32x4 *y4 = reinterpret_cast<f32x4 *>(yp + head);
        for (int64_t i = tid; i < body4; i += nthreads) __builtin_nontemporal_store(__builtin_nontemporal_load(x4 + i) * g, y4 + i);
        const int64_t tail0 = head + body4 * 4;
        if (tid < hw - tail0) yp[tail0 + tid] = g * xp[tail0 + tid];
    } else {
        for (int64_t i = tid; i < hw; i += nthreads) __builtin_nontemporal_store(g * xp[i], yp + i);
    }
}

// mean over the H x W map of the bicubic upsample of a coarse plane, from the coarse plane alone: the upsample is linear and separable, so
// the mean is (1 / HW) sum_ij cy[i] cx[j] x[i, j] with cy, cx the column sums of the two 1-D interpolation matrices (clamped taps land in
// the border columns).  One workgroup per plane:
//   1. tap tables of the H rows and W columns -> LDS;   2. thread s adds up, in output order, the taps that land on source index s
//   (they belong to outputs whose second tap is s - 2 .. s + 1);   3. the weighted sum of the plane, accumulated as plane_mean4_kernel does
//   (a running sum per thread, the wave sum, the four wave totals in order, the division).
__global__ __launch_bounds__(256) void bicubic_plane_mean_kernel(const float *__restrict__ x, int C, int64_t out_obj_stride, int h, int w, int H, int W,
                                                                 float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bc_lds[];
    f32x4 *tw = reinterpret_cast<f32x4 *>(bc_lds);          // [H + W]: rows, then columns
    int *ti = reinterpret_cast<int *>(tw + H + W);          // [H + W]
    float *cs = reinterpret_cast<float *>(ti + H + W);      // [h + w]: cy, then cx
    float *wsum = cs + h + w;                               // [4]
    for (int i = threadIdx.x; i < H + W; i += 256) {
        int i0;
        tw[i] = i < H ? bicubic_taps(i, h, H, i0) : bicubic_taps(i - H, w, W, i0);
        ti[i] = i0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < h + w; i += 256) {
        const bool rows = i < h;
        const int s = rows ? i : i - h, in = rows ? h : w, on = rows ? H : W, base = rows ? 0 : H;
        // the first output whose second tap is >= s - 2
        int o = (in > 1 && s > 2) ? (int)(((int64_t)(s - 2) * (on - 1) + in - 2) / (in - 1)) : 0;
        float acc = 0.0f;
        for (; o < on; ++o) {
            const int i0 = ti[base + o];
            if (i0 > s + 1) break;
            const f32x4 wt = tw[base + o];
            if (clampi(i0 - 1, in - 1) == s) acc += wt.x;
            if (clampi(i0, in - 1) == s) acc += wt.y;
            if (clampi(i0 + 1, in - 1) == s) acc += wt.z;
            if (clampi(i0 + 2, in - 1) == s) acc += wt.w;
        }
        cs[i] = acc;
    }
    __syncthreads();
    const float *xp = x + (size_t)blockIdx.x * h * w;
    const int total = h * w;
    const int dr = 256 / w, dj = 256 - dr * w;
    int r = threadIdx.x / w, j = threadIdx.x - r * w;
    float acc = 0.0f;
    for (int f = threadIdx.x; f < total; f += 256) {
        acc += (cs[r] * cs[h + j]) * xp[f];
        r += dr;
        j += dj;
        if (j >= w) { j -= w; ++r; }
    }
    acc = aoc_wave_sum(acc);
    if (aoc_lane() == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int p = blockIdx.x, n = p / C;
        out[(size_t)n * out_obj_stride + (p - n * C)] = (wsum[0] + wsum[1] + wsum[2] + wsum[3]) / (float)((int64_t)H * W);
    }
}

// The prediction head (decoding_module.py:144-147) in one launch.  Workgroup = 64 pixels x NW waves; wave q owns objects q, q + NW, ...,
// so every x[n, c, p] is read once; an object's fg and bg logits come from the same loads.  The channel sum keeps object_logit_kernel's order
// (sequential over c, bias last; 16 loads in flight instead of 8 changes no addition), so fg and bg are bit-equal to aoc_object_logit's.
// pred[n >= 1] = fg[n];  pred[0] = fg[0] + min_{n >= 1} bg[n]  (N > 1);  bg[0] is never computed.
constexpr int LH_MAXW = 4;
__global__ __launch_bounds__(64 * LH_MAXW) void logit_head_kernel(const float *__restrict__ x, const float *__restrict__ wb_fg, const float *__restrict__ wb_bg,
                                                                  int64_t stride, int N, int C, int64_t hw, float *__restrict__ pred) {
    __shared__ float lmin[LH_MAXW][64];
    __shared__ float lfg0[64];
    const int lane = threadIdx.x, q = __builtin_amdgcn_readfirstlane(threadIdx.y), nw = blockDim.y;      // a wave has one q
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;
    const bool live = p < hw;
    const int64_t pc = live ? p : hw - 1;                 // clamped: dead lanes load a valid address and store nothing
    float mn = INFINITY;
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
            mn = sb < mn ? sb : mn;
            if (live) pred[(size_t)n * hw + p] = sf;
        } else {
            lfg0[lane] = sf;
        }
    }
    lmin[q][lane] = mn;
    __syncthreads();
    if (q == 0 && live) {
        float s = lfg0[lane];
        if (N > 1) {
            float m = lmin[0][lane];
            for (int k = 1; k < nw; ++k) m = lmin[k][lane] < m ? lmin[k][lane] : m;
            s += m;
        }
        pred[p] = s;
    }
}

// augment_background_logit (decoding_module.py:213-225) on logits that already exist: pred[n] = fg[n], pred[0] += min_{n >= 1} bg[n]
__global__ __launch_bounds__(256) void background_merge_kernel(const float *__restrict__ fg, const float *__restrict__ bg, int N, int64_t hw,
                                                               float *__restrict__ pred) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    float m = INFINITY;
    for (int n = 1; n < N; ++n) {
        const float b = bg[(size_t)n * hw + p];
        m = b < m ? b : m;
        pred[(size_t)n * hw + p] = fg[(size_t)n * hw + p];
    }
    pred[p] = N > 1 ? fg[p] + m : fg[p];
}

size_t bicubic_scale_lds(int R, int w, int W) { return (size_t)(W + R) * 20 + (size_t)R * w * sizeof(float); }

// rows per workgroup: at least ~2048 workgroups where the map has the rows for it, not fewer than 16 rows (the column table is rebuilt per
// workgroup), halved until the band fits the LDS; 0 = not even one row fits
int bicubic_band_rows(int64_t planes, int w, int H, int W) {
    const int64_t bands = (2048 + planes - 1) / planes;
    int R = (int)((H + bands - 1) / bands);
    if (R < 16) R = 16;
    if (R > H) R = H;
    while (R > 1 && bicubic_scale_lds(R, w, W) > 48 * 1024) R = (R + 1) / 2;
    return bicubic_scale_lds(R, w, W) <= BC_LDS_MAX ? R : 0;
}

bool bicubic_sizes_ok(int h, int w, int H, int W) {
    return h >= 1 && w >= 1 && H >= 1 && W >= 1 && (int64_t)h * w < (1ll << 31) && (int64_t)H * W < (1ll << 31);
}

size_t plane_mean_lds(int h, int w, int H, int W) { return (size_t)(H + W) * 20 + (size_t)(h + w + 4) * sizeof(float); }

int bicubic_plane_mean_launch(const float *in, int64_t P, int C, int64_t out_obj_stride, int h, int w, int H, int W, float *out, aoc_stream_t stream) {
    hipLaunchKernelGGL(bicubic_plane_mean_kernel, dim3((unsigned)P), dim3(256), plane_mean_lds(h, w, H, W), aoc_hip_stream(stream), in, C, out_obj_stride,
                       h, w, H, W, out);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int cat_scale_check(const float *x, const float *low, int N, int Ce, int Cr, int h, int w, int H, int W, const float *out) {
    if (!x || !out || (Cr > 0 && !low) || N < 1 || Ce < 1 || Cr < 0 || !bicubic_sizes_ok(h, w, H, W)) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (int64_t)N * Ce > 65535 || Cr > 65535 || bicubic_band_rows((int64_t)N * Ce, w, H, W) == 0) return AOC_ERR_UNSUPPORTED;
    return AOC_OK;
}

struct StageWs { size_t px, head, gain, total; };
StageWs stage_ws(int N, int Ce, int Cr, int D) {
    StageWs s;
    const size_t ct = (size_t)Ce + Cr;
    s.px = 0;
    s.head = s.px + aoc_align_up((size_t)N * ct * sizeof(float), 256);
    s.gain = s.head + aoc_align_up((size_t)N * (D + ct) * sizeof(float), 256);
    s.total = s.gain + aoc_align_up((size_t)N * ct * sizeof(float), 256);
    return s;
}

}  // namespace

extern "C" {

int aoc_bicubic_plane_mean(const float *in, int64_t P, int h, int w, int H, int W, float *out, aoc_stream_t stream) {
    if (!in || !out || P < 1 || !bicubic_sizes_ok(h, w, H, W)) return AOC_ERR_INVALID_ARG;
    if (P > 0x7fffffff || plane_mean_lds(h, w, H, W) > BC_LDS_MAX) return AOC_ERR_UNSUPPORTED;
    return bicubic_plane_mean_launch(in, P, (int)P, 0, h, w, H, W, out, stream);
}

int aoc_bicubic_cat_scale(const float *x, const float *low, const float *gain, int N, int Ce, int Cr, int h, int w, int H, int W, float *out,
                          aoc_stream_t stream) {
    const int rc = cat_scale_check(x, low, N, Ce, Cr, h, w, H, W, out);
    if (rc != AOC_OK) return rc;
    const int R = bicubic_band_rows((int64_t)N * Ce, w, H, W);
    hipLaunchKernelGGL(bicubic_scale_kernel, dim3((unsigned)((H + R - 1) / R), (unsigned)(N * Ce)), dim3(256), bicubic_scale_lds(R, w, W),
                       aoc_hip_stream(stream), x, gain, Ce, Ce + Cr, h, w, H, W, R, out);
    AOC_RETURN_IF_LAUNCH_FAILED();
    if (Cr > 0) {
        const int64_t hw = (int64_t)H * W;
        int bx = (int)((hw / 4 + 1023) / 1024);
        if (bx < 1) bx = 1;
        if (bx > 8) bx = 8;
        hipLaunchKernelGGL(cat_scale_low_kernel, dim3(bx, (unsigned)Cr, (unsigned)N), dim3(256), 0, aoc_hip_stream(stream), low, gain, Ce, Cr, hw, out);
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    return AOC_OK;
}

size_t aoc_shortcut_stage_workspace_bytes(int N, int Ce, int Cr, int head_dim) {
    if (N < 1 || N > AOC_MAX_OBJECTS || Ce < 1 || Cr < 0 || head_dim < 1) return 0;
    return stage_ws(N, Ce, Cr, head_dim).total;
}

int aoc_shortcut_stage_enqueue(const float *x, const float *low, const float *IA_head, const float *weight, const float *bias, int N, int Ce, int Cr,
                               int head_dim, int h, int w, int H, int W, float *out, float *plane_means, float *gain_out, void *workspace,
                               size_t workspace_bytes, aoc_stream_t stream) {
    if (!IA_head || !weight || !workspace || head_dim < 1) return AOC_ERR_INVALID_ARG;
    int rc = cat_scale_check(x, low, N, Ce, Cr, h, w, H, W, out);
    if (rc != AOC_OK) return rc;
    if (plane_mean_lds(h, w, H, W) > BC_LDS_MAX) return AOC_ERR_UNSUPPORTED;
    const StageWs s = stage_ws(N, Ce, Cr, head_dim);
    if (workspace_bytes < s.total) return AOC_ERR_WORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const int Ctot = Ce + Cr;
    float *px = plane_means ? plane_means : reinterpret_cast<float *>(ws + s.px);
    float *head = reinterpret_cast<float *>(ws + s.head);
    float *gain = gain_out ? gain_out : reinterpret_cast<float *>(ws + s.gain);
    // :172 on the concatenation that is never materialised: the upsampled planes from the coarse map, the shortcut planes as they are
    if ((rc = bicubic_plane_mean_launch(x, (int64_t)N * Ce, Ce, Ctot, h, w, H, W, px, stream)) != AOC_OK) return rc;
    for (int n = 0; n < N && Cr > 0; ++n)
        if ((rc = aoc_plane_mean(low + (size_t)n * Cr * H * W, Cr, (int64_t)H * W, px + (size_t)n * Ctot + Ce, stream)) != AOC_OK) return rc;
    if ((rc = aoc_head_delta(IA_head, head_dim, px, N, Ctot, head, stream)) != AOC_OK) return rc;              // :173-174, the cat of :176
    if ((rc = aoc_film_gain(head, weight, bias, N, head_dim + Ctot, Ctot, gain, stream)) != AOC_OK) return rc;    // ATT:13-14
    return aoc_bicubic_cat_scale(x, low, gain, N, Ce, Cr, h, w, H, W, out, stream);                             // :163, :170, ATT:15-16
}

int aoc_logit_head(const float *x, const float *wb_fg, const float *wb_bg, int64_t stride, int N, int C, int64_t hw, float *pred, aoc_stream_t stream) {
    if (!x || !wb_fg || !pred || N < 1 || C < 1 || hw < 1 || stride < C + 1 || (N > 1 && !wb_bg)) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (hw + 63) / 64 > 0x7fffffff) return AOC_ERR_UNSUPPORTED;
    const int nw = N < LH_MAXW ? N : LH_MAXW;
    hipLaunchKernelGGL(logit_head_kernel, dim3((unsigned)((hw + 63) / 64)), dim3(64, nw), 0, aoc_hip_stream(stream), x, wb_fg, wb_bg ? wb_bg : wb_fg, stride,
                       N, C, hw, pred);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_background_merge(const float *fg, const float *bg, int N, int64_t hw, float *pred, aoc_stream_t stream) {
    if (!fg || !pred || N < 1 || hw < 1 || (N > 1 && !bg)) return AOC_ERR_INVALID_ARG;
    if (N > AOC_MAX_OBJECTS || (hw + 255) / 256 > 0x7fffffff) return AOC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(background_merge_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, aoc_hip_stream(stream), fg, bg, N, hw, pred);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
