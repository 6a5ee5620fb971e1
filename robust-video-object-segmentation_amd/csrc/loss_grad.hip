// Training criterion: what aocnet.py:71-82 and networks/layers/loss.py:52-97 (Concat_CrossEntropyLoss) do with a sample's logits, without
// ever forming the upsampled logits.  Eight entry points (include/aoc_hip.h); aoc_amd.loss_train wires them into autograd.
//
//   forward   one thread per fine pixel: the bilinear tap (align_corners=True) of every channel, recomputed for the second channel loop
//             instead of kept; lse = m + logf(sum expf(x_c - m)), channels ascending; loss = lse - x[label]; the lowest channel of a tie
//             is the argmax; one count of valid pixels per block of 256 pixels.
//   top-k     a radix select over the monotone integer image of the floats: four passes of eight bits, many workgroups, integer
//             histograms (integer atomics only: their result does not depend on the order).  Pass p resolves digit p - 1 from its complete
//             histogram and counts digit p.  Then a sum of the values above the threshold over contiguous chunks, and one thread that adds
//             the chunks.
//   mask      the ties at the threshold are taken in ascending pixel order: a count of ties per chunk, then an ordered scan inside the chunk.
//   gradient  the adjoint of the upsample in GATHER form (tail_grad.hip's pass A with two taps).  The channels are independent once lse is
//             known (softmax_c = expf(x_c - lse)), so a workgroup owns a band of coarse rows of ONE channel and walks the fine rows that
//             reach the band through LDS.  Nothing of size C * H * W is written.
//
// No float atomics.  Every float sum runs in an order fixed by the shapes:
//   chunk sums       thread t of 256 adds the chunk's elements t, t + 256, ... in ascending order, the xor butterfly of aoc_wave_sum, the
//                    four wave sums in ascending order; then the chunks in ascending order from 0.0f
//   bilinear adjoint u[I, j] = the fine columns J in ascending order, tap 0 then tap 1 of each; grad[i, j] = the fine rows I in ascending
//                    order, tap 0 then tap 1; every product is rounded, then added (-ffp-contract=off), from 0.0f
#include "aoc_common.h"

namespace {

constexpr int LG_MAX_C = 31;
constexpr size_t LG_LDS_MAX = 64 * 1024;         // dynamic LDS a launch may ask for without an attribute
constexpr int LG_MAX_CHUNKS = 1024;

// ------------------------------------------------------------------------------------------ the bilinear tap
// torch's upsample_bilinear2d with align_corners=True, in float: scale = (float)(in - 1) / (float)(out - 1) (0 when out == 1),
// src = (float)o * scale, i0 = min((int)src, in - 1), i1 = min(i0 + 1, in - 1), w1 = min(max(src - (float)i0, 0), 1), w0 = 1.0f - w1
struct Tap { int i0, i1; float w0, w1; };

__device__ __forceinline__ Tap lg_tap(int o, int in, int out) {
    Tap t;
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    const float src = (float)o * scale;
    int i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    float w1 = src - (float)i0;
    w1 = w1 < 0.0f ? 0.0f : (w1 > 1.0f ? 1.0f : w1);
    t.i0 = i0;
    t.i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    t.w1 = w1;
    t.w0 = 1.0f - w1;
    return t;
}

// a tap whose weight is exactly 0 is not multiplied in: the identity geometry hands the logits through bit for bit
__device__ __forceinline__ float lg_row(const float *r, const Tap tx) {
    if (tx.w1 == 0.0f) return tx.w0 * r[tx.i0];
    if (tx.w0 == 0.0f) return tx.w1 * r[tx.i1];
    return tx.w0 * r[tx.i0] + tx.w1 * r[tx.i1];
}
// x = w0y * (w0x * a + w1x * b) + w1y * (w0x * c + w1x * d)
__device__ __forceinline__ float lg_interp(const float *plane, int w, const Tap ty, const Tap tx) {
    if (ty.w1 == 0.0f) return ty.w0 * lg_row(plane + (size_t)ty.i0 * w, tx);
    if (ty.w0 == 0.0f) return ty.w1 * lg_row(plane + (size_t)ty.i1 * w, tx);
    return ty.w0 * lg_row(plane + (size_t)ty.i0 * w, tx) + ty.w1 * lg_row(plane + (size_t)ty.i1 * w, tx);
}

__device__ __forceinline__ bool lg_valid(int label, int C, int ignore_index) { return label != ignore_index && label >= 0 && label < C; }

// ------------------------------------------------------------------------------------------ 1: the forward
__global__ __launch_bounds__(256) void ce_forward_kernel(const float *__restrict__ pred, const int32_t *__restrict__ labels, int C, int h, int w, int H, int W,
                                                         int ignore_index, float *__restrict__ loss, float *__restrict__ lse_out,
                                                         int32_t *__restrict__ argmax, int32_t *__restrict__ valid_partial, int32_t *__restrict__ bad) {
    __shared__ int wcnt[4];
    const int64_t n = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = p < n;
    const int64_t pc = live ? p : n - 1;                  // clamped: dead lanes load valid addresses and store nothing
    const int I = (int)(pc / W), J = (int)(pc - (int64_t)I * W);
    const Tap ty = lg_tap(I, h, H), tx = lg_tap(J, w, W);
    const size_t hw = (size_t)h * w;
    const int label = labels[pc];
    float m = lg_interp(pred, w, ty, tx);
    float xl = label == 0 ? m : 0.0f;
    int am = 0;
    for (int c = 1; c < C; ++c) {
        const float x = lg_interp(pred + c * hw, w, ty, tx);
        if (x > m) { m = x; am = c; }
        if (c == label) xl = x;
    }
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s += expf(lg_interp(pred + c * hw, w, ty, tx) - m);
    const float lse = m + logf(s);
    const bool valid = lg_valid(label, C, ignore_index);
    if (live) {
        if (loss) loss[p] = valid ? lse - xl : 0.0f;
        if (lse_out) lse_out[p] = lse;
        if (argmax) argmax[p] = am;
        if (bad && !valid && label != ignore_index) atomicAdd(bad, 1);
    }
    if (valid_partial) {
        const unsigned long long b = __ballot(valid && live);
        if (aoc_lane() == 0) wcnt[threadIdx.x >> 6] = __popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) valid_partial[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
}

// ------------------------------------------------------------------------------------------ 2: the k-th largest value and the mean above it
__device__ __forceinline__ uint32_t lg_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float lg_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

struct Sel { uint32_t prefix, left; };            // the digits resolved so far; how many of the k largest lie inside that prefix

// the bin of a complete histogram (256 words in LDS) that holds the left-th largest key, walking down from bin 255
__device__ __forceinline__ Sel lg_select(const uint32_t *hist, const Sel prev, int shift) {
    uint32_t above = 0;
    int b = 255;
    for (; b > 0; --b) {
        const uint32_t c = hist[b];
        if (above + c >= prev.left) break;
        above += c;
    }
    return Sel{prev.prefix | ((uint32_t)b << shift), prev.left - above};
}

struct TopkWs { size_t hist, sel, partial, total; };
__host__ __device__ inline int64_t lg_chunk(int64_t n) {
    int64_t c = (n + LG_MAX_CHUNKS - 1) / LG_MAX_CHUNKS;
    c = (c + 255) / 256 * 256;
    return c < 4096 ? 4096 : c;
}
inline int lg_chunks(int64_t n) { return (int)((n + lg_chunk(n) - 1) / lg_chunk(n)); }
TopkWs topk_ws(int64_t n) {
    TopkWs s;
    s.hist = 0;
    s.sel = 4 * 256 * sizeof(uint32_t);
    s.partial = s.sel + 256;
    s.total = s.partial + aoc_align_up((size_t)lg_chunks(n) * sizeof(float), 256);
    return s;
}

// pass 0..3: digit pass - 1 is resolved from its complete histogram (block 0 records it in sel[pass - 1]), digit `pass` of the keys that
// still match is counted.  hist [4][256] is zero when pass 0 starts.
__global__ __launch_bounds__(256) void topk_pass_kernel(const float *__restrict__ loss, int64_t n, uint32_t k, int pass, uint32_t *__restrict__ hist,
                                                        Sel *__restrict__ sel) {
    __shared__ uint32_t lh[256], ph[256];
    __shared__ Sel cur;
    lh[threadIdx.x] = 0;
    if (pass > 0) ph[threadIdx.x] = hist[(pass - 1) * 256 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        if (pass == 0) {
            cur = Sel{0u, k};
        } else {
            cur = lg_select(ph, pass == 1 ? Sel{0u, k} : sel[pass - 2], 8 * (4 - pass));
            if (blockIdx.x == 0) sel[pass - 1] = cur;
        }
    }
    __syncthreads();
    const uint32_t prefix = cur.prefix, mask = pass == 0 ? 0u : 0xffffffffu << (8 * (4 - pass)), shift = 8 * (3 - pass);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t key = lg_key(loss[i]);
        if ((key & mask) == prefix) atomicAdd(&lh[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&hist[pass * 256 + threadIdx.x], lh[threadIdx.x]);
}

// partial[b] = the sum of chunk b's values whose key lies above the threshold's (all values: every value); a NaN is always added.
// The last digit is resolved here; block 0 records the threshold's key and its rank among its equals in sel[3].
__global__ __launch_bounds__(256) void topk_sum_kernel(const float *__restrict__ loss, int64_t n, int64_t chunk, int all, const uint32_t *__restrict__ hist,
                                                       Sel *__restrict__ sel, float *__restrict__ partial) {
    __shared__ uint32_t ph[256];
    __shared__ Sel cur;
    __shared__ float wsum[4];
    uint32_t tk = 0;
    if (!all) {
        ph[threadIdx.x] = hist[3 * 256 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            cur = lg_select(ph, sel[2], 0);
            if (blockIdx.x == 0) sel[3] = cur;
        }
        __syncthreads();
        tk = cur.prefix;
    }
    const int64_t base = (int64_t)blockIdx.x * chunk, end = base + chunk < n ? base + chunk : n;
    float acc = 0.0f;
    for (int64_t i = base + threadIdx.x; i < end; i += 256) {
        const float v = loss[i];
        if (all || lg_key(v) > tk || v != v) acc += v;
    }
    acc = aoc_wave_sum(acc);
    if (aoc_lane() == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// mean = (S + (float)(k - n_gt) * thr) / (float)k, S = the chunks in ascending order from 0.0f
__global__ void topk_finish_kernel(const float *__restrict__ partial, int chunks, uint32_t k, const Sel *__restrict__ sel, float *__restrict__ mean,
                                   float *__restrict__ thr_out, int32_t *__restrict__ n_gt_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = 0.0f;
    for (int b = 0; b < chunks; ++b) s += partial[b];
    const Sel fin = sel[3];
    const float thr = lg_unkey(fin.prefix);
    if (mean) *mean = (s + (float)fin.left * thr) / (float)k;
    if (thr_out) *thr_out = thr;
    if (n_gt_out) *n_gt_out = (int32_t)(k - fin.left);
}

// mean = S / (float)n_valid, n_valid = the blocks' counts in ascending order (0 / 0 = NaN, as torch's mean over no pixel)
__global__ void valid_finish_kernel(const float *__restrict__ partial, int chunks, const int32_t *__restrict__ valid_partial, int64_t n_partial,
                                    float *__restrict__ mean, int32_t *__restrict__ n_valid_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = 0.0f;
    for (int b = 0; b < chunks; ++b) s += partial[b];
    int32_t nv = 0;
    for (int64_t b = 0; b < n_partial; ++b) nv += valid_partial[b];
    if (mean) *mean = s / (float)nv;
    if (n_valid_out) *n_valid_out = nv;
}

// ------------------------------------------------------------------------------------------ 3: the mask
__global__ __launch_bounds__(256) void tie_count_kernel(const float *__restrict__ loss, int64_t n, int64_t chunk, const float *__restrict__ thr,
                                                        uint32_t *__restrict__ tie_partial) {
    __shared__ uint32_t cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const uint32_t tk = lg_key(*thr);
    const int64_t base = (int64_t)blockIdx.x * chunk, end = base + chunk < n ? base + chunk : n;
    uint32_t c = 0;
    for (int64_t i = base + threadIdx.x; i < end; i += 256) c += lg_key(loss[i]) == tk;
    if (c) atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) tie_partial[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(256) void select_mask_kernel(const float *__restrict__ loss, int64_t n, int64_t chunk, uint32_t k, const float *__restrict__ thr,
                                                          const int32_t *__restrict__ n_gt, const uint32_t *__restrict__ tie_partial,
                                                          uint8_t *__restrict__ mask) {
    __shared__ uint32_t before, wcnt[4];
    if (threadIdx.x == 0) before = 0;
    __syncthreads();
    uint32_t c = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) c += tie_partial[b];
    if (c) atomicAdd(&before, c);
    __syncthreads();
    uint32_t running = before;                            // ties at lower pixel indices
    const uint32_t tk = lg_key(*thr), take = k - (uint32_t)*n_gt;
    const int lane = aoc_lane(), wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * chunk, end = base + chunk < n ? base + chunk : n;
    for (int64_t t0 = base; t0 < end; t0 += 256) {
        const int64_t i = t0 + threadIdx.x;
        const bool live = i < end;
        const uint32_t key = live ? lg_key(loss[i]) : 0u;
        const bool tie = live && key == tk;
        const unsigned long long b = __ballot(tie);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        uint32_t mine = running + __popcll(b & ((1ull << lane) - 1ull));
        for (int q = 0; q < wave; ++q) mine += wcnt[q];
        if (live) mask[i] = (key > tk || (tie && mine < take)) ? 1 : 0;
        running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void valid_mask_kernel(const int32_t *__restrict__ labels, int64_t n, int C, int ignore_index, uint8_t *__restrict__ mask) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) mask[p] = lg_valid(labels[p], C, ignore_index) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ 4: the gradient
// grid (C, bands): a workgroup owns the coarse rows [r0, r1) of one channel and walks the fine rows that reach them in chunks of RB rows:
//   a. g[I, J] = mask * scale * (expf(x_c - lse) - [label == c]) of the chunk -> LDS (x_c by the forward's own expression);
//   b. the horizontal adjoint u[rr][j] -> LDS (thread = one (row, coarse column), its fine columns in ascending order);
//   c. the vertical adjoint into the band's accumulators in LDS (thread = one coarse pixel, the chunk's rows in ascending order).
// Neighbouring bands recompute the fine rows they share.
struct GradLds { size_t tap, cj, ri, g, u, acc, total; };
__host__ __device__ inline GradLds grad_lds(int w, int H, int W, int R, int RB) {
    GradLds L;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t r = off; off += (bytes + 15) / 16 * 16; return r; };
    L.tap = take((size_t)(H + W) * sizeof(Tap));  // rows, then columns
    L.cj = take((size_t)2 * w * 4);               // per coarse column: first and one-past-last fine column that can reach it
    L.ri = take((size_t)2 * R * 4);               // per coarse row of the band: the same for fine rows
    L.g = take((size_t)RB * W * 4);
    L.u = take((size_t)RB * w * 4);
    L.acc = take((size_t)R * w * 4);
    L.total = off;
    return L;
}

// the first of `count` taps (i0 ascending) whose i0 is >= s
__device__ __forceinline__ int lg_first(const Tap *t, int count, int s) {
    int lo = 0, hi = count;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid].i0 < s) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// acc += the taps of fine index o that land on source index s, tap 0 then tap 1; a tap of weight 0 was not multiplied in by the forward
__device__ __forceinline__ float lg_gather(float acc, const Tap t, int s, float v) {
    if (t.i0 == s && t.w0 != 0.0f) acc += t.w0 * v;
    if (t.i1 == s && t.w1 != 0.0f) acc += t.w1 * v;
    return acc;
}

__global__ __launch_bounds__(256) void ce_grad_kernel(const float *__restrict__ pred, const int32_t *__restrict__ labels, const float *__restrict__ lse,
                                                      const uint8_t *__restrict__ mask, const float *__restrict__ grad_out, int64_t k,
                                                      const int32_t *__restrict__ n_valid, int C, int h, int w, int H, int W, int ignore_index, int R, int RB,
                                                      float *__restrict__ grad_pred) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lg_lds[];
    const GradLds L = grad_lds(w, H, W, R, RB);
    Tap *tap = reinterpret_cast<Tap *>(lg_lds + L.tap);
    int *cj = reinterpret_cast<int *>(lg_lds + L.cj);
    int *ri = reinterpret_cast<int *>(lg_lds + L.ri);
    float *gb = reinterpret_cast<float *>(lg_lds + L.g);
    float *ub = reinterpret_cast<float *>(lg_lds + L.u);
    float *acc = reinterpret_cast<float *>(lg_lds + L.acc);
    const int c = blockIdx.x;
    const int r0 = blockIdx.y * R, r1 = min(r0 + R, h), nr = r1 - r0;
    const int tid = threadIdx.x;
    const float scale = grad_out[0] / (k > 0 ? (float)k : (float)n_valid[0]);
    const float *plane = pred + (size_t)c * h * w;
    for (int i = tid; i < H + W; i += 256) tap[i] = i < H ? lg_tap(i, h, H) : lg_tap(i - H, w, W);
    for (int f = tid; f < nr * w; f += 256) acc[f] = 0.0f;
    __syncthreads();
    for (int i = tid; i < w + nr; i += 256) {
        if (i < w) {
            cj[2 * i] = lg_first(tap + H, W, i - 1);
            cj[2 * i + 1] = lg_first(tap + H, W, i + 1);
        } else {
            const int s = r0 + i - w;
            ri[2 * (i - w)] = lg_first(tap, H, s - 1);
            ri[2 * (i - w) + 1] = lg_first(tap, H, s + 1);
        }
    }
    __syncthreads();
    const int I_lo = ri[0], I_end = ri[2 * (nr - 1) + 1];
    for (int I0 = I_lo; I0 < I_end; I0 += RB) {
        const int nb = min(RB, I_end - I0);
        for (int f = tid; f < nb * W; f += 256) {
            const int rr = f / W, J = f - rr * W, I = I0 + rr;
            const size_t p = (size_t)I * W + J;
            float g = 0.0f;
            if (mask[p]) {
                const int label = labels[p];
                if (lg_valid(label, C, ignore_index)) {
                    const float pr = expf(lg_interp(plane, w, tap[I], tap[H + J]) - lse[p]);
                    g = scale * (label == c ? pr - 1.0f : pr);
                }
            }
            gb[f] = g;
        }
        __syncthreads();
        for (int f = tid; f < nb * w; f += 256) {
            const int rr = f / w, j = f - rr * w;
            const float *grow = gb + rr * W;
            const int J1 = cj[2 * j + 1];
            float a = 0.0f;
            for (int J = cj[2 * j]; J < J1; ++J) a = lg_gather(a, tap[H + J], j, grow[J]);
            ub[f] = a;
        }
        __syncthreads();
        for (int f = tid; f < nr * w; f += 256) {
            const int rr = f / w, j = f - rr * w;
            const int Ia = max(ri[2 * rr], I0), Ib = min(ri[2 * rr + 1], I0 + nb);
            float a = acc[f];
            for (int I = Ia; I < Ib; ++I) a = lg_gather(a, tap[I], r0 + rr, ub[(I - I0) * w + j]);
            acc[f] = a;
        }
        __syncthreads();
    }
    float *out = grad_pred + (size_t)c * h * w + (size_t)r0 * w;
    for (int f = tid; f < nr * w; f += 256) out[f] = acc[f];
}

struct GradPlan { int R, RB, bands; size_t lds; };
// bands so that about 1 024 workgroups exist where the map has the rows for it, not fewer than 4 coarse rows each (the seam rows are computed
// twice); the chunk and the band are halved until the workgroup's LDS fits.  First choices, not tuned.  R == 0: not even one row fits.
GradPlan grad_plan(int C, int h, int w, int H, int W) {
    GradPlan p;
    const int want = (1024 + C - 1) / C;
    int R = (h + want - 1) / want;
    if (R < 4) R = 4;
    if (R > h) R = h;
    int RB = 8;
    if (RB > H) RB = H;
    while (R > 1 && (size_t)R * w * 4 > 24 * 1024) R = (R + 1) / 2;
    while (RB > 1 && grad_lds(w, H, W, R, RB).total > LG_LDS_MAX) RB = (RB + 1) / 2;
    while (R > 1 && grad_lds(w, H, W, R, RB).total > LG_LDS_MAX) R = (R + 1) / 2;
    p.lds = grad_lds(w, H, W, R, RB).total;
    p.R = p.lds <= LG_LDS_MAX ? R : 0;
    p.RB = RB;
    p.bands = p.R ? (h + p.R - 1) / p.R : 0;
    return p;
}

int ce_check(int C, int h, int w, int H, int W) {
    if (C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return AOC_ERR_INVALID_ARG;
    if (C > LG_MAX_C || (int64_t)H * W >= (1ll << 31) || (int64_t)C * h * w >= (1ll << 31)) return AOC_ERR_UNSUPPORTED;
    return AOC_OK;
}

int topk_check(int64_t n) {
    if (n < 1) return AOC_ERR_INVALID_ARG;
    return n >= (1ll << 31) ? AOC_ERR_UNSUPPORTED : AOC_OK;
}

unsigned pass_grid(int64_t n) {
    const int64_t b = (n + 2047) / 2048;
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

}  // namespace

extern "C" {

int64_t aoc_upsample_ce_partials(int64_t n) { return n < 1 ? 0 : (n + 255) / 256; }

int aoc_upsample_ce_forward(const float *pred, const int32_t *labels, int C, int h, int w, int H, int W, int ignore_index, float *loss, float *lse,
                            int32_t *argmax, int32_t *valid_partial, int32_t *bad, aoc_stream_t stream) {
    if (!pred || !labels) return AOC_ERR_INVALID_ARG;
    const int rc = ce_check(C, h, w, H, W);
    if (rc != AOC_OK) return rc;
    if (!loss && !lse && !argmax && !valid_partial && !bad) return AOC_OK;
    hipStream_t st = aoc_hip_stream(stream);
    if (bad && hipMemsetAsync(bad, 0, sizeof(int32_t), st) != hipSuccess) return AOC_ERR_LAUNCH;
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(ce_forward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pred, labels, C, h, w, H, W, ignore_index, loss, lse, argmax,
                       valid_partial, bad);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

size_t aoc_topk_mean_workspace_bytes(int64_t n) { return topk_check(n) == AOC_OK ? topk_ws(n).total : 0; }

int aoc_topk_mean(const float *loss, int64_t n, int64_t k, float *mean, float *thr, int32_t *n_gt, void *workspace, size_t workspace_bytes,
                  aoc_stream_t stream) {
    if (!loss) return AOC_ERR_INVALID_ARG;
    const int rc = topk_check(n);
    if (rc != AOC_OK) return rc;
    if (k < 1 || k > n) return AOC_ERR_INVALID_ARG;
    const TopkWs s = topk_ws(n);
    if (!workspace || workspace_bytes < s.total) return AOC_ERR_WORKSPACE;
    if (!mean && !thr && !n_gt) return AOC_OK;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + s.hist);
    Sel *sel = reinterpret_cast<Sel *>(ws + s.sel);
    float *partial = reinterpret_cast<float *>(ws + s.partial);
    hipStream_t st = aoc_hip_stream(stream);
    if (hipMemsetAsync(hist, 0, 4 * 256 * sizeof(uint32_t), st) != hipSuccess) return AOC_ERR_LAUNCH;
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(topk_pass_kernel, dim3(pass_grid(n)), dim3(256), 0, st, loss, n, (uint32_t)k, pass, hist, sel);
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    const int chunks = lg_chunks(n);
    hipLaunchKernelGGL(topk_sum_kernel, dim3((unsigned)chunks), dim3(256), 0, st, loss, n, lg_chunk(n), 0, hist, sel, partial);
    AOC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(topk_finish_kernel, dim3(1), dim3(64), 0, st, partial, chunks, (uint32_t)k, sel, mean, thr, n_gt);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_valid_mean(const float *loss, int64_t n, const int32_t *valid_partial, int64_t n_partial, float *mean, int32_t *n_valid, void *workspace,
                   size_t workspace_bytes, aoc_stream_t stream) {
    if (!loss || !valid_partial || n_partial < 1) return AOC_ERR_INVALID_ARG;
    const int rc = topk_check(n);
    if (rc != AOC_OK) return rc;
    const TopkWs s = topk_ws(n);
    if (!workspace || workspace_bytes < s.total) return AOC_ERR_WORKSPACE;
    if (!mean && !n_valid) return AOC_OK;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *partial = reinterpret_cast<float *>(ws + s.partial);
    hipStream_t st = aoc_hip_stream(stream);
    const int chunks = lg_chunks(n);
    hipLaunchKernelGGL(topk_sum_kernel, dim3((unsigned)chunks), dim3(256), 0, st, loss, n, lg_chunk(n), 1, (const uint32_t *)nullptr, (Sel *)nullptr, partial);
    AOC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(valid_finish_kernel, dim3(1), dim3(64), 0, st, partial, chunks, valid_partial, n_partial, mean, n_valid);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

size_t aoc_topk_select_mask_workspace_bytes(int64_t n) {
    return topk_check(n) == AOC_OK ? aoc_align_up((size_t)lg_chunks(n) * sizeof(uint32_t), 256) : 0;
}

int aoc_topk_select_mask(const float *loss, int64_t n, int64_t k, const float *thr, const int32_t *n_gt, uint8_t *mask, void *workspace,
                         size_t workspace_bytes, aoc_stream_t stream) {
    if (!loss || !thr || !n_gt || !mask) return AOC_ERR_INVALID_ARG;
    const int rc = topk_check(n);
    if (rc != AOC_OK) return rc;
    if (k < 1 || k > n) return AOC_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < aoc_topk_select_mask_workspace_bytes(n)) return AOC_ERR_WORKSPACE;
    uint32_t *tie_partial = static_cast<uint32_t *>(workspace);
    hipStream_t st = aoc_hip_stream(stream);
    const int chunks = lg_chunks(n);
    hipLaunchKernelGGL(tie_count_kernel, dim3((unsigned)chunks), dim3(256), 0, st, loss, n, lg_chunk(n), thr, tie_partial);
    AOC_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(select_mask_kernel, dim3((unsigned)chunks), dim3(256), 0, st, loss, n, lg_chunk(n), (uint32_t)k, thr, n_gt, tie_partial, mask);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_valid_mask(const int32_t *labels, int64_t n, int C, int ignore_index, uint8_t *mask, aoc_stream_t stream) {
    if (!labels || !mask || C < 1) return AOC_ERR_INVALID_ARG;
    const int rc = topk_check(n);
    if (rc != AOC_OK) return rc;
    if (C > LG_MAX_C) return AOC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(valid_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, aoc_hip_stream(stream), labels, n, C, ignore_index, mask);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

// the forward of one sample as one call: the entries above in their order, the words and counts between them in the workspace
struct CritWs { size_t topk, tie, words, partial, total; };
CritWs crit_ws(int64_t n) {
    CritWs s;
    s.topk = 0;
    s.tie = topk_ws(n).total;
    s.words = s.tie + aoc_align_up((size_t)lg_chunks(n) * sizeof(uint32_t), 256);
    s.partial = s.words + 256;
    s.total = s.partial + aoc_align_up((size_t)((n + 255) / 256) * sizeof(int32_t), 256);
    return s;
}

size_t aoc_criterion_forward_workspace_bytes(int64_t n) { return topk_check(n) == AOC_OK ? crit_ws(n).total : 0; }

int aoc_criterion_forward(const float *pred, const int32_t *labels, int C, int h, int w, int H, int W, int ignore_index, int64_t k, float *loss, float *lse,
                          int32_t *argmax, uint8_t *mask, float *mean, int32_t *n_valid, int32_t *bad, void *workspace, size_t workspace_bytes,
                          aoc_stream_t stream) {
    if (!pred || !labels || !loss || !mean || k < 0) return AOC_ERR_INVALID_ARG;
    int rc = ce_check(C, h, w, H, W);
    if (rc != AOC_OK) return rc;
    const int64_t n = (int64_t)H * W;
    if (k > n) return AOC_ERR_INVALID_ARG;
    const CritWs s = crit_ws(n);
    if (!workspace || workspace_bytes < s.total) return AOC_ERR_WORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *thr = reinterpret_cast<float *>(ws + s.words);
    int32_t *n_gt = reinterpret_cast<int32_t *>(ws + s.words + 16), *nv = n_valid ? n_valid : reinterpret_cast<int32_t *>(ws + s.words + 32);
    int32_t *partial = reinterpret_cast<int32_t *>(ws + s.partial);
    // every argument is validated above: the calls below can only fail in a launch
    if ((rc = aoc_upsample_ce_forward(pred, labels, C, h, w, H, W, ignore_index, loss, lse, argmax, k == 0 ? partial : nullptr, bad, stream)) != AOC_OK) return rc;
    if (k == 0) {
        if ((rc = aoc_valid_mean(loss, n, partial, (n + 255) / 256, mean, nv, ws + s.topk, s.tie, stream)) != AOC_OK) return rc;
        return mask ? aoc_valid_mask(labels, n, C, ignore_index, mask, stream) : AOC_OK;
    }
    if ((rc = aoc_topk_mean(loss, n, k, mean, thr, n_gt, ws + s.topk, s.tie, stream)) != AOC_OK) return rc;
    return mask ? aoc_topk_select_mask(loss, n, k, thr, n_gt, mask, ws + s.tie, s.words - s.tie, stream) : AOC_OK;
}

int aoc_upsample_ce_grad(const float *pred, const int32_t *labels, const float *lse, const uint8_t *mask, const float *grad_out, int64_t k,
                         const int32_t *n_valid, int C, int h, int w, int H, int W, int ignore_index, float *grad_pred, aoc_stream_t stream) {
    if (!pred || !labels || !lse || !mask || !grad_out || !grad_pred || k < 0 || (k == 0 && !n_valid)) return AOC_ERR_INVALID_ARG;
    const int rc = ce_check(C, h, w, H, W);
    if (rc != AOC_OK) return rc;
    if (k > (int64_t)H * W) return AOC_ERR_INVALID_ARG;
    const GradPlan p = grad_plan(C, h, w, H, W);
    if (p.R == 0 || p.bands > 65535) return AOC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ce_grad_kernel, dim3((unsigned)C, (unsigned)p.bands), dim3(256), p.lds, aoc_hip_stream(stream), pred, labels, lse, mask, grad_out, k,
                       n_valid, C, h, w, H, W, ignore_index, p.R, p.RB, grad_pred);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
