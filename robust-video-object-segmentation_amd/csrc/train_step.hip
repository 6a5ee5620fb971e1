// The hand-over between two frames of one training step: what train_manager_mm.py:241-284 does with the prediction once the model has
// returned it --
//   :277        iou = pytorch_iou(all_pred.unsqueeze(1), curr_labels, obj_nums)                 utils/metric.py:3-34
//   :281-282    running_losses[idx].update(loss.item() * seq_len); running_ious[idx].update(iou.item())       utils/meters.py
//   :258-259    prev_labels = all_pred.unsqueeze(1), which aocnet.py:134-135 shrinks with interpolate(mode='nearest').int()
// as ONE call per frame for the whole batch (aoc_frame_handover) and device-resident meters (aoc_meters_update, aoc_meters_reset), so that
// nothing between two frames waits for the device.
//
// Two launches, no atomics on global memory, no float atomics, nothing zeroed in front:
//   count    one workgroup of 256 threads per (sample, strip of 256 columns, band of rows).  A thread owns ONE column of the strip over the
//            band's rows.  Mode 0 (the reference as it is called, per column): the column's two counters stay in registers and are written
//            to the workgroup's own slab row.  Mode 1 (per object): the <= 90 object counters go through LDS integer atomics and the workgroup
//            writes its 90 words.  The workgroups behind the counting ones shrink `pred` by torch's nearest rule (label_onehot_nearest_kernel's
//            expression, memory_policy.hip).  The samples' object numbers travel in the launch's arguments, 256 samples per launch; the first
//            workgroup of a sample leaves its number in the workspace for the finish.
//   finish   one workgroup: per sample the slabs' integer sums (any order: integers), the ratios, the sample's mean in the order stated in
//            include/aoc_hip.h, then the batch mean serially; writes the counts where asked and updates the optional meter.
// Every pointer is class 4: labels are read one element per lane (a column owner's neighbours in the wave read the neighbouring elements, so a
// wave reads whole lines whatever the misalignment), the int64 maps through a 4-byte-aligned type; 16-byte loads would need a thread to own four
// columns and buy nothing at 1.7 MB per call, which is bound by its launches.  Every slab word the finish reads is written by the count launch
// of the same call: the workspace may hold anything.
#include "plane_stream.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_GROUP = 256;                                    // samples per count launch (their obj_num in the arguments)
constexpr int TS_MAX_BANDS = 32;
constexpr int TS_OBJ_WORDS = 3 * AOC_MAX_OBJECTS;                // I, #pred, #gt per object
constexpr int64_t TS_MAX_PLANE = (int64_t)1 << 24;
constexpr int64_t TS_MAX_INDEX = (int64_t)1 << 31;

typedef int64_t i64_a4 __attribute__((aligned(4)));

struct TsNums { uint8_t n[TS_GROUP]; };
struct TsPlan { int strips, bands, rows, blocks; };              // rows per band; blocks per sample = strips * bands

// strips of 256 columns; bands so that the batch fills about 256 workgroups, at most 32 per sample (the finish adds them up) and at most H
TsPlan ts_plan(int bs, int H, int W) {
    TsPlan p;
    p.strips = (W + TS_THREADS - 1) / TS_THREADS;
    const int64_t per = (int64_t)bs * p.strips;
    int64_t bands = (256 + per - 1) / per;
    if (bands > TS_MAX_BANDS) bands = TS_MAX_BANDS;
    if (bands > H) bands = H;
    p.rows = (int)((H + bands - 1) / bands);
    p.bands = (H + p.rows - 1) / p.rows;
    p.blocks = p.strips * p.bands;
    return p;
}

size_t ts_nums_bytes(int bs) { return aoc_align_up((size_t)bs * sizeof(int32_t), 16); }
size_t ts_slab_words(int bs, int W, const TsPlan &p) {
    const size_t columns = (size_t)bs * p.bands * W * 2, objects = (size_t)bs * p.blocks * TS_OBJ_WORDS;
    return columns > objects ? columns : objects;
}

// the object a label names among 1 .. n, else 0: v == o as numbers, so 255, negatives, larger ids and non-integers name nothing
__device__ __forceinline__ int ts_id(const void *__restrict__ p, int code, int64_t i, int n) {
    if (code == AOC_LABEL_I32) {
        const int32_t v = static_cast<const int32_t *>(p)[i];
        return (v >= 1 && v <= n) ? v : 0;
    }
    if (code == AOC_LABEL_I64) {
        const int64_t v = static_cast<const i64_a4 *>(p)[i];
        return (v >= 1 && v <= n) ? (int)v : 0;
    }
    const float v = static_cast<const float *>(p)[i];
    if (!(v >= 1.0f && v <= (float)n)) return 0;
    const int k = (int)v;
    return (float)k == v ? k : 0;
}

// the label as aocnet.py:134-135 hands it on: interpolate(mask.float()).int()
__device__ __forceinline__ int32_t ts_value(const void *__restrict__ p, int code, int64_t i) {
    if (code == AOC_LABEL_I32) return static_cast<const int32_t *>(p)[i];
    if (code == AOC_LABEL_I64) return (int32_t) static_cast<const i64_a4 *>(p)[i];
    return (int)static_cast<const float *>(p)[i];
}

struct TsCount {
    const void *pred, *gt;
    int pcode, gcode;
    int sample0, n_samples;                                      // this launch's samples
    int H, W;
    TsPlan plan;
    unsigned count_blocks;                                       // n_samples * plan.blocks, or 0: only the resize
    uint32_t *slab;
    int32_t *nums;                                               // [bs] in the workspace
    int32_t *prev_small;                                         // or NULL
    int sh, sw;
    float fy, fx;
};

template <int MODE>
__global__ __launch_bounds__(TS_THREADS) void ts_count_kernel(const TsCount a, const TsNums nums) {
    __shared__ uint32_t cnt[TS_OBJ_WORDS];
    const int tid = threadIdx.x;
    if (blockIdx.x >= a.count_blocks) {                          // uniform: the resize workgroups
        const int64_t small = (int64_t)a.sh * a.sw;
        const int64_t j = (int64_t)(blockIdx.x - a.count_blocks) * TS_THREADS + tid;
        if (j >= small * a.n_samples) return;
        const int64_t s = a.sample0 + j / small, r = j % small;
        const int y = (int)(r / a.sw), x = (int)(r % a.sw);
        const int sy = min((int)floorf((float)y * a.fy), a.H - 1);           // torch nearest: floor(dst * in / out)
        const int sx = min((int)floorf((float)x * a.fx), a.W - 1);
        a.prev_small[s * small + r] = ts_value(a.pred, a.pcode, (s * a.H + sy) * a.W + sx);
        return;
    }
    const int band = blockIdx.x % a.plan.bands;
    const int strip = (blockIdx.x / a.plan.bands) % a.plan.strips;
    const int sl = blockIdx.x / a.plan.blocks;
    const int64_t s = a.sample0 + sl;
    const int n = nums.n[sl];
    const int x = strip * TS_THREADS + tid;
    const int y0 = band * a.plan.rows, y1 = min(a.H, y0 + a.plan.rows);
    if (blockIdx.x % a.plan.blocks == 0 && tid == 0) a.nums[s] = n;
    if (MODE == 1) {
        if (tid < TS_OBJ_WORDS) cnt[tid] = 0;
        __syncthreads();
    }
    uint32_t I = 0, U = 0;
    if (x < a.W) {
        int64_t i = (s * a.H + y0) * a.W + x;
#pragma unroll 4
        for (int y = y0; y < y1; ++y, i += a.W) {
            const int p = ts_id(a.pred, a.pcode, i, n), g = ts_id(a.gt, a.gcode, i, n);
            const bool both = p != 0 && p == g;
            if (MODE == 0) {
                I += both;
                U += (uint32_t)(p != 0) + (uint32_t)(g != 0) - (uint32_t)both;
            } else {
                if (p) atomicAdd(&cnt[3 * (p - 1) + 1], 1u);
                if (g) atomicAdd(&cnt[3 * (g - 1) + 2], 1u);
                if (both) atomicAdd(&cnt[3 * (p - 1)], 1u);
            }
        }
        if (MODE == 0) {
            uint32_t *o = a.slab + ((s * a.plan.bands + band) * a.W + x) * 2;
            o[0] = I;
            o[1] = U;
        }
    }
    if (MODE == 1) {
        __syncthreads();
        if (tid < TS_OBJ_WORDS) a.slab[(s * a.plan.blocks + blockIdx.x % a.plan.blocks) * TS_OBJ_WORDS + tid] = cnt[tid];
    }
}

// utils/meters.py:19-23 with x a double
__device__ __forceinline__ void ts_meter_add(aoc_meter *m, double x, int64_t n) {
    const double sum = m->sum + x * (double)n;
    const int64_t count = m->count + n;
    m->val = (float)x;
    m->sum = sum;
    m->count = count;
    m->avg = (float)(sum / (double)count);
}

template <int MODE>
__global__ __launch_bounds__(TS_THREADS) void ts_finish_kernel(const uint32_t *__restrict__ slab, const int32_t *__restrict__ nums, int bs, int W,
                                                               TsPlan plan, float eps, float *__restrict__ iou, float *__restrict__ per_sample,
                                                               uint32_t *__restrict__ counts, aoc_meter *meter) {
    __shared__ float wsum[4];
    const int tid = threadIdx.x;
    float batch = 0.0f;
    int counted = 0;
    for (int64_t s = 0; s < bs; ++s) {
        const int n = nums[s];                                   // uniform
        float acc = 0.0f;
        if (MODE == 0) {
            for (int x = tid; x < W; x += TS_THREADS) {
                uint32_t I = 0, U = 0;
                for (int b = 0; b < plan.bands; ++b) {
                    const uint32_t *c = slab + ((s * plan.bands + b) * W + x) * 2;
                    I += c[0];
                    U += c[1];
                }
                if (counts) {
                    counts[(s * W + x) * 2] = I;
                    counts[(s * W + x) * 2 + 1] = U;
                }
                if (n > 0) acc += ((float)I + eps) / ((float)U + eps);
            }
        } else if (tid < AOC_MAX_OBJECTS) {
            uint32_t I = 0, P = 0, G = 0;
            for (int b = 0; b < plan.blocks; ++b) {
                const uint32_t *c = slab + (s * plan.blocks + b) * TS_OBJ_WORDS + 3 * tid;
                I += c[0];
                P += c[1];
                G += c[2];
            }
            if (counts) {
                uint32_t *o = counts + (s * AOC_MAX_OBJECTS + tid) * 3;
                o[0] = I;
                o[1] = P;
                o[2] = G;
            }
            if (tid < n) acc += ((float)I + eps) / ((float)(P + G - I) + eps);
        }
        const float total = aoc_block_sum256(acc, wsum);
        const float v = n > 0 ? total / (float)(MODE == 0 ? W : n) : 1.0f;
        if (tid == 0) {
            if (per_sample) per_sample[s] = v;
            if (n > 0) {
                batch += v;
                ++counted;
            }
        }
    }
    if (tid == 0) {
        const float r = counted ? batch / (float)counted : 1.0f;
        if (iou) iou[0] = r;
        if (meter) ts_meter_add(meter, (double)r, 1);
    }
}

struct TsMeterArgs {
    const float *value[AOC_METERS_PER_CALL];
    double scale[AOC_METERS_PER_CALL];
    int64_t n[AOC_METERS_PER_CALL];
    int32_t index[AOC_METERS_PER_CALL];
};

__global__ void ts_meters_update_kernel(aoc_meter *__restrict__ meters, const TsMeterArgs a, int k) {
#pragma unroll
    for (int j = 0; j < AOC_METERS_PER_CALL; ++j)                // constant indices into the argument struct
        if ((int)threadIdx.x == j && j < k) ts_meter_add(meters + a.index[j], (double)a.value[j][0] * a.scale[j], a.n[j]);
}

__global__ void ts_meters_reset_kernel(aoc_meter *__restrict__ meters, int n_meters, uint64_t mask) {
    const int i = threadIdx.x;
    if (i < n_meters && ((mask >> i) & 1)) {
        meters[i].val = 0.0f;
        meters[i].avg = 0.0f;
        meters[i].sum = 0.0;
        meters[i].count = 0;
    }
}

bool ts_off(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" {

size_t aoc_frame_handover_workspace_bytes(int bs, int H, int W) {
    if (bs < 1 || H < 1 || W < 1 || (int64_t)H * W > TS_MAX_PLANE || (int64_t)bs * H * W >= TS_MAX_INDEX) return 0;
    return ts_nums_bytes(bs) + ts_slab_words(bs, W, ts_plan(bs, H, W)) * sizeof(uint32_t);
}

int aoc_frame_handover(const void *pred, int pred_dtype, const void *gt, int gt_dtype, int bs, int H, int W, const int32_t *obj_num_host,
                       float epsilon, int mode, int small_h, int small_w, float *iou, float *iou_per_sample, uint32_t *counts, int32_t *prev_small,
                       aoc_meter *meter, void *workspace, size_t workspace_bytes, aoc_stream_t stream) {
    if (bs < 1 || H < 1 || W < 1) return AOC_ERR_INVALID_ARG;
    if ((int64_t)H * W > TS_MAX_PLANE || (int64_t)bs * H * W >= TS_MAX_INDEX) return AOC_ERR_UNSUPPORTED;
    const bool need_counts = iou || iou_per_sample || counts || meter;
    if (!need_counts && !prev_small) return AOC_ERR_INVALID_ARG;
    if (!pred || pred_dtype < AOC_LABEL_I32 || pred_dtype > AOC_LABEL_F32 || ts_off(pred, 4)) return AOC_ERR_INVALID_ARG;
    if (ts_off(iou, 4) || ts_off(iou_per_sample, 4) || ts_off(counts, 4) || ts_off(prev_small, 4) || ts_off(meter, 8)) return AOC_ERR_INVALID_ARG;
    if (prev_small) {
        if (small_h < 1 || small_w < 1) return AOC_ERR_INVALID_ARG;
        if ((int64_t)bs * small_h * small_w >= TS_MAX_INDEX) return AOC_ERR_UNSUPPORTED;
    }
    TsPlan plan = ts_plan(bs, H, W);
    if (need_counts) {
        if (!gt || gt_dtype < AOC_LABEL_I32 || gt_dtype > AOC_LABEL_F32 || ts_off(gt, 4)) return AOC_ERR_INVALID_ARG;
        if ((mode != AOC_IOU_PER_COLUMN && mode != AOC_IOU_PER_OBJECT) || !obj_num_host || !(epsilon >= 0.0f)) return AOC_ERR_INVALID_ARG;
        for (int s = 0; s < bs; ++s) {
            if (obj_num_host[s] < 0) return AOC_ERR_INVALID_ARG;
            if (obj_num_host[s] > AOC_MAX_OBJECTS) return AOC_ERR_UNSUPPORTED;
        }
        if (!workspace || ts_off(workspace, 4)) return AOC_ERR_INVALID_ARG;
        if (workspace_bytes < aoc_frame_handover_workspace_bytes(bs, H, W)) return AOC_ERR_WORKSPACE;
    }
    const int group = bs < TS_GROUP ? bs : TS_GROUP;
    const int64_t resize_blocks = prev_small ? ((int64_t)group * small_h * small_w + TS_THREADS - 1) / TS_THREADS : 0;
    if ((need_counts ? (int64_t)group * plan.blocks : 0) + resize_blocks >= TS_MAX_INDEX) return AOC_ERR_UNSUPPORTED;

    TsCount a;
    a.pred = pred, a.gt = gt, a.pcode = pred_dtype, a.gcode = gt_dtype;
    a.H = H, a.W = W, a.plan = plan;
    a.nums = static_cast<int32_t *>(workspace);
    a.slab = need_counts ? reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(workspace) + ts_nums_bytes(bs)) : nullptr;
    a.prev_small = prev_small, a.sh = small_h, a.sw = small_w;
    a.fy = prev_small ? (float)H / (float)small_h : 0.0f;
    a.fx = prev_small ? (float)W / (float)small_w : 0.0f;
    for (int s0 = 0; s0 < bs; s0 += TS_GROUP) {
        a.sample0 = s0;
        a.n_samples = bs - s0 < TS_GROUP ? bs - s0 : TS_GROUP;
        a.count_blocks = need_counts ? (unsigned)a.n_samples * (unsigned)plan.blocks : 0u;
        TsNums nums = {};
        for (int s = 0; need_counts && s < a.n_samples; ++s) nums.n[s] = (uint8_t)obj_num_host[s0 + s];
        const int64_t small = prev_small ? ((int64_t)a.n_samples * small_h * small_w + TS_THREADS - 1) / TS_THREADS : 0;
        const dim3 grid((unsigned)(a.count_blocks + small));
        if (need_counts && mode == AOC_IOU_PER_OBJECT) hipLaunchKernelGGL(ts_count_kernel<1>, grid, dim3(TS_THREADS), 0, aoc_hip_stream(stream), a, nums);
        else hipLaunchKernelGGL(ts_count_kernel<0>, grid, dim3(TS_THREADS), 0, aoc_hip_stream(stream), a, nums);
        AOC_RETURN_IF_LAUNCH_FAILED();
    }
    if (!need_counts) return AOC_OK;
    if (mode == AOC_IOU_PER_OBJECT)
        hipLaunchKernelGGL(ts_finish_kernel<1>, dim3(1), dim3(TS_THREADS), 0, aoc_hip_stream(stream), a.slab, a.nums, bs, W, plan, epsilon, iou, iou_per_sample,
                           counts, meter);
    else
        hipLaunchKernelGGL(ts_finish_kernel<0>, dim3(1), dim3(TS_THREADS), 0, aoc_hip_stream(stream), a.slab, a.nums, bs, W, plan, epsilon, iou, iou_per_sample,
                           counts, meter);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_meters_update(aoc_meter *meters, int n_meters, const int32_t *index_host, const float *const *values_host, const double *scale_host,
                      const int64_t *n_host, int k, aoc_stream_t stream) {
    if (!meters || ts_off(meters, 8) || n_meters < 1 || k < 0 || (k > 0 && (!index_host || !values_host || !scale_host || !n_host))) return AOC_ERR_INVALID_ARG;
    if (k > AOC_METERS_PER_CALL) return AOC_ERR_UNSUPPORTED;
    TsMeterArgs a = {};
    for (int j = 0; j < k; ++j) {
        if (index_host[j] < 0 || index_host[j] >= n_meters || !values_host[j] || ts_off(values_host[j], 4) || n_host[j] < 1) return AOC_ERR_INVALID_ARG;
        for (int i = 0; i < j; ++i)
            if (index_host[i] == index_host[j]) return AOC_ERR_INVALID_ARG;          // two updates of one meter in one launch would race
        a.value[j] = values_host[j], a.scale[j] = scale_host[j], a.n[j] = n_host[j], a.index[j] = index_host[j];
    }
    if (k == 0) return AOC_OK;
    hipLaunchKernelGGL(ts_meters_update_kernel, dim3(1), dim3(64), 0, aoc_hip_stream(stream), meters, a, k);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

int aoc_meters_reset(aoc_meter *meters, int n_meters, uint64_t mask, aoc_stream_t stream) {
    if (!meters || ts_off(meters, 8) || n_meters < 1) return AOC_ERR_INVALID_ARG;
    if (n_meters > 64) return AOC_ERR_UNSUPPORTED;
    if (n_meters < 64 && (mask >> n_meters) != 0) return AOC_ERR_INVALID_ARG;
    if (mask == 0) return AOC_OK;
    hipLaunchKernelGGL(ts_meters_reset_kernel, dim3(1), dim3(64), 0, aoc_hip_stream(stream), meters, n_meters, mask);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}

}  // extern "C"
