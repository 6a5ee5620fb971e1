// Test-time augmentation merge (--flip / --ms of tools/eval_net_mm_rpa.py:21-23): the tail of one frame of
// networks/engine/eval_manager_mm.py for a LIST of augmented samples, as ONE launch.  Per augmentation the reference runs
// interpolate(bilinear, align_corners=True) of the decoder's logits to image size and a soft-max (networks/aoc/aocnet.py:103-106), zeroes the
// never-seen channels (:253-265), flips the maps of a mirrored sample back (:285-286); then cat / mean / argmax (:318-320), the join of newly
// annotated objects (:321-326), the Shannon entropy (networks/layers/shannon_entropy.py:10-13) and the substitution of 125 (:339-346, :357-361).
// All of it is a per-pixel function of the A x n_ch low-resolution logit planes (L2-resident, every value reused by ~16 output pixels).
#include "aoc_common.h"

namespace {

// align_corners=True source position of local_match.hip's bilinear_src (torch's area_pixel_compute_source_index), same roundings
__device__ __forceinline__ void tta_src(int dst, float scale, int in_size, int &i0, int &i1, float &l0, float &l1) {
    const float real = scale * (float)dst;
    i0 = (int)real;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
    float lam = real - (float)i0;
    lam = fminf(fmaxf(lam, 0.0f), 1.0f);
    l1 = lam;
    l0 = 1.0f - lam;
}

// p[c] = softmax_c(bilinear(logits)[c]) at source column position xs of the augmentation's own orientation, never-seen channels zeroed AFTER the
// soft-max (no renormalisation).  Channels >= n_ch (the bucket's padding) are 0.
template <int NC>
__device__ __forceinline__ void tta_probs(const float *__restrict__ logits, int64_t plane_stride, int n_ch, uint32_t exist_bits, int w, float sw,
                                          size_t row0, size_t row1, float hy0, float hy1, int xs, float (&p)[NC]) {
    int x0, x1;
    float wx0, wx1;
    tta_src(xs, sw, w, x0, x1, wx0, wx1);
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c < n_ch) {
            const float *ip = logits + (size_t)c * plane_stride;
            const float v00 = ip[row0 + x0], v01 = ip[row0 + x1], v10 = ip[row1 + x0], v11 = ip[row1 + x1];
            p[c] = hy0 * (wx0 * v00 + wx1 * v01) + hy1 * (wx0 * v10 + wx1 * v11);      // the blend of resize_bilinear_planes_kernel
            m = fmaxf(m, p[c]);
        }
    }
    float den = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        p[c] = (c < n_ch) ? expf(p[c] - m) : 0.0f;
        den += p[c];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = (c < n_ch && ((exist_bits >> c) & 1u)) ? p[c] / den : 0.0f;     // :257-259 zeros_like for unseen labels
}

template <int NC>
__device__ __forceinline__ float tta_entropy(const float (&p)[NC], int n_ch, uint32_t seen_bits) {
    float ent = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (c < n_ch && ((seen_bits >> c) & 1u)) ent += p[c] * logf(p[c] + 1e-6f);      // shannon_entropy.py:11 over all_pred_exist
    return -1.0f * ent;
}

// PX values to PX consecutive elements of a row: one 16- / 8-byte store when all PX are live and the address allows, scalar stores otherwise
template <typename T, int PX>
__device__ __forceinline__ void tta_store(T *__restrict__ dst, const T (&v)[PX], int x0, int W) {
    if (PX == 4 && x0 >= 0 && x0 + 4 <= W && (reinterpret_cast<uintptr_t>(dst + x0) & 15u) == 0) {
        typedef T vec4 __attribute__((ext_vector_type(4)));
        vec4 q = {v[0], v[PX > 1 ? 1 : 0], v[PX > 2 ? 2 : 0], v[PX > 3 ? 3 : 0]};
        *reinterpret_cast<vec4 *>(dst + x0) = q;
        return;
    }
    if (PX == 2 && x0 >= 0 && x0 + 2 <= W && (reinterpret_cast<uintptr_t>(dst + x0) & 7u) == 0) {
        typedef T vec2 __attribute__((ext_vector_type(2)));
        vec2 q = {v[0], v[PX > 1 ? 1 : 0]};
        *reinterpret_cast<vec2 *>(dst + x0) = q;
        return;
    }
#pragma unroll
    for (int i = 0; i < PX; ++i)
        if (x0 + i >= 0 && x0 + i < W) dst[x0 + i] = v[i];
}

// One thread owns PX consecutive pixels of one output row: the row weights of every augmentation are computed once, the NC per-channel sums of
// each pixel stay in registers (every channel loop is unrolled over the compile-time bucket NC >= n_ch).  The PX-pixel groups of row y start at
// -((y W) mod PX), so that a whole group is PX-aligned in the [H, W] maps whatever W is.
template <int NC, int PX>
__global__ __launch_bounds__(256) void tta_merge_kernel(const aoc_tta_desc d, int groups_per_row) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)groups_per_row * d.H) return;
    const int y = (int)(idx / groups_per_row);
    const int W = d.W;
    const int x0 = (int)(idx - (int64_t)y * groups_per_row) * PX - (int)(((int64_t)y * W) & (PX - 1));
    if (x0 >= W) return;
    const int n_ch = d.n_ch, n_aug = d.n_aug;

    float s[PX][NC];
    float ent[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        ent[i] = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; ++c) s[i][c] = 0.0f;
    }
    for (int a = 0; a < n_aug; ++a) {
        const float *logits = d.logits[a];
        const int64_t plane_stride = d.plane_stride[a];
        const int w = d.w[a], flip = d.flip[a];
        const uint32_t bits = d.exist_bits[a];
        const float sw = d.scale_w[a];
        int y0, y1;
        float hy0, hy1;
        tta_src(y, d.scale_h[a], d.h[a], y0, y1, hy0, hy1);
        const size_t row0 = (size_t)y0 * w, row1 = (size_t)y1 * w;
        const bool own = d.mode == 0 && a == n_aug - 1;         // mode 0: the entropy of the LAST augmentation's maps (:306 / :339 read what the loop left)
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int x = min(max(x0 + i, 0), W - 1);            // dead pixels of an edge group compute a live one's values and store nothing
            float p[NC];
            tta_probs<NC>(logits, plane_stride, n_ch, bits, w, sw, row0, row1, hy0, hy1, flip ? W - 1 - x : x, p);   // :285-286 flipped back
#pragma unroll
            for (int c = 0; c < NC; ++c) s[i][c] += p[c];
            if (own) {
                // ... in ITS OWN orientation: all_pred_exist is built before the flip of :286.  A mirrored last augmentation is sampled again
                // at x (cheaper than exchanging the values with the thread that owns W - 1 - x)
                if (flip) tta_probs<NC>(logits, plane_stride, n_ch, bits, w, sw, row0, row1, hy0, hy1, x, p);
                ent[i] = tta_entropy<NC>(p, n_ch, bits);
            }
        }
    }

    const uint32_t seen = d.exist_bits[n_aug - 1];
    const float fa = (float)n_aug;
    int32_t label[PX], conf[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        float best = 0.0f;
        int arg = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < n_ch && (c == 0 || s[i][c] > best)) { best = s[i][c]; arg = c; }     // first maximum (torch.argmax); mean = s / A keeps the order
        if (d.mode != 0) {
            float m[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) m[c] = s[i][c] / fa;
            ent[i] = tta_entropy<NC>(m, n_ch, seen);
        }
        int lab = arg;
        float e = ent[i];
        const int x = x0 + i;
        if (d.join_label && x >= 0 && x < W) {
            const int jl = d.join_label[(size_t)y * W + x];
            const int keep = (jl == 0) ? 1 : 0;                                           // :321-323
            lab = lab * keep + jl * (1 - keep);
            e = e * (float)keep + ((jl < 0) ? 1.0f : 0.0f) * (float)(1 - keep);           // :341-343
        }
        const int region = (e > d.unc_ratio) ? 1 : 0;                                     // :345
        label[i] = lab;
        conf[i] = lab * (1 - region) + 125 * region;                                      // :346
        ent[i] = e;
    }

    const size_t row = (size_t)y * W;
    if (d.label) tta_store<int32_t, PX>(d.label + row, label, x0, W);
    if (d.confident) tta_store<int32_t, PX>(d.confident + row, conf, x0, W);
    if (d.entropy) tta_store<float, PX>(d.entropy + row, ent, x0, W);
    if (d.label_flipped || d.confident_flipped) {
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int x = x0 + i;
            if (x < 0 || x >= W) continue;
            if (d.label_flipped) d.label_flipped[row + (W - 1 - x)] = label[i];           // :327-329 flip_tensor(pred_label, 1)
            if (d.confident_flipped) d.confident_flipped[row + (W - 1 - x)] = conf[i];
        }
    }
    if (d.mean_probs) {
        const size_t hw = (size_t)d.H * W;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < n_ch) {
                float m[PX];
#pragma unroll
                for (int i = 0; i < PX; ++i) m[i] = s[i][c] / fa;
                tta_store<float, PX>(d.mean_probs + c * hw + row, m, x0, W);
            }
        }
    }
}

template <int NC, int PX>
void tta_launch(const aoc_tta_desc &d, hipStream_t st) {
    const int groups_per_row = (d.W + PX - 1) / PX + (PX > 1 ? 1 : 0);      // + 1: the first group of a row may start left of it
    const int64_t total = (int64_t)groups_per_row * d.H;
    hipLaunchKernelGGL((tta_merge_kernel<NC, PX>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d, groups_per_row);
}

}  // namespace

extern "C" int aoc_tta_merge(const aoc_tta_desc *desc, aoc_stream_t stream) {
    if (!desc) return AOC_ERR_INVALID_ARG;
    aoc_tta_desc d = *desc;
    if (d.n_aug < 1 || d.n_ch < 1 || d.H < 1 || d.W < 1 || (d.mode != 0 && d.mode != 1)) return AOC_ERR_INVALID_ARG;
    if (d.n_aug > AOC_MAX_TTA_AUGS || d.n_ch > 32) return AOC_ERR_UNSUPPORTED;
    if ((int64_t)d.H * d.W > (int64_t)1 << 30) return AOC_ERR_UNSUPPORTED;
    for (int a = 0; a < d.n_aug; ++a) {
        if (!d.logits[a] || d.h[a] < 1 || d.w[a] < 1 || d.plane_stride[a] < (int64_t)d.h[a] * d.w[a]) return AOC_ERR_INVALID_ARG;
        if (d.flip[a] != 0 && d.flip[a] != 1) return AOC_ERR_INVALID_ARG;
        if ((int64_t)d.h[a] * d.w[a] > (int64_t)1 << 30) return AOC_ERR_UNSUPPORTED;
        d.scale_h[a] = d.H > 1 ? (float)(d.h[a] - 1) / (float)(d.H - 1) : 0.0f;      // align_corners=True
        d.scale_w[a] = d.W > 1 ? (float)(d.w[a] - 1) / (float)(d.W - 1) : 0.0f;
    }
    if (d.mode == 0 && d.confident_flipped) return AOC_ERR_INVALID_ARG;   // the reference's entropy has no mirrored counterpart
    if (!d.label && !d.confident && !d.label_flipped && !d.confident_flipped && !d.entropy && !d.mean_probs) return AOC_ERR_INVALID_ARG;
    hipStream_t st = aoc_hip_stream(stream);
    if (d.n_ch <= 4) tta_launch<4, 4>(d, st);
    else if (d.n_ch <= 8) tta_launch<8, 4>(d, st);
    else if (d.n_ch <= 16) tta_launch<16, 2>(d, st);
    else tta_launch<32, 1>(d, st);
    AOC_RETURN_IF_LAUNCH_FAILED();
    return AOC_OK;
}
