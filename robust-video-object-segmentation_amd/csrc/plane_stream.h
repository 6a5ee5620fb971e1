// The toolkit of the kernels that stream activation planes [planes, hw] (calibration.hip and the *_grad.hip files beside it).
//
// A streamed plane is cut by the alignment of ONE pointer -- the plane that is written, or the gradient plane that is read where nothing is
// written: aoc_front(p, hw) scalar floats in front (up to three), 16 bytes per lane for the body, up to three scalars behind.  Every other
// operand is accessed 16 bytes per lane through a vector type that promises the compiler 4-byte alignment only (one global_load_dwordx4
// whatever the misalignment), so planes at other misalignments (odd hw, several base pointers) never fall back to scalars.  The cut is part of
// every plane sum's order, and with it of the result's bits: a forward and its gradient that must agree on a sum take the cut here.
#pragma once
#include "aoc_common.h"

typedef f32x4 f32x4_a4 __attribute__((aligned(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef i32x4 i32x4_a4 __attribute__((aligned(4)));

__device__ __forceinline__ f32x4 aoc_load4(const float *p) { return *reinterpret_cast<const f32x4_a4 *>(p); }
// the same load for a plane that is read once
__device__ __forceinline__ f32x4 aoc_stream_load4(const float *p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4_a4 *>(p)); }
__device__ __forceinline__ i32x4 aoc_load4i(const int32_t *p) { return *reinterpret_cast<const i32x4_a4 *>(p); }
__device__ __forceinline__ void aoc_store4_a4(float *p, const f32x4 v) { *reinterpret_cast<f32x4_a4 *>(p) = v; }
// 16 bytes per lane to a destination that shares the cut's alignment (nontemporal: a pure stream-out), else at 4-byte alignment
__device__ __forceinline__ void aoc_store4(float *p, const f32x4 v, bool aligned16) {
    if (aligned16) __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(p));
    else aoc_store4_a4(p, v);
}
// floats from p up to the 16-byte grid, at most the whole plane
__device__ __forceinline__ int64_t aoc_front(const void *p, int64_t hw) {
    const int64_t n = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4;
    return n < hw ? n : hw;
}

__device__ __forceinline__ float aoc_sign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }      // torch.sign: sign(0) = 0
// acc + <a, b>: components .x .y .z .w in turn, each product rounded before it is added (-ffp-contract=off)
__device__ __forceinline__ float aoc_dot4(float acc, const f32x4 a, const f32x4 b) {
    acc += a[0] * b[0]; acc += a[1] * b[1]; acc += a[2] * b[2]; acc += a[3] * b[3];
    return acc;
}
// Sum over a workgroup of 256 threads, on every thread: the xor butterfly of aoc_wave_sum, then the four wave sums as (0 + 1) + (2 + 3).
// wsum: four floats of LDS; holds two barriers.
__device__ __forceinline__ float aoc_block_sum256(float v, float *wsum) {
    v = aoc_wave_sum(v);
    __syncthreads();                       // wsum may still be read from the previous use
    if (aoc_lane() == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// Host arrays of device pointers travel in the kernel's argument struct.
constexpr int AOC_PTR_LIST = 8;
struct AocSrcList { const float *p[AOC_PTR_LIST]; };
struct AocDstList { float *p[AOC_PTR_LIST]; };
// the pointer of set k out of the argument struct without a dynamically indexed private array
template <typename List>
__device__ __forceinline__ auto aoc_pick(const List &s, int k) {
    auto p = s.p[0];
#pragma unroll
    for (int j = 1; j < AOC_PTR_LIST; ++j)
        if (k == j) p = s.p[j];
    return p;
}

// slices (workgroups of 256 threads on grid.y) of an apply pass over one plane: one float4 per thread, at most eight slices
static inline unsigned aoc_plane_slices(int64_t hw) {
    const int64_t bx = (hw / 4 + 255) / 256;
    return (unsigned)(bx < 1 ? 1 : (bx > 8 ? 8 : bx));
}
