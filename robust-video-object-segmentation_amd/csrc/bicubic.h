// The bicubic tap weights of the decoder tail (decoder_tail.hip) and of its adjoint (tail_grad.hip): the forward and its adjoint share every
// weight's bits because both take them from here.
//
// Semantics are those of PyTorch's upsample_bicubic2d (A = -0.75, four taps per axis at floor(src) - 1 .. + 2, tap indices clamped to the map,
// src = o (in - 1) / (out - 1) or 0 for out = 1), with the coordinate split in integers: the tap index is exact and the fraction
// t = float(o (in - 1) mod (out - 1)) / float(out - 1) carries one rounding.
#pragma once
#include "aoc_common.h"

constexpr float BC_A = -0.75f;

// weights of the four taps of output index o and the index of the second one (taps at i0 - 1 .. i0 + 2, clamped by the caller).
// Nothing fuses (-ffp-contract=off): tests/decoder_tail_bounds.py restates these expressions rounding by rounding.
__device__ __forceinline__ f32x4 bicubic_taps(int o, int in, int out, int &i0) {
    float t = 0.0f;
    i0 = 0;
    if (out > 1) {
        const int64_t num = (int64_t)o * (in - 1);
        i0 = (int)(num / (out - 1));
        t = (float)(int)(num - (int64_t)i0 * (out - 1)) / (float)(out - 1);
    }
    const float x0 = t + 1.0f, u = 1.0f - t, x3 = u + 1.0f;
    f32x4 wt;
    wt.x = ((BC_A * x0 - 5.0f * BC_A) * x0 + 8.0f * BC_A) * x0 - 4.0f * BC_A;
    wt.y = ((BC_A + 2.0f) * t - (BC_A + 3.0f)) * t * t + 1.0f;
    wt.z = ((BC_A + 2.0f) * u - (BC_A + 3.0f)) * u * u + 1.0f;
    wt.w = ((BC_A * x3 - 5.0f * BC_A) * x3 + 8.0f * BC_A) * x3 - 4.0f * BC_A;
    return wt;
}
