// What the windowed matching kernels of local_match.hip (inference) and local_grad.hip (training, with an argmin) share on the host and
// at their start: the radii struct, its validation, the ring -> class table.  The register-operand kernels of the two files
// (local_window_reg_kernel, lg_window_reg_argmin_kernel) are still two texts of one walk, their fills written out: STATUS.md has what the two
// attempts at one body cost.
#pragma once
#include "aoc_common.h"

constexpr int LW_MAX_RADII = 8;
struct LocalRadii {
    int32_t r[LW_MAX_RADII];
    int32_t n;
};

// Host: radii_host (pixels, strictly ascending, >= 0) -> radii in units of the atrous rate: ring a = max(|dy|, |dx|) / rate, only offsets
// that are multiples of the rate exist (AEM:949 pad_max_distance = max - max % rate with the unfold's stride = atrous_rate, AEM:1039
// local_dis // rate).  The window half-size in pixels is rate * radii.r[n - 1].  The caller has checked 1 <= n_radii <= LW_MAX_RADII and
// atrous_rate >= 1.
static inline int lw_radii_from_host(const int32_t *radii_host, int n_radii, int atrous_rate, LocalRadii &radii) {
    radii.n = n_radii;
    for (int i = 0; i < n_radii; ++i) {
        if (radii_host[i] < 0 || (i > 0 && radii_host[i] <= radii_host[i - 1])) return AOC_ERR_INVALID_ARG;
        radii.r[i] = radii_host[i] / atrous_rate;
    }
    for (int i = n_radii; i < LW_MAX_RADII; ++i) radii.r[i] = radii.r[n_radii - 1];
    return AOC_OK;
}

// Device: lcls[a] = the first class (nested window) whose radius reaches ring a, a = 0 .. RA = radii.r[radii.n - 1] (the window half-size
// in atrous units, which every caller has at hand); thread a writes entry a.  The caller synchronises before the table is read.
__device__ __forceinline__ void lw_ring_classes(const LocalRadii &radii, int RA, int32_t *lcls) {
    if ((int)threadIdx.x <= RA) {
        int c = 0;
        while (radii.r[c] < (int)threadIdx.x) ++c;
        lcls[threadIdx.x] = c;
    }
}
