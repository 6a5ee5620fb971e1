// The backward of gct_gate_body (calibration.hip) on one parameter set, by a workgroup of 256 threads: aoc_gct_gate_grad (gate_grad.hip),
// every set of aoc_gct_gate_multi_grad and the concatenation's GCT of aoc_groupnorm_cat_relu_grad (aspp_grad.hip) run THIS routine, so a set
// of the multi entry carries the bits of the single one.
//
// The workgroup walks the samples n in ascending order; the thread that owns channel c adds sample n's term to the three parameter gradients
// of c (a plain read-modify-write of its own element: no other thread touches it).  The two sums over c per sample (M and the dM numerator)
// are block sums: per thread ascending c, then aoc_block_sum256.  wsum: four floats of LDS.
#pragma once
#include "plane_stream.h"

__device__ __forceinline__ void gct_gate_grad_body(const float *__restrict__ dgate, const float *__restrict__ gate, const float *__restrict__ s,
                                                   const float *__restrict__ alpha, const float *__restrict__ gamma, int N, int C, float eps, int l1,
                                                   float *__restrict__ dsum, float *__restrict__ grad_alpha, float *__restrict__ grad_gamma,
                                                   float *__restrict__ grad_beta, float *wsum) {
    for (int n = 0; n < N; ++n) {
        const size_t row = (size_t)n * C;
        float pm = 0.0f, pd = 0.0f;
        for (int c = threadIdx.x; c < C; c += 256) {
            const float sv = s[row + c];
            const float e = l1 ? sv * alpha[c] : sqrtf(sv + eps) * alpha[c];
            const float t = gate[row + c] - 1.0f;
            const float du = dgate[row + c] * (1.0f - t * t);
            pm += l1 ? fabsf(e) : e * e;
            pd += (du * e) * gamma[c];
        }
        const float M = aoc_block_sum256(pm, wsum) / (float)C;
        const float num = aoc_block_sum256(pd, wsum);
        // l2: norm = gamma / r, r = sqrt(M + eps), dM = -1/2 num / (r (M + eps));   l1: norm = gamma / q, q = M + eps, dM = -num / q^2
        const float q = M + eps;
        const float r = l1 ? q : sqrtf(q);
        const float dM = l1 ? -num / (q * q) : -0.5f * num / (r * q);
        for (int c = threadIdx.x; c < C; c += 256) {
            const float sv = s[row + c];
            const float root = l1 ? sv : sqrtf(sv + eps);               // de/dalpha
            const float e = root * alpha[c];
            const float t = gate[row + c] - 1.0f;
            const float du = dgate[row + c] * (1.0f - t * t);
            const float de = l1 ? du * (gamma[c] / r) + aoc_sign(e) * dM / (float)C : du * (gamma[c] / r) + 2.0f * e * dM / (float)C;
            if (dsum) dsum[row + c] = l1 ? de * alpha[c] : de * alpha[c] / (2.0f * root);
            if (grad_alpha) grad_alpha[c] = (n ? grad_alpha[c] : 0.0f) + de * root;
            if (grad_gamma) grad_gamma[c] = (n ? grad_gamma[c] : 0.0f) + du * e / r;
            if (grad_beta) grad_beta[c] = (n ? grad_beta[c] : 0.0f) + du;
        }
    }
}
