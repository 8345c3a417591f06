// Online (max, sum) log-sum-exp pairs shared by the test-time normalisation kernels (nr_hubnorm.hip, nr_sinknorm.hip).  Every
// operation says how it is rounded (nr_round.h): a difference of maxima and a sum are values of their own, the rescaled sum is one
// fused multiply-add.
#pragma once
#include "nr_round.h"

#define NR_HN_ROWS 64          // rows per column-partial block: the workspace holds ceil(n / 64) pairs per column

// (m, s) <- (m, s) merged with one more pair (m2, s2); entries equal to the larger max scale by exactly 1.  Symmetric in its
// two arguments, bit for bit (fp32 addition and multiplication commute).
__device__ __forceinline__ void nr_hn_merge(float& m, float& s, float m2, float s2) {
    if (s2 == 0.f) return;                       // an empty pair (no entry)
    if (s == 0.f) { m = m2; s = s2; return; }
    if (m2 > m) {
        s = fmaf(s, expf(nr_rn_sub(m, m2)), s2);
        m = m2;
    } else if (m2 == m) {
        s = nr_rn_add(s, s2);
    } else {
        s = fmaf(s2, expf(nr_rn_sub(m2, m)), s);
    }
}

__device__ __forceinline__ void nr_hn_add(float& m, float& s, float beta, float x) {
    if (x != x) return;                          // NaN: skipped
    nr_hn_merge(m, s, nr_rn_mul(beta, x), 1.f);
}

__device__ __forceinline__ float nr_hn_lse(float m, float s) { return s > 0.f ? nr_rn_add(m, logf(s)) : -INFINITY; }
