// The mutual-proximity formulas (DESIGN.md "Mutual proximity"), stated once for the exhaustive kernels (nr_mutualprox.hip) and the
// candidate kernel (nr_cand_mutualprox.hip): the same inputs give the same bits in both.
//
//   emp:   r2(s, X) = 2 #{x in X : x < s} + #{x in X : x == s},  c(X) = #{x in X : x is not NaN}
//          T = fl(fl(fl(r2_row) / fl(2 c_row)) fl(fl(r2_col) / fl(2 c_col)))
//   gauss: z = fl(fl(s - mean) / max(sd, EPS)),  Q = fl(0.5 erfc(fl(z fl(1 / sqrt 2)))),  T = -fl(fl(Q_r + Q_c) - fl(Q_r Q_c))
//          EPS = NR_SCALE_EPS = 2^-20, the max is nr_floor (nr_common.h): it keeps a NaN sd
//
// Every float operation is rounded once: products, sums and differences are nr_round.h's, the divide is the correctly rounded one.
// The product and the sum are commutative: neither formula needs to know which of its two lines is the row.
#pragma once
#include "nr_round.h"

#define NR_MP_LINE_MAX (1 << 23)                 // 2 c must stay below 2^24: the counts convert to fp32 exactly
#define NR_MP_RSQRT2 0.707106781186547524f       // fl(1 / sqrt 2)

// 2 [x < s] + [x == s] = [x < s] + [x <= s]: two compares and two adds per pair; a NaN on either side adds nothing
__device__ __forceinline__ int nr_mp_pair(float x, float s) { return (int)(x < s) + (int)(x <= s); }

__device__ __forceinline__ float nr_mp_emp_score(float s, int r2, float row_den, int c2, int col_cnt) {
    const float p = __fdiv_rn((float)r2, row_den);
    const float q = __fdiv_rn((float)c2, (float)(2 * col_cnt));
    return s != s ? s : nr_rn_mul(p, q);
}

__device__ __forceinline__ float nr_mp_tail(float s, float mean, float sd) {
    const float z = __fdiv_rn(nr_rn_sub(s, mean), nr_floor(sd, NR_SCALE_EPS));
    return nr_rn_mul(0.5f, erfcf(nr_rn_mul(z, NR_MP_RSQRT2)));
}

__device__ __forceinline__ float nr_mp_gauss_score(float s, float rm, float rs, float cm, float cs) {
    const float a = nr_mp_tail(s, rm, rs), b = nr_mp_tail(s, cm, cs);
    return -nr_rn_sub(nr_rn_add(a, b), nr_rn_mul(a, b));
}
