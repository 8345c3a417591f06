// The local-scaling formulas (DESIGN.md "Local scaling"), stated once for the exhaustive kernel (nr_localscale.hip) and the
// candidate kernel (nr_cand_localscale.hip): the same inputs give the same bits in both.
//
//   csls:  fl(fl(2 s - row) - col)                                                    row, col: the neighbourhood means
//   nicdm: -fl(d / fl(sqrt(fl(a b)))),  d = max(fl(1 - s), 0),  a = max(fl(1 - row), EPS),  b likewise     (means)
//   ls:    -fl(fl(d d) / fl(a b))                                                                          (k-th values)
//
// Every operation is rounded once: products, sums and differences are nr_round.h's, the divide and the square root are the
// correctly rounded ones.  A NaN passes through every max.
#pragma once
#include "nr_round.h"
#include "../../include/nr_hip.h"

// EPS = NR_SCALE_EPS = 2^-20 (nr_common.h: mutual proximity floors its deviations at the same constant).
// What the score takes of an item's statistic: the statistic itself for csls, its floored distance scale for nicdm / ls.  A caller
// with many scores of one item computes it once.
__device__ __forceinline__ float nr_ls_operand(int mode, float stat) {
    return mode == NR_LOCALSCALE_CSLS ? stat : nr_floor(nr_rn_sub(1.f, stat), NR_SCALE_EPS);
}

// One corrected score from the raw score s and the row's and the column's nr_ls_operand.
__device__ __forceinline__ float nr_ls_score(int mode, float s, float row, float col) {
    if (mode == NR_LOCALSCALE_CSLS) return nr_rn_sub(nr_rn_sub(nr_rn_mul(2.f, s), row), col);
    const float d = nr_floor(nr_rn_sub(1.f, s), 0.f);
    const float ab = nr_rn_mul(row, col);
    if (mode == NR_LOCALSCALE_NICDM) return -__fdiv_rn(d, __fsqrt_rn(ab));
    return -__fdiv_rn(nr_rn_mul(d, d), ab);
}
