// fp32 products, sums and differences that are rounded on their own (DESIGN.md "What is rounded once").
//
// hipcc's __fmul_rn / __fadd_rn / __fsub_rn do not do this: they are plain operators, compiled under the default contraction, and
// once they are inlined next to a sum the compiler may fuse the pair into one multiply-add -- whether it does depends on how many
// uses the product has and on what got inlined where.  The three below are compiled with contraction off, so their result is a
// value of its own wherever they end up.  A formula that wants the fused form says fmaf.
#pragma once
#include "nr_common.h"

__device__ __forceinline__ float nr_rn_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float nr_rn_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float nr_rn_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
