// Local scaling of a similarity slab (DESIGN.md "Local scaling"): CSLS, NICDM and LS rescale every score by statistics of the
// two items' k-nearest neighbourhoods, taken from the top-k lists of nr_topk.hip.
//
//   mean = fl(fl(sum of the present values of a list, one by one in list order) / fl(count));   kth = the last present value
//   csls:  T[i,j] = fl(fl(2 s - mean_row[i]) - mean_col[j])
//   nicdm: T[i,j] = -fl(d / fl(sqrt(fl(a[i] b[j])))),  d = max(fl(1 - s), 0),  a = max(fl(1 - mean), EPS)
//   ls:    T[i,j] = -fl(fl(d d) / fl(a[i] b[j])),                              a = max(fl(1 - kth), EPS)
//
// Every operation is rounded once (no fused multiply-add), NaN passes through every max, the sum of a list has a fixed order:
// the same inputs give the same bits, whatever the slab split.  No scratch, no float atomics, no hand-off between workgroups.
#include "nr_localscale.h"
#include "nr_slab.h"

#define NR_LS_K_MAX 128                          // the longest list nr_topk.hip writes

// ---- statistics of the lists: one thread per line -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nr_localscale_stats_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                                 int n, int k, float* __restrict__ mean, float* __restrict__ kth) {
    const int line = blockIdx.x * 256 + threadIdx.x;
    if (line >= n) return;
    const int32_t* li = idx + (long long)line * k;
    const float* lv = val + (long long)line * k;
    float sum = 0.f, last = 0.f;
    int c = 0;
    for (int e = 0; e < k; ++e) {
        if (li[e] < 0) continue;                 // an absent slot
        const float x = lv[e];
        sum = c ? nr_rn_add(sum, x) : x;           // the sum starts from the first present value
        last = x;
        ++c;
    }
    const float none = __builtin_nanf("");
    mean[line] = c ? __fdiv_rn(sum, (float)c) : none;
    kth[line] = c ? last : none;
}

extern "C" int nr_localscale_stats(const int32_t* idx, const float* val, int n, int k, float* mean, float* kth, void* stream) {
    if (!idx || !val || !mean || !kth) return NR_EINVAL;
    if (n < 0 || k < 1 || k > NR_LS_K_MAX) return NR_EINVAL;
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(nr_localscale_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, val,
                       n, k, mean, kth);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- apply: one read of S, one write of T (the loop is nr_slab.h's) -----------------------------------------------------------------
// The formulas are nr_localscale.h's with the mode a compile-time constant; the row's operand (a[i] for nicdm / ls) is taken once
// per group.
template <int MODE>
struct nr_ls_apply {
    static constexpr int OUTS = 1;
    const float* row_stat;
    const float* col_stat;
    __device__ float row(int i) const { return nr_ls_operand(MODE, row_stat[i]); }
    template <int VEC>
    __device__ void values(int, const float (&s)[VEC], float r, int j0, long long, float (&t)[VEC]) const {
        float c[VEC];
        nr_slab_load<VEC>(col_stat + j0, c);
#pragma unroll
        for (int q = 0; q < VEC; ++q) t[q] = nr_ls_score(MODE, s[q], r, nr_ls_operand(MODE, c[q]));
    }
};

template <int MODE>
static int nr_localscale_apply_launch(const float* S, int n, int L, const float* row_stat, const float* col_stat, float* T,
                                      void* stream) {
    return nr_slab_apply<nr_ls_apply<MODE>>(S, n, L, T, nullptr, {col_stat}, stream, row_stat, col_stat);
}
extern "C" int nr_localscale_apply(const float* S, int n, int L, int mode, const float* row_stat, const float* col_stat, float* T,
                                   void* stream) {
    if (!S || !row_stat || !col_stat || !T) return NR_EINVAL;
    if (n < 0 || L < 0) return NR_EINVAL;
    if (mode != NR_LOCALSCALE_CSLS && mode != NR_LOCALSCALE_NICDM && mode != NR_LOCALSCALE_LS) return NR_EINVAL;
    if (n == 0 || L == 0) return NR_OK;
    if (mode == NR_LOCALSCALE_CSLS) return nr_localscale_apply_launch<NR_LOCALSCALE_CSLS>(S, n, L, row_stat, col_stat, T, stream);
    if (mode == NR_LOCALSCALE_NICDM) return nr_localscale_apply_launch<NR_LOCALSCALE_NICDM>(S, n, L, row_stat, col_stat, T, stream);
    return nr_localscale_apply_launch<NR_LOCALSCALE_LS>(S, n, L, row_stat, col_stat, T, stream);
}
