// Local scaling and re-ranking of candidate lists: the search-time stage of CSLS / NICDM / LS on two-stage retrieval
// (DESIGN.md "Local scaling of two-stage retrieval").  The reference has no such path.
//
// The line, its present rule, its order and the wave layout are nr_cand_line.h's; the formulas are nr_localscale.h's.
//   query statistic   the line's top-ls_k list of the RAW scores, c <= ls_k entries:
//                     q_mean = fl(fl(sum of the c values, one by one in list order from the first) / fl(c)), q_kth = the c-th value;
//                     c = 0: both NaN (nr_localscale_stats on that list)
//   corrected score   nr_ls_score with (row, col) = (query, gallery item) where query_is_row, else swapped; means for csls and
//                     nicdm, k-th values for ls
//   output            the top k of the corrected scores over the present non-NaN slots; missing entries -1 / -inf
//
// Two placements against integer keys in LDS: the raw scores' (the slots of place < ls_k write their value to LDS at their place,
// every lane then adds the list up in order) and the corrected scores'.  A query's output depends on its own line only.
#include "nr_cand_line.h"
#include "nr_localscale.h"

__global__ __launch_bounds__(NR_CAND_WAVES * 64) void nr_cand_localscale_rerank_kernel(
    const float* __restrict__ fine, const int32_t* __restrict__ cand, int n, int C, int n_gallery,
    const float* __restrict__ g_stat, int mode, int ls_k, int query_is_row, int k, int32_t* __restrict__ out_idx,
    float* __restrict__ out_val, float* __restrict__ out_corr, float* __restrict__ out_qstat) {
    __shared__ __attribute__((aligned(16))) uint32_t keys1[NR_CAND_WAVES][NR_CAND_MAX_C];
    __shared__ __attribute__((aligned(16))) uint32_t keys2[NR_CAND_WAVES][NR_CAND_MAX_C];
    __shared__ __attribute__((aligned(16))) float vals[NR_CAND_WAVES][NR_CAND_MAX_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * NR_CAND_WAVES + wave;
    const bool live = q < n;                                   // the last workgroup may hold fewer than NR_CAND_WAVES queries
    const long long base = live ? q * C : 0;

    int c[2];
    float f[2];
    bool present[2];
    uint32_t key1[2];
    nr_cand_line_load(fine, cand, base, live, C, n_gallery, lane, c, f, present, key1);
#pragma unroll
    for (int s = 0; s < 2; ++s) keys1[wave][lane + 64 * s] = key1[s];
    __syncthreads();

    // the query's neighbourhood: the raw scores of place < ls_k, written at their place (ls_k <= C <= 128)
    int place[2];
    nr_cand_line_places(keys1[wave], C, lane, key1, place);
#pragma unroll
    for (int s = 0; s < 2; ++s)
        if (key1[s] != 0u && place[s] < ls_k) vals[wave][place[s]] = f[s];
    const int n_sel1 = nr_cand_line_selectable(key1);
    const int cnt = n_sel1 < ls_k ? n_sel1 : ls_k;
    __syncthreads();

    // every lane adds the list up in its order: the same sum in every lane (LDS broadcasts), no hand-off
    float q_mean = __builtin_nanf(""), q_kth = __builtin_nanf("");
    if (cnt > 0) {
        const f32x4_t* vw = reinterpret_cast<const f32x4_t*>(vals[wave]);
        float sum = 0.f;
        const int groups = (cnt + 3) >> 2;
        for (int g = 0; g < groups; ++g) {
            const f32x4_t v = vw[g];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * g + e;
                if (j < cnt) sum = j ? nr_rn_add(sum, v[e]) : v[e];        // the sum starts from the first value
            }
        }
        q_mean = __fdiv_rn(sum, (float)cnt);
        q_kth = vals[wave][cnt - 1];
    }
    const float q_op = nr_ls_operand(mode, mode == NR_LOCALSCALE_LS ? q_kth : q_mean);

    float corr[2];
    uint32_t key2[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        corr[s] = -INFINITY;
        if (present[s]) {
            const float g_op = nr_ls_operand(mode, g_stat[c[s]]);
            corr[s] = nr_ls_score(mode, f[s], query_is_row ? q_op : g_op, query_is_row ? g_op : q_op);
        }
        key2[s] = present[s] ? nr_order_key(corr[s]) : 0u;
        keys2[wave][lane + 64 * s] = key2[s];
    }
    if (live) {
        if (out_qstat && lane == 0) {
            out_qstat[2 * q] = q_mean;
            out_qstat[2 * q + 1] = q_kth;
        }
        nr_cand_line_write_corr(out_corr, base, C, lane, corr);
    }
    __syncthreads();
    if (!live) return;

    nr_cand_line_places(keys2[wave], C, lane, key2, place);
    nr_cand_line_emit(out_idx + q * k, out_val + q * k, k, lane, key2, place, c, corr);
}

extern "C" int nr_cand_localscale_rerank(const float* fine, const int32_t* cand, int n, int C, int n_gallery, const float* g_stat,
                                         int mode, int ls_k, int query_is_row, int k, int32_t* out_idx, float* out_val,
                                         float* out_corr, float* out_qstat, void* stream) {
    if (!fine || !cand || !g_stat || !out_idx || !out_val) return NR_EINVAL;
    if (!nr_cand_line_shape_ok(n, C, n_gallery, k)) return NR_EINVAL;
    if (ls_k < 1 || ls_k > C) return NR_EINVAL;
    if (mode != NR_LOCALSCALE_CSLS && mode != NR_LOCALSCALE_NICDM && mode != NR_LOCALSCALE_LS) return NR_EINVAL;
    if (query_is_row != 0 && query_is_row != 1) return NR_EINVAL;
    hipLaunchKernelGGL(nr_cand_localscale_rerank_kernel, dim3(nr_cand_line_blocks(n)), dim3(NR_CAND_WAVES * 64), 0,
                       (hipStream_t)stream, fine, cand, n, C, n_gallery, g_stat, mode, ls_k, query_is_row, k, out_idx, out_val,
                       out_corr, out_qstat);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
