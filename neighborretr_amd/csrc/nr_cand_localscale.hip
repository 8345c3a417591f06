// Local scaling and re-ranking of candidate lists: the search-time stage of CSLS / NICDM / LS on two-stage retrieval
// (DESIGN.md "Local scaling of two-stage retrieval").  The reference has no such path.
//
// One query's line: C <= 128 slots (cand[i,p], fine[i,p]) in ascending gallery index.  A slot is PRESENT iff
// 0 <= cand < n_gallery; an absent slot never forms an address into g_stat, its corrected score is -inf and it is never selected.
// Selectable = present and not NaN; the order everywhere is value descending, ties by lower position, -0.0 == +0.0 (nr_topk.hip).
//   query statistic   the line's top-ls_k list of the RAW scores, c <= ls_k entries:
//                     q_mean = fl(fl(sum of the c values, one by one in list order from the first) / fl(c)), q_kth = the c-th value;
//                     c = 0: both NaN (nr_localscale_stats on that list)
//   corrected score   the formulas of nr_localscale.hip with (row, col) = (query, gallery item) where query_is_row, else swapped:
//                       csls:  fl(fl(2 s - row) - col)                          (means)
//                       nicdm: -fl(d / fl(sqrt(fl(a b)))), d = max(fl(1 - s), 0), a = max(fl(1 - row), EPS), b likewise   (means)
//                       ls:    -fl(fl(d d) / fl(a b))                                                                     (k-th values)
//                     every operation rounded once, a NaN passes through every max
//   output            the top k of the corrected scores over the present non-NaN slots; missing entries -1 / -inf
//
// One wave per query, two slots per lane (p = lane, lane + 64), NR_CL_WAVES queries per workgroup, as nr_cand_norm.hip.  Two
// placements against integer keys in LDS: the raw scores' (the slots of place < ls_k write their value to LDS at their place, every
// lane then adds the list up in order) and the corrected scores'.  Integer comparisons order both, no atomics, no scratch, no
// hand-off between waves or workgroups: a query's output depends on its own line only.
#include "nr_common.h"
#include "../../include/nr_hip.h"

#define NR_CL_MAX_C 128
#define NR_CL_WAVES 4
#define NR_CL_EPS 9.5367431640625e-07f           // 2^-20, NR_LS_EPS of nr_localscale.hip

__device__ __forceinline__ uint32_t nr_cl_key(float x) {       // nr_topk_key: NaN -> 0, both zeros one key
    uint32_t u = __float_as_uint(x);
    if (x != x) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// max(x, lo) that keeps a NaN x (fmaxf would return lo)
__device__ __forceinline__ float nr_cl_floor(float x, float lo) { return x < lo ? lo : x; }

// One corrected score.  The pragma keeps every product apart from the sum that follows it (no fused multiply-add); the divide and
// the square root are the correctly rounded ones.
__device__ __forceinline__ float nr_cl_score(int mode, float s, float row, float col) {
#pragma clang fp contract(off)
    if (mode == NR_LOCALSCALE_CSLS) {
        const float t = 2.f * s;
        const float u = t - row;
        return u - col;
    }
    const float d = nr_cl_floor(1.f - s, 0.f);
    const float a = nr_cl_floor(1.f - row, NR_CL_EPS);
    const float b = nr_cl_floor(1.f - col, NR_CL_EPS);
    const float ab = a * b;
    if (mode == NR_LOCALSCALE_NICDM) return -__fdiv_rn(d, __fsqrt_rn(ab));
    const float dd = d * d;
    return -__fdiv_rn(dd, ab);
}

// place[s] = the number of slots of the wave's line that beat slot s (larger key; equal keys by lower position)
__device__ __forceinline__ void nr_cl_places(const uint32_t* line, int C, int lane, const uint32_t key[2], int place[2]) {
    place[0] = place[1] = 0;
    const u32x4_t* kw = reinterpret_cast<const u32x4_t*>(line);
    const int groups = (C + 3) >> 2;
    for (int g = 0; g < groups; ++g) {
        const u32x4_t kv = kw[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t kj = kv[e];
            const int pj = 4 * g + e;
#pragma unroll
            for (int s = 0; s < 2; ++s) place[s] += (kj > key[s]) || (kj == key[s] && pj < lane + 64 * s);
        }
    }
}

__global__ __launch_bounds__(NR_CL_WAVES * 64) void nr_cand_localscale_rerank_kernel(
    const float* __restrict__ fine, const int32_t* __restrict__ cand, int n, int C, int n_gallery,
    const float* __restrict__ g_stat, int mode, int ls_k, int query_is_row, int k, int32_t* __restrict__ out_idx,
    float* __restrict__ out_val, float* __restrict__ out_corr, float* __restrict__ out_qstat) {
    __shared__ __attribute__((aligned(16))) uint32_t keys1[NR_CL_WAVES][NR_CL_MAX_C];
    __shared__ __attribute__((aligned(16))) uint32_t keys2[NR_CL_WAVES][NR_CL_MAX_C];
    __shared__ __attribute__((aligned(16))) float vals[NR_CL_WAVES][NR_CL_MAX_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * NR_CL_WAVES + wave;
    const bool live = q < n;                                   // the last workgroup may hold fewer than NR_CL_WAVES queries
    const long long base = live ? q * C : 0;

    int c[2];
    float f[2];
    bool present[2];
    uint32_t key1[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int p = lane + 64 * s;
        const bool in = live && p < C;
        c[s] = in ? cand[base + p] : -1;
        f[s] = in ? fine[base + p] : -INFINITY;
        present[s] = c[s] >= 0 && c[s] < n_gallery;
        key1[s] = present[s] ? nr_cl_key(f[s]) : 0u;
        keys1[wave][p] = key1[s];                              // slots p >= C hold 0: they beat nothing
    }
    __syncthreads();

    // the query's neighbourhood: the raw scores of place < ls_k, written at their place (ls_k <= C <= 128)
    int place[2];
    nr_cl_places(keys1[wave], C, lane, key1, place);
#pragma unroll
    for (int s = 0; s < 2; ++s)
        if (key1[s] != 0u && place[s] < ls_k) vals[wave][place[s]] = f[s];
    const int n_sel1 = __popcll(__ballot(key1[0] != 0u)) + __popcll(__ballot(key1[1] != 0u));
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
                if (j < cnt) sum = j ? __fadd_rn(sum, v[e]) : v[e];        // the sum starts from the first value
            }
        }
        q_mean = __fdiv_rn(sum, (float)cnt);
        q_kth = vals[wave][cnt - 1];
    }
    const float q_stat = mode == NR_LOCALSCALE_LS ? q_kth : q_mean;

    float corr[2];
    uint32_t key2[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        corr[s] = -INFINITY;
        if (present[s]) {
            const float g = g_stat[c[s]];
            corr[s] = nr_cl_score(mode, f[s], query_is_row ? q_stat : g, query_is_row ? g : q_stat);
        }
        key2[s] = present[s] ? nr_cl_key(corr[s]) : 0u;
        keys2[wave][lane + 64 * s] = key2[s];
    }
    if (live) {
        if (out_qstat && lane == 0) {
            out_qstat[2 * q] = q_mean;
            out_qstat[2 * q + 1] = q_kth;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (out_corr && lane + 64 * s < C) out_corr[base + lane + 64 * s] = corr[s];
    }
    __syncthreads();
    if (!live) return;

    // a slot's place in the output = the number of selectable slots ahead of it (positions are distinct)
    nr_cl_places(keys2[wave], C, lane, key2, place);
    const int n_sel = __popcll(__ballot(key2[0] != 0u)) + __popcll(__ballot(key2[1] != 0u));
    int32_t* io = out_idx + q * k;
    float* vo = out_val + q * k;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (key2[s] != 0u && place[s] < k) {
            io[place[s]] = c[s];
            vo[place[s]] = corr[s];
        }
        const int t = lane + 64 * s;
        if (t >= n_sel && t < k) {
            io[t] = -1;
            vo[t] = -INFINITY;
        }
    }
}

extern "C" int nr_cand_localscale_rerank(const float* fine, const int32_t* cand, int n, int C, int n_gallery, const float* g_stat,
                                         int mode, int ls_k, int query_is_row, int k, int32_t* out_idx, float* out_val,
                                         float* out_corr, float* out_qstat, void* stream) {
    if (!fine || !cand || !g_stat || !out_idx || !out_val) return NR_EINVAL;
    if (n <= 0 || n_gallery <= 0 || k <= 0 || C < 1 || C > NR_CL_MAX_C || k > C) return NR_EINVAL;
    if (ls_k < 1 || ls_k > C) return NR_EINVAL;
    if (mode != NR_LOCALSCALE_CSLS && mode != NR_LOCALSCALE_NICDM && mode != NR_LOCALSCALE_LS) return NR_EINVAL;
    if (query_is_row != 0 && query_is_row != 1) return NR_EINVAL;
    const int blocks = (n + NR_CL_WAVES - 1) / NR_CL_WAVES;
    hipLaunchKernelGGL(nr_cand_localscale_rerank_kernel, dim3(blocks), dim3(NR_CL_WAVES * 64), 0, (hipStream_t)stream, fine, cand, n,
                       C, n_gallery, g_stat, mode, ls_k, query_is_row, k, out_idx, out_val, out_corr, out_qstat);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
