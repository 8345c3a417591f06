// Query-bank normalisation and re-ranking of candidate lists: the search-time stage of QB-Norm on two-stage retrieval
// (DESIGN.md "Query-bank normalisation of two-stage retrieval").  The reference has no such path.
//
// One query's line: C <= 128 slots (cand[i,p], fine[i,p]) in ascending gallery index.  A slot is PRESENT iff
// 0 <= cand < n_gallery; an absent slot never forms an address into norm / active, its corrected score is -inf and it is never
// selected.  Top-1 = the present slot with the largest non-NaN fine score, ties by lower position, -0.0 == +0.0 (the order of
// nr_topk.hip).  gate = 0 without norm; 1 with norm and without active; else 1 iff a top-1 exists and active[cand[top1]] != 0.
// corr = fl(fl(beta fine) - norm[cand]) where gate = 1 (two roundings, no fused multiply-add: the `is` expression of
// nr_hubnorm_apply), fine where gate = 0: a line is entirely raw or entirely normalised.  Output: the top k of corr over the
// present non-NaN slots, value descending, ties by lower position; missing entries -1 / -inf.
//
// One wave per query, two slots per lane (p = lane, lane + 64), NR_CN_WAVES queries per workgroup.  Scores become the
// order-preserving integer keys of nr_topk.hip (0 = not selectable); the top-1 is a wave reduction on (key, position); the final
// position of a slot is the number of slots that beat it, counted against the wave's keys in LDS.  Integer comparisons only, no
// atomics, no scratch, no hand-off between waves or workgroups: a query's output depends on its own line only.
#include "nr_common.h"
#include "../../include/nr_hip.h"

#define NR_CN_MAX_C 128
#define NR_CN_WAVES 4

__device__ __forceinline__ uint32_t nr_cn_key(float x) {       // nr_topk_key: NaN -> 0, both zeros one key
    uint32_t u = __float_as_uint(x);
    if (x != x) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// fl(fl(beta f) - c): two roundings.  The pragma keeps the compiler from contracting the pair into one fused multiply-add
// (__fmul_rn / __fsub_rn are plain operators to it), so NumPy float32 gives the same bits.
__device__ __forceinline__ float nr_cn_is(float beta, float f, float c) {
#pragma clang fp contract(off)
    const float b = beta * f;
    return b - c;
}

// (key, position) of the better of two slots: larger key, equal keys by lower position
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void nr_cn_best_step(uint32_t& key, int& pos) {
    const uint32_t ok = (uint32_t)nr_dpp<CTRL, ROW_MASK>((int)key, (int)key);
    const int op = nr_dpp<CTRL, ROW_MASK>(pos, pos);
    const bool take = ok > key || (ok == key && op < pos);
    key = take ? ok : key;
    pos = take ? op : pos;
}

__global__ __launch_bounds__(NR_CN_WAVES * 64) void nr_cand_norm_rerank_kernel(
    const float* __restrict__ fine, const int32_t* __restrict__ cand, int n, int C, int n_gallery,
    const float* __restrict__ norm, const int32_t* __restrict__ active, float beta, int k, int32_t* __restrict__ out_idx,
    float* __restrict__ out_val, float* __restrict__ out_corr, int32_t* __restrict__ out_gate) {
    __shared__ __attribute__((aligned(16))) uint32_t keys[NR_CN_WAVES][NR_CN_MAX_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * NR_CN_WAVES + wave;
    const bool live = q < n;                                   // the last workgroup may hold fewer than NR_CN_WAVES queries
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
        key1[s] = present[s] ? nr_cn_key(f[s]) : 0u;
    }

    // top-1 of the raw scores: the lane's better slot (slot 0 has the lower position), then the wave's
    uint32_t bkey = key1[1] > key1[0] ? key1[1] : key1[0];
    int bpos = key1[1] > key1[0] ? lane + 64 : lane;
    nr_cn_best_step<NR_DPP_XOR1, 0xF>(bkey, bpos);
    nr_cn_best_step<NR_DPP_XOR2, 0xF>(bkey, bpos);
    nr_cn_best_step<NR_DPP_HALF_MIRROR, 0xF>(bkey, bpos);
    nr_cn_best_step<NR_DPP_MIRROR, 0xF>(bkey, bpos);
    nr_cn_best_step<NR_DPP_BCAST15, 0xA>(bkey, bpos);
    nr_cn_best_step<NR_DPP_BCAST31, 0xC>(bkey, bpos);
    bkey = (uint32_t)__builtin_amdgcn_readlane((int)bkey, 63);
    bpos = __builtin_amdgcn_readlane(bpos, 63);

    int gate = 0;
    if (norm) {
        gate = 1;
        if (active) gate = (live && bkey != 0u) ? (active[cand[base + bpos]] != 0) : 0;     // bkey != 0: slot bpos is present
    }

    float corr[2];
    uint32_t key2[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        corr[s] = -INFINITY;
        if (present[s]) corr[s] = gate ? nr_cn_is(beta, f[s], norm[c[s]]) : f[s];
        key2[s] = present[s] ? nr_cn_key(corr[s]) : 0u;
        keys[wave][lane + 64 * s] = key2[s];                   // slots p >= C hold 0: they beat nothing
    }
    if (live) {
        if (out_gate && lane == 0) out_gate[q] = gate;
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (out_corr && lane + 64 * s < C) out_corr[base + lane + 64 * s] = corr[s];
    }
    __syncthreads();
    if (!live) return;

    // a slot's place in the list = the number of selectable slots ahead of it (positions are distinct)
    int rank[2] = {0, 0};
    const u32x4_t* kw = reinterpret_cast<const u32x4_t*>(keys[wave]);
    const int groups = (C + 3) >> 2;
    for (int g = 0; g < groups; ++g) {
        const u32x4_t kv = kw[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t kj = kv[e];
            const int pj = 4 * g + e;
#pragma unroll
            for (int s = 0; s < 2; ++s) rank[s] += (kj > key2[s]) || (kj == key2[s] && pj < lane + 64 * s);
        }
    }
    const int n_sel = __popcll(__ballot(key2[0] != 0u)) + __popcll(__ballot(key2[1] != 0u));
    int32_t* io = out_idx + q * k;
    float* vo = out_val + q * k;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (key2[s] != 0u && rank[s] < k) {
            io[rank[s]] = c[s];
            vo[rank[s]] = corr[s];
        }
        const int t = lane + 64 * s;
        if (t >= n_sel && t < k) {
            io[t] = -1;
            vo[t] = -INFINITY;
        }
    }
}

extern "C" int nr_cand_norm_rerank(const float* fine, const int32_t* cand, int n, int C, int n_gallery, const float* norm,
                                   const int32_t* active, float beta, int k, int32_t* out_idx, float* out_val, float* out_corr,
                                   int32_t* out_gate, void* stream) {
    if (!fine || !cand || !out_idx || !out_val) return NR_EINVAL;
    if (n <= 0 || n_gallery <= 0 || k <= 0 || C < 1 || C > NR_CN_MAX_C || k > C) return NR_EINVAL;
    if (active && !norm) return NR_EINVAL;
    if (norm && !(beta > 0.f && beta <= 3.402823466e+38f)) return NR_EINVAL;       // finite and > 0 (a NaN fails both)
    const int blocks = (n + NR_CN_WAVES - 1) / NR_CN_WAVES;
    hipLaunchKernelGGL(nr_cand_norm_rerank_kernel, dim3(blocks), dim3(NR_CN_WAVES * 64), 0, (hipStream_t)stream, fine, cand, n, C,
                       n_gallery, norm, active, beta, k, out_idx, out_val, out_corr, out_gate);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
