// Query-bank normalisation and re-ranking of candidate lists: the search-time stage of QB-Norm on two-stage retrieval
// (DESIGN.md "Query-bank normalisation of two-stage retrieval").  The reference has no such path.
//
// The line, its present rule, its order and the wave layout are nr_cand_line.h's.  Top-1 = the present slot with the largest
// non-NaN fine score, ties by lower position.  gate = 0 without norm; 1 with norm and without active; else 1 iff a top-1 exists and
// active[cand[top1]] != 0.  corr = fl(fl(beta fine) - norm[cand]) where gate = 1 (two roundings, no fused multiply-add: the `is`
// expression of nr_hubnorm_apply), fine where gate = 0: a line is entirely raw or entirely normalised.  Output: the top k of corr
// over the present non-NaN slots, value descending, ties by lower position; missing entries -1 / -inf.
//
// The top-1 is a wave reduction on (key, position); one placement against the corrected scores' keys in LDS gives the output.  A
// query's output depends on its own line only.
#include "nr_cand_line.h"
#include "nr_round.h"
#include "../../include/nr_hip.h"

// fl(fl(beta f) - c): two roundings (nr_round.h), so NumPy float32 gives the same bits.
__device__ __forceinline__ float nr_cn_is(float beta, float f, float c) { return nr_rn_sub(nr_rn_mul(beta, f), c); }

// (key, position) of the better of two slots: larger key, equal keys by lower position
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void nr_cn_best_step(uint32_t& key, int& pos) {
    const uint32_t ok = (uint32_t)nr_dpp<CTRL, ROW_MASK>((int)key, (int)key);
    const int op = nr_dpp<CTRL, ROW_MASK>(pos, pos);
    const bool take = ok > key || (ok == key && op < pos);
    key = take ? ok : key;
    pos = take ? op : pos;
}

__global__ __launch_bounds__(NR_CAND_WAVES * 64) void nr_cand_norm_rerank_kernel(
    const float* __restrict__ fine, const int32_t* __restrict__ cand, int n, int C, int n_gallery,
    const float* __restrict__ norm, const int32_t* __restrict__ active, float beta, int k, int32_t* __restrict__ out_idx,
    float* __restrict__ out_val, float* __restrict__ out_corr, int32_t* __restrict__ out_gate) {
    __shared__ __attribute__((aligned(16))) uint32_t keys[NR_CAND_WAVES][NR_CAND_MAX_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * NR_CAND_WAVES + wave;
    const bool live = q < n;                                   // the last workgroup may hold fewer than NR_CAND_WAVES queries
    const long long base = live ? q * C : 0;

    int c[2];
    float f[2];
    bool present[2];
    uint32_t key1[2];
    nr_cand_line_load(fine, cand, base, live, C, n_gallery, lane, c, f, present, key1);

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
        key2[s] = present[s] ? nr_order_key(corr[s]) : 0u;
        keys[wave][lane + 64 * s] = key2[s];
    }
    if (live) {
        if (out_gate && lane == 0) out_gate[q] = gate;
        nr_cand_line_write_corr(out_corr, base, C, lane, corr);
    }
    __syncthreads();
    if (!live) return;

    int place[2];
    nr_cand_line_places(keys[wave], C, lane, key2, place);
    nr_cand_line_emit(out_idx + q * k, out_val + q * k, k, lane, key2, place, c, corr);
}

extern "C" int nr_cand_norm_rerank(const float* fine, const int32_t* cand, int n, int C, int n_gallery, const float* norm,
                                   const int32_t* active, float beta, int k, int32_t* out_idx, float* out_val, float* out_corr,
                                   int32_t* out_gate, void* stream) {
    if (!fine || !cand || !out_idx || !out_val) return NR_EINVAL;
    if (!nr_cand_line_shape_ok(n, C, n_gallery, k)) return NR_EINVAL;
    if (active && !norm) return NR_EINVAL;
    if (norm && !(beta > 0.f && beta <= 3.402823466e+38f)) return NR_EINVAL;       // finite and > 0 (a NaN fails both)
    hipLaunchKernelGGL(nr_cand_norm_rerank_kernel, dim3(nr_cand_line_blocks(n)), dim3(NR_CAND_WAVES * 64), 0, (hipStream_t)stream,
                       fine, cand, n, C, n_gallery, norm, active, beta, k, out_idx, out_val, out_corr, out_gate);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
