// Mutual proximity and re-ranking of candidate lists: the search-time stage of emp / gauss on two-stage retrieval
// (DESIGN.md "Mutual proximity of two-stage retrieval").  The reference has no such path.
//
// The line, its present rule, its order and the wave layout are nr_cand_line.h's; the formulas are nr_mutualprox.h's.
//   query line        the selectable slots of the query's own line, c_q of them:
//                     q_mean, q_sd = the mean and the population sd of their RAW scores, accumulated in fp64 in position order (first
//                     the sum, then the squared distances from the fp64 mean), delivered as fp32; c_q = 0: both NaN
//   item line         g_line [n_gallery, M]: item g's M scores against a query bank, g_cnt [n_gallery] its non-NaN count, g_mean /
//                     g_sd [n_gallery] its moments, all computed once per gallery
//   emp               r2_q = 2 #{x in the query's line : x < s} + #{x == s} on the integer keys in LDS (key 0 counts nothing),
//                     r2_g = sum of nr_mp_pair(x, s) over g_line[g, :M];  T = nr_mp_emp_score(s, r2_q, fl(2 c_q), r2_g, g_cnt[g])
//   gauss             T = nr_mp_gauss_score(s, q_mean, q_sd, g_mean[g], g_sd[g])
//   output            the top k of T over the present slots whose T is not NaN; missing entries -1 / -inf
//
// The item side of emp is the hot loop: for every present slot whose score is not NaN the wave takes the slot's item and score
// from the owning lane (v_readlane: both are wave-uniform from there on), its 64 lanes read the item's line 64 floats at a time,
// eight loads in flight, and add up nr_mp_pair; one integer wave sum on DPP follows and the owning lane keeps it.  The first
// round of the next slot's line is loaded before the current slot's compares (measured: 78 us against 84.5 us without, 4917 x 64
// slots, M = 512).  Integers: no order of summation.
// No atomics, no scratch, no hand-off between waves or workgroups: a query's output depends on its own line only.
#include "nr_cand_line.h"
#include "nr_mutualprox.h"
#include "../../include/nr_hip.h"

#define NR_CAND_MP_FLIGHT 8                      // loads of an item's line a lane has in flight: 8 x 64 floats = one line of M = 512

// wave-wide integer sum in all lanes: nr_wave_sum's steps on integers
__device__ __forceinline__ int nr_cand_mp_wave_sum(int v) {
    v += nr_dpp<NR_DPP_XOR1>(v, v);
    v += nr_dpp<NR_DPP_XOR2>(v, v);
    v += nr_dpp<NR_DPP_HALF_MIRROR>(v, v);
    v += nr_dpp<NR_DPP_MIRROR>(v, v);
    v += nr_dpp<NR_DPP_BCAST15, 0xA>(0, v);
    v += nr_dpp<NR_DPP_BCAST31, 0xC>(0, v);
    return __builtin_amdgcn_readlane(v, 63);
}

// r2[s] = 2 #{keys of the wave's line in LDS below key[s]} + #{equal to it}; key 0 (not selectable) counts nothing and is counted
// against nothing.  k - 1 wraps key 0 to the largest word: one unsigned compare drops it.
__device__ __forceinline__ void nr_cand_mp_line_counts(const uint32_t* line, int C, const uint32_t key[2], int r2[2]) {
    r2[0] = r2[1] = 0;
    const uint32_t ks[2] = {key[0] - 1u, key[1] - 1u};
    const u32x4_t* kw = reinterpret_cast<const u32x4_t*>(line);
    const int groups = (C + 3) >> 2;
    for (int g = 0; g < groups; ++g) {
        const u32x4_t kv = kw[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t kj = kv[e] - 1u;
#pragma unroll
            for (int s = 0; s < 2; ++s) r2[s] += (int)(kj < ks[s]) + (int)(kj <= ks[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) r2[s] = key[s] != 0u ? r2[s] : 0;
}

// The moments of the wave's line in LDS (vals: the raw scores, NaN where the slot is not selectable; slots p >= C hold NaN) over
// its c entries: every lane walks the line in position order, the same fp64 sums in every lane (LDS broadcasts).
__device__ __forceinline__ void nr_cand_mp_moments(const float* vals, int C, int c, float& mean, float& sd) {
#pragma clang fp contract(off)
    const f32x4_t* vw = reinterpret_cast<const f32x4_t*>(vals);
    const int groups = (C + 3) >> 2;
    double sum = 0.0;
    for (int g = 0; g < groups; ++g) {
        const f32x4_t v = vw[g];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] == v[e]) sum += (double)v[e];
    }
    const double mu = sum / (double)c;                         // c = 0: 0 / 0 = NaN
    double m2 = 0.0;
    for (int g = 0; g < groups; ++g) {
        const f32x4_t v = vw[g];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] == v[e]) {
                const double d = (double)v[e] - mu;
                m2 += d * d;
            }
    }
    mean = (float)mu;
    sd = (float)sqrt(m2 / (double)c);
}

// The lowest slot left, taken off its mask; -1: none.  todo: the wave-uniform mask of the slots base .. base + 63 in hand, rest:
// that of the slots 64 .. 127 while base is 0.
__device__ __forceinline__ int nr_cand_mp_next(unsigned long long& todo, unsigned long long& rest, int& base) {
    if (!todo) {
        todo = rest;
        rest = 0;
        base = 64;
    }
    if (!todo) return -1;
    const int p = base + __ffsll(todo) - 1;
    todo &= todo - 1;
    return p;
}

// slot p's word of the wave's line, wave-uniform: lane p of v0 (p < 64) or lane p - 64 of v1
__device__ __forceinline__ int nr_cand_mp_lane_int(int v0, int v1, int p) {
    return p < 64 ? __builtin_amdgcn_readlane(v0, p) : __builtin_amdgcn_readlane(v1, p - 64);
}

// one round of item g's line (0 <= g < n_gallery): the entries e0 + lane, e0 + lane + 64, ...; the ragged tail past M is not read
// and holds NaN, which counts nothing
__device__ __forceinline__ void nr_cand_mp_fetch(const float* __restrict__ g_line, int g, int M, int e0, int lane,
                                                 float (&x)[NR_CAND_MP_FLIGHT]) {
    const float* __restrict__ line = g_line + (size_t)g * M;
#pragma unroll
    for (int u = 0; u < NR_CAND_MP_FLIGHT; ++u) {
        const int e = e0 + 64 * u + lane;
        x[u] = e < M ? line[e] : __builtin_nanf("");
    }
}

template <int MODE>
__global__ __launch_bounds__(NR_CAND_WAVES * 64) void nr_cand_mutualprox_rerank_kernel(
    const float* __restrict__ fine, const int32_t* __restrict__ cand, int n, int C, int n_gallery,
    const float* __restrict__ g_line, const int32_t* __restrict__ g_cnt, int M, const float* __restrict__ g_mean,
    const float* __restrict__ g_sd, int k, int32_t* __restrict__ out_idx, float* __restrict__ out_val,
    float* __restrict__ out_corr, float* __restrict__ out_qstat) {
    __shared__ __attribute__((aligned(16))) uint32_t keys1[NR_CAND_WAVES][NR_CAND_MAX_C];
    __shared__ __attribute__((aligned(16))) uint32_t keys2[NR_CAND_WAVES][NR_CAND_MAX_C];
    __shared__ __attribute__((aligned(16))) float vals[NR_CAND_WAVES][NR_CAND_MAX_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * NR_CAND_WAVES + wave;
    const bool live = q < n;                                   // the last workgroup may hold fewer than NR_CAND_WAVES queries
    const long long base = live ? q * C : 0;
    const float none = __builtin_nanf("");

    int c[2];
    float f[2];
    bool present[2];
    uint32_t key1[2];
    nr_cand_line_load(fine, cand, base, live, C, n_gallery, lane, c, f, present, key1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        keys1[wave][lane + 64 * s] = key1[s];
        vals[wave][lane + 64 * s] = key1[s] != 0u ? f[s] : none;
    }
    __syncthreads();

    // the query's line: its count and its ordered moments (both modes report them), its counts for emp
    const int c_q = nr_cand_line_selectable(key1);
    float q_mean, q_sd;
    nr_cand_mp_moments(vals[wave], C, c_q, q_mean, q_sd);

    float corr[2] = {-INFINITY, -INFINITY};
    if (MODE == NR_MUTUALPROX_EMP) {
        int r2q[2], r2g[2] = {0, 0};
        nr_cand_mp_line_counts(keys1[wave], C, key1, r2q);
        // The item side.  The slots that count -- present, score not NaN (a NaN counts nothing and its T is NaN: its line is not
        // read) -- are two wave-uniform masks; a slot's item and score become wave-uniform (v_readlane), the lanes share the
        // item's line.  The first loads of the next slot's line are issued before the current slot's compares.
        unsigned long long todo = __ballot(present[0] && f[0] == f[0]), rest = __ballot(present[1] && f[1] == f[1]);
        int slot_base = 0;
        float ahead[NR_CAND_MP_FLIGHT];
        int p = nr_cand_mp_next(todo, rest, slot_base);
        if (p >= 0) nr_cand_mp_fetch(g_line, nr_cand_mp_lane_int(c[0], c[1], p), M, 0, lane, ahead);
        while (p >= 0) {
            const int g = nr_cand_mp_lane_int(c[0], c[1], p);
            const float sc = __builtin_bit_cast(float, nr_cand_mp_lane_int(__builtin_bit_cast(int, f[0]), __builtin_bit_cast(int, f[1]), p));
            float x[NR_CAND_MP_FLIGHT];
#pragma unroll
            for (int u = 0; u < NR_CAND_MP_FLIGHT; ++u) x[u] = ahead[u];
            const int pn = nr_cand_mp_next(todo, rest, slot_base);
            if (pn >= 0) nr_cand_mp_fetch(g_line, nr_cand_mp_lane_int(c[0], c[1], pn), M, 0, lane, ahead);
            int acc = 0;
#pragma unroll
            for (int u = 0; u < NR_CAND_MP_FLIGHT; ++u) acc += nr_mp_pair(x[u], sc);
            for (int e0 = 64 * NR_CAND_MP_FLIGHT; e0 < M; e0 += 64 * NR_CAND_MP_FLIGHT) {       // lines longer than one round
                nr_cand_mp_fetch(g_line, g, M, e0, lane, x);
#pragma unroll
                for (int u = 0; u < NR_CAND_MP_FLIGHT; ++u) acc += nr_mp_pair(x[u], sc);
            }
            acc = nr_cand_mp_wave_sum(acc);
            if (lane == (p & 63)) {
                if (p < 64) r2g[0] = acc; else r2g[1] = acc;
            }
            p = pn;
        }
        const float q_den = (float)(2 * c_q);
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (present[s]) corr[s] = nr_mp_emp_score(f[s], r2q[s], q_den, r2g[s], g_cnt[c[s]]);
    } else {
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (present[s]) corr[s] = nr_mp_gauss_score(f[s], q_mean, q_sd, g_mean[c[s]], g_sd[c[s]]);
    }

    uint32_t key2[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        key2[s] = present[s] ? nr_order_key(corr[s]) : 0u;
        keys2[wave][lane + 64 * s] = key2[s];
    }
    if (live) {
        if (out_qstat && lane == 0) {
            out_qstat[3 * q] = (float)c_q;
            out_qstat[3 * q + 1] = q_mean;
            out_qstat[3 * q + 2] = q_sd;
        }
        nr_cand_line_write_corr(out_corr, base, C, lane, corr);
    }
    __syncthreads();
    if (!live) return;

    int place[2];
    nr_cand_line_places(keys2[wave], C, lane, key2, place);
    nr_cand_line_emit(out_idx + q * k, out_val + q * k, k, lane, key2, place, c, corr);
}

extern "C" int nr_cand_mutualprox_rerank(const float* fine, const int32_t* cand, int n, int C, int n_gallery, int mode,
                                         const float* g_line, const int32_t* g_cnt, int M, const float* g_mean, const float* g_sd,
                                         int k, int32_t* out_idx, float* out_val, float* out_corr, float* out_qstat, void* stream) {
    if (!fine || !cand || !out_idx || !out_val) return NR_EINVAL;
    if (!nr_cand_line_shape_ok(n, C, n_gallery, k)) return NR_EINVAL;
    if (mode != NR_MUTUALPROX_EMP && mode != NR_MUTUALPROX_GAUSS) return NR_EINVAL;
    if (mode == NR_MUTUALPROX_EMP && (!g_line || !g_cnt || M < 1 || M >= NR_MP_LINE_MAX)) return NR_EINVAL;
    if (mode == NR_MUTUALPROX_GAUSS && (!g_mean || !g_sd)) return NR_EINVAL;
    const dim3 grid(nr_cand_line_blocks(n)), block(NR_CAND_WAVES * 64);
    if (mode == NR_MUTUALPROX_EMP) {
        hipLaunchKernelGGL(nr_cand_mutualprox_rerank_kernel<NR_MUTUALPROX_EMP>, grid, block, 0, (hipStream_t)stream, fine, cand, n, C,
                           n_gallery, g_line, g_cnt, M, g_mean, g_sd, k, out_idx, out_val, out_corr, out_qstat);
    } else {
        hipLaunchKernelGGL(nr_cand_mutualprox_rerank_kernel<NR_MUTUALPROX_GAUSS>, grid, block, 0, (hipStream_t)stream, fine, cand, n, C,
                           n_gallery, g_line, g_cnt, M, g_mean, g_sd, k, out_idx, out_val, out_corr, out_qstat);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}
