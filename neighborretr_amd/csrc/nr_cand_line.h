// What the candidate re-rank kernels (nr_cand_norm.hip, nr_cand_localscale.hip, nr_cand_mutualprox.hip) share: one query's line of
// candidates.
//
// A line: C <= NR_CAND_MAX_C slots (cand[i,p], fine[i,p]) in ascending gallery index.  A slot is PRESENT iff 0 <= cand < n_gallery;
// an absent slot never forms an address into a per-item array, its corrected score is -inf and it is never selected.  Selectable =
// present and not NaN; the order everywhere is value descending, ties by lower position, -0.0 == +0.0 (nr_order_key).
//
// One wave per query, two slots per lane (p = lane, lane + 64), NR_CAND_WAVES queries per workgroup.  Scores become order keys
// (0 = not selectable); a slot's place in a list is the number of slots that beat it, counted against the wave's keys in LDS.
// Integer comparisons only, no atomics, no scratch, no hand-off between waves or workgroups.  The helpers hold no barrier and no
// LDS of their own: the kernel owns both.
#pragma once
#include "nr_common.h"

#define NR_CAND_MAX_C 128
#define NR_CAND_WAVES 4

// host: the shape both entry points accept, and their grid
static inline bool nr_cand_line_shape_ok(int n, int C, int n_gallery, int k) {
    return n > 0 && n_gallery > 0 && k > 0 && C >= 1 && C <= NR_CAND_MAX_C && k <= C;
}
static inline int nr_cand_line_blocks(int n) { return (n + NR_CAND_WAVES - 1) / NR_CAND_WAVES; }

// The lane's two slots of line `base` (base = 0 and live = false for the waves past n of the last workgroup); slots p >= C are
// absent.  key = the raw scores' keys.
__device__ __forceinline__ void nr_cand_line_load(const float* __restrict__ fine, const int32_t* __restrict__ cand, long long base,
                                                  bool live, int C, int n_gallery, int lane, int c[2], float f[2], bool present[2],
                                                  uint32_t key[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int p = lane + 64 * s;
        const bool in = live && p < C;
        c[s] = in ? cand[base + p] : -1;
        f[s] = in ? fine[base + p] : -INFINITY;
        present[s] = c[s] >= 0 && c[s] < n_gallery;
        key[s] = present[s] ? nr_order_key(f[s]) : 0u;
    }
}

// place[s] = the number of slots of the wave's line in LDS (all 128 keys posted by the kernel; slots p >= C hold 0: they beat nothing)
// that beat slot s (larger key; equal keys by lower position).  Positions are distinct: the selectable slots' places are 0 .. n_sel - 1.
__device__ __forceinline__ void nr_cand_line_places(const uint32_t* line, int C, int lane, const uint32_t key[2], int place[2]) {
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

// the number of selectable slots of the wave's line
__device__ __forceinline__ int nr_cand_line_selectable(const uint32_t key[2]) {
    return __popcll(__ballot(key[0] != 0u)) + __popcll(__ballot(key[1] != 0u));
}

// the corrected scores of the whole line, absent slots -inf
__device__ __forceinline__ void nr_cand_line_write_corr(float* __restrict__ out_corr, long long base, int C, int lane,
                                                        const float corr[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
        if (out_corr && lane + 64 * s < C) out_corr[base + lane + 64 * s] = corr[s];
}

// The top k of the line: the selectable slots of place < k at their place, the entries past the last selectable slot -1 / -inf.
__device__ __forceinline__ void nr_cand_line_emit(int32_t* __restrict__ io, float* __restrict__ vo, int k, int lane,
                                                  const uint32_t key[2], const int place[2], const int c[2], const float corr[2]) {
    const int n_sel = nr_cand_line_selectable(key);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (key[s] != 0u && place[s] < k) {
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
