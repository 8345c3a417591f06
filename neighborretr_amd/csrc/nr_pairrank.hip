// Ranks of every relevant (sentence, video) pair from a ROW SLAB (DESIGN.md "Rank-aware IR metrics").
//
// Rows are sentences (n_total of them), columns videos (V); pair s is (row s, column g(s)), where video g owns the global rows
// [group_end[g-1], group_end[g]) -- the convention of nr_group_slab_ranks -- and own[s] = M[s, g(s)] (gathered by the caller).
// Entry x at index i of a line is AHEAD of pair s when x > own[s], or x == own[s] and i lies below the pair's own index on that
// line (plain IEEE compares: both zeros are equal, a NaN entry is never ahead).  A pair whose own score is NaN or infinite is
// unranked.
//   row_rank[i]  = #{j : M[row0 + i, j] ahead of pair row0 + i}, index j, own index g(s)       (complete; -1 when unranked)
//   col_ahead[s] = #{i < n_rows : M[row0 + i, g(s)] ahead of pair s}, index row0 + i, own index s   (this slab's PART; 0 when unranked)
//
// Row side: one wave per slab row, one pass over the row.  Column side: a workgroup owns 64 consecutive pairs; lane l of each of
// its four waves keeps the threshold own[s] and the index s of pair l in registers, wave q streams the slab's rows q, q + 4, ...
// of column g(s) past them, and the four counts meet in LDS.  Adjacent pairs read adjacent columns (single-sentence sets:
// coalesced) or the same column (the sentences of one video: one address per wave, broadcast), element stride V from row to row,
// as the column top-k kernel reads.  Every output has exactly one writer: integers only, no atomics, no hand-off between
// workgroups; the result depends on the inputs alone.
#include "nr_common.h"
#include "../../include/nr_hip.h"

#define NR_PAIR_THREADS 256
#define NR_PAIR_UNROLL 8
#define NR_PAIR_PARTS (NR_PAIR_THREADS / NR_WAVE)          // waves of a column workgroup: each walks a quarter of the slab's rows

// the group of global row s: the first g with group_end[g] > s (V - 1 if there is none: always a valid column)
__device__ __forceinline__ int nr_pair_group(const int32_t* __restrict__ group_end, int V, int s) {
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (group_end[mid] > s) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ bool nr_pair_unranked(float own) { return own != own || fabsf(own) == INFINITY; }

__global__ __launch_bounds__(NR_PAIR_THREADS) void nr_pair_row_ranks_kernel(const float* __restrict__ M, int n, int V, int row0,
                                                                            const int32_t* __restrict__ group_end,
                                                                            const float* __restrict__ own,
                                                                            int32_t* __restrict__ row_rank) {
    const int lane = threadIdx.x & (NR_WAVE - 1);
    const int i = blockIdx.x * (NR_PAIR_THREADS / NR_WAVE) + (threadIdx.x / NR_WAVE);
    if (i >= n) return;
    const int s = row0 + i;
    const int g = nr_pair_group(group_end, V, s);
    const float* row = M + (size_t)i * V;
    const float o = own[s];
    int ahead = 0;
    for (int j = lane; j < V; j += NR_WAVE) {
        const float x = row[j];
        ahead += (x > o) || (x == o && j < g);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ahead += __shfl_xor(ahead, off, NR_WAVE);
    if (lane == 0) row_rank[i] = nr_pair_unranked(o) ? -1 : ahead;
}

__global__ __launch_bounds__(NR_PAIR_THREADS) void nr_pair_col_ahead_kernel(const float* __restrict__ M, int n, int V, int row0,
                                                                            int n_total, const int32_t* __restrict__ group_end,
                                                                            const float* __restrict__ own,
                                                                            int32_t* __restrict__ col_ahead) {
    __shared__ int32_t part[NR_PAIR_PARTS][NR_WAVE];
    const int lane = threadIdx.x & (NR_WAVE - 1), q = threadIdx.x / NR_WAVE;
    const int s = blockIdx.x * NR_WAVE + lane;
    const bool live = s < n_total;
    const float o = live ? own[s] : INFINITY;
    int ahead = 0;
    if (!nr_pair_unranked(o)) {
        const float* col = M + nr_pair_group(group_end, V, s);
        const int before = min(max(s - row0, 0), n);      // slab rows whose global index lies below s: they win exact ties
        int i = q;                                        // wave q walks the slab rows q, q + 4, ...
        for (; i + NR_PAIR_PARTS * (NR_PAIR_UNROLL - 1) < n; i += NR_PAIR_PARTS * NR_PAIR_UNROLL) {
            float x[NR_PAIR_UNROLL];
#pragma unroll
            for (int k = 0; k < NR_PAIR_UNROLL; ++k) x[k] = col[(size_t)(i + NR_PAIR_PARTS * k) * V];
#pragma unroll
            for (int k = 0; k < NR_PAIR_UNROLL; ++k) ahead += (x[k] > o) || (x[k] == o && i + NR_PAIR_PARTS * k < before);
        }
        for (; i < n; i += NR_PAIR_PARTS) {
            const float x = col[(size_t)i * V];
            ahead += (x > o) || (x == o && i < before);
        }
    }
    part[q][lane] = ahead;
    __syncthreads();
    if (q == 0 && live) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < NR_PAIR_PARTS; ++w) total += part[w][lane];
        col_ahead[s] = total;
    }
}

extern "C" int nr_pair_ranks(const float* M_slab, int n_rows, int V, int row0, int n_total, const int32_t* group_end,
                             const float* own, int32_t* row_rank, int32_t* col_ahead, void* stream) {
    if (n_rows < 0 || V < 1 || row0 < 0 || n_total < 0 || (int64_t)row0 + n_rows > n_total) return NR_EINVAL;
    if (!group_end || !own || (n_rows > 0 && !M_slab)) return NR_EINVAL;
    if (n_rows == 0) {                                    // an empty slab is ahead of nothing
        if (col_ahead && n_total) {
            const hipError_t e = hipMemsetAsync(col_ahead, 0, sizeof(int32_t) * (size_t)n_total, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
        }
        return NR_OK;
    }
    if (row_rank) {
        const int per = NR_PAIR_THREADS / NR_WAVE;
        hipLaunchKernelGGL(nr_pair_row_ranks_kernel, dim3((unsigned)((n_rows + per - 1) / per)), dim3(NR_PAIR_THREADS), 0,
                           (hipStream_t)stream, M_slab, n_rows, V, row0, group_end, own, row_rank);
        NR_LAUNCH_CHECK();
    }
    if (col_ahead) {
        hipLaunchKernelGGL(nr_pair_col_ahead_kernel, dim3((unsigned)((n_total + NR_WAVE - 1) / NR_WAVE)),
                           dim3(NR_PAIR_THREADS), 0, (hipStream_t)stream, M_slab, n_rows, V, row0, n_total, group_end, own,
                           col_ahead);
        NR_LAUNCH_CHECK();
    }
    return NR_OK;
}
