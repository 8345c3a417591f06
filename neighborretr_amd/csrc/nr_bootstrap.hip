// Bootstrap of rank statistics (DESIGN.md "Bootstrap confidence intervals"): resample b draws U of the U units (queries, or videos in
// a multi-sentence set) with replacement and reports, over the multiset of rank entries of the drawn units, exact integers:
//   n, sum, the two middle order statistics, and hits[k] = #{r < cuts[k]}.
//
//   SM64(seed, c) = the (c + 1)-th output of SplitMix64 seeded with `seed`
//   u(b, t) = ((SM64(seed, (b << 32) | t) >> 32) * U) >> 32,   t in [0, U)
//
// The draws are counter-based: every pass recomputes them, nothing is stored per resample.  One workgroup per resample; a V = 2 call
// walks both rankings with the same draws.  This file holds the draw rule, the walk over a thread's drawn entries, the kernels' LDS
// and orchestration and the entry points; pass 0, the radix select of the order statistics and the sums of per-unit columns are the
// resampling engine's (nr_resample.h), shared with nr_permtest.hip.  No global atomics, no scratch; the result is a function of
// (seed, b, inputs) alone, the same for any grid and any split of the resamples over calls.
#include "nr_common.h"
#include "nr_resample.h"
#include "../../include/nr_hip.h"

// the unit that position t of the resample draws
__device__ __forceinline__ int nr_boot_draw(uint64_t base, int t, uint32_t U) {
    const uint64_t x = nr_boot_mix(base + (uint64_t)(uint32_t)t * NR_BOOT_GOLDEN);
    return (int)__umulhi((uint32_t)(x >> 32), U);
}

// f(r) for every entry r this thread owns: the entries of the units that positions t = tid, tid + 256, ... draw (a gather)
template <class F>
__device__ __forceinline__ void nr_boot_entries(const NrBootRanking& R, uint32_t U, uint64_t base, F f) {
    for (int t = threadIdx.x; t < (int)U; t += NR_BOOT_THREADS) {
        int lo, hi;
        nr_boot_unit(R, nr_boot_draw(base, t, U), lo, hi);
        for (int e = lo; e <= hi; ++e) f(R.ranks[e]);
    }
}

// the statistics of one ranking of the resample into out[4 + K]
__device__ __forceinline__ void nr_boot_ranking(const NrBootRanking R, uint32_t U, const NrBootCuts cuts, int K, uint64_t base,
                                                int64_t* __restrict__ out, uint32_t* hist, int64_t (*red)[NR_BOOT_STATS],
                                                uint32_t* wave_tot, int64_t* pick) {
    const auto entries = [&](auto f) { nr_boot_entries(R, U, base, f); };
    int64_t acc[NR_BOOT_STATS];
    int rmax;
    nr_resample_pass0(entries, cuts, acc, rmax);
    __syncthreads();                                  // the previous ranking's readers of red / wave_tot / pick are done
    nr_resample_pass0_store(acc, rmax, &red[0][0], NR_BOOT_STATS, wave_tot, 1);
    __syncthreads();
    nr_resample_pass0_total(acc, rmax, &red[0][0], NR_BOOT_STATS, wave_tot, 1, K, out);
    nr_resample_select(entries, acc[0], rmax, out, hist, wave_tot, pick);
}

__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_bootstrap_rank_stats_kernel(NrBootRanking A, NrBootRanking B, int V, uint32_t U,
                                                                                  NrBootCuts cuts, int K, uint64_t seed, uint32_t b0,
                                                                                  int64_t* __restrict__ out) {
    __shared__ uint32_t hist[NR_BOOT_BINS];
    __shared__ int64_t red[NR_BOOT_WAVES][NR_BOOT_STATS];
    __shared__ uint32_t wave_tot[NR_BOOT_WAVES];
    __shared__ int64_t pick[3];
    const uint64_t base = nr_resample_base(seed, b0);
    int64_t* o = out + (size_t)blockIdx.x * V * (4 + K);
    nr_boot_ranking(A, U, cuts, K, base, o, hist, red, wave_tot, pick);
    if (V == 2) nr_boot_ranking(B, U, cuts, K, base, o + (4 + K), hist, red, wave_tot, pick);      // the same draws
}

extern "C" int nr_bootstrap_rank_stats(const int32_t* ranks_a, const int32_t* unit_end_a, int E_a, const int32_t* ranks_b,
                                       const int32_t* unit_end_b, int E_b, int U, const int32_t* cuts, int K, uint64_t seed, int b0,
                                       int n_boot, int64_t* out, void* stream) {
    NrBootCuts c;
    if (!nr_resample_range_ok(U, b0, n_boot) || !nr_resample_cuts(cuts, K, c)) return NR_EINVAL;
    if (E_a < 0 || !ranks_a || !unit_end_a || !out) return NR_EINVAL;
    const int V = ranks_b ? 2 : 1;
    if (V == 2 && (E_b < 0 || !unit_end_b)) return NR_EINVAL;
    if (n_boot == 0) return NR_OK;
    const NrBootRanking A = {ranks_a, unit_end_a, E_a};
    const NrBootRanking B = {ranks_b, unit_end_b, V == 2 ? E_b : 0};
    hipLaunchKernelGGL(nr_bootstrap_rank_stats_kernel, dim3((unsigned)n_boot), dim3(NR_BOOT_THREADS), 0, (hipStream_t)stream, A, B, V,
                       (uint32_t)U, c, K, seed, (uint32_t)b0, out);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- bootstrap of per-unit sums (DESIGN.md "Rank-aware IR metrics") --------------------------------------------------------------
// out[b, q] = sum over t < U of values[u(b, t), q] with the draws u(b, t) of the kernel above (nr_boot_draw): resample b is the same
// multiset of units in both.  One workgroup per resample; the body is the engine's nr_resample_unit_sums over the drawn rows.
__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_bootstrap_unit_sums_kernel(const int64_t* __restrict__ values, uint32_t U, int Q,
                                                                                 uint64_t seed, uint32_t b0,
                                                                                 int64_t* __restrict__ out) {
    const uint64_t base = nr_resample_base(seed, b0);
    nr_resample_unit_sums([&](int t) { return values + (size_t)nr_boot_draw(base, t, U) * Q; }, U, Q, out + (size_t)blockIdx.x * Q);
}

extern "C" int nr_bootstrap_unit_sums(const int64_t* values, int U, int Q, uint64_t seed, int b0, int n_boot, int64_t* out,
                                      void* stream) {
    if (!nr_resample_range_ok(U, b0, n_boot) || Q < 1 || Q > NR_BOOT_MAX_COLS) return NR_EINVAL;
    if (!values || !out) return NR_EINVAL;
    if (n_boot == 0) return NR_OK;
    hipLaunchKernelGGL(nr_bootstrap_unit_sums_kernel, dim3((unsigned)n_boot), dim3(NR_BOOT_THREADS), 0, (hipStream_t)stream, values,
                       (uint32_t)U, Q, seed, (uint32_t)b0, out);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
