// Paired permutation (randomisation) test of two rankings over the same U units (DESIGN.md "Paired permutation tests"): permutation p
// swaps the two rankings' entries unit by unit and reports, for both sides of the relabelling, the exact integers of the bootstrap:
//   n, sum, the two middle order statistics, and hits[k] = #{r < cuts[k]}.
//
//   SM64(seed, c) = the (c + 1)-th output of SplitMix64 seeded with `seed`
//   s(p, u) = SM64(seed ^ 0x7065726D74657374, (p << 32) | u) >> 63,   u in [0, U)
//
// Side X takes unit u's entries from A when s = 0 and from B when s = 1; side Y takes the other ranking's entries of that unit.  The
// swap bits are counter-based: every pass recomputes them, nothing is stored per permutation.  One workgroup per permutation.  Where
// the bootstrap gathers (position t reads a DRAWN unit), here position u reads unit u of one of the two rankings: the threads stride
// over u, so `unit_end` and the entries are read coalesced -- the one structural gain over nr_bootstrap.hip, and why the two entry
// walks stay apart.  This file holds the walk over a thread's entries of one side, the kernels' LDS and orchestration (pass 0 serves
// both sides behind one barrier, then one select per side) and the entry points; the swap rule with its salt (shared with
// nr_hubperm.hip), pass 0, the radix select of the order statistics and the sums of per-unit columns are the resampling engine's
// (nr_resample.h), shared with nr_bootstrap.hip.  No global atomics, no scratch, no hand-off between workgroups: the result is a function of (seed, p, inputs)
// alone, the same for any grid and any split of the permutations over calls.
#include "nr_common.h"
#include "nr_resample.h"
#include "../../include/nr_hip.h"

// f(r) for every entry r of `side` (0: X, 1: Y) that this thread owns: the entries of unit u = tid, tid + 256, ... of the ranking
// the swap bit gives that side
template <class F>
__device__ __forceinline__ void nr_perm_entries(const NrBootRanking& A, const NrBootRanking& B, uint32_t U, uint64_t base, int side,
                                                F f) {
    for (int u = threadIdx.x; u < (int)U; u += NR_BOOT_THREADS) {
        const bool from_b = (nr_perm_swap(base, u) ^ side) != 0;
        NrBootRanking R;
        R.ranks = from_b ? B.ranks : A.ranks;
        R.unit_end = from_b ? B.unit_end : A.unit_end;
        R.E = from_b ? B.E : A.E;
        int lo, hi;
        nr_boot_unit(R, u, lo, hi);
        for (int e = lo; e <= hi; ++e) f(R.ranks[e]);
    }
}

__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_permtest_rank_stats_kernel(NrBootRanking A, NrBootRanking B, uint32_t U,
                                                                                 NrBootCuts cuts, int K, uint64_t seed, uint32_t p0,
                                                                                 int64_t* __restrict__ out) {
    __shared__ uint32_t hist[NR_BOOT_BINS];
    __shared__ int64_t red[NR_BOOT_WAVES][2][NR_BOOT_STATS];
    __shared__ uint32_t wave_max[NR_BOOT_WAVES][2];
    __shared__ uint32_t wave_tot[NR_BOOT_WAVES];
    __shared__ int64_t pick[3];
    const uint64_t base = nr_resample_base(seed ^ NR_PERM_SALT, p0);
    int64_t* o = out + (size_t)blockIdx.x * 2 * (4 + K);

    // ---- pass 0 serves both sides at once: one barrier ----
    int64_t acc[2][NR_BOOT_STATS];
    int rmax[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        nr_resample_pass0([&](auto f) { nr_perm_entries(A, B, U, base, side, f); }, cuts, acc[side], rmax[side]);
        nr_resample_pass0_store(acc[side], rmax[side], &red[0][side][0], 2 * NR_BOOT_STATS, &wave_max[0][side], 2);
    }
    __syncthreads();
#pragma unroll
    for (int side = 0; side < 2; ++side)
        nr_resample_pass0_total(acc[side], rmax[side], &red[0][side][0], 2 * NR_BOOT_STATS, &wave_max[0][side], 2, K,
                                o + side * (4 + K));

    // ---- the order statistics, one side after the other ----
#pragma unroll
    for (int side = 0; side < 2; ++side)
        nr_resample_select([&](auto f) { nr_perm_entries(A, B, U, base, side, f); }, acc[side][0], rmax[side], o + side * (4 + K), hist,
                           wave_tot, pick);
}

extern "C" int nr_permtest_rank_stats(const int32_t* ranks_a, const int32_t* unit_end_a, int E_a, const int32_t* ranks_b,
                                      const int32_t* unit_end_b, int E_b, int U, const int32_t* cuts, int K, uint64_t seed, int p0,
                                      int n_perm, int64_t* out, void* stream) {
    NrBootCuts c;
    if (!nr_resample_range_ok(U, p0, n_perm) || !nr_resample_cuts(cuts, K, c)) return NR_EINVAL;
    if (E_a < 0 || E_b < 0 || !ranks_a || !unit_end_a || !ranks_b || !unit_end_b || !out) return NR_EINVAL;
    if (n_perm == 0) return NR_OK;
    const NrBootRanking A = {ranks_a, unit_end_a, E_a};
    const NrBootRanking B = {ranks_b, unit_end_b, E_b};
    hipLaunchKernelGGL(nr_permtest_rank_stats_kernel, dim3((unsigned)n_perm), dim3(NR_BOOT_THREADS), 0, (hipStream_t)stream, A, B,
                       (uint32_t)U, c, K, seed, (uint32_t)p0, out);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- permutation of per-unit sums (the IR metrics' columns) ----------------------------------------------------------------------
// out[p, q] = sum over u < U of (s(p, u) ? values_b : values_a)[u, q]: side X with the swap bits of the kernel above; side Y is the
// two inputs' totals minus X, which the host takes.  One workgroup per permutation; the body is the engine's nr_resample_unit_sums
// over rows read in order (coalesced).
__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_permtest_unit_sums_kernel(const int64_t* __restrict__ values_a,
                                                                                const int64_t* __restrict__ values_b, uint32_t U, int Q,
                                                                                uint64_t seed, uint32_t p0, int64_t* __restrict__ out) {
    const uint64_t base = nr_resample_base(seed ^ NR_PERM_SALT, p0);
    nr_resample_unit_sums([&](int u) { return (nr_perm_swap(base, u) ? values_b : values_a) + (size_t)u * Q; }, U, Q,
                          out + (size_t)blockIdx.x * Q);
}

extern "C" int nr_permtest_unit_sums(const int64_t* values_a, const int64_t* values_b, int U, int Q, uint64_t seed, int p0, int n_perm,
                                     int64_t* out, void* stream) {
    if (!nr_resample_range_ok(U, p0, n_perm) || Q < 1 || Q > NR_BOOT_MAX_COLS) return NR_EINVAL;
    if (!values_a || !values_b || !out) return NR_EINVAL;
    if (n_perm == 0) return NR_OK;
    hipLaunchKernelGGL(nr_permtest_unit_sums_kernel, dim3((unsigned)n_perm), dim3(NR_BOOT_THREADS), 0, (hipStream_t)stream, values_a,
                       values_b, (uint32_t)U, Q, seed, (uint32_t)p0, out);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
