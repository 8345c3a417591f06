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
// over u, so `unit_end` and the entries are read coalesced -- the one structural gain over nr_bootstrap.hip.  Pass 0 serves both
// sides at once; the order statistics of each side come from a sibling of nr_boot_ranking's radix select on the rank VALUE (an LDS
// histogram of one 10-bit digit per pass, LDS atomics, a scan, a descent; one more pass for position n / 2 when it lies past the last
// entry equal to position (n - 1) / 2).  No global atomics, no scratch, no hand-off between workgroups: the result is a function of
// (seed, p, inputs) alone, the same for any grid and any split of the permutations over calls.
#include "nr_common.h"
#include "nr_resample.h"
#include "../../include/nr_hip.h"

#define NR_PERM_SALT 0x7065726D74657374ull
#define NR_PERM_STATS (NR_BOOT_MAX_CUTS + 2)

// s(p, u); base = (seed ^ salt) + ((p << 32) + 1) * golden
__device__ __forceinline__ int nr_perm_swap(uint64_t base, int u) {
    return (int)(nr_boot_mix(base + (uint64_t)(uint32_t)u * NR_BOOT_GOLDEN) >> 63);
}

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

// med_lo / med_hi of one side with n > 0 entries, the largest of them rmax, into out[2], out[3]
__device__ __forceinline__ void nr_perm_select(const NrBootRanking& A, const NrBootRanking& B, uint32_t U, uint64_t base, int side,
                                               int64_t n, int rmax, int64_t* __restrict__ out, uint32_t* hist, uint32_t* wave_tot,
                                               int64_t* pick) {
    const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1), wave = tid / NR_WAVE;
    // ---- radix select of position (n - 1) / 2: one digit per pass, from the top digit of the largest rank down ----
    const int passes = rmax >= (1 << (2 * NR_BOOT_DIGIT)) ? 3 : rmax >= NR_BOOT_BINS ? 2 : 1;
    uint32_t want = (uint32_t)((n - 1) >> 1);         // position inside the current bin
    int64_t below = 0;                                // entries smaller than the current bin's first value
    uint32_t prefix = 0, equal = 0;
    for (int p = 0; p < passes; ++p) {
        const int shift = NR_BOOT_DIGIT * (passes - 1 - p);
        __syncthreads();                              // the previous pass's (side's) readers of hist / pick / wave_tot are done
#pragma unroll
        for (int j = 0; j < NR_BOOT_BINS_PER_THREAD; ++j) hist[tid + j * NR_BOOT_THREADS] = 0;
        __syncthreads();
        nr_perm_entries(A, B, U, base, side, [&](int r) {
            const uint32_t d = (uint32_t)r >> shift;
            if ((d >> NR_BOOT_DIGIT) == prefix) atomicAdd(&hist[d & (NR_BOOT_BINS - 1)], 1u);
        });
        __syncthreads();
        // thread i owns bins 4 i .. 4 i + 3; an exclusive scan of the threads' totals finds the owner of position `want`
        uint32_t h[NR_BOOT_BINS_PER_THREAD], mine = 0;
#pragma unroll
        for (int j = 0; j < NR_BOOT_BINS_PER_THREAD; ++j) {
            h[j] = hist[tid * NR_BOOT_BINS_PER_THREAD + j];
            mine += h[j];
        }
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < NR_WAVE; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, NR_WAVE);
            if (lane >= off) incl += o;
        }
        if (lane == NR_WAVE - 1) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t excl = incl - mine;
#pragma unroll
        for (int w = 0; w < NR_BOOT_WAVES; ++w)
            if (w < wave) excl += wave_tot[w];
        if (want >= excl && want < excl + mine) {     // exactly one thread: the bins of this pass hold more than `want` entries
            uint32_t before = excl;
            int bin = 0;
#pragma unroll
            for (int j = 0; j < NR_BOOT_BINS_PER_THREAD - 1; ++j)
                if (bin == j && want >= before + h[j]) {
                    before += h[j];
                    bin = j + 1;
                }
            uint32_t cnt = h[0];
#pragma unroll
            for (int j = 1; j < NR_BOOT_BINS_PER_THREAD; ++j) cnt = bin == j ? h[j] : cnt;
            pick[0] = tid * NR_BOOT_BINS_PER_THREAD + bin;
            pick[1] = before;
            pick[2] = cnt;
        }
        __syncthreads();
        prefix = (prefix << NR_BOOT_DIGIT) | (uint32_t)pick[0];
        below += pick[1];
        want -= (uint32_t)pick[1];
        equal = (uint32_t)pick[2];
    }
    const int med_lo = (int)prefix;
    int med_hi = med_lo;
    // position n / 2 is one further: past the last entry equal to med_lo it is the smallest larger rank (uniform over the workgroup)
    if ((n >> 1) >= below + (int64_t)equal) {
        int best = 0x7FFFFFFF;
        nr_perm_entries(A, B, U, base, side, [&](int r) { best = (r > med_lo && r < best) ? r : best; });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(best, off, NR_WAVE);
            best = o < best ? o : best;
        }
        __syncthreads();                              // the last pass's readers of wave_tot are done
        if (lane == 0) wave_tot[wave] = (uint32_t)best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NR_BOOT_WAVES; ++w) best = (int)wave_tot[w] < best ? (int)wave_tot[w] : best;
        med_hi = best;
    }
    if (tid == 0) {
        out[2] = med_lo;
        out[3] = med_hi;
    }
}

__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_permtest_rank_stats_kernel(NrBootRanking A, NrBootRanking B, uint32_t U,
                                                                                 NrBootCuts cuts, int K, uint64_t seed, uint32_t p0,
                                                                                 int64_t* __restrict__ out) {
    __shared__ uint32_t hist[NR_BOOT_BINS];
    __shared__ int64_t red[NR_BOOT_WAVES][2][NR_PERM_STATS];
    __shared__ uint32_t wave_max[NR_BOOT_WAVES][2];
    __shared__ uint32_t wave_tot[NR_BOOT_WAVES];
    __shared__ int64_t pick[3];
    const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1), wave = tid / NR_WAVE;
    const uint64_t p = (uint64_t)p0 + blockIdx.x;
    const uint64_t base = (seed ^ NR_PERM_SALT) + ((p << 32) + 1ull) * NR_BOOT_GOLDEN;
    int64_t* o = out + (size_t)blockIdx.x * 2 * (4 + K);

    // ---- pass 0, both sides: n, sum, hits and the largest rank ----
    int64_t acc[2][NR_PERM_STATS];
    int rmax[2] = {0, 0};
#pragma unroll
    for (int side = 0; side < 2; ++side) {
#pragma unroll
        for (int k = 0; k < NR_PERM_STATS; ++k) acc[side][k] = 0;
        nr_perm_entries(A, B, U, base, side, [&](int r) {
            acc[side][0] += 1;
            acc[side][1] += r;
#pragma unroll
            for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k) acc[side][2 + k] += (int64_t)(r < cuts.c[k]);
            rmax[side] = r > rmax[side] ? r : rmax[side];
        });
#pragma unroll
        for (int k = 0; k < NR_PERM_STATS; ++k) acc[side][k] = nr_boot_wave_sum(acc[side][k]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int other = __shfl_xor(rmax[side], off, NR_WAVE);
            rmax[side] = other > rmax[side] ? other : rmax[side];
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NR_PERM_STATS; ++k) red[wave][side][k] = acc[side][k];
            wave_max[wave][side] = (uint32_t)rmax[side];
        }
    }
    __syncthreads();
#pragma unroll
    for (int side = 0; side < 2; ++side) {
#pragma unroll
        for (int k = 0; k < NR_PERM_STATS; ++k) {
            int64_t s = 0;
#pragma unroll
            for (int w = 0; w < NR_BOOT_WAVES; ++w) s += red[w][side][k];
            acc[side][k] = s;
        }
#pragma unroll
        for (int w = 0; w < NR_BOOT_WAVES; ++w) rmax[side] = (int)wave_max[w][side] > rmax[side] ? (int)wave_max[w][side] : rmax[side];
        if (tid == 0) {
            int64_t* os = o + side * (4 + K);
            os[0] = acc[side][0];
            os[1] = acc[side][1];
#pragma unroll
            for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k)
                if (k < K) os[4 + k] = acc[side][2 + k];
        }
    }

    // ---- the order statistics, one side after the other (n and rmax are uniform over the workgroup) ----
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        int64_t* os = o + side * (4 + K);
        if (acc[side][0] == 0) {
            if (tid == 0) os[2] = os[3] = -1;
        } else {
            nr_perm_select(A, B, U, base, side, acc[side][0], rmax[side], os, hist, wave_tot, pick);
        }
    }
}

extern "C" int nr_permtest_rank_stats(const int32_t* ranks_a, const int32_t* unit_end_a, int E_a, const int32_t* ranks_b,
                                      const int32_t* unit_end_b, int E_b, int U, const int32_t* cuts, int K, uint64_t seed, int p0,
                                      int n_perm, int64_t* out, void* stream) {
    if (U < 1 || U > NR_BOOT_MAX_UNITS || K < 1 || K > NR_BOOT_MAX_CUTS) return NR_EINVAL;
    if (E_a < 0 || E_b < 0 || p0 < 0 || n_perm < 0 || (int64_t)p0 + n_perm > 2147483647ll) return NR_EINVAL;
    if (!ranks_a || !unit_end_a || !ranks_b || !unit_end_b || !cuts || !out) return NR_EINVAL;
    NrBootCuts c;
    for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k) c.c[k] = 0;
    for (int k = 0; k < K; ++k) {                     // the cut-offs are host memory: they travel as kernel arguments
        if (cuts[k] < 1 || (k && cuts[k] <= cuts[k - 1])) return NR_EINVAL;
        c.c[k] = cuts[k];
    }
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
// two inputs' totals minus X, which the host takes.  One workgroup per permutation, the threads stride over the rows (coalesced),
// every thread keeps its Q <= 16 sums in int64 registers, the waves combine by shuffles, the workgroup through LDS.  No atomics.
__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_permtest_unit_sums_kernel(const int64_t* __restrict__ values_a,
                                                                                const int64_t* __restrict__ values_b, uint32_t U, int Q,
                                                                                uint64_t seed, uint32_t p0, int64_t* __restrict__ out) {
    __shared__ int64_t red[NR_BOOT_WAVES][NR_BOOT_MAX_COLS];
    const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1), wave = tid / NR_WAVE;
    const uint64_t p = (uint64_t)p0 + blockIdx.x;
    const uint64_t base = (seed ^ NR_PERM_SALT) + ((p << 32) + 1ull) * NR_BOOT_GOLDEN;
    int64_t acc[NR_BOOT_MAX_COLS];
#pragma unroll
    for (int q = 0; q < NR_BOOT_MAX_COLS; ++q) acc[q] = 0;
    for (int u = tid; u < (int)U; u += NR_BOOT_THREADS) {
        const int64_t* row = (nr_perm_swap(base, u) ? values_b : values_a) + (size_t)u * Q;
#pragma unroll
        for (int q = 0; q < NR_BOOT_MAX_COLS; ++q)
            if (q < Q) acc[q] += row[q];
    }
#pragma unroll
    for (int q = 0; q < NR_BOOT_MAX_COLS; ++q) acc[q] = nr_boot_wave_sum(acc[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NR_BOOT_MAX_COLS; ++q) red[wave][q] = acc[q];
    }
    __syncthreads();
    if (tid < Q) {
        int64_t s = 0;
#pragma unroll
        for (int w = 0; w < NR_BOOT_WAVES; ++w) s += red[w][tid];
        out[(size_t)blockIdx.x * Q + tid] = s;
    }
}

extern "C" int nr_permtest_unit_sums(const int64_t* values_a, const int64_t* values_b, int U, int Q, uint64_t seed, int p0, int n_perm,
                                     int64_t* out, void* stream) {
    if (U < 1 || U > NR_BOOT_MAX_UNITS || Q < 1 || Q > NR_BOOT_MAX_COLS) return NR_EINVAL;
    if (p0 < 0 || n_perm < 0 || (int64_t)p0 + n_perm > 2147483647ll) return NR_EINVAL;
    if (!values_a || !values_b || !out) return NR_EINVAL;
    if (n_perm == 0) return NR_OK;
    hipLaunchKernelGGL(nr_permtest_unit_sums_kernel, dim3((unsigned)n_perm), dim3(NR_BOOT_THREADS), 0, (hipStream_t)stream, values_a,
                       values_b, (uint32_t)U, Q, seed, (uint32_t)p0, out);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
