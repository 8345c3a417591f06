// Bootstrap of rank statistics (DESIGN.md "Bootstrap confidence intervals"): resample b draws U of the U units (queries, or videos in
// a multi-sentence set) with replacement and reports, over the multiset of rank entries of the drawn units, exact integers:
//   n, sum, the two middle order statistics, and hits[k] = #{r < cuts[k]}.
//
//   SM64(seed, c) = the (c + 1)-th output of SplitMix64 seeded with `seed`
//   u(b, t) = ((SM64(seed, (b << 32) | t) >> 32) * U) >> 32,   t in [0, U)
//
// The draws are counter-based: every pass recomputes them, nothing is stored per resample.  One workgroup per resample; a V = 2 call
// walks both rankings with the same draws.  The order statistics come from a radix select on the rank VALUE: an LDS histogram of one
// 10-bit digit per pass (LDS atomics), a scan, then a descent into the bin that holds position (n - 1) / 2; as many passes as the
// resample's largest rank has 10-bit digits (at most three for r < 2^30).  Position n / 2 is the same value unless it lies past the
// last entry equal to it, in which case one more pass takes the smallest larger rank.  No global atomics, no scratch; the result is
// a function of (seed, b, inputs) alone, the same for any grid and any split of the resamples over calls.
#include "nr_common.h"
#include "nr_resample.h"
#include "../../include/nr_hip.h"

// the statistics of one ranking of resample b into out[4 + K]
__device__ __forceinline__ void nr_boot_ranking(const NrBootRanking R, uint32_t U, const NrBootCuts cuts, int K, uint64_t base,
                                                int64_t* __restrict__ out, uint32_t* hist, int64_t (*red)[NR_BOOT_MAX_CUTS + 2],
                                                uint32_t* wave_tot, int64_t* pick) {
    const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1), wave = tid / NR_WAVE;

    // ---- pass 0: n, sum, hits and the largest rank ----
    int64_t acc[NR_BOOT_MAX_CUTS + 2];
#pragma unroll
    for (int k = 0; k < NR_BOOT_MAX_CUTS + 2; ++k) acc[k] = 0;
    int rmax = 0;
    for (int t = tid; t < (int)U; t += NR_BOOT_THREADS) {
        int lo, hi;
        nr_boot_unit(R, nr_boot_draw(base, t, U), lo, hi);
        for (int e = lo; e <= hi; ++e) {
            const int r = R.ranks[e];
            acc[0] += 1;
            acc[1] += r;
#pragma unroll
            for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k) acc[2 + k] += (int64_t)(r < cuts.c[k]);
            rmax = r > rmax ? r : rmax;
        }
    }
#pragma unroll
    for (int k = 0; k < NR_BOOT_MAX_CUTS + 2; ++k) acc[k] = nr_boot_wave_sum(acc[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(rmax, off, NR_WAVE);
        rmax = o > rmax ? o : rmax;
    }
    __syncthreads();                                  // the previous ranking's readers of red / pick are done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NR_BOOT_MAX_CUTS + 2; ++k) red[wave][k] = acc[k];
        wave_tot[wave] = (uint32_t)rmax;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NR_BOOT_MAX_CUTS + 2; ++k) {
        int64_t s = 0;
#pragma unroll
        for (int w = 0; w < NR_BOOT_WAVES; ++w) s += red[w][k];
        acc[k] = s;
    }
#pragma unroll
    for (int w = 0; w < NR_BOOT_WAVES; ++w) rmax = (int)wave_tot[w] > rmax ? (int)wave_tot[w] : rmax;
    const int64_t n = acc[0];
    if (tid == 0) {
        out[0] = n;
        out[1] = acc[1];
#pragma unroll
        for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k)
            if (k < K) out[4 + k] = acc[2 + k];
    }
    if (n == 0) {                                     // uniform over the workgroup
        if (tid == 0) out[2] = out[3] = -1;
        return;
    }

    // ---- radix select of position (n - 1) / 2: one digit per pass, from the top digit of the largest rank down ----
    const int passes = rmax >= (1 << (2 * NR_BOOT_DIGIT)) ? 3 : rmax >= NR_BOOT_BINS ? 2 : 1;
    uint32_t want = (uint32_t)((n - 1) >> 1);         // position inside the current bin
    int64_t below = 0;                                // entries smaller than the current bin's first value
    uint32_t prefix = 0, equal = 0;
    for (int p = 0; p < passes; ++p) {
        const int shift = NR_BOOT_DIGIT * (passes - 1 - p);
        __syncthreads();                              // the previous pass's readers of hist / pick / wave_tot are done
#pragma unroll
        for (int j = 0; j < NR_BOOT_BINS_PER_THREAD; ++j) hist[tid + j * NR_BOOT_THREADS] = 0;
        __syncthreads();
        for (int t = tid; t < (int)U; t += NR_BOOT_THREADS) {
            int lo, hi;
            nr_boot_unit(R, nr_boot_draw(base, t, U), lo, hi);
            for (int e = lo; e <= hi; ++e) {
                const uint32_t d = (uint32_t)R.ranks[e] >> shift;
                if ((d >> NR_BOOT_DIGIT) == prefix) atomicAdd(&hist[d & (NR_BOOT_BINS - 1)], 1u);
            }
        }
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
        for (int t = tid; t < (int)U; t += NR_BOOT_THREADS) {
            int lo, hi;
            nr_boot_unit(R, nr_boot_draw(base, t, U), lo, hi);
            for (int e = lo; e <= hi; ++e) {
                const int r = R.ranks[e];
                best = (r > med_lo && r < best) ? r : best;
            }
        }
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

__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_bootstrap_rank_stats_kernel(NrBootRanking A, NrBootRanking B, int V, uint32_t U,
                                                                                  NrBootCuts cuts, int K, uint64_t seed, uint32_t b0,
                                                                                  int64_t* __restrict__ out) {
    __shared__ uint32_t hist[NR_BOOT_BINS];
    __shared__ int64_t red[NR_BOOT_WAVES][NR_BOOT_MAX_CUTS + 2];
    __shared__ uint32_t wave_tot[NR_BOOT_WAVES];
    __shared__ int64_t pick[3];
    const uint64_t b = (uint64_t)b0 + blockIdx.x;
    const uint64_t base = seed + ((b << 32) + 1ull) * NR_BOOT_GOLDEN;
    int64_t* o = out + (size_t)blockIdx.x * V * (4 + K);
    nr_boot_ranking(A, U, cuts, K, base, o, hist, red, wave_tot, pick);
    if (V == 2) nr_boot_ranking(B, U, cuts, K, base, o + (4 + K), hist, red, wave_tot, pick);
}

extern "C" int nr_bootstrap_rank_stats(const int32_t* ranks_a, const int32_t* unit_end_a, int E_a, const int32_t* ranks_b,
                                       const int32_t* unit_end_b, int E_b, int U, const int32_t* cuts, int K, uint64_t seed, int b0,
                                       int n_boot, int64_t* out, void* stream) {
    if (U < 1 || U > NR_BOOT_MAX_UNITS || K < 1 || K > NR_BOOT_MAX_CUTS) return NR_EINVAL;
    if (E_a < 0 || b0 < 0 || n_boot < 0 || (int64_t)b0 + n_boot > 2147483647ll) return NR_EINVAL;
    if (!ranks_a || !unit_end_a || !cuts || !out) return NR_EINVAL;
    const int V = ranks_b ? 2 : 1;
    if (V == 2 && (E_b < 0 || !unit_end_b)) return NR_EINVAL;
    NrBootCuts c;
    for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k) c.c[k] = 0;
    for (int k = 0; k < K; ++k) {                     // the cut-offs are host memory: they travel as kernel arguments
        if (cuts[k] < 1 || (k && cuts[k] <= cuts[k - 1])) return NR_EINVAL;
        c.c[k] = cuts[k];
    }
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
// multiset of units in both.  One workgroup per resample; every thread keeps its Q <= 16 sums in int64 registers, the waves combine
// by shuffles, the workgroup through LDS.  Nothing is stored per resample, no atomics: a function of (seed, b, inputs) alone.
__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_bootstrap_unit_sums_kernel(const int64_t* __restrict__ values, uint32_t U, int Q,
                                                                                 uint64_t seed, uint32_t b0,
                                                                                 int64_t* __restrict__ out) {
    __shared__ int64_t red[NR_BOOT_WAVES][NR_BOOT_MAX_COLS];
    const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1), wave = tid / NR_WAVE;
    const uint64_t b = (uint64_t)b0 + blockIdx.x;
    const uint64_t base = seed + ((b << 32) + 1ull) * NR_BOOT_GOLDEN;
    int64_t acc[NR_BOOT_MAX_COLS];
#pragma unroll
    for (int q = 0; q < NR_BOOT_MAX_COLS; ++q) acc[q] = 0;
    for (int t = tid; t < (int)U; t += NR_BOOT_THREADS) {
        const int64_t* row = values + (size_t)nr_boot_draw(base, t, U) * Q;
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

extern "C" int nr_bootstrap_unit_sums(const int64_t* values, int U, int Q, uint64_t seed, int b0, int n_boot, int64_t* out,
                                      void* stream) {
    if (U < 1 || U > NR_BOOT_MAX_UNITS || Q < 1 || Q > NR_BOOT_MAX_COLS) return NR_EINVAL;
    if (b0 < 0 || n_boot < 0 || (int64_t)b0 + n_boot > 2147483647ll) return NR_EINVAL;
    if (!values || !out) return NR_EINVAL;
    if (n_boot == 0) return NR_OK;
    hipLaunchKernelGGL(nr_bootstrap_unit_sums_kernel, dim3((unsigned)n_boot), dim3(NR_BOOT_THREADS), 0, (hipStream_t)stream, values,
                       (uint32_t)U, Q, seed, (uint32_t)b0, out);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
