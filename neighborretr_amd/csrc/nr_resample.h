// The resampling engine of nr_bootstrap.hip, nr_permtest.hip and nr_hubperm.hip: the workgroup shape, the limits, the descriptor of one ranking,
// SplitMix64's output function, the swap rule of the permutation tests, what the entry points check alike, and the three device templates both files instantiate -- pass 0
// (n, sum, hits, the largest rank), the radix select of the two middle order statistics, and the sums of per-unit columns.  A file
// brings its resampling rule as a callable: `entries(f)` calls f(r) for every rank r the calling thread owns, `row(t)` is the row
// of values that unit position t reads.  Every thread of the workgroup calls a template with the same multiset of entries spread
// over the threads in any way; the result does not depend on the spread.
#pragma once
#include "nr_common.h"

#define NR_BOOT_THREADS 256
#define NR_BOOT_WAVES (NR_BOOT_THREADS / NR_WAVE)
#define NR_BOOT_DIGIT 10
#define NR_BOOT_BINS (1 << NR_BOOT_DIGIT)
#define NR_BOOT_BINS_PER_THREAD (NR_BOOT_BINS / NR_BOOT_THREADS)
#define NR_BOOT_MAX_CUTS 8
#define NR_BOOT_STATS (NR_BOOT_MAX_CUTS + 2)      // what pass 0 accumulates: n, sum, hits[0 .. 7]
#define NR_BOOT_MAX_UNITS (1 << 24)
#define NR_BOOT_MAX_COLS 16
#define NR_BOOT_RANK_LIMIT (1 << 30)
#define NR_BOOT_GOLDEN 0x9E3779B97F4A7C15ull

struct NrBootCuts {
    int32_t c[NR_BOOT_MAX_CUTS];          // cuts beyond K are 0: no rank lies below them
};

struct NrBootRanking {
    const int32_t* ranks;
    const int32_t* unit_end;
    int E;
};

// ---- what the entry points check alike ------------------------------------------------------------------------------------------
// U units and the resamples first .. first + count - 1: 1 <= U <= 2^24, first, count >= 0, first + count <= 2^31 - 1
inline bool nr_resample_range_ok(int U, int first, int count) {
    return U >= 1 && U <= NR_BOOT_MAX_UNITS && first >= 0 && count >= 0 && (int64_t)first + count <= 2147483647ll;
}

// the K cut-offs (host memory: they travel as kernel arguments) into c; false unless 1 <= K <= 8, positive, strictly increasing
inline bool nr_resample_cuts(const int32_t* cuts, int K, NrBootCuts& c) {
    if (!cuts || K < 1 || K > NR_BOOT_MAX_CUTS) return false;
    for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k) c.c[k] = 0;
    for (int k = 0; k < K; ++k) {
        if (cuts[k] < 1 || (k && cuts[k] <= cuts[k - 1])) return false;
        c.c[k] = cuts[k];
    }
    return true;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------
// SplitMix64's output function of the state z
__device__ __forceinline__ uint64_t nr_boot_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the state of this workgroup's resample first + blockIdx.x: position t of it mixes base + t * golden
__device__ __forceinline__ uint64_t nr_resample_base(uint64_t seed, uint32_t first) {
    return seed + ((((uint64_t)first + blockIdx.x) << 32) + 1ull) * NR_BOOT_GOLDEN;
}

// the swap bit s(p, u) of the paired permutation tests (nr_permtest.hip, nr_hubperm.hip); base = nr_resample_base(seed ^ salt, p0):
// (seed ^ salt) + ((p << 32) + 1) * golden.  The salt keeps the stream apart from the bootstrap's draws at equal seeds.
#define NR_PERM_SALT 0x7065726D74657374ull
__device__ __forceinline__ int nr_perm_swap(uint64_t base, int u) {
    return (int)(nr_boot_mix(base + (uint64_t)(uint32_t)u * NR_BOOT_GOLDEN) >> 63);
}

// entries [lo, hi] of unit u, clamped to the ranking's extent
__device__ __forceinline__ void nr_boot_unit(const NrBootRanking& R, int u, int& lo, int& hi) {
    lo = u > 0 ? R.unit_end[u - 1] + 1 : 0;
    hi = R.unit_end[u];
    lo = lo < 0 ? 0 : lo;
    hi = hi >= R.E ? R.E - 1 : hi;
}

__device__ __forceinline__ int64_t nr_boot_wave_sum(int64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, NR_WAVE);
    return v;
}

// ---- pass 0: n, sum, hits and the largest rank ----
// This thread's entries into acc = (n, sum, hits[0 .. 7]) and rmax, reduced over the wave.  The workgroup step is two calls with a
// __syncthreads() of the caller's between them: the callers lay `red` out differently (one ranking at a time, or both sides at once).
template <class Entries>
__device__ __forceinline__ void nr_resample_pass0(Entries entries, const NrBootCuts cuts, int64_t (&acc)[NR_BOOT_STATS], int& rmax) {
    int64_t a[NR_BOOT_STATS];                         // a local: summing into the caller's array costs the entry loop instructions
#pragma unroll
    for (int k = 0; k < NR_BOOT_STATS; ++k) a[k] = 0;
    int m = 0;
    entries([&](int r) {
        a[0] += 1;
        a[1] += r;
#pragma unroll
        for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k) a[2 + k] += (int64_t)(r < cuts.c[k]);
        m = r > m ? r : m;
    });
#pragma unroll
    for (int k = 0; k < NR_BOOT_STATS; ++k) acc[k] = nr_boot_wave_sum(a[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(m, off, NR_WAVE);
        m = o > m ? o : m;
    }
    rmax = m;
}

// lane 0 of every wave: its wave's statistics into red[wave * stride + k] and wave_max[wave * max_stride]
__device__ __forceinline__ void nr_resample_pass0_store(const int64_t (&acc)[NR_BOOT_STATS], int rmax, int64_t* red, int stride,
                                                        uint32_t* wave_max, int max_stride) {
    const int lane = threadIdx.x & (NR_WAVE - 1), wave = threadIdx.x / NR_WAVE;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NR_BOOT_STATS; ++k) red[wave * stride + k] = acc[k];
        wave_max[wave * max_stride] = (uint32_t)rmax;
    }
}

// after the barrier: every thread takes the workgroup's acc and rmax (uniform from here on), thread 0 writes n, sum and the K hits
__device__ __forceinline__ void nr_resample_pass0_total(int64_t (&acc)[NR_BOOT_STATS], int& rmax, const int64_t* red, int stride,
                                                        const uint32_t* wave_max, int max_stride, int K, int64_t* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < NR_BOOT_STATS; ++k) {
        int64_t s = 0;
#pragma unroll
        for (int w = 0; w < NR_BOOT_WAVES; ++w) s += red[w * stride + k];
        acc[k] = s;
    }
#pragma unroll
    for (int w = 0; w < NR_BOOT_WAVES; ++w) rmax = (int)wave_max[w * max_stride] > rmax ? (int)wave_max[w * max_stride] : rmax;
    if (threadIdx.x == 0) {
        out[0] = acc[0];
        out[1] = acc[1];
#pragma unroll
        for (int k = 0; k < NR_BOOT_MAX_CUTS; ++k)
            if (k < K) out[4 + k] = acc[2 + k];
    }
}

// ---- the order statistics at positions (n - 1) / 2 and n / 2 of the n entries, the largest of them rmax, into out[2], out[3] ----
// (-1, -1 when n = 0.)  n and rmax are uniform over the workgroup, and so is every barrier below.  A radix select on the rank VALUE:
// an LDS histogram of one 10-bit digit per pass (LDS atomics), a scan, then a descent into the bin that holds position (n - 1) / 2;
// as many passes as rmax has 10-bit digits (at most three for r < 2^30).  hist [NR_BOOT_BINS], wave_tot [NR_BOOT_WAVES] and pick [3]
// are the caller's LDS; a workgroup may call this again (the second ranking, the other side) without a barrier of its own.
template <class Entries>
__device__ __forceinline__ void nr_resample_select(Entries entries, int64_t n, int rmax, int64_t* __restrict__ out, uint32_t* hist,
                                                   uint32_t* wave_tot, int64_t* pick) {
    const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1), wave = tid / NR_WAVE;
    if (n == 0) {
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
        __syncthreads();                              // the previous pass's (call's) readers of hist / pick / wave_tot are done
#pragma unroll
        for (int j = 0; j < NR_BOOT_BINS_PER_THREAD; ++j) hist[tid + j * NR_BOOT_THREADS] = 0;
        __syncthreads();
        entries([&](int r) {
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
        entries([&](int r) { best = (r > med_lo && r < best) ? r : best; });
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

// ---- sums of per-unit columns: out[q] = sum over t < U of row(t)[q], q < Q <= 16 ----
// The threads stride over t, every thread keeps its sums in int64 registers, the waves combine by shuffles, the workgroup through
// LDS.  No atomics: a function of the rows alone.
template <class Row>
__device__ __forceinline__ void nr_resample_unit_sums(Row row, uint32_t U, int Q, int64_t* __restrict__ out) {
    __shared__ int64_t red[NR_BOOT_WAVES][NR_BOOT_MAX_COLS];
    const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1), wave = tid / NR_WAVE;
    int64_t acc[NR_BOOT_MAX_COLS];
#pragma unroll
    for (int q = 0; q < NR_BOOT_MAX_COLS; ++q) acc[q] = 0;
    for (int t = tid; t < (int)U; t += NR_BOOT_THREADS) {
        const int64_t* r = row(t);
#pragma unroll
        for (int q = 0; q < NR_BOOT_MAX_COLS; ++q)
            if (q < Q) acc[q] += r[q];
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
        out[tid] = s;
    }
}
