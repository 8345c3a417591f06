// What the resampling kernels share (nr_bootstrap.hip, nr_permtest.hip): the workgroup shape, the limits, the descriptor of one ranking,
// SplitMix64's output function and the walk from a unit to its entries.
#pragma once
#include "nr_common.h"

#define NR_BOOT_THREADS 256
#define NR_BOOT_WAVES (NR_BOOT_THREADS / NR_WAVE)
#define NR_BOOT_DIGIT 10
#define NR_BOOT_BINS (1 << NR_BOOT_DIGIT)
#define NR_BOOT_BINS_PER_THREAD (NR_BOOT_BINS / NR_BOOT_THREADS)
#define NR_BOOT_MAX_CUTS 8
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

// SplitMix64's output function of the state z
__device__ __forceinline__ uint64_t nr_boot_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the unit that position t of the resample draws; base = seed + ((b << 32) + 1) * golden
__device__ __forceinline__ int nr_boot_draw(uint64_t base, int t, uint32_t U) {
    const uint64_t x = nr_boot_mix(base + (uint64_t)(uint32_t)t * NR_BOOT_GOLDEN);
    return (int)__umulhi((uint32_t)(x >> 32), U);
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
