// Paired permutation (randomisation) test of hubness (DESIGN.md "Permutation test of hubness"): two rankings A and B as top-k lists
// over the same queries and the same gallery of G items, the lists grouped into U units.  Permutation p swaps the two rankings' lists
// unit by unit with the swap bits s(p, u) of nr_permtest.hip (nr_perm_swap, nr_resample.h) and reports, for both sides of the
// relabelling, the exact integers from which the host takes every hubness figure of a side:
//   S1 = sum N, S2 = sum N^2, S3 = sum N^3, #{N = 0}, #{N G > 2 S1}, the sum of N over those hubs, #{hub and N - GN > GN}, sum GN, max N
// with N[j] = the side's lists that hold item j and GN[j] = those for which j lies in the list's ground-truth range.
//
// One workgroup per permutation.  It builds side X's counters in LDS with integer LDS atomics, one 32-bit word per gallery item: N in
// the low half, GN in the high half (a list holds an item at most once, so N <= n_lists < 65 536 and the halves never carry).  Side Y
// needs no second histogram: every list goes to exactly one side, so N_Y = N_A + N_B - N_X and likewise GN; the A + B totals come in
// as two int32 [G] vectors.  After one barrier a first sweep over the items gives both sides' S1, S2, S3, anti-hubs, good occurrences
// and max; a second sweep gives the three hub figures against each side's own threshold.  Reductions are int64, by wave shuffles and
// through LDS.
//
// The walk.  A wave takes 64 consecutive units at a time: lane i reads unit_end of unit u0 + i (coalesced) and recomputes its swap bit;
// the 64 bits travel as one ballot.  The lists of those units are one contiguous run of rows, so the wave then reads that run of
// `idx` word by word, lane i at word base + i: consecutive words, whatever k is.  The unit of a word's list is the first lane whose
// unit ends at or after it -- a 6-step lower bound over the lanes' `hi` by shuffles, no memory.  Nothing is stored per unit.
//
// No global atomics, no float atomics, no scratch, no hand-off between workgroups: the output is a function of (seed, p, inputs) alone,
// for any grid and any split over p0.  The kernel stays in bounds whatever unit_end and idx hold: list indices are clamped to
// [0, n_lists), items outside [0, G) are not counted, and nothing read from memory is used as an index unclamped.
#include "nr_common.h"
#include "nr_resample.h"
#include "../../include/nr_hip.h"

#define NR_HUBPERM_MAX_GALLERY 32768
#define NR_HUBPERM_MAX_LISTS 65535
#define NR_HUBPERM_MAX_K 128
#define NR_HUBPERM_OUT 9
#define NR_HUBPERM_SUMS1 5                          // sweep 1, per side: S1, S2, S3, anti, good (and the max beside them)
#define NR_HUBPERM_SUMS2 3                          // sweep 2, per side: hubs, hub_occ, bad_hubs
#define NR_HUBPERM_RED1 (2 * (NR_HUBPERM_SUMS1 + 1))
#define NR_HUBPERM_RED2 (2 * NR_HUBPERM_SUMS2)
#define NR_HUBPERM_RED_BYTES (NR_BOOT_WAVES * (NR_HUBPERM_RED1 + NR_HUBPERM_RED2) * 8)      // 576: a multiple of 16

struct NrHubPermLists {
    const int32_t* idx_a;
    const int32_t* idx_b;
    const int32_t* unit_end;
    const int32_t* gt_begin;
    const int32_t* gt_end;
    int n_lists, k;
};

__device__ __forceinline__ int64_t nr_hubperm_wave_max(int64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t o = __shfl_xor(v, off, NR_WAVE);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(NR_BOOT_THREADS) void nr_permtest_hubness_kernel(NrHubPermLists L, uint32_t U, int G,
                                                                              const int32_t* __restrict__ occ_ab,
                                                                              const int32_t* __restrict__ good_ab, uint64_t seed,
                                                                              uint32_t p0, int64_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int64_t* red1 = reinterpret_cast<int64_t*>(smem);                            // [waves][NR_HUBPERM_RED1]
    int64_t* red2 = red1 + NR_BOOT_WAVES * NR_HUBPERM_RED1;                      // [waves][NR_HUBPERM_RED2]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + NR_HUBPERM_RED_BYTES);    // [G]: N_X | GN_X << 16
    const int tid = threadIdx.x, lane = tid & (NR_WAVE - 1), wave = tid / NR_WAVE;
    const uint64_t base = nr_resample_base(seed ^ NR_PERM_SALT, p0);

    for (int j = tid; j < G; j += NR_BOOT_THREADS) cnt[j] = 0;
    __syncthreads();

    // ---- side X's histogram ----
    const int k = L.k, last_list = L.n_lists - 1;
    for (int u0 = wave * NR_WAVE; u0 < (int)U; u0 += NR_BOOT_THREADS) {          // wave-uniform
        const int u = u0 + lane;
        int lo = 0, hi = L.n_lists, s = 0;                                       // a lane past U: never the lower bound of a list
        if (u < (int)U) {
            int prev = u > 0 ? L.unit_end[u - 1] : -1;
            prev = prev < -1 ? -1 : prev > last_list ? last_list : prev;         // clamped before the + 1: lo in [0, n_lists]
            lo = prev + 1;
            hi = L.unit_end[u];
            hi = hi > last_list ? last_list : hi;
            s = nr_perm_swap(base, u);
        }
        const uint64_t swaps = __ballot(s);
        const int n_valid = (int)U - u0 < NR_WAVE ? (int)U - u0 : NR_WAVE;
        const int first = __shfl(lo, 0, NR_WAVE), last = __shfl(hi, n_valid - 1, NR_WAVE);      // this wave's run of lists
        const int w_end = (last + 1) * k;                                        // < 2^23
        for (int w0 = first * k; w0 < w_end; w0 += NR_WAVE) {                    // wave-uniform: every lane takes part in the shuffles
            const int w = w0 + lane;
            const bool live = w < w_end;
            const int q = live ? w / k : last;                                   // in [0, n_lists) where live
            int pos = 0;                                                         // the first lane with hi >= q
#pragma unroll
            for (int step = NR_WAVE / 2; step > 0; step >>= 1) {
                const int h = __shfl(hi, pos + step - 1, NR_WAVE);
                pos += h < q ? step : 0;
            }
            if (live) {
                const int32_t* idx = ((swaps >> pos) & 1ull) ? L.idx_b : L.idx_a;
                const int j = idx[w];
                if ((uint32_t)j < (uint32_t)G) {
                    const uint32_t is_gt = (j >= L.gt_begin[q] && j < L.gt_end[q]) ? 1u : 0u;
                    atomicAdd(&cnt[j], 1u | (is_gt << 16));
                }
            }
        }
    }
    __syncthreads();

    // ---- sweep 1: both sides' S1, S2, S3, anti-hubs, good occurrences, max ----
    int64_t acc[2][NR_HUBPERM_SUMS1], mx[2] = {0, 0};
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int i = 0; i < NR_HUBPERM_SUMS1; ++i) acc[side][i] = 0;
    for (int j = tid; j < G; j += NR_BOOT_THREADS) {
        const uint32_t c = cnt[j];
        int64_t n[2], g[2];
        n[0] = c & 0xFFFFu;
        g[0] = c >> 16;
        n[1] = (int64_t)occ_ab[j] - n[0];
        g[1] = (int64_t)good_ab[j] - g[0];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            acc[side][0] += n[side];
            acc[side][1] += n[side] * n[side];
            acc[side][2] += n[side] * n[side] * n[side];
            acc[side][3] += (int64_t)(n[side] == 0);
            acc[side][4] += g[side];
            mx[side] = n[side] > mx[side] ? n[side] : mx[side];
        }
    }
#pragma unroll
    for (int side = 0; side < 2; ++side) {
#pragma unroll
        for (int i = 0; i < NR_HUBPERM_SUMS1; ++i) {
            const int64_t v = nr_boot_wave_sum(acc[side][i]);
            if (lane == 0) red1[wave * NR_HUBPERM_RED1 + side * (NR_HUBPERM_SUMS1 + 1) + i] = v;
        }
        const int64_t m = nr_hubperm_wave_max(mx[side]);
        if (lane == 0) red1[wave * NR_HUBPERM_RED1 + side * (NR_HUBPERM_SUMS1 + 1) + NR_HUBPERM_SUMS1] = m;
    }
    __syncthreads();
    int64_t tot[2][NR_HUBPERM_SUMS1 + 1];                                        // uniform over the workgroup
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int i = 0; i <= NR_HUBPERM_SUMS1; ++i) {
            int64_t v = 0;
#pragma unroll
            for (int w = 0; w < NR_BOOT_WAVES; ++w) {
                const int64_t r = red1[w * NR_HUBPERM_RED1 + side * (NR_HUBPERM_SUMS1 + 1) + i];
                v = i < NR_HUBPERM_SUMS1 ? v + r : (r > v ? r : v);
            }
            tot[side][i] = v;
        }

    // ---- sweep 2: hubs (N G > 2 S1), their occurrences, bad hubs (N - GN > GN), each side against its own S1 ----
    int64_t hub[2][NR_HUBPERM_SUMS2];
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int i = 0; i < NR_HUBPERM_SUMS2; ++i) hub[side][i] = 0;
    for (int j = tid; j < G; j += NR_BOOT_THREADS) {
        const uint32_t c = cnt[j];
        int64_t n[2], g[2];
        n[0] = c & 0xFFFFu;
        g[0] = c >> 16;
        n[1] = (int64_t)occ_ab[j] - n[0];
        g[1] = (int64_t)good_ab[j] - g[0];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const bool is_hub = n[side] * (int64_t)G > 2 * tot[side][0];
            hub[side][0] += (int64_t)is_hub;
            hub[side][1] += is_hub ? n[side] : 0;
            hub[side][2] += (int64_t)(is_hub && n[side] - g[side] > g[side]);
        }
    }
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int i = 0; i < NR_HUBPERM_SUMS2; ++i) {
            const int64_t v = nr_boot_wave_sum(hub[side][i]);
            if (lane == 0) red2[wave * NR_HUBPERM_RED2 + side * NR_HUBPERM_SUMS2 + i] = v;
        }
    __syncthreads();
    if (tid == 0) {
        int64_t* o = out + (size_t)blockIdx.x * 2 * NR_HUBPERM_OUT;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            int64_t h[NR_HUBPERM_SUMS2];
#pragma unroll
            for (int i = 0; i < NR_HUBPERM_SUMS2; ++i) {
                h[i] = 0;
#pragma unroll
                for (int w = 0; w < NR_BOOT_WAVES; ++w) h[i] += red2[w * NR_HUBPERM_RED2 + side * NR_HUBPERM_SUMS2 + i];
            }
            int64_t* r = o + side * NR_HUBPERM_OUT;
            r[0] = tot[side][0];
            r[1] = tot[side][1];
            r[2] = tot[side][2];
            r[3] = tot[side][3];
            r[4] = h[0];
            r[5] = h[1];
            r[6] = h[2];
            r[7] = tot[side][4];
            r[8] = tot[side][5];
        }
    }
}

extern "C" int nr_permtest_hubness(const int32_t* idx_a, const int32_t* idx_b, int n_lists, int k, const int32_t* unit_end, int U,
                                   int n_gallery, const int32_t* gt_begin, const int32_t* gt_end, const int32_t* occ_ab,
                                   const int32_t* good_ab, uint64_t seed, int p0, int n_perm, int64_t* out, void* stream) {
    if (!nr_resample_range_ok(U, p0, n_perm) || k < 1 || k > NR_HUBPERM_MAX_K || n_lists < 0 || n_gallery < 1) return NR_EINVAL;
    if (!idx_a || !idx_b || !unit_end || !gt_begin || !gt_end || !occ_ab || !good_ab || !out) return NR_EINVAL;
    if (n_gallery > NR_HUBPERM_MAX_GALLERY || n_lists > NR_HUBPERM_MAX_LISTS) return NR_EUNSUPPORTED;
    if (n_perm == 0) return NR_OK;
    const size_t lds = NR_HUBPERM_RED_BYTES + 4 * (size_t)n_gallery;
    if (lds > 64 * 1024) {      // per device and cheap: asked again at every such launch rather than cached
        hipError_t e = hipFuncSetAttribute((const void*)nr_permtest_hubness_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const NrHubPermLists L = {idx_a, idx_b, unit_end, gt_begin, gt_end, n_lists, k};
    hipLaunchKernelGGL(nr_permtest_hubness_kernel, dim3((unsigned)n_perm), dim3(NR_BOOT_THREADS), lds, (hipStream_t)stream, L,
                       (uint32_t)U, n_gallery, occ_ab, good_ab, seed, (uint32_t)p0, out);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
