// Inverted-file (IVF) prefilter of two-stage retrieval.  The reference has no such path: it scores every pair.
//
// The gallery's pooled vectors are dealt to L k-means lists; `rows` holds them list by list (list l = the rows
// [list_offsets[l], list_offsets[l + 1]), members in ascending gallery index, list_items[r] = the gallery index of row r).  A query
// scans only the P lists whose centroids it is closest to:
//   nr_ivf_list_sums   the per-list sums of the k-means update (index build, not on the search path)
//   nr_ivf_scan        the coarse scores of every (query, member of a probed list) pair, LIST-MAJOR: the (query, probe) pairs of a
//                      chunk arrive grouped by list, one workgroup scores 16 queries of one list's group against 16 consecutive
//                      rows of that list on v_mfma_f32_16x16x4_f32 -- the body of nr_gemm_nt_f32_kernel with an indirection on
//                      the A rows, so that every score has the bits nr_gemm_nt_f32 gives that (query, item) pair
//   nr_ivf_select      one workgroup per query: the top C of its pool by (score descending, gallery index ascending), emitted
//                      in ascending gallery index -- a radix select on the 64-bit keys (score key << 32) | ~item
// No float atomics, no scratch memory; every output element is written by exactly one workgroup; only integer counts decide.
#include "nr_common.h"
#include "../../include/nr_hip.h"

#define NR_IVF_MAX_C 128
#define NR_IVF_MAX_PROBE 128
#define NR_IVF_CACHE_KEYS 16384      // 128 KB of 64-bit keys in LDS per workgroup (of 160 KB); longer lines re-read memory
#define NR_IVF_SELECT_FIXED 2576     // bytes of the select kernel's LDS ahead of the key cache (a multiple of 16)

// ---- per-list sums ------------------------------------------------------------------------------------------------------------
// One workgroup per list, threads over d; the members are added in list order (ascending gallery index), one sequential fp32
// addition per component: a float32 loop on the host reproduces the bits.  Four members' loads are in flight per trip.
__global__ __launch_bounds__(256) void nr_ivf_list_sums_kernel(const float* __restrict__ x, const int32_t* __restrict__ list_items,
                                                              const int32_t* __restrict__ list_offsets, int n_items, int d,
                                                              float* __restrict__ sums) {
    const int l = blockIdx.x;
    const int begin = min(max(list_offsets[l], 0), n_items), end = min(max(list_offsets[l + 1], begin), n_items);
    for (int c = threadIdx.x; c < d; c += 256) {
        float acc = 0.f;
        int m = begin;
        for (; m + 4 <= end; m += 4) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int g = list_items[m + u];
                v[u] = (g >= 0 && g < n_items) ? x[(size_t)g * d + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += v[u];
        }
        for (; m < end; ++m) {
            const int g = list_items[m];
            acc += (g >= 0 && g < n_items) ? x[(size_t)g * d + c] : 0.f;
        }
        sums[(size_t)l * d + c] = acc;
    }
}

extern "C" int nr_ivf_list_sums(const float* x, const int32_t* list_items, const int32_t* list_offsets, int n_items, int n_lists,
                                int d, float* sums, void* stream) {
    if (!x || !list_items || !list_offsets || !sums) return NR_EINVAL;
    if (n_items <= 0 || n_lists <= 0 || n_lists > n_items || d <= 0) return NR_EINVAL;
    hipLaunchKernelGGL(nr_ivf_list_sums_kernel, dim3(n_lists), dim3(256), 0, (hipStream_t)stream, x, list_items, list_offsets,
                       n_items, d, sums);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- list-major scan ------------------------------------------------------------------------------------------------------------
// The 16 x 16 tile of nr_gemm_nt_f32_kernel (nr_small.hip) between row pointers: pa / pb = this lane's operand rows, already
// advanced by 4 * (lane >> 4).  The K blocks are dealt to the four waves in that kernel's pattern (wave w: the 16-wide blocks w,
// w + 4, ..., four of them per trip), the MFMA sequence inside a wave is the same, and the caller combines the four partial tiles
// as (acc + p1) + (p2 + p3): an element's bits depend on its two rows and K only, and equal those of nr_gemm_nt_f32.
// tests/test_ivf_gpu.py holds the two kernels together bit for bit.
__device__ __forceinline__ f32x4_t nr_ivf_tile_partial(const float* __restrict__ pa, const float* __restrict__ pb, int K, int wave) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = wave * 16; k0 < K; k0 += 256) {
        f32x4_t va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * 64;
            const bool ok = k < K;
            va[u] = ok ? *reinterpret_cast<const f32x4_t*>(pa + k) : f32x4_t{0.f, 0.f, 0.f, 0.f};
            vb[u] = ok ? *reinterpret_cast<const f32x4_t*>(pb + k) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va[u][s], vb[u][s], acc, 0, 0, 0);
    }
    return acc;
}

__device__ __forceinline__ int nr_ivf_list_size(const int32_t* __restrict__ list_offsets, int list, int n_lists, int n_items) {
    if (list < 0 || list >= n_lists) return 0;               // a missing probe (-1) is an empty list
    const int b = min(max(list_offsets[list], 0), n_items);
    return min(max(list_offsets[list + 1], b), n_items) - b;
}

// Buckets: b < n_lists = list b, b = n_lists = the (query, probe) pairs without a list (probe outside [0, n_lists): nothing to
// score, but the pair may still be the one that writes its query's pool_len).  pair_order [n * P]: the pair ids q * P + rank,
// grouped by bucket, in ascending id inside a bucket; group_offsets [n_lists + 2]: where each bucket's pairs start;
// tile_offsets [n_lists + 2]: where each bucket's 16-query tiles start (bucket b owns ceil(count_b / 16) of them).
// blockIdx.x = a 16-query tile (surplus ones exit), blockIdx.y = 16 rows of the tile's list (those past its size exit).
__global__ __launch_bounds__(256) void nr_ivf_scan_kernel(const float* __restrict__ q, int n, const float* __restrict__ rows,
                                                         const int32_t* __restrict__ list_items,
                                                         const int32_t* __restrict__ list_offsets, int n_items, int n_lists, int d,
                                                         const int32_t* __restrict__ probes, int P,
                                                         const int32_t* __restrict__ pair_order,
                                                         const int32_t* __restrict__ group_offsets,
                                                         const int32_t* __restrict__ tile_offsets, float* __restrict__ pool_score,
                                                         int32_t* __restrict__ pool_item, int32_t* __restrict__ pool_len, int stride) {
    __shared__ f32x4_t s_part[3][64];
    __shared__ int s_q[16], s_rank[16], s_base[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    if (tile >= tile_offsets[n_lists + 1]) return;
    int lo = 0, hi = n_lists;                                // the last bucket whose first tile is <= tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_offsets[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    const int bucket = lo;
    const long long n_pairs = (long long)n * P;
    const long long g0 = (long long)group_offsets[bucket] + 16ll * (tile - tile_offsets[bucket]);
    const long long g1 = min((long long)group_offsets[bucket + 1], min(g0 + 16, n_pairs));
    const int cnt = (g0 >= 0 && g1 > g0) ? (int)(g1 - g0) : 0;
    const int size = nr_ivf_list_size(list_offsets, bucket, n_lists, n_items);
    const int row_lo = blockIdx.y * 16;
    if (cnt == 0 || (row_lo > 0 && row_lo >= size)) return;

    // pair p of the tile: its query, its probe rank and its base = the sizes of the query's probed lists of lower rank;
    // 16 threads per pair share the sum (integers: any order)
    {
        const int p = tid >> 4, sub = tid & 15;
        int qi = -1, rank = 0, part = 0;
        if (p < cnt) {
            const int id = pair_order[g0 + p];
            if (id >= 0 && id < n_pairs) {
                qi = id / P;
                rank = id - qi * P;
                for (int r = sub; r < rank; r += 16) part += nr_ivf_list_size(list_offsets, probes[(long long)qi * P + r], n_lists, n_items);
            }
        }
        part += __shfl_xor(part, 8);
        part += __shfl_xor(part, 4);
        part += __shfl_xor(part, 2);
        part += __shfl_xor(part, 1);
        if (sub == 0) { s_q[p] = qi; s_rank[p] = rank; s_base[p] = part; }
    }
    __syncthreads();
    if (row_lo == 0 && tid < 16 && s_q[tid] >= 0 && s_rank[tid] == P - 1) pool_len[s_q[tid]] = min(s_base[tid] + size, stride);
    if (row_lo >= size) return;

    // operand rows clamped as nr_gemm_nt_f32_kernel clamps them: a ragged tile repeats its last valid row, nothing of it is stored
    int aq = s_q[min(lane & 15, cnt - 1)];
    aq = aq < 0 ? 0 : aq;
    const int begin = min(max(list_offsets[bucket], 0), n_items);
    const int br = begin + min(row_lo + (lane & 15), size - 1);
    const float* pa = q + (size_t)aq * d + 4 * (lane >> 4);
    const float* pb = rows + (size_t)br * d + 4 * (lane >> 4);
    const f32x4_t acc = nr_ivf_tile_partial(pa, pb, d, wave);
    if (wave > 0) s_part[wave - 1][lane] = acc;
    __syncthreads();
    if (wave > 0) return;
    const f32x4_t p1 = s_part[0][lane], p2 = s_part[1][lane], p3 = s_part[2][lane];
    const int col = row_lo + (lane & 15);
    if (col >= size) return;
    const int item = list_items[begin + col];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = (lane >> 4) * 4 + j;
        if (p >= cnt || s_q[p] < 0) continue;
        const long long slot = (long long)s_base[p] + col;
        if (slot >= stride) continue;                        // never with stride >= the sum of the P largest lists
        const long long at = (long long)s_q[p] * stride + slot;
        pool_score[at] = (acc[j] + p1[j]) + (p2[j] + p3[j]);
        pool_item[at] = item;
    }
}

// an upper bound of the 16-query tiles of n_pairs pairs in at most n_buckets groups: sum ceil(c / 16) <= (n_pairs + 15 groups) / 16
static long long nr_ivf_tile_bound(long long n_pairs, long long n_buckets) {
    const long long groups = n_pairs < n_buckets ? n_pairs : n_buckets;
    return (n_pairs + 15 * groups) / 16;
}

extern "C" int nr_ivf_scan(const float* q, int n, const float* rows, const int32_t* list_items, const int32_t* list_offsets,
                           int n_items, int n_lists, int d, const int32_t* probes, int n_probe, const int32_t* pair_order,
                           const int32_t* group_offsets, const int32_t* tile_offsets, int max_list_size, float* pool_score,
                           int32_t* pool_item, int32_t* pool_len, int stride, void* stream) {
    if (!q || !rows || !list_items || !list_offsets || !probes || !pair_order || !group_offsets || !tile_offsets) return NR_EINVAL;
    if (!pool_score || !pool_item || !pool_len) return NR_EINVAL;
    if (n <= 0 || n_items <= 0 || n_lists <= 0 || n_lists > n_items || d <= 0 || (d % 16) != 0) return NR_EINVAL;
    if (n_probe < 1 || n_probe > NR_IVF_MAX_PROBE || n_probe > n_lists) return NR_EINVAL;
    if (max_list_size < 0 || max_list_size > n_items || stride < 1) return NR_EINVAL;
    const long long tiles = nr_ivf_tile_bound((long long)n * n_probe, (long long)n_lists + 1);
    const int row_tiles = max_list_size > 0 ? (max_list_size + 15) / 16 : 1;
    if (tiles > 0x7fffffffLL || row_tiles > 65535) return NR_EUNSUPPORTED;
    hipLaunchKernelGGL(nr_ivf_scan_kernel, dim3((unsigned)tiles, (unsigned)row_tiles), dim3(256), 0, (hipStream_t)stream, q, n, rows,
                       list_items, list_offsets, n_items, n_lists, d, probes, n_probe, pair_order, group_offsets, tile_offsets,
                       pool_score, pool_item, pool_len, stride);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- selection ----------------------------------------------------------------------------------------------------------------
// larger key = earlier in (score descending, gallery index ascending); the keys of a pool are distinct because its items are
__device__ __forceinline__ unsigned long long nr_ivf_key(float score, int32_t item) {
    return ((unsigned long long)nr_order_key(score) << 32) | (unsigned long long)(~(uint32_t)item);
}

// One workgroup per query.  Eight 8-bit radix passes with a 256-bin LDS histogram find T = the kk-th largest key (kk = min(C,
// pool_len)); the entries with key >= T and a non-NaN score are kept (exactly kk of them, fewer when NaNs reach into the top kk)
// and ordered by counting.  CACHED: the keys stay in LDS after the first pass.
template <bool CACHED>
__global__ __launch_bounds__(256) void nr_ivf_select_kernel(const float* __restrict__ pool_score, const int32_t* __restrict__ pool_item,
                                                           const int32_t* __restrict__ pool_len, int stride, int C,
                                                           int32_t* __restrict__ cand, float* __restrict__ score_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* sel_key = reinterpret_cast<unsigned long long*>(smem);              // [128]
    int* hist = reinterpret_cast<int*>(smem + 1024);                                          // [256]
    int* sel_pos = reinterpret_cast<int*>(smem + 2048);                                       // [128]
    int* s_misc = reinterpret_cast<int*>(smem + 2560);                                        // digit, above, n_kept
    unsigned long long* cache = reinterpret_cast<unsigned long long*>(smem + NR_IVF_SELECT_FIXED);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long line = (long long)blockIdx.x * stride;
    const float* ps = pool_score + line;
    const int32_t* pi = pool_item + line;
    const int len = min(max(pool_len[blockIdx.x], 0), stride);
    const int kk = min(C, len);
    int32_t* co = cand + (long long)blockIdx.x * C;
    float* so = score_out ? score_out + (long long)blockIdx.x * C : nullptr;
    if (kk == 0) {
        if (tid < C) {
            co[tid] = -1;
            if (so) so[tid] = -INFINITY;
        }
        return;
    }

    unsigned long long prefix = 0, pmask = 0;
    int rem = kk;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int e = tid; e < len; e += 256) {
            unsigned long long key;
            if (CACHED && shift != 56) {
                key = cache[e];
            } else {
                key = nr_ivf_key(ps[e], pi[e]);
                if (CACHED) cache[e] = key;
            }
            if ((key & pmask) == prefix) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (wave == 0) {
            // lane l holds bins 4l..4l+3; the digit is the bin where the count from the top first reaches rem
            const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
            const int s = c0 + c1 + c2 + c3;
            int suf = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_down(suf, o);
                if (lane + o < 64) suf += t;
            }
            int a = suf - s;
            if (a < rem && rem <= a + c3) { s_misc[0] = 4 * lane + 3; s_misc[1] = a; }
            a += c3;
            if (a < rem && rem <= a + c2) { s_misc[0] = 4 * lane + 2; s_misc[1] = a; }
            a += c2;
            if (a < rem && rem <= a + c1) { s_misc[0] = 4 * lane + 1; s_misc[1] = a; }
            a += c1;
            if (a < rem && rem <= a + c0) { s_misc[0] = 4 * lane; s_misc[1] = a; }
        }
        __syncthreads();
        prefix |= (unsigned long long)s_misc[0] << shift;
        pmask |= 0xFFull << shift;
        rem -= s_misc[1];
    }
    const unsigned long long T = prefix;

    if (tid == 0) s_misc[2] = 0;
    __syncthreads();
    for (int e = tid; e < len; e += 256) {
        const unsigned long long key = CACHED ? cache[e] : nr_ivf_key(ps[e], pi[e]);
        if (key >= T && (key >> 32) != 0ull) {
            const int p = atomicAdd(&s_misc[2], 1);
            if (p < NR_IVF_MAX_C) { sel_key[p] = key; sel_pos[p] = e; }
        }
    }
    __syncthreads();
    const int n_sel = min(s_misc[2], kk);

    // ascending gallery index: the place of a kept entry = the number of kept entries with a lower item
    if (tid < n_sel) {
        const uint32_t item = ~(uint32_t)sel_key[tid];
        int rank = 0;
        for (int j = 0; j < n_sel; ++j) {
            const uint32_t ij = ~(uint32_t)sel_key[j];
            rank += (ij < item) || (ij == item && j < tid);
        }
        co[rank] = (int32_t)item;
        if (so) so[rank] = ps[sel_pos[tid]];
    } else if (tid < C) {
        co[tid] = -1;
        if (so) so[tid] = -INFINITY;
    }
}

extern "C" int nr_ivf_select(const float* pool_score, const int32_t* pool_item, const int32_t* pool_len, int n, int stride, int C,
                             int32_t* cand, float* score_out, void* stream) {
    if (!pool_score || !pool_item || !pool_len || !cand) return NR_EINVAL;
    if (n <= 0 || stride < 1 || C < 1 || C > NR_IVF_MAX_C) return NR_EINVAL;
    if (stride <= NR_IVF_CACHE_KEYS) {
        const size_t lds = NR_IVF_SELECT_FIXED + (size_t)stride * sizeof(unsigned long long);
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)nr_ivf_select_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(nr_ivf_select_kernel<true>, dim3(n), dim3(256), lds, (hipStream_t)stream, pool_score, pool_item, pool_len,
                           stride, C, cand, score_out);
    } else {
        hipLaunchKernelGGL(nr_ivf_select_kernel<false>, dim3(n), dim3(256), NR_IVF_SELECT_FIXED, (hipStream_t)stream, pool_score,
                           pool_item, pool_len, stride, C, cand, score_out);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}
