// Deterministic top-k selection over similarity slabs (hubness evaluation, DESIGN.md "Top-k lists and hubness").
//
// Order of one query's line of scores: score descending, equal scores by gallery index ascending; -0.0 ties with +0.0;
// +inf above every finite score, -inf below; NaN is never selected.  A line with fewer than k selectable entries is padded
// with index -1 / value -inf.  Values are the exact bits of S.
//
// Selection (one workgroup per line): every score becomes an order-preserving 32-bit key (NaN -> 0, below -inf's key;
// both zeros -> the same key).  Four 8-bit radix passes with a 256-bin LDS histogram find the k-th largest key T and how
// many entries equal to T the list takes; one compaction pass over the line in index order keeps the keys above T and the
// first such ties; the <= 128 kept entries are ordered by counting.  No line is sorted.  Lines of up to
// NR_TOPK_CACHE_KEYS entries keep their keys in LDS after the first pass, so S is read from memory once (plus the k
// selected values); longer lines are re-read from memory by each of the five passes.  Every count is an integer, so the
// result does not depend on the order in which threads meet: bitwise reproducible, and independent of the slab split.
#include "nr_common.h"
#include "../../include/nr_hip.h"

#define NR_TOPK_MAX 128
#define NR_TOPK_CACHE_KEYS 12288   // 48 KB of dynamic LDS per workgroup

// One list per line.  Line l starts at S + l * line_stride, its entry e sits at + e * elem_stride and is reported as
// index idx0 + e.  Rows of a slab: (N, 1, 0); columns: (1, N, row0).
template <bool CACHED>
__global__ __launch_bounds__(256) void nr_topk_lines_kernel(const float* __restrict__ S, int L, long long line_stride,
                                                           long long elem_stride, int idx0, int k,
                                                           int32_t* __restrict__ idx_out, float* __restrict__ val_out) {
    extern __shared__ uint32_t cache[];
    __shared__ int hist[256];
    __shared__ uint32_t sel_key[NR_TOPK_MAX];
    __shared__ int sel_pos[NR_TOPK_MAX];
    __shared__ int wave_cnt[4];
    __shared__ int s_digit, s_above, n_gt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* line = S + (long long)blockIdx.x * line_stride;
    const int kk = min(k, L);

    // radix select of the kk-th largest key: prefix = its leading digits so far, rem = its rank among the keys sharing them
    uint32_t prefix = 0, pmask = 0;
    int rem = kk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int e = tid; e < L; e += 256) {
            uint32_t key;
            if (CACHED) {
                if (shift == 24) {
                    key = nr_order_key(line[(long long)e * elem_stride]);
                    cache[e] = key;
                } else {
                    key = cache[e];
                }
            } else {
                key = nr_order_key(line[(long long)e * elem_stride]);
            }
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1);
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
            int a = suf - s;                     // entries in the bins of the lanes above
            if (a < rem && rem <= a + c3) { s_digit = 4 * lane + 3; s_above = a; }
            a += c3;
            if (a < rem && rem <= a + c2) { s_digit = 4 * lane + 2; s_above = a; }
            a += c2;
            if (a < rem && rem <= a + c1) { s_digit = 4 * lane + 1; s_above = a; }
            a += c1;
            if (a < rem && rem <= a + c0) { s_digit = 4 * lane; s_above = a; }
        }
        __syncthreads();
        prefix |= (uint32_t)s_digit << shift;
        pmask |= 255u << shift;
        rem -= s_above;
    }
    const uint32_t T = prefix;                   // the kk-th largest key
    const int n_above = kk - rem;                // entries with a key above T: all selected
    const bool take_ties = T != 0u;              // T = 0: the line has fewer than kk non-NaN entries
    const int n_sel = take_ties ? kk : n_above;

    // compaction in index order: keys above T in any order (ordered below), ties at T lowest index first
    if (tid == 0) n_gt = 0;
    __syncthreads();
    int tie_base = 0;
    for (int base = 0; base < L; base += 256) {
        const int e = base + tid;
        const bool in = e < L;
        uint32_t key = 0;
        if (in) key = CACHED ? cache[e] : nr_order_key(line[(long long)e * elem_stride]);
        if (in && key > T) {
            const int p = atomicAdd(&n_gt, 1);
            if (p < NR_TOPK_MAX) { sel_key[p] = key; sel_pos[p] = e; }
        }
        const bool tie = in && take_ties && key == T;
        const unsigned long long m = __ballot(tie);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = tie_base;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        tie_base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (tie) {
            const int t = off + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (t < rem && n_above + t < NR_TOPK_MAX) { sel_key[n_above + t] = key; sel_pos[n_above + t] = e; }
        }
        __syncthreads();
    }

    // position of every kept entry = the number of kept entries ahead of it (positions are distinct: indices are)
    int32_t* io = idx_out + (long long)blockIdx.x * k;
    float* vo = val_out + (long long)blockIdx.x * k;
    if (tid < n_sel) {
        const uint32_t key = sel_key[tid];
        const int pos = sel_pos[tid];
        int rank = 0;
        for (int j = 0; j < n_sel; ++j) {
            const uint32_t kj = sel_key[j];
            rank += (kj > key) || (kj == key && sel_pos[j] < pos);
        }
        io[rank] = idx0 + pos;
        vo[rank] = line[(long long)pos * elem_stride];
    } else if (tid < k) {
        io[tid] = -1;
        vo[tid] = -INFINITY;
    }
}

static int nr_topk_lines(const float* S, int n_lines, int L, long long line_stride, long long elem_stride, int idx0, int k,
                         int32_t* idx_out, float* val_out, void* stream) {
    if (L <= NR_TOPK_CACHE_KEYS) {
        hipLaunchKernelGGL(nr_topk_lines_kernel<true>, dim3(n_lines), dim3(256), (size_t)L * sizeof(uint32_t),
                           (hipStream_t)stream, S, L, line_stride, elem_stride, idx0, k, idx_out, val_out);
    } else {
        hipLaunchKernelGGL(nr_topk_lines_kernel<false>, dim3(n_lines), dim3(256), 0, (hipStream_t)stream, S, L, line_stride,
                           elem_stride, idx0, k, idx_out, val_out);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}

extern "C" int nr_slab_topk_rows(const float* S_slab, int n_rows, int N, int k, int32_t* idx_out, float* val_out,
                                 void* stream) {
    if (!S_slab || !idx_out || !val_out) return NR_EINVAL;
    if (k < 1 || k > NR_TOPK_MAX || n_rows <= 0 || N <= 0) return NR_EINVAL;
    return nr_topk_lines(S_slab, n_rows, N, (long long)N, 1, 0, k, idx_out, val_out, stream);
}

extern "C" int nr_slab_topk_cols(const float* S_slab, int n_rows, int N, int row0, int k, int32_t* idx_out, float* val_out,
                                 void* stream) {
    if (!S_slab || !idx_out || !val_out) return NR_EINVAL;
    if (k < 1 || k > NR_TOPK_MAX || n_rows <= 0 || N <= 0 || row0 < 0 || (long long)row0 + n_rows > 0x7fffffffLL)
        return NR_EINVAL;
    return nr_topk_lines(S_slab, N, n_rows, 1, (long long)N, row0, k, idx_out, val_out, stream);
}

// ---- merge of partial lists -----------------------------------------------------------------------------------------
// List w of item i: idx / val [(w * n_items + i) * k, + k), in the order above with its absent entries (index < 0 or a NaN
// value) last -- what the two kernels above write.  One workgroup per item: the final position of an entry is its
// position in its own list plus, for every other list, how many of that list's entries are ahead of it (a binary search:
// each list is ordered).  An index present in several lists with the same key is ordered by list number, so positions
// stay distinct and the result deterministic whatever the input.
__device__ __forceinline__ bool nr_topk_ahead(int32_t i_b, float v_b, int list_b, uint32_t key, int32_t idx, int list) {
    if (i_b < 0 || v_b != v_b) return false;
    const uint32_t kb = nr_order_key(v_b);
    return kb > key || (kb == key && (i_b < idx || (i_b == idx && list_b < list)));
}

__global__ __launch_bounds__(256) void nr_topk_merge_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                           int n_lists, int n_items, int k, int32_t* __restrict__ idx_out,
                                                           float* __restrict__ val_out) {
    __shared__ int n_valid;
    const int item = blockIdx.x;
    if (threadIdx.x == 0) n_valid = 0;
    __syncthreads();
    int32_t* io = idx_out + (long long)item * k;
    float* vo = val_out + (long long)item * k;
    const int total = n_lists * k;
    int mine = 0;
    for (int c = threadIdx.x; c < total; c += 256) {
        const int l = c / k, p = c - l * k;
        const long long at = ((long long)l * n_items + item) * k + p;
        const int32_t i = idx[at];
        const float v = val[at];
        if (i < 0 || v != v) continue;
        const uint32_t key = nr_order_key(v);
        int rank = p;
        for (int b = 0; b < n_lists && rank < k; ++b) {
            if (b == l) continue;
            const long long base = ((long long)b * n_items + item) * k;
            int lo = 0, hi = k;                  // first entry of list b not ahead of (key, i, l)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (nr_topk_ahead(idx[base + mid], val[base + mid], b, key, i, l)) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            io[rank] = i;
            vo[rank] = v;
        }
        ++mine;
    }
    if (mine) atomicAdd(&n_valid, mine);
    __syncthreads();
    for (int t = n_valid + threadIdx.x; t < k; t += 256) {
        io[t] = -1;
        vo[t] = -INFINITY;
    }
}

extern "C" int nr_topk_merge(int n_lists, const int32_t* idx, const float* val, int n_items, int k, int32_t* idx_out,
                             float* val_out, void* stream) {
    if (!idx || !val || !idx_out || !val_out) return NR_EINVAL;
    if (k < 1 || k > NR_TOPK_MAX || n_lists <= 0 || n_items <= 0 || (long long)n_lists * k > 0x7fffffffLL) return NR_EINVAL;
    hipLaunchKernelGGL(nr_topk_merge_kernel, dim3(n_items), dim3(256), 0, (hipStream_t)stream, idx, val, n_lists, n_items, k,
                       idx_out, val_out);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- k-occurrence counts ----------------------------------------------------------------------------------------------
// occ[j] = #{queries whose list holds j}, good[j] = the subset whose ground-truth range [gt_begin[q], gt_end[q]) holds j.
// One thread per list slot, integer atomics (sums of integers do not depend on their order); absent slots (index < 0)
// and indices outside [0, n_gallery) are not counted.
__global__ __launch_bounds__(256) void nr_topk_occurrences_kernel(const int32_t* __restrict__ idx, long long n_slots, int k,
                                                                 int n_gallery, const int32_t* __restrict__ gt_begin,
                                                                 const int32_t* __restrict__ gt_end,
                                                                 int32_t* __restrict__ occ, int32_t* __restrict__ good) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_slots) return;
    const int j = idx[t];
    if (j < 0 || j >= n_gallery) return;
    const long long q = t / k;
    atomicAdd(&occ[j], 1);
    if (j >= gt_begin[q] && j < gt_end[q]) atomicAdd(&good[j], 1);
}

extern "C" int nr_topk_occurrences(const int32_t* idx, int n_q, int k, int n_gallery, const int32_t* gt_begin,
                                   const int32_t* gt_end, int32_t* occ, int32_t* good, void* stream) {
    if (!occ || !good || (n_q > 0 && (!idx || !gt_begin || !gt_end))) return NR_EINVAL;
    if (k < 1 || k > NR_TOPK_MAX || n_q < 0 || n_gallery <= 0) return NR_EINVAL;
    hipError_t e = hipMemsetAsync(occ, 0, (size_t)n_gallery * sizeof(int32_t), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(good, 0, (size_t)n_gallery * sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const long long n_slots = (long long)n_q * k;
    if (n_slots == 0) return NR_OK;
    const long long blocks = (n_slots + 255) / 256;
    if (blocks > 0x7fffffffLL) return NR_EINVAL;
    hipLaunchKernelGGL(nr_topk_occurrences_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, idx, n_slots, k,
                       n_gallery, gt_begin, gt_end, occ, good);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
