// Mutual proximity of a similarity slab (DESIGN.md "Mutual proximity"): every score is replaced by the probability that it beats
// the scores of its row's reference line and of its column's reference line, in the independent form MP_I = P_row P_col.
//
//   emp:   r2(s, X) = 2 #{x in X : x < s} + #{x in X : x == s},  c(X) = #{x in X : x is not NaN}
//          T[i,j] = fl(fl(fl(r2_row) / fl(2 c_row)) fl(fl(r2_col) / fl(2 c_col)))
//   gauss: z = fl(fl(s - mean) / max(sd, EPS)),  Q = fl(0.5 erfc(fl(z fl(1 / sqrt 2)))),  T[i,j] = -fl(fl(Q_r + Q_c) - fl(Q_r Q_c))
//          EPS = NR_SCALE_EPS = 2^-20, the max is nr_floor (nr_common.h): it keeps a NaN sd
//
// The counts are integers (no order of summation), every float operation is rounded once (no fused multiply-add), the moments are
// accumulated in fp64 in a fixed order.  No scratch, no float atomics, no hand-off between workgroups.
#include "nr_slab.h"
#include "nr_mutualprox.h"
#include "../../include/nr_hip.h"

#define NR_MP_TILE 16                            // scores a lane keeps in registers while the reference values stream past
#define NR_MP_ROW_CHUNK 1024                     // floats of a reference row staged through LDS at a time
#define NR_MP_COL_BLOCK_ROWS 64                  // rows of S a workgroup of the column kernel covers: 4 waves x NR_MP_TILE

// ---- row counts: one wave per (row, 1024 columns); the reference row goes through LDS and is read as a broadcast ----------------
__global__ __launch_bounds__(64) void nr_mp_row_counts_kernel(const float* __restrict__ S, const float* __restrict__ R, int L, int Lr,
                                                              int32_t* __restrict__ r2) {
    __shared__ __attribute__((aligned(16))) float ref[NR_MP_ROW_CHUNK];
    const int lane = threadIdx.x;
    const size_t row = blockIdx.y;
    const int j0 = blockIdx.x * (64 * NR_MP_TILE) + lane;        // this lane's columns: j0 + 64 q
    const float none = __builtin_nanf("");
    float s[NR_MP_TILE];
    int cnt[NR_MP_TILE];
#pragma unroll
    for (int q = 0; q < NR_MP_TILE; ++q) {
        const int j = j0 + 64 * q;
        s[q] = j < L ? S[row * L + j] : none;
        cnt[q] = 0;
    }
    const float* line = R + row * Lr;
    for (int c0 = 0; c0 < Lr; c0 += NR_MP_ROW_CHUNK) {
        const int len = min(NR_MP_ROW_CHUNK, Lr - c0);
        const int len4 = (len + 3) & ~3;                         // the tail of the last group of four: NaN, which counts nothing
        __syncthreads();
        for (int e = lane; e < len4; e += 64) ref[e] = e < len ? line[c0 + e] : none;
        __syncthreads();
        for (int e = 0; e < len4; e += 4) {
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(ref + e);      // every lane the same address: a broadcast
#pragma unroll
            for (int q = 0; q < NR_MP_TILE; ++q)
                cnt[q] += nr_mp_pair(x[0], s[q]) + nr_mp_pair(x[1], s[q]) + nr_mp_pair(x[2], s[q]) + nr_mp_pair(x[3], s[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < NR_MP_TILE; ++q) {
        const int j = j0 + 64 * q;
        if (j < L) r2[row * L + j] = cnt[q];
    }
}

extern "C" int nr_mp_row_counts(const float* S, int n, int L, const float* R, int Lr, int32_t* r2, void* stream) {
    if (!S || !R || !r2) return NR_EINVAL;
    if (n < 0 || L < 0 || Lr < 0 || Lr >= NR_MP_LINE_MAX) return NR_EINVAL;
    if (n == 0 || L == 0) return NR_OK;
    const int tiles = (L + 64 * NR_MP_TILE - 1) / (64 * NR_MP_TILE);
    for (int i0 = 0; i0 < n; i0 += 65535) {                      // the grid's y extent
        const int rows = std::min(65535, n - i0);
        hipLaunchKernelGGL(nr_mp_row_counts_kernel, dim3((unsigned)tiles, (unsigned)rows), dim3(64), 0, (hipStream_t)stream,
                           S + (size_t)i0 * L, R + (size_t)i0 * Lr, L, Lr, r2 + (size_t)i0 * L);
        NR_LAUNCH_CHECK();
    }
    return NR_OK;
}

// ---- column counts: lanes own consecutive columns, a wave owns 16 rows of S; the reference rows are read coalesced --------------
__global__ __launch_bounds__(256) void nr_mp_col_counts_kernel(const float* __restrict__ S, int n, int L, const float* __restrict__ Q,
                                                               int m, int32_t* __restrict__ c2, int accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int i0 = blockIdx.y * NR_MP_COL_BLOCK_ROWS + wave * NR_MP_TILE;
    if (i0 >= n) return;                                         // wave-uniform; the kernel has no barrier
    const bool live = j < L;
    const int jc = live ? j : L - 1;                             // a lane past the last column reads the last one and stores nothing
    const float none = __builtin_nanf("");
    float s[NR_MP_TILE];
    int cnt[NR_MP_TILE];
#pragma unroll
    for (int q = 0; q < NR_MP_TILE; ++q) {
        s[q] = i0 + q < n ? S[(size_t)(i0 + q) * L + jc] : none;
        cnt[q] = 0;
    }
    const float* col = Q + jc;
    int r = 0;
    for (; r + 4 <= m; r += 4) {
        float x[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = col[(size_t)(r + t) * L];
#pragma unroll
        for (int q = 0; q < NR_MP_TILE; ++q)
            cnt[q] += nr_mp_pair(x[0], s[q]) + nr_mp_pair(x[1], s[q]) + nr_mp_pair(x[2], s[q]) + nr_mp_pair(x[3], s[q]);
    }
    for (; r < m; ++r) {
        const float x = col[(size_t)r * L];
#pragma unroll
        for (int q = 0; q < NR_MP_TILE; ++q) cnt[q] += nr_mp_pair(x, s[q]);
    }
    if (!live) return;
#pragma unroll
    for (int q = 0; q < NR_MP_TILE; ++q) {
        if (i0 + q < n) {
            const size_t at = (size_t)(i0 + q) * L + j;
            c2[at] = accumulate ? c2[at] + cnt[q] : cnt[q];
        }
    }
}

extern "C" int nr_mp_col_counts(const float* S, int n, int L, const float* Q, int m, int32_t* c2, int accumulate, void* stream) {
    if (!S || !c2 || (!Q && m > 0)) return NR_EINVAL;
    if (n < 0 || L < 0 || m < 0 || m >= NR_MP_LINE_MAX) return NR_EINVAL;
    if (accumulate != 0 && accumulate != 1) return NR_EINVAL;
    if (n == 0 || L == 0 || (m == 0 && accumulate)) return NR_OK;
    const int per = 65535 * NR_MP_COL_BLOCK_ROWS;
    for (int i0 = 0; i0 < n; i0 += per) {
        const int rows = std::min(per, n - i0);
        hipLaunchKernelGGL(nr_mp_col_counts_kernel, dim3((unsigned)((L + 63) / 64), (unsigned)((rows + NR_MP_COL_BLOCK_ROWS - 1) / NR_MP_COL_BLOCK_ROWS)),
                           dim3(256), 0, (hipStream_t)stream, S + (size_t)i0 * L, rows, L, Q, m, c2 + (size_t)i0 * L, accumulate);
        NR_LAUNCH_CHECK();
    }
    return NR_OK;
}

// ---- non-NaN counts of the lines ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int nr_mp_wave_sum_int(int v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void nr_mp_row_line_counts_kernel(const float* __restrict__ R, int n, int Lr, int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* line = R + (size_t)row * Lr;
    int c = 0;
    for (int e = lane; e < Lr; e += 64) c += (int)(line[e] == line[e]);
    c = nr_mp_wave_sum_int(c);
    if (lane == 0) cnt[row] = c;
}

// 64 columns x 4 groups of rows per workgroup; group g takes rows g, g + 4, ...; integers: the order does not matter
__global__ __launch_bounds__(256) void nr_mp_col_line_counts_kernel(const float* __restrict__ Q, int m, int L, int32_t* __restrict__ cnt) {
    __shared__ int part[4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    int c = 0;
    if (j < L)
        for (int r = g; r < m; r += 4) {
            const float x = Q[(size_t)r * L + j];
            c += (int)(x == x);
        }
    part[g][lane] = c;
    __syncthreads();
    if (g == 0 && j < L) cnt[j] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}

extern "C" int nr_mp_line_counts(const float* R, int n, int Lr, int32_t* row_cnt, const float* Q, int m, int L, int32_t* col_cnt,
                                 void* stream) {
    if (!row_cnt && !col_cnt) return NR_EINVAL;
    if (n < 0 || Lr < 0 || m < 0 || L < 0) return NR_EINVAL;
    if (row_cnt && !R && n > 0 && Lr > 0) return NR_EINVAL;
    if (col_cnt && !Q && m > 0 && L > 0) return NR_EINVAL;
    if (row_cnt && n > 0) {
        hipLaunchKernelGGL(nr_mp_row_line_counts_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, R, n, Lr,
                           row_cnt);
        NR_LAUNCH_CHECK();
    }
    if (col_cnt && L > 0) {
        hipLaunchKernelGGL(nr_mp_col_line_counts_kernel, dim3((unsigned)((L + 63) / 64)), dim3(256), 0, (hipStream_t)stream, Q, m, L,
                           col_cnt);
        NR_LAUNCH_CHECK();
    }
    return NR_OK;
}

// ---- the two applies: one read of every input, one write of T (emp's loop is nr_slab.h's, the formulas nr_mutualprox.h's) ----------
struct nr_mp_emp {
    static constexpr int OUTS = 1;
    const int32_t* r2;
    const int32_t* c2;
    const int32_t* row_cnt;
    const int32_t* col_cnt;
    __device__ float row(int i) const { return (float)(2 * row_cnt[i]); }
    template <int VEC>
    __device__ void values(int, const float (&s)[VEC], float row_den, int j0, long long e0, float (&t)[VEC]) const {
        int32_t a[VEC], b[VEC], c[VEC];
        nr_slab_load<VEC>(r2 + e0, a);
        nr_slab_load<VEC>(c2 + e0, b);
        nr_slab_load<VEC>(col_cnt + j0, c);
#pragma unroll
        for (int q = 0; q < VEC; ++q) t[q] = nr_mp_emp_score(s[q], a[q], row_den, b[q], c[q]);
    }
};

// gauss stays written out: on the skeleton the same operations were scheduled with four more registers and ten more hazard nops,
// 4-5 % slower (the kernel is the one apply that is bound by its arithmetic, two erfc per entry, not by memory).
template <int VEC>
__global__ __launch_bounds__(256) void nr_mp_gauss_apply_kernel(const float* __restrict__ S, int n, int L, const float* __restrict__ row_mean,
                                                                const float* __restrict__ row_sd, const float* __restrict__ col_mean,
                                                                const float* __restrict__ col_sd, float* __restrict__ T) {
    const long long n_groups = (long long)n * L / VEC;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (long long)gridDim.x * 256) {
        const long long e0 = g * VEC;
        const int i = (int)(e0 / L);
        const int j0 = (int)(e0 - (long long)i * L);
        const float rm = row_mean[i], rs = row_sd[i];
        if (VEC == 4) {
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(S + e0);
            const f32x4_t cm = *reinterpret_cast<const f32x4_t*>(col_mean + j0);
            const f32x4_t cs = *reinterpret_cast<const f32x4_t*>(col_sd + j0);
            f32x4_t t;
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] = nr_mp_gauss_score(x[q], rm, rs, cm[q], cs[q]);
            *reinterpret_cast<f32x4_t*>(T + e0) = t;
        } else {
            T[e0] = nr_mp_gauss_score(S[e0], rm, rs, col_mean[j0], col_sd[j0]);
        }
    }
}

extern "C" int nr_mp_emp_apply(const float* S, int n, int L, const int32_t* r2, const int32_t* c2, const int32_t* row_cnt,
                               const int32_t* col_cnt, float* T, void* stream) {
    if (!S || !r2 || !c2 || !row_cnt || !col_cnt || !T) return NR_EINVAL;
    if (n < 0 || L < 0) return NR_EINVAL;
    if (n == 0 || L == 0) return NR_OK;
    return nr_slab_apply<nr_mp_emp>(S, n, L, T, nullptr, {r2, c2, col_cnt}, stream, r2, c2, row_cnt, col_cnt);
}

extern "C" int nr_mp_gauss_apply(const float* S, int n, int L, const float* row_mean, const float* row_sd, const float* col_mean,
                                 const float* col_sd, float* T, void* stream) {
    if (!S || !row_mean || !row_sd || !col_mean || !col_sd || !T) return NR_EINVAL;
    if (n < 0 || L < 0) return NR_EINVAL;
    if (n == 0 || L == 0) return NR_OK;
    const bool vec = nr_slab_vec(L, {S, col_mean, col_sd, T});
    const long long groups = (long long)n * L / (vec ? 4 : 1);
    const dim3 blocks((unsigned)std::min<long long>((groups + 255) / 256, 16384));
    if (vec) {
        hipLaunchKernelGGL(nr_mp_gauss_apply_kernel<4>, blocks, dim3(256), 0, (hipStream_t)stream, S, n, L, row_mean, row_sd, col_mean, col_sd, T);
    } else {
        hipLaunchKernelGGL(nr_mp_gauss_apply_kernel<1>, blocks, dim3(256), 0, (hipStream_t)stream, S, n, L, row_mean, row_sd, col_mean, col_sd, T);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// The fp64 sums below are compiled with contraction off, as they always were: a squared distance is rounded before it is added.
#pragma clang fp contract(off)
// ---- moments for gauss: fp64, two passes (the sum, then the squared distances from the mean), fixed orders --------------------
__device__ __forceinline__ double nr_mp_wave_sum_f64(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);      // a butterfly: every lane ends with the same bits
    return v;
}

// one wave per row: lane l takes the entries l, l + 64, ... in order
__global__ __launch_bounds__(256) void nr_mp_row_moments_kernel(const float* __restrict__ R, int n, int Lr, float* __restrict__ mean,
                                                                float* __restrict__ sd) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* line = R + (size_t)row * Lr;
    double sum = 0.0;
    int c = 0;
    for (int e = lane; e < Lr; e += 64) {
        const float x = line[e];
        if (x == x) { sum += (double)x; ++c; }
    }
    sum = nr_mp_wave_sum_f64(sum);
    c = nr_mp_wave_sum_int(c);
    const double mu = sum / (double)c;                       // c = 0: 0 / 0 = NaN
    double m2 = 0.0;
    for (int e = lane; e < Lr; e += 64) {
        const float x = line[e];
        if (x == x) { const double d = (double)x - mu; m2 += d * d; }
    }
    m2 = nr_mp_wave_sum_f64(m2);
    if (lane == 0) {
        mean[row] = (float)mu;
        sd[row] = (float)sqrt(m2 / (double)c);
    }
}

// Chan's update of (count, mean, M2) by another triple; a triple with count 0 changes nothing.  The mean is taken as the weighted
// mean of the two (not mu + delta cb / tot), so that an infinite mean stays the infinity a plain sum would give.
__device__ __forceinline__ void nr_mp_chan(double& c, double& mu, double& m2, double cb, double mub, double m2b) {
    if (cb == 0.0) return;
    if (c == 0.0) { c = cb; mu = mub; m2 = m2b; return; }
    const double tot = c + cb, delta = mub - mu;
    m2 = (m2 + m2b) + (delta * delta) * (c * cb / tot);
    mu = (c * mu + cb * mub) / tot;
    c = tot;
}

// 64 columns x 4 groups of rows per workgroup: group g takes the g-th quarter of the rows in order; the quarters' sums are added in
// order, every group measures its squared distances from the slab's mean, and those are added in order
__global__ __launch_bounds__(256) void nr_mp_col_moments_kernel(const float* __restrict__ Q, int m, int L, double* __restrict__ parts) {
    __shared__ double sh[4][64];
    __shared__ int shc[4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int per = (m + 3) / 4;
    const int lo = min(g * per, m), hi = min(lo + per, m);
    double sum = 0.0;
    int c = 0;
    if (j < L)
        for (int r = lo; r < hi; ++r) {
            const float x = Q[(size_t)r * L + j];
            if (x == x) { sum += (double)x; ++c; }
        }
    sh[g][lane] = sum;
    shc[g][lane] = c;
    __syncthreads();
    const int tc = shc[0][lane] + shc[1][lane] + shc[2][lane] + shc[3][lane];
    const double mu = (((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane]) / (double)tc;
    __syncthreads();
    double m2 = 0.0;
    if (j < L)
        for (int r = lo; r < hi; ++r) {
            const float x = Q[(size_t)r * L + j];
            if (x == x) { const double d = (double)x - mu; m2 += d * d; }
        }
    sh[g][lane] = m2;
    __syncthreads();
    if (g == 0 && j < L) {
        parts[j] = (double)tc;
        parts[(size_t)L + j] = tc == 0 ? 0.0 : mu;
        parts[2 * (size_t)L + j] = tc == 0 ? 0.0 : ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
    }
}

__global__ __launch_bounds__(256) void nr_mp_moments_combine_kernel(int P, const double* __restrict__ parts, int L, float* __restrict__ mean,
                                                                    float* __restrict__ sd) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L) return;
    double c = 0.0, mu = 0.0, m2 = 0.0;
    for (int p = 0; p < P; ++p) {
        const double* q = parts + (size_t)p * 3 * L;
        nr_mp_chan(c, mu, m2, q[j], q[(size_t)L + j], q[2 * (size_t)L + j]);
    }
    const float none = __builtin_nanf("");
    mean[j] = c == 0.0 ? none : (float)mu;
    sd[j] = c == 0.0 ? none : (float)sqrt(m2 / c);
}

extern "C" int nr_mp_row_moments(const float* R, int n, int Lr, float* mean, float* sd, void* stream) {
    if (!mean || !sd || (!R && n > 0 && Lr > 0)) return NR_EINVAL;
    if (n < 0 || Lr < 0) return NR_EINVAL;
    if (n == 0) return NR_OK;
    hipLaunchKernelGGL(nr_mp_row_moments_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, R, n, Lr, mean, sd);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

extern "C" int nr_mp_col_moments(const float* Q, int m, int L, double* parts, void* stream) {
    if (!parts || (!Q && m > 0 && L > 0)) return NR_EINVAL;
    if (m < 0 || L < 0) return NR_EINVAL;
    if (L == 0) return NR_OK;
    hipLaunchKernelGGL(nr_mp_col_moments_kernel, dim3((unsigned)((L + 63) / 64)), dim3(256), 0, (hipStream_t)stream, Q, m, L, parts);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

extern "C" int nr_mp_moments_combine(int P, const double* parts, int L, float* mean, float* sd, void* stream) {
    if (!mean || !sd || (!parts && P > 0 && L > 0)) return NR_EINVAL;
    if (P < 0 || L < 0) return NR_EINVAL;
    if (L == 0) return NR_OK;
    hipLaunchKernelGGL(nr_mp_moments_combine_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, parts, L, mean,
                       sd);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
