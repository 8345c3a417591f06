// Test-time Sinkhorn normalisation of a similarity slab (DESIGN.md "Test-time Sinkhorn normalisation"): the log-domain
// iteration of the reference's uniform regularisation (until_module.py:223-266) applied to the test similarity.
//
//   a[i,j] = fl(beta S[i,j]);   u[i] = log_mu[i] - LSE_j(a[i,j] + v[j]);   v[j] = log_nu[j] - LSE_i(a[i,j] + u[i])
//   T[i,j] = fl(fl(a[i,j] + u[i]) + v[j])
//
// One iteration is plain launches on the caller's stream: the row half-step (one wave per row, writes u), the column
// partials (blocks of 64 rows write (max, sum) pairs to the caller's workspace) and the column finish (pairs merged in index
// order, writes v).  The (max, sum) pairs are those of nr_hubnorm.hip: NaN entries are skipped, an entry equal to the max adds
// exactly 1, every reduction runs in a fixed order (lanes, a fixed butterfly; blocks in index order).  No float atomics, no
// hand-off between workgroups: bitwise reproducible run to run.  A line whose LSE is not finite keeps potential 0.
#include "nr_hubnorm.h"
#include "../../include/nr_hip.h"

// one more entry of a line: x = fl(beta s), shifted by the other side's potential(s)
__device__ __forceinline__ void nr_sn_add(float& m, float& s, float beta, float x, float p) {
    if (x != x) return;                          // NaN: carries no mass
    nr_hn_merge(m, s, __fadd_rn(__fmul_rn(beta, x), p), 1.f);
}
__device__ __forceinline__ void nr_sn_add2(float& m, float& s, float beta, float x, float u, float v) {
    if (x != x) return;
    nr_hn_merge(m, s, __fadd_rn(__fadd_rn(__fmul_rn(beta, x), u), v), 1.f);
}

__device__ __forceinline__ bool nr_sn_finite(float x) { return fabsf(x) < INFINITY; }      // false for NaN too

// ---- row half-step: one wave per row ------------------------------------------------------------------------------------------
// ERR = false: out[i] = u[i] = log_mu[i] - LSE_j(a[i,j] + v[j]), 0 when the LSE is not finite.
// ERR = true:  out[i] = |exp(LSE_j(fl(fl(a[i,j] + u[i]) + v[j]) - log_mu[i]) - 1|, the row's distance from its marginal, 0 for
//              a row that takes no part.
template <bool VEC, bool ERR>
__global__ __launch_bounds__(256) void nr_sinknorm_row_kernel(const float* __restrict__ S, int n, int L, float beta,
                                                             const float* __restrict__ u, const float* __restrict__ v,
                                                             const float* __restrict__ log_mu, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                        // whole waves leave together: the shuffles below stay full-wave
    const float* line = S + (long long)row * L;
    const float ui = ERR ? u[row] : 0.f;
    float m = -INFINITY, s = 0.f;
    if (VEC) {
        const f32x4_t* l4 = reinterpret_cast<const f32x4_t*>(line);
        const f32x4_t* v4 = reinterpret_cast<const f32x4_t*>(v);
        for (int c = lane; c < (L >> 2); c += 64) {
            const f32x4_t x = l4[c];
            const f32x4_t p = v4[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (ERR) nr_sn_add2(m, s, beta, x[k], ui, p[k]);
                else nr_sn_add(m, s, beta, x[k], p[k]);
            }
        }
    } else {
        for (int e = lane; e < L; e += 64) {
            if (ERR) nr_sn_add2(m, s, beta, line[e], ui, v[e]);
            else nr_sn_add(m, s, beta, line[e], v[e]);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        nr_hn_merge(m, s, m2, s2);
    }
    if (lane == 0) {
        const float lse = nr_hn_lse(m, s);
        if (ERR) out[row] = nr_sn_finite(lse) ? fabsf(expf(lse - log_mu[row]) - 1.f) : 0.f;
        else out[row] = nr_sn_finite(lse) ? log_mu[row] - lse : 0.f;
    }
}

template <bool ERR>
static int nr_sinknorm_row_launch(const float* S, int n, int L, float beta, const float* u, const float* v, const float* log_mu,
                                  float* out, void* stream) {
    const bool vec = (L % 4 == 0) && ((uintptr_t)S % 16 == 0) && ((uintptr_t)v % 16 == 0);
    const dim3 grid((n + 3) / 4);
    if (vec) {
        hipLaunchKernelGGL((nr_sinknorm_row_kernel<true, ERR>), grid, dim3(256), 0, (hipStream_t)stream, S, n, L, beta, u, v,
                           log_mu, out);
    } else {
        hipLaunchKernelGGL((nr_sinknorm_row_kernel<false, ERR>), grid, dim3(256), 0, (hipStream_t)stream, S, n, L, beta, u, v,
                           log_mu, out);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}

static bool nr_sn_bad(int n, int L, float beta) { return n < 0 || L < 0 || !(beta > 0.f) || !(beta < INFINITY); }

extern "C" int nr_sinknorm_row(const float* S, int n, int L, float beta, const float* v, const float* log_mu, float* u,
                               void* stream) {
    if (!S || !v || !log_mu || !u) return NR_EINVAL;
    if (nr_sn_bad(n, L, beta)) return NR_EINVAL;
    if (n == 0) return NR_OK;
    return nr_sinknorm_row_launch<false>(S, n, L, beta, nullptr, v, log_mu, u, stream);
}

extern "C" int nr_sinknorm_row_err(const float* S, int n, int L, float beta, const float* u, const float* v, const float* log_mu,
                                   float* err, void* stream) {
    if (!S || !u || !v || !log_mu || !err) return NR_EINVAL;
    if (nr_sn_bad(n, L, beta)) return NR_EINVAL;
    if (n == 0) return NR_OK;
    return nr_sinknorm_row_launch<true>(S, n, L, beta, u, v, log_mu, err, stream);
}

// ---- column half-step: partial pairs per block of NR_HN_ROWS rows ---------------------------------------------------------------
// Partial p of column c: part[(2p) L + c] = max, part[(2p + 1) L + c] = sum of fl(a[r,c] + u[r]) over the block's rows in row
// order (u[r] is uniform per row: a scalar load), so a column's partial does not depend on VEC.
template <int VEC>
__global__ __launch_bounds__(256) void nr_sinknorm_col_part_kernel(const float* __restrict__ S, int n, int L, float beta,
                                                                  const float* __restrict__ u, float* __restrict__ part) {
    const long long c0 = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (c0 >= L) return;
    const int p = blockIdx.y;
    const int r0 = p * NR_HN_ROWS, r1 = min(n, r0 + NR_HN_ROWS);
    float m[VEC], s[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { m[k] = -INFINITY; s[k] = 0.f; }
    for (int r = r0; r < r1; ++r) {
        const float* at = S + (long long)r * L + c0;
        const float ur = u[r];
        if (VEC == 4) {
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(at);
#pragma unroll
            for (int k = 0; k < VEC; ++k) nr_sn_add(m[k], s[k], beta, x[k], ur);
        } else {
            nr_sn_add(m[0], s[0], beta, at[0], ur);
        }
    }
    float* pm = part + (long long)(2 * p) * L + c0;
    float* ps = pm + L;
    if (VEC == 4) {
        *reinterpret_cast<f32x4_t*>(pm) = f32x4_t{m[0], m[1], m[2], m[3]};
        *reinterpret_cast<f32x4_t*>(ps) = f32x4_t{s[0], s[1], s[2], s[3]};
    } else {
        pm[0] = m[0];
        ps[0] = s[0];
    }
}

extern "C" int nr_sinknorm_col_stats(const float* S, int n, int L, float beta, const float* u, void* workspace, float* stats,
                                     void* stream) {
    if (n > 0 && (!S || !u || !workspace)) return NR_EINVAL;
    if (n == 0 && !stats) return NR_EINVAL;      // nothing to write at all
    if (nr_sn_bad(n, L, beta)) return NR_EINVAL;
    if (L == 0) return NR_OK;
    const int P = (n + NR_HN_ROWS - 1) / NR_HN_ROWS;
    float* part = static_cast<float*>(workspace);
    if (P > 0) {
        const bool vec = (L % 4 == 0) && ((uintptr_t)S % 16 == 0) && ((uintptr_t)part % 16 == 0);
        if (vec) {
            const dim3 grid((unsigned)((L / 4 + 255) / 256), (unsigned)P);
            hipLaunchKernelGGL(nr_sinknorm_col_part_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, S, n, L, beta, u, part);
        } else {
            const dim3 grid((unsigned)((L + 255) / 256), (unsigned)P);
            hipLaunchKernelGGL(nr_sinknorm_col_part_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, S, n, L, beta, u, part);
        }
        NR_LAUNCH_CHECK();
    }
    if (!stats) return NR_OK;                    // the caller finishes from the workspace's P pairs
    return nr_hubnorm_combine(P, part, L, stats, nullptr, stream);           // P = 0: every column (-inf, 0)
}

// P pairs per column, parts [P, 2, L], merged in index order -> v[j] = log_nu[j] - lse, 0 when the lse is not finite.
__global__ __launch_bounds__(256) void nr_sinknorm_finish_cols_kernel(int P, const float* __restrict__ parts, int L,
                                                                     const float* __restrict__ log_nu, float* __restrict__ v) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= L) return;
    float m = -INFINITY, s = 0.f;
    for (int p = 0; p < P; ++p) nr_hn_merge(m, s, parts[(long long)(2 * p) * L + c], parts[(long long)(2 * p + 1) * L + c]);
    const float lse = nr_hn_lse(m, s);
    v[c] = nr_sn_finite(lse) ? log_nu[c] - lse : 0.f;
}

extern "C" int nr_sinknorm_finish_cols(int P, const float* parts, int L, const float* log_nu, float* v, void* stream) {
    if (!log_nu || !v || (P > 0 && !parts)) return NR_EINVAL;
    if (P < 0 || L < 0) return NR_EINVAL;
    if (L == 0) return NR_OK;
    hipLaunchKernelGGL(nr_sinknorm_finish_cols_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P,
                       parts, L, log_nu, v);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- apply: one read of S, one write of T -----------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void nr_sinknorm_apply_kernel(const float* __restrict__ S, int n, int L, float beta,
                                                               const float* __restrict__ u, const float* __restrict__ v,
                                                               float* __restrict__ T) {
    const long long n_groups = (long long)n * L / VEC;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (long long)gridDim.x * 256) {
        const long long e0 = g * VEC;
        const int i = (int)(e0 / L);
        const int j0 = (int)(e0 - (long long)i * L);         // VEC == 4: L % 4 == 0, the group lies in one row
        const float ui = u[i];
        if (VEC == 4) {
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(S + e0);
            f32x4_t t;
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = __fadd_rn(__fadd_rn(__fmul_rn(beta, x[k]), ui), v[j0 + k]);
            *reinterpret_cast<f32x4_t*>(T + e0) = t;
        } else {
            T[e0] = __fadd_rn(__fadd_rn(__fmul_rn(beta, S[e0]), ui), v[j0]);
        }
    }
}

extern "C" int nr_sinknorm_apply(const float* S, int n, int L, float beta, const float* u, const float* v, float* T,
                                 void* stream) {
    if (!S || !u || !v || !T) return NR_EINVAL;
    if (nr_sn_bad(n, L, beta)) return NR_EINVAL;
    if (n == 0 || L == 0) return NR_OK;
    const bool vec = (L % 4 == 0) && ((uintptr_t)S % 16 == 0) && ((uintptr_t)T % 16 == 0);
    const long long groups = (long long)n * L / (vec ? 4 : 1);
    const unsigned blocks = (unsigned)std::min<long long>((groups + 255) / 256, 16384);
    if (vec) {
        hipLaunchKernelGGL(nr_sinknorm_apply_kernel<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, S, n, L, beta, u, v, T);
    } else {
        hipLaunchKernelGGL(nr_sinknorm_apply_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, S, n, L, beta, u, v, T);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}
