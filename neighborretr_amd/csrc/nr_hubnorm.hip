// Test-time hubness reduction over similarity slabs: IS, DSL and QB-Norm (DESIGN.md "Test-time hubness reduction").
//
// All four kernels are single passes over fp32 slabs and bound by memory bandwidth.
//   - log-sum-exp statistics: every line of beta * S is reduced to a (max, sum) pair, sum = sum of exp(beta x - max) over its
//     non-NaN entries, entries equal to the max adding exactly 1 (so +inf and all -inf lines are defined); lse = max +
//     log(sum), -inf for a line with no entry.  Rows: one wave per row.  Columns: row blocks write partial pairs to a
//     caller-provided workspace and a second launch combines them in block order.  Every reduction runs in a fixed order
//     (lanes, then a fixed butterfly; blocks, then index order): no float atomics, no hand-off between workgroups, bitwise
//     reproducible run to run.
//   - apply: T (column normaliser, per-row gate) and V (row normaliser, per-column gate) from one read of S.
#include "nr_hubnorm.h"
#include "../../include/nr_hip.h"

// ---- row statistics: one wave per row ------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void nr_hubnorm_row_lse_kernel(const float* __restrict__ S, int n, int L, float beta,
                                                                float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                        // whole waves leave together: the shuffles below stay full-wave
    const float* line = S + (long long)row * L;
    float m = -INFINITY, s = 0.f;
    if (VEC) {
        const f32x4_t* l4 = reinterpret_cast<const f32x4_t*>(line);
        for (int c = lane; c < (L >> 2); c += 64) {
            const f32x4_t x = l4[c];
            nr_hn_add(m, s, beta, x[0]);
            nr_hn_add(m, s, beta, x[1]);
            nr_hn_add(m, s, beta, x[2]);
            nr_hn_add(m, s, beta, x[3]);
        }
    } else {
        for (int e = lane; e < L; e += 64) nr_hn_add(m, s, beta, line[e]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        nr_hn_merge(m, s, m2, s2);
    }
    if (lane == 0) lse[row] = nr_hn_lse(m, s);
}

extern "C" int nr_hubnorm_row_lse(const float* S, int n, int L, float beta, float* lse, void* stream) {
    if (!S || !lse) return NR_EINVAL;
    if (n < 0 || L < 0 || !(beta > 0.f) || !(beta < INFINITY)) return NR_EINVAL;
    if (n == 0) return NR_OK;
    const bool vec = (L % 4 == 0) && ((uintptr_t)S % 16 == 0);
    const dim3 grid((n + 3) / 4);
    if (vec) {
        hipLaunchKernelGGL(nr_hubnorm_row_lse_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, S, n, L, beta, lse);
    } else {
        hipLaunchKernelGGL(nr_hubnorm_row_lse_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, S, n, L, beta, lse);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- column statistics: partial pairs per block of NR_HN_ROWS rows, then a combine in block order ---------------------------
// Partial p of column c: part[(2p) L + c] = max, part[(2p + 1) L + c] = sum.  Each thread walks its VEC columns down the
// block's rows in row order, so a column's partial does not depend on VEC.
template <int VEC>
__global__ __launch_bounds__(256) void nr_hubnorm_col_part_kernel(const float* __restrict__ S, int n, int L, float beta,
                                                                 float* __restrict__ part) {
    const long long c0 = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (c0 >= L) return;
    const int p = blockIdx.y;
    const int r0 = p * NR_HN_ROWS, r1 = min(n, r0 + NR_HN_ROWS);
    float m[VEC], s[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { m[v] = -INFINITY; s[v] = 0.f; }
    for (int r = r0; r < r1; ++r) {
        const float* at = S + (long long)r * L + c0;
        if (VEC == 4) {
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(at);
#pragma unroll
            for (int v = 0; v < VEC; ++v) nr_hn_add(m[v], s[v], beta, x[v]);
        } else {
            nr_hn_add(m[0], s[0], beta, at[0]);
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

// P pairs per item, parts [P, 2, L], merged in index order p = 0, 1, ...  -> stats [2, L] (max, sum) and / or lse [L].
__global__ __launch_bounds__(256) void nr_hubnorm_combine_kernel(int P, const float* __restrict__ parts, int L,
                                                                float* __restrict__ stats, float* __restrict__ lse) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= L) return;
    float m = -INFINITY, s = 0.f;
    for (int p = 0; p < P; ++p) nr_hn_merge(m, s, parts[(long long)(2 * p) * L + c], parts[(long long)(2 * p + 1) * L + c]);
    if (stats) {
        stats[c] = m;
        stats[L + c] = s;
    }
    if (lse) lse[c] = nr_hn_lse(m, s);
}

static int nr_hubnorm_combine_launch(int P, const float* parts, int L, float* stats, float* lse, void* stream) {
    hipLaunchKernelGGL(nr_hubnorm_combine_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P,
                       parts, L, stats, lse);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

extern "C" size_t nr_hubnorm_col_workspace(int n, int L) {
    if (n <= 0 || L <= 0) return 0;
    return (size_t)((n + NR_HN_ROWS - 1) / NR_HN_ROWS) * 2 * (size_t)L * sizeof(float);
}

extern "C" int nr_hubnorm_col_stats(const float* S, int n, int L, float beta, void* workspace, float* stats, void* stream) {
    if (!stats || (n > 0 && (!S || !workspace))) return NR_EINVAL;
    if (n < 0 || L < 0 || !(beta > 0.f) || !(beta < INFINITY)) return NR_EINVAL;
    if (L == 0) return NR_OK;
    const int P = (n + NR_HN_ROWS - 1) / NR_HN_ROWS;
    float* part = static_cast<float*>(workspace);
    if (P > 0) {
        const bool vec = (L % 4 == 0) && ((uintptr_t)S % 16 == 0) && ((uintptr_t)part % 16 == 0);
        if (vec) {
            const dim3 grid((unsigned)((L / 4 + 255) / 256), (unsigned)P);
            hipLaunchKernelGGL(nr_hubnorm_col_part_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, S, n, L, beta, part);
        } else {
            const dim3 grid((unsigned)((L + 255) / 256), (unsigned)P);
            hipLaunchKernelGGL(nr_hubnorm_col_part_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, S, n, L, beta, part);
        }
        NR_LAUNCH_CHECK();
    }
    return nr_hubnorm_combine_launch(P, part, L, stats, nullptr, stream);     // P = 0: every column (-inf, 0)
}

extern "C" int nr_hubnorm_combine(int P, const float* parts, int L, float* stats, float* lse, void* stream) {
    if ((!stats && !lse) || (P > 0 && !parts)) return NR_EINVAL;
    if (P < 0 || L < 0) return NR_EINVAL;
    if (L == 0) return NR_OK;
    return nr_hubnorm_combine_launch(P, parts, L, stats, lse, stream);
}

// ---- apply ------------------------------------------------------------------------------------------------------------------
// is:  fl(fl(beta s) - c), no fused multiply-add (NumPy float32 gives the same bits).
// dsl: s * exp(beta s - c).  The exponent is carried to about one rounding: b = fl(beta s) with its exact residual (fma), and
// d = fl(b - c) with its exact residual (two-sum); exp(d) * (1 + residuals).  Non-finite cases keep the plain form.
__device__ __forceinline__ float nr_hn_is(float b, float c) { return __fsub_rn(b, c); }

__device__ __forceinline__ float nr_hn_dsl(float s, float beta, float b, float c) {
    const float lo = fmaf(beta, s, -b);
    const float d = __fsub_rn(b, c);
    const float z = __fsub_rn(d, b);
    const float e = __fadd_rn(__fsub_rn(b, __fsub_rn(d, z)), __fsub_rn(-c, z));
    float t = __fadd_rn(e, lo);
    if (!(fabsf(t) < 1e-3f)) t = 0.f;            // inf / NaN operands: no correction
    const float x = __fmul_rn(s, expf(d));
    return fmaf(x, t, x);
}

template <int MODE>
__device__ __forceinline__ float nr_hn_norm(float s, float beta, float b, float c) {
    return MODE == NR_HUBNORM_IS ? nr_hn_is(b, c) : nr_hn_dsl(s, beta, b, c);
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void nr_hubnorm_apply_kernel(const float* __restrict__ S, int n, int L, float beta,
                                                              const float* __restrict__ col_norm,
                                                              const int32_t* __restrict__ row_gate, float* __restrict__ T,
                                                              const float* __restrict__ row_norm,
                                                              const int32_t* __restrict__ col_gate, float* __restrict__ V) {
    const long long n_groups = (long long)n * L / VEC;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (long long)gridDim.x * 256) {
        const long long e0 = g * VEC;
        const int i = (int)(e0 / L);
        const int j0 = (int)(e0 - (long long)i * L);         // VEC == 4: L % 4 == 0, the group lies in one row
        float s[VEC];
        if (VEC == 4) {
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(S + e0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) s[v] = x[v];
        } else {
            s[0] = S[e0];
        }
        float b[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) b[v] = __fmul_rn(beta, s[v]);
        if (T) {
            const bool on = !row_gate || row_gate[i] != 0;
            float t[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) t[v] = on ? nr_hn_norm<MODE>(s[v], beta, b[v], col_norm[j0 + v]) : s[v];
            if (VEC == 4) *reinterpret_cast<f32x4_t*>(T + e0) = f32x4_t{t[0], t[1], t[2], t[3]};
            else T[e0] = t[0];
        }
        if (V) {
            const float c = row_norm[i];
            float w[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const bool on = !col_gate || col_gate[j0 + v] != 0;
                w[v] = on ? nr_hn_norm<MODE>(s[v], beta, b[v], c) : s[v];
            }
            if (VEC == 4) *reinterpret_cast<f32x4_t*>(V + e0) = f32x4_t{w[0], w[1], w[2], w[3]};
            else V[e0] = w[0];
        }
    }
}

template <int MODE>
static void nr_hubnorm_apply_launch(bool vec, const float* S, int n, int L, float beta, const float* col_norm,
                                    const int32_t* row_gate, float* T, const float* row_norm, const int32_t* col_gate, float* V,
                                    hipStream_t stream) {
    const long long groups = (long long)n * L / (vec ? 4 : 1);
    const unsigned blocks = (unsigned)std::min<long long>((groups + 255) / 256, 16384);
    if (vec) {
        hipLaunchKernelGGL((nr_hubnorm_apply_kernel<MODE, 4>), dim3(blocks), dim3(256), 0, stream, S, n, L, beta, col_norm,
                           row_gate, T, row_norm, col_gate, V);
    } else {
        hipLaunchKernelGGL((nr_hubnorm_apply_kernel<MODE, 1>), dim3(blocks), dim3(256), 0, stream, S, n, L, beta, col_norm,
                           row_gate, T, row_norm, col_gate, V);
    }
}

extern "C" int nr_hubnorm_apply(const float* S, int n, int L, float beta, int mode, const float* col_norm,
                                const int32_t* row_gate, float* T, const float* row_norm, const int32_t* col_gate, float* V,
                                void* stream) {
    if (!S || (!T && !V) || (T && !col_norm) || (V && !row_norm)) return NR_EINVAL;
    if (n < 0 || L < 0 || !(beta > 0.f) || !(beta < INFINITY)) return NR_EINVAL;
    if (mode != NR_HUBNORM_IS && mode != NR_HUBNORM_DSL) return NR_EINVAL;
    if (n == 0 || L == 0) return NR_OK;
    const bool vec = (L % 4 == 0) && ((uintptr_t)S % 16 == 0) && (!T || (uintptr_t)T % 16 == 0) &&
                     (!V || (uintptr_t)V % 16 == 0);
    if (mode == NR_HUBNORM_IS) {
        nr_hubnorm_apply_launch<NR_HUBNORM_IS>(vec, S, n, L, beta, col_norm, row_gate, T, row_norm, col_gate, V,
                                               (hipStream_t)stream);
    } else {
        nr_hubnorm_apply_launch<NR_HUBNORM_DSL>(vec, S, n, L, beta, col_norm, row_gate, T, row_norm, col_gate, V,
                                                (hipStream_t)stream);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}
