// The four kernel skeletons of the test-time corrections over fp32 slabs S [n, L] (nr_hubnorm.hip, nr_sinknorm.hip,
// nr_localscale.hip, the emp apply of nr_mutualprox.hip).  A family states its formulas in a small struct; the loops, the loads and
// stores, the launch geometry and the choice between the 16-byte and the 4-byte path live here, once.  The struct's members travel
// as kernel parameters of their own, in declaration order (the launchers' trailing arguments), and the kernel puts the struct
// together again: a pointer that is a kernel parameter can be __restrict__, a pointer inside a by-value struct cannot.  They sit
// between the slab's shape and the outputs, where the kernels always had them.  (The struct passed by value in that same place gives
// the same code for the column partials and the hubnorm rows, but not for the merge kernels -- nr_sinknorm_finish_cols 142
// instructions against 136 -- nor for the Sinkhorn row kernels: there the stores and loads through member pointers lose what
// __restrict__ says.  The parameter form is the one that was measured, profiles/slab_kernels_times.txt.)
//
//   apply    out_k[i, j0..] = f.values<VEC>(k, S[i, j0..], f.row(i), j0, i L + j0) for the outputs k < F::OUTS whose pointer is set
//   rows     out[i] = f.finish(pair of row i, i): one wave per row, f.add_line<VEC>(m, s, S[i, j0..], f.row(i), j0) per group
//   columns  part [P, 2, L]: the pair of every column over each block of NR_HN_ROWS rows, f.add(m, s, S[r,c], f.row(r)) per entry
//   merge    f.finish(c, pair): the P pairs of item c merged in index order
//
// The pairs are nr_hubnorm.h's (max, sum).  Every order is fixed (a lane's entries in index order, then one butterfly; a block's
// rows in row order; the partials in index order) and does not depend on the path: the same inputs give the same bits.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "nr_hubnorm.h"

template <class T> struct nr_slab_param { typedef T type; };
template <class T> struct nr_slab_param<T*> { typedef T* __restrict__ type; };

static inline bool nr_slab_aligned(const void* p) { return (uintptr_t)p % 16 == 0; }     // a null pointer is: nothing is read

// The 16-byte path needs rows that are whole groups of four and every pointer it widens on a 16-byte boundary.
static inline bool nr_slab_vec(int L, std::initializer_list<const void*> ptrs) {
    return L % 4 == 0 && std::all_of(ptrs.begin(), ptrs.end(), nr_slab_aligned);
}

// VEC entries (fp32 or int32) from `at`: one 16-byte load when VEC == 4.  The families read their column operands with it too.
template <int VEC, class T>
__device__ __forceinline__ void nr_slab_load(const T* at, T (&x)[VEC]) {
    if (VEC == 4) {
        typedef T __attribute__((ext_vector_type(4))) vec4_t;
        const vec4_t q = *reinterpret_cast<const vec4_t*>(at);
#pragma unroll
        for (int v = 0; v < VEC; ++v) x[v] = q[v];
    } else {
        x[0] = at[0];
    }
}

template <int VEC>
__device__ __forceinline__ void nr_slab_store(float* at, const float (&x)[VEC]) {
    if (VEC == 4) *reinterpret_cast<f32x4_t*>(at) = f32x4_t{x[0], x[1], x[2], x[3]};
    else at[0] = x[0];
}

// ---- apply: one read of S, one write of every output --------------------------------------------------------------------------
// A grid-stride loop over groups of VEC entries; VEC == 4: L % 4 == 0, a group lies in one row.  Output k is written where its
// pointer is set; a family with F::OUTS = 1 leaves out1 null.
template <int VEC, class F, class... A>
__global__ __launch_bounds__(256) void nr_slab_apply_kernel(const float* __restrict__ S, int n, int L, typename nr_slab_param<A>::type... a,
                                                           float* __restrict__ out0, float* __restrict__ out1) {
    const F f{a...};
    float* const out[2] = {out0, out1};
    const long long n_groups = (long long)n * L / VEC;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (long long)gridDim.x * 256) {
        const long long e0 = g * VEC;
        const int i = (int)(e0 / L);
        const int j0 = (int)(e0 - (long long)i * L);
        const auto row = f.row(i);
        float s[VEC];
        nr_slab_load<VEC>(S + e0, s);
#pragma unroll
        for (int k = 0; k < F::OUTS; ++k) {
            if (F::OUTS > 1 && !out[k]) continue;      // one output: always wanted
            float t[VEC];
            f.template values<VEC>(k, s, row, j0, e0, t);
            nr_slab_store<VEC>(out[k] + e0, t);
        }
    }
}

// vec_operands: what f.values reads with nr_slab_load besides S; the 16-byte path wants them aligned like S and the outputs.
template <class F, class... A>
static int nr_slab_apply(const float* S, int n, int L, float* out0, float* out1, std::initializer_list<const void*> vec_operands,
                         void* stream, A... a) {
    const bool vec = nr_slab_vec(L, {S, out0, out1}) && nr_slab_vec(L, vec_operands);
    const long long groups = (long long)n * L / (vec ? 4 : 1);
    const unsigned blocks = (unsigned)std::min<long long>((groups + 255) / 256, 16384);
    if (vec) {
        hipLaunchKernelGGL((nr_slab_apply_kernel<4, F, A...>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, S, n, L, a..., out0, out1);
    } else {
        hipLaunchKernelGGL((nr_slab_apply_kernel<1, F, A...>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, S, n, L, a..., out0, out1);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- rows: one wave per row, four rows per workgroup ------------------------------------------------------------------------------
template <bool VEC, class F, class... A>
__global__ __launch_bounds__(256) void nr_slab_rows_kernel(const float* __restrict__ S, int n, int L, typename nr_slab_param<A>::type... a,
                                                          float* __restrict__ out) {
    const F f{a...};
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                        // whole waves leave together: the shuffles below stay full-wave
    const float* line = S + (long long)row * L;
    const auto ctx = f.row(row);
    float m = -INFINITY, s = 0.f;
    if (VEC) {
        for (int c = lane; c < (L >> 2); c += 64) {
            float x[4];
            nr_slab_load<4>(line + 4 * c, x);
            f.template add_line<4>(m, s, x, ctx, 4 * c);
        }
    } else {
        for (int e = lane; e < L; e += 64) {
            const float x[1] = {line[e]};
            f.template add_line<1>(m, s, x, ctx, e);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        nr_hn_merge(m, s, m2, s2);
    }
    if (lane == 0) out[row] = f.finish(m, s, row);
}

// vec_operands: what f.add_line reads with nr_slab_load.
template <class F, class... A>
static int nr_slab_rows(const float* S, int n, int L, float* out, std::initializer_list<const void*> vec_operands, void* stream,
                        A... a) {
    const dim3 grid((n + 3) / 4);
    if (nr_slab_vec(L, {S}) && nr_slab_vec(L, vec_operands)) {
        hipLaunchKernelGGL((nr_slab_rows_kernel<true, F, A...>), grid, dim3(256), 0, (hipStream_t)stream, S, n, L, a..., out);
    } else {
        hipLaunchKernelGGL((nr_slab_rows_kernel<false, F, A...>), grid, dim3(256), 0, (hipStream_t)stream, S, n, L, a..., out);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- columns: partial pairs per block of NR_HN_ROWS rows ---------------------------------------------------------------------------
// Partial p of column c: part[(2p) L + c] = max, part[(2p + 1) L + c] = sum.  Each thread walks its VEC columns down the block's
// rows in row order, so a column's partial does not depend on VEC.
template <int VEC, class F, class... A>
__global__ __launch_bounds__(256) void nr_slab_col_part_kernel(const float* __restrict__ S, int n, int L, typename nr_slab_param<A>::type... a,
                                                              float* __restrict__ part) {
    const F f{a...};
    const long long c0 = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (c0 >= L) return;
    const int p = blockIdx.y;
    const int r0 = p * NR_HN_ROWS, r1 = min(n, r0 + NR_HN_ROWS);
    float m[VEC], s[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { m[v] = -INFINITY; s[v] = 0.f; }
    for (int r = r0; r < r1; ++r) {
        float x[VEC];
        nr_slab_load<VEC>(S + (long long)r * L + c0, x);
        const auto ctx = f.row(r);
#pragma unroll
        for (int v = 0; v < VEC; ++v) f.add(m[v], s[v], x[v], ctx);
    }
    float* pm = part + (long long)(2 * p) * L + c0;
    nr_slab_store<VEC>(pm, m);
    nr_slab_store<VEC>(pm + L, s);
}

// The ceil(n / NR_HN_ROWS) partials of a slab with n > 0 rows.
template <class F, class... A>
static int nr_slab_col_parts(const float* S, int n, int L, float* part, void* stream, A... a) {
    const unsigned P = (unsigned)((n + NR_HN_ROWS - 1) / NR_HN_ROWS);
    if (nr_slab_vec(L, {S, part})) {
        hipLaunchKernelGGL((nr_slab_col_part_kernel<4, F, A...>), dim3((unsigned)((L / 4 + 255) / 256), P), dim3(256), 0,
                           (hipStream_t)stream, S, n, L, a..., part);
    } else {
        hipLaunchKernelGGL((nr_slab_col_part_kernel<1, F, A...>), dim3((unsigned)((L + 255) / 256), P), dim3(256), 0,
                           (hipStream_t)stream, S, n, L, a..., part);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// ---- merge: P pairs per item, parts [P, 2, L], in index order p = 0, 1, ...; P = 0: every item (-inf, 0) -----------------------------
template <class F, class... A>
__global__ __launch_bounds__(256) void nr_slab_merge_kernel(int P, const float* __restrict__ parts, int L, typename nr_slab_param<A>::type... a) {
    const F f{a...};
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= L) return;
    float m = -INFINITY, s = 0.f;
    for (int p = 0; p < P; ++p) nr_hn_merge(m, s, parts[(long long)(2 * p) * L + c], parts[(long long)(2 * p + 1) * L + c]);
    f.finish(c, m, s);
}

template <class F, class... A>
static int nr_slab_merge(int P, const float* parts, int L, void* stream, A... a) {
    hipLaunchKernelGGL((nr_slab_merge_kernel<F, A...>), dim3((unsigned)((L + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, parts, L,
                       a...);
    NR_LAUNCH_CHECK();
    return NR_OK;
}
