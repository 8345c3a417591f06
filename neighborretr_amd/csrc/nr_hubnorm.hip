// Test-time hubness reduction over similarity slabs: IS, DSL and QB-Norm (DESIGN.md "Test-time hubness reduction").
//
// All four kernels are single passes over fp32 slabs and bound by memory bandwidth; their loops are nr_slab.h's.
//   - log-sum-exp statistics: every line of fl(beta * S) is reduced to a (max, sum) pair, sum = sum of exp(beta x - max) over its
//     non-NaN entries, entries equal to the max adding exactly 1 (so +inf and all -inf lines are defined); lse = max +
//     log(sum), -inf for a line with no entry.  Rows: one wave per row.  Columns: row blocks write partial pairs to a
//     caller-provided workspace and a second launch combines them in block order.  Every reduction runs in a fixed order
//     (lanes, then a fixed butterfly; blocks, then index order): no float atomics, no hand-off between workgroups, bitwise
//     reproducible run to run.
//   - apply: T (column normaliser, per-row gate) and V (row normaliser, per-column gate) from one read of S.
#include "nr_slab.h"
#include "../../include/nr_hip.h"

static bool nr_hn_bad(int n, int L, float beta) { return n < 0 || L < 0 || !(beta > 0.f) || !(beta < INFINITY); }

// ---- row and column statistics -------------------------------------------------------------------------------------------
// one more entry of a line: fl(beta x), a value of its own (nr_hn_add)
struct nr_hn_line {
    float beta;
    __device__ int row(int) const { return 0; }
    __device__ void add(float& m, float& s, float x, int) const { nr_hn_add(m, s, beta, x); }
    template <int VEC>
    __device__ void add_line(float& m, float& s, const float (&x)[VEC], int, int) const {
#pragma unroll
        for (int v = 0; v < VEC; ++v) nr_hn_add(m, s, beta, x[v]);
    }
    __device__ float finish(float m, float s, int) const { return nr_hn_lse(m, s); }
};

// merged pairs -> stats [2, L] (max, sum) and / or lse [L]
struct nr_hn_combine {
    int L;
    float* stats;
    float* lse;
    __device__ void finish(long long c, float m, float s) const {
        if (stats) {
            stats[c] = m;
            stats[L + c] = s;
        }
        if (lse) lse[c] = nr_hn_lse(m, s);
    }
};

extern "C" int nr_hubnorm_row_lse(const float* S, int n, int L, float beta, float* lse, void* stream) {
    if (!S || !lse) return NR_EINVAL;
    if (nr_hn_bad(n, L, beta)) return NR_EINVAL;
    if (n == 0) return NR_OK;
    return nr_slab_rows<nr_hn_line>(S, n, L, lse, {}, stream, beta);
}

extern "C" size_t nr_hubnorm_col_workspace(int n, int L) {
    if (n <= 0 || L <= 0) return 0;
    return (size_t)((n + NR_HN_ROWS - 1) / NR_HN_ROWS) * 2 * (size_t)L * sizeof(float);
}

extern "C" int nr_hubnorm_col_stats(const float* S, int n, int L, float beta, void* workspace, float* stats, void* stream) {
    if (!stats || (n > 0 && (!S || !workspace))) return NR_EINVAL;
    if (nr_hn_bad(n, L, beta)) return NR_EINVAL;
    if (L == 0) return NR_OK;
    float* part = static_cast<float*>(workspace);
    if (n > 0) {
        const int rc = nr_slab_col_parts<nr_hn_line>(S, n, L, part, stream, beta);
        if (rc != NR_OK) return rc;
    }
    return nr_slab_merge<nr_hn_combine>((n + NR_HN_ROWS - 1) / NR_HN_ROWS, part, L, stream, L, stats, (float*)nullptr);
}

extern "C" int nr_hubnorm_combine(int P, const float* parts, int L, float* stats, float* lse, void* stream) {
    if ((!stats && !lse) || (P > 0 && !parts)) return NR_EINVAL;
    if (P < 0 || L < 0) return NR_EINVAL;
    if (L == 0) return NR_OK;
    return nr_slab_merge<nr_hn_combine>(P, parts, L, stream, L, stats, lse);
}

// ---- apply ------------------------------------------------------------------------------------------------------------------
// b = fl(beta s) is a value of its own in both modes.
// is:  fl(b - c): two roundings, no fused multiply-add (NumPy float32 gives the same bits).
// dsl: s * exp(beta s - c).  The exponent is carried to about one rounding: b with its exact residual (fma), and d = fl(b - c)
// with its exact residual (two-sum); exp(d) * (1 + residuals).  Non-finite cases keep the plain form.
__device__ __forceinline__ float nr_hn_is(float b, float c) { return nr_rn_sub(b, c); }

__device__ __forceinline__ float nr_hn_dsl(float s, float beta, float b, float c) {
    const float lo = fmaf(beta, s, -b);
    const float d = nr_rn_sub(b, c);
    const float z = nr_rn_sub(d, b);
    const float e = nr_rn_add(nr_rn_sub(b, nr_rn_sub(d, z)), nr_rn_sub(-c, z));
    float t = nr_rn_add(e, lo);
    if (!(fabsf(t) < 1e-3f)) t = 0.f;            // inf / NaN operands: no correction
    const float x = nr_rn_mul(s, expf(d));
    return fmaf(x, t, x);
}

// Output 0 = T: the column normaliser on the rows whose gate is set; output 1 = V: the row normaliser on the gated columns.  A row
// or column whose gate is 0 keeps S; no gate: every one is set.  A row operand whose output is not wanted is null and not read.
template <int MODE>
struct nr_hn_apply {
    static constexpr int OUTS = 2;
    float beta;
    const float* col_norm;
    const int32_t* row_gate;
    const float* row_norm;
    const int32_t* col_gate;
    struct Row { bool on; float norm; };
    __device__ Row row(int i) const { return {!row_gate || row_gate[i] != 0, row_norm ? row_norm[i] : 0.f}; }
    __device__ float value(int k, float s, Row r, int j) const {
        const float b = nr_rn_mul(beta, s);
        const bool on = k == 0 ? r.on : (!col_gate || col_gate[j] != 0);
        if (!on) return s;
        const float c = k == 0 ? col_norm[j] : r.norm;
        return MODE == NR_HUBNORM_IS ? nr_hn_is(b, c) : nr_hn_dsl(s, beta, b, c);
    }
    template <int VEC>
    __device__ void values(int k, const float (&s)[VEC], Row r, int j0, long long, float (&t)[VEC]) const {
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[v] = value(k, s[v], r, j0 + v);
    }
};

extern "C" int nr_hubnorm_apply(const float* S, int n, int L, float beta, int mode, const float* col_norm,
                                const int32_t* row_gate, float* T, const float* row_norm, const int32_t* col_gate, float* V,
                                void* stream) {
    if (!S || (!T && !V) || (T && !col_norm) || (V && !row_norm)) return NR_EINVAL;
    if (nr_hn_bad(n, L, beta)) return NR_EINVAL;
    if (mode != NR_HUBNORM_IS && mode != NR_HUBNORM_DSL) return NR_EINVAL;
    if (n == 0 || L == 0) return NR_OK;
    if (!T) row_gate = nullptr;
    if (!V) row_norm = nullptr;
    if (mode == NR_HUBNORM_IS)
        return nr_slab_apply<nr_hn_apply<NR_HUBNORM_IS>>(S, n, L, T, V, {}, stream, beta, col_norm, row_gate, row_norm, col_gate);
    return nr_slab_apply<nr_hn_apply<NR_HUBNORM_DSL>>(S, n, L, T, V, {}, stream, beta, col_norm, row_gate, row_norm, col_gate);
}
