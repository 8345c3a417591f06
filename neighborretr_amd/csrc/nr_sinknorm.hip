// Test-time Sinkhorn normalisation of a similarity slab (DESIGN.md "Test-time Sinkhorn normalisation"): the log-domain
// iteration of the reference's uniform regularisation (until_module.py:223-266) applied to the test similarity.
//
//   au[i,j] = fma(beta, S[i,j], u[i]);   av[i,j] = fma(beta, S[i,j], v[j])       one rounding each: product plus first potential
//   u[i] = log_mu[i] - LSE_j(av[i,j]);   v[j] = log_nu[j] - LSE_i(au[i,j]);   T[i,j] = fl(au[i,j] + v[j])
//
// Two roundings per entry of T, not the three of fl(fl(fl(beta S) + u) + v): the product is never a value of its own here, unlike
// the `is` apply of nr_hubnorm.hip, which rounds fl(beta S) first.  nr_sn_shift is the one place that says so.
//
// One iteration is plain launches on the caller's stream: the row half-step (one wave per row, writes u), the column
// partials (blocks of 64 rows write (max, sum) pairs to the caller's workspace) and the column finish (pairs merged in index
// order, writes v); the loops are nr_slab.h's.  The (max, sum) pairs are those of nr_hubnorm.hip: NaN entries are skipped, an
// entry equal to the max adds exactly 1, every reduction runs in a fixed order (lanes, a fixed butterfly; blocks in index order).
// No float atomics, no hand-off between workgroups: bitwise reproducible run to run.  A line whose LSE is not finite keeps
// potential 0.
#include "nr_slab.h"
#include "../../include/nr_hip.h"

// beta s + p in one rounding; every kernel of this file takes its entries through here
__device__ __forceinline__ float nr_sn_shift(float beta, float s, float p) { return fmaf(beta, s, p); }

__device__ __forceinline__ bool nr_sn_finite(float x) { return fabsf(x) < INFINITY; }      // false for NaN too

// line i's potential from its pairs' lse: its marginal's log (read only then) minus the lse, 0 when the lse is not finite
__device__ __forceinline__ float nr_sn_potential(const float* log_marginal, long long i, float m, float s) {
    const float lse = nr_hn_lse(m, s);
    return nr_sn_finite(lse) ? nr_rn_sub(log_marginal[i], lse) : 0.f;
}

static bool nr_sn_bad(int n, int L, float beta) { return n < 0 || L < 0 || !(beta > 0.f) || !(beta < INFINITY); }

// ---- row half-step ------------------------------------------------------------------------------------------------------------
// ERR = false: out[i] = u[i] = log_mu[i] - LSE_j(av[i,j]), 0 when the LSE is not finite.
// ERR = true:  out[i] = |exp(LSE_j(T[i,j]) - log_mu[i]) - 1|, the row's distance from its marginal, 0 for a row that takes no part.
template <bool ERR>
struct nr_sn_row {
    float beta;
    const float* u;
    const float* v;
    const float* log_mu;
    __device__ float row(int i) const { return ERR ? u[i] : 0.f; }
    template <int VEC>
    __device__ void add_line(float& m, float& s, const float (&x)[VEC], float ui, int j0) const {
        float p[VEC];
        nr_slab_load<VEC>(v + j0, p);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (x[k] != x[k]) continue;          // NaN: carries no mass
            nr_hn_merge(m, s, ERR ? nr_rn_add(nr_sn_shift(beta, x[k], ui), p[k]) : nr_sn_shift(beta, x[k], p[k]), 1.f);
        }
    }
    __device__ float finish(float m, float s, int i) const {
        if (!ERR) return nr_sn_potential(log_mu, i, m, s);
        const float lse = nr_hn_lse(m, s);
        return nr_sn_finite(lse) ? fabsf(nr_rn_sub(expf(nr_rn_sub(lse, log_mu[i])), 1.f)) : 0.f;
    }
};

extern "C" int nr_sinknorm_row(const float* S, int n, int L, float beta, const float* v, const float* log_mu, float* u,
                               void* stream) {
    if (!S || !v || !log_mu || !u) return NR_EINVAL;
    if (nr_sn_bad(n, L, beta)) return NR_EINVAL;
    if (n == 0) return NR_OK;
    return nr_slab_rows<nr_sn_row<false>>(S, n, L, u, {v}, stream, beta, (const float*)nullptr, v, log_mu);
}

extern "C" int nr_sinknorm_row_err(const float* S, int n, int L, float beta, const float* u, const float* v, const float* log_mu,
                                   float* err, void* stream) {
    if (!S || !u || !v || !log_mu || !err) return NR_EINVAL;
    if (nr_sn_bad(n, L, beta)) return NR_EINVAL;
    if (n == 0) return NR_OK;
    return nr_slab_rows<nr_sn_row<true>>(S, n, L, err, {v}, stream, beta, u, v, log_mu);
}

// ---- column half-step: the pairs of au down the columns (u[r] is uniform per row: a scalar load) ----------------------------------
struct nr_sn_col {
    float beta;
    const float* u;
    __device__ float row(int r) const { return u[r]; }
    __device__ void add(float& m, float& s, float x, float ur) const {
        if (x != x) return;
        nr_hn_merge(m, s, nr_sn_shift(beta, x, ur), 1.f);
    }
};

extern "C" int nr_sinknorm_col_stats(const float* S, int n, int L, float beta, const float* u, void* workspace, float* stats,
                                     void* stream) {
    if (n > 0 && (!S || !u || !workspace)) return NR_EINVAL;
    if (n == 0 && !stats) return NR_EINVAL;      // nothing to write at all
    if (nr_sn_bad(n, L, beta)) return NR_EINVAL;
    if (L == 0) return NR_OK;
    float* part = static_cast<float*>(workspace);
    if (n > 0) {
        const int rc = nr_slab_col_parts<nr_sn_col>(S, n, L, part, stream, beta, u);
        if (rc != NR_OK) return rc;
    }
    if (!stats) return NR_OK;                    // the caller finishes from the workspace's P pairs
    return nr_hubnorm_combine((n + NR_HN_ROWS - 1) / NR_HN_ROWS, part, L, stats, nullptr, stream);      // n = 0: every column (-inf, 0)
}

// merged pairs -> v[j] = log_nu[j] - lse, 0 when the lse is not finite
struct nr_sn_finish {
    const float* log_nu;
    float* v;
    __device__ void finish(long long c, float m, float s) const { v[c] = nr_sn_potential(log_nu, c, m, s); }
};

extern "C" int nr_sinknorm_finish_cols(int P, const float* parts, int L, const float* log_nu, float* v, void* stream) {
    if (!log_nu || !v || (P > 0 && !parts)) return NR_EINVAL;
    if (P < 0 || L < 0) return NR_EINVAL;
    if (L == 0) return NR_OK;
    return nr_slab_merge<nr_sn_finish>(P, parts, L, stream, log_nu, v);
}

// ---- apply: one read of S, one write of T -----------------------------------------------------------------------------------------
struct nr_sn_apply {
    static constexpr int OUTS = 1;
    float beta;
    const float* u;
    const float* v;
    __device__ float row(int i) const { return u[i]; }
    template <int VEC>
    __device__ void values(int, const float (&s)[VEC], float ui, int j0, long long, float (&t)[VEC]) const {
#pragma unroll
        for (int k = 0; k < VEC; ++k) t[k] = nr_rn_add(nr_sn_shift(beta, s[k], ui), v[j0 + k]);
    }
};

extern "C" int nr_sinknorm_apply(const float* S, int n, int L, float beta, const float* u, const float* v, float* T,
                                 void* stream) {
    if (!S || !u || !v || !T) return NR_EINVAL;
    if (nr_sn_bad(n, L, beta)) return NR_EINVAL;
    if (n == 0 || L == 0) return NR_OK;
    return nr_slab_apply<nr_sn_apply>(S, n, L, T, nullptr, {}, stream, beta, u, v);
}
