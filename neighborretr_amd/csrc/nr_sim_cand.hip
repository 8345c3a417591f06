// Fused local_level of CANDIDATE LISTS (reference: NeighborRetr/models/modeling.py:483-514, scored for chosen pairs only).
//
// out[i, c] = local_level(query i, gallery item cand[i, c]): the second stage of two-stage retrieval, where a cheap
// prefilter has picked C gallery items per query and only those pairs get the token-level score.
//
// One workgroup handles ONE query and a run of TB = BN / Ng of its candidates.  Operand A of the MFMA tile
// (nr_gemm_tile.h) is the query's Nq token rows (BM = 32 MI >= Nq, rows past the query are discarded); operand B is
// GATHERED: tile row r is token r % Ng of item cand[i, c0 + r / Ng] (NrGemmTile::run_gather -- the per-lane source
// address of the LDS-DMA pieces makes the row gather free).  A list entry outside [0, n_g), the padding -1 included,
// reads the zero row instead of forming an address, and its output is -inf.
// The epilogue is phases A-C of nr_sim_kernel (nr_sim.hip) with TA = 1:
//   phase A: P[t, cand]  = max_v C[t, cand*Ng+v]  (x w_q[t])
//   phase B: Q[col]      = max_t C[t, col]        (x w_g[col])
//   phase C: S[cand]     = 0.5 * (sum_t P + sum_v Q)   (J lanes per pair, shuffle-reduced)
// Every output element is produced inside one workgroup in an order that depends on (Nq, Ng, d) only -- not on the
// position of the item in the list and not on C --, so identical pairs give identical bits.  No atomics, no scratch.
#include "nr_gemm_tile.h"
#include "../../include/nr_hip.h"

struct NrSimCandArgs {
    const uint16_t *q_hi, *q_lo, *g_hi, *g_lo;
    const float *w_q, *w_g;
    const int32_t* cand;
    float* out;
    int n_q, Nq, n_g, Ng, K, C;
    int TB, runs;
    int ldc;      // floats per LDS C row
    int J;        // lanes per pair in phase C (power of two, <= 64)
    int off_pw, off_qw, off_wt;   // byte offsets of the LDS scratch arrays
};

template <int MI, int NI, bool X3>
__global__ __launch_bounds__(256) void nr_sim_cand_kernel(NrSimCandArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using Tile = NrGemmTile<MI, NI, X3>;
    constexpr int BM = Tile::BM, BN = Tile::BN;
    const int tid = threadIdx.x;
    const int q = blockIdx.x / p.runs, run = blockIdx.x - q * p.runs;
    const int Nq = p.Nq, Ng = p.Ng, TB = p.TB;
    const int c0 = run * TB;
    const int cnt = min(TB, p.C - c0);                       // list entries of this run
    const int32_t* list = p.cand + (size_t)q * p.C + c0;
    const int row0 = q * Nq;
    const int ncol = TB * Ng;

    float* sC = reinterpret_cast<float*>(smem);
    float* sPW = reinterpret_cast<float*>(smem + p.off_pw);
    float* sQW = reinterpret_cast<float*>(smem + p.off_qw);
    float* sWT = reinterpret_cast<float*>(smem + p.off_wt);     // token weights of the tile's rows / columns,
    float* sWV = sWT + BM;                                      // 0 for rows / columns outside the problem

    // token weights into LDS up front: their global latency hides under the main loop
    for (int r = tid; r < BM; r += 256) sWT[r] = r < Nq ? p.w_q[row0 + r] : 0.f;
    for (int c = tid; c < BN; c += 256) {
        const int bl = c / Ng;
        const int item = bl < cnt ? list[bl] : -1;
        const bool on = item >= 0 && item < p.n_g;
        sWV[c] = on ? p.w_g[(size_t)item * Ng + (c - bl * Ng)] : 0.f;
    }

    Tile tile;
    tile.zero();
    tile.run_gather(p.q_hi, p.q_lo, row0, p.n_q * Nq, p.g_hi, p.g_lo, list, cnt, Ng, p.n_g, p.K, smem);

    const int ldc = p.ldc;
    tile.store_lds(sC, ldc);
    __syncthreads();

    // ---- phase A: max over the gallery tokens of each (query token, candidate) --------------------
    const bool vec_a = (Ng & 3) == 0;
    for (int i = tid; i < Nq * TB; i += 256) {
        int r = i / TB, bl = i - r * TB;
        const float* c = sC + r * ldc + bl * Ng;
        float m;
        if (vec_a) {
            f32x4_t x = *reinterpret_cast<const f32x4_t*>(c);
            m = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
            for (int v = 4; v < Ng; v += 4) {
                x = *reinterpret_cast<const f32x4_t*>(c + v);
                m = fmaxf(m, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
            }
        } else {
            m = c[0];
            for (int v = 1; v < Ng; ++v) m = fmaxf(m, c[v]);
        }
        sPW[i] = m * sWT[r];
    }
    // ---- phase B: max over the query tokens of each column; 4 adjacent columns per thread ---------
    const int ngrp = (ncol + 3) >> 2;
    for (int cg = tid; cg < ngrp; cg += 256) {
        const float* col = sC + cg * 4;
        f32x4_t m = *reinterpret_cast<const f32x4_t*>(col);
        for (int t = 1; t < Nq; ++t) {
            f32x4_t x = *reinterpret_cast<const f32x4_t*>(col + t * ldc);
            m[0] = fmaxf(m[0], x[0]);
            m[1] = fmaxf(m[1], x[1]);
            m[2] = fmaxf(m[2], x[2]);
            m[3] = fmaxf(m[3], x[3]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int c = cg * 4 + e;
            if (c < ncol) sQW[c] = m[e] * sWV[c];
        }
    }
    __syncthreads();

    // ---- phase C: weighted sums per pair ---------------------------------------------------------
    const int J = p.J;
    const int groups = 256 / J;
    const int g = tid / J, j = tid - g * J;
    for (int base = 0; base < TB; base += groups) {
        int bl = base + g;
        float s = 0.f;
        if (bl < TB) {
            for (int t = j; t < Nq; t += J) s += sPW[t * TB + bl];
            for (int v = j; v < Ng; v += J) s += sQW[bl * Ng + v];
        }
        for (int o = J >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (j == 0 && bl < cnt) {
            const int item = list[bl];
            const bool on = item >= 0 && item < p.n_g;
            p.out[(size_t)q * p.C + c0 + bl] = on ? 0.5f * s : -__builtin_inff();
        }
    }
}

// ---- host side -------------------------------------------------------------------------------
// the column extent (96 / 128) that wastes the fewest MFMA columns on padding: whole items per run.  (64 columns never win:
// 128 hold twice as many items of any size, so there is no NI = 2 instantiation.)
static int nr_cand_pick_cols(int n_tok, int* ni_out) {
    int best_ni = 0;
    double best_eff = -1.0;
    for (int ni = 3; ni <= 4; ++ni) {
        int ext = 32 * ni;
        int t = ext / n_tok;
        if (t <= 0) continue;
        double eff = (double)(t * n_tok) / ext;
        if (eff > best_eff + 1e-9 || (eff > best_eff - 1e-9 && ni > best_ni)) {
            best_eff = eff;
            best_ni = ni;
        }
    }
    if (best_ni == 0) return 0;
    *ni_out = best_ni;
    return (32 * best_ni) / n_tok;
}

template <int MI, int NI, bool X3>
static int nr_sim_cand_launch(NrSimCandArgs& a, unsigned grid, size_t lds, hipStream_t st) {
    auto kern = nr_sim_cand_kernel<MI, NI, X3>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, a);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

extern "C" int nr_local_level_cand(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* g_hi, const uint16_t* g_lo,
                                   const float* w_q, const float* w_g, int n_q, int Nq, int n_g, int Ng, int d, int prec,
                                   const int32_t* cand, int C, float* out, void* stream) {
    if (!q_hi || !g_hi || !w_q || !w_g || !cand || !out) return NR_EINVAL;
    if (n_q <= 0 || n_g <= 0 || Nq <= 0 || Ng <= 0 || d <= 0 || (d % 64) != 0) return NR_EINVAL;
    if (C < 1 || C > 128) return NR_EINVAL;
    if (prec != NR_PREC_BF16 && prec != NR_PREC_BF16X3) return NR_EINVAL;
    if (prec == NR_PREC_BF16X3 && (!q_lo || !g_lo)) return NR_EINVAL;
    if (Nq > 128 || Ng > 128) return NR_EUNSUPPORTED;
    if (d > 1024) return NR_EUNSUPPORTED;                        // the zero row of absent candidates is 1024 elements long
    if ((long long)n_q * Nq > 0x7fffffffLL || (long long)n_g * Ng > 0x7fffffffLL) return NR_EUNSUPPORTED;

    const int mi = (Nq + 31) / 32;
    int ni = 0;
    const int TB = nr_cand_pick_cols(Ng, &ni);                   // never clamped to C: a pair's arithmetic does not depend on C
    if (TB == 0) return NR_EUNSUPPORTED;
    const int runs = (C + TB - 1) / TB;
    if ((long long)n_q * runs > 0x7fffffffLL) return NR_EUNSUPPORTED;

    NrSimCandArgs a;
    a.q_hi = q_hi; a.q_lo = q_lo; a.g_hi = g_hi; a.g_lo = g_lo;
    a.w_q = w_q; a.w_g = w_g; a.cand = cand; a.out = out;
    a.n_q = n_q; a.Nq = Nq; a.n_g = n_g; a.Ng = Ng; a.K = d; a.C = C; a.TB = TB; a.runs = runs;
    const int BM = 32 * mi, BN = 32 * ni;
    a.ldc = BN + 4;
    int J = 64;
    while (J > 1 && J * TB > 256) J >>= 1;
    a.J = J;
    size_t stage = (size_t)2 * (BM + BN) * 128 * (prec == NR_PREC_BF16X3 ? 2 : 1);   // DMA ring
    size_t cbytes = (size_t)BM * a.ldc * 4;
    size_t base = stage > cbytes ? stage : cbytes;
    base = (base + 15) & ~(size_t)15;
    a.off_pw = (int)base;
    size_t pw = ((size_t)Nq * TB * 4 + 15) & ~(size_t)15;
    a.off_qw = (int)(base + pw);
    size_t qw = ((size_t)TB * Ng * 4 + 15) & ~(size_t)15;
    a.off_wt = (int)(base + pw + qw);
    size_t lds = base + pw + qw + (size_t)(BM + BN) * 4;
    if (lds > 160 * 1024) return NR_EUNSUPPORTED;

    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)n_q * (unsigned)runs;
    const bool x3 = prec == NR_PREC_BF16X3;
#define NR_CAND_CASE(M_, N_)                                                      \
    if (mi == M_ && ni == N_)                                                     \
        return x3 ? nr_sim_cand_launch<M_, N_, true>(a, grid, lds, st) : nr_sim_cand_launch<M_, N_, false>(a, grid, lds, st);
    NR_CAND_CASE(1, 3) NR_CAND_CASE(1, 4)
    NR_CAND_CASE(2, 3) NR_CAND_CASE(2, 4)
    NR_CAND_CASE(3, 3) NR_CAND_CASE(3, 4)
    NR_CAND_CASE(4, 3) NR_CAND_CASE(4, 4)
#undef NR_CAND_CASE
    return NR_EUNSUPPORTED;
}
