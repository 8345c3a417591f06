// One CTM + TCBlock stage (reference cluster.py:670-717 + :938-965, no-grad forward) for a GROUP of
// independent problems -- in the training step: the text and the video tokens -- in SEVEN launches:
//   shift|split -> conv GEMM (+x) -> front (LayerNorm, score, norm1, distances) -> back (DPC-KNN, merge, norm1)
//   -> q and kv GEMMs (one grouped launch) -> score-biased attention -> proj GEMM (+merged +bias)
// Every launch carries the workgroups of all problems of the group (workgroup -> problem through a prefix
// table), so the two modalities advance in lockstep inside the same grids instead of competing from two
// streams: measured on MI355X, two clustering branches on two streams overlap to only ~0.68 of their
// summed time, while a grid that holds both costs max(text, video).  All GEMMs run split-bf16 on the MFMA
// tile engine (nr_linear.hip); their A operands are written hi/lo directly by the producing kernel.
#include <cstdlib>
#include "nr_ctm_bodies.h"
#include "nr_linear.h"
#include "../../include/nr_hip.h"

// plain rows as bf16 pairs: NR_SHIFT_ROWS rows per 256-thread workgroup, a float4 (one 8-byte pair store each) per thread and turn
#define NR_SHIFT_ROWS 8
__global__ __launch_bounds__(256) void nr_group_shift_kernel(NrGroupOf<NrShiftArgs> g) {
    NR_CRITICAL_PATH();
    const int gi = g.find(blockIdx.x);
    const NrShiftArgs& a = g.p[gi];
    const size_t e0 = (size_t)(blockIdx.x - g.start[gi]) * NR_SHIFT_ROWS * a.C, e1 = (size_t)a.N * a.C;      // (a.N: ALL rows of the problem here)
    for (size_t e = e0 + 4 * threadIdx.x; e < e0 + (size_t)NR_SHIFT_ROWS * a.C && e < e1; e += 1024) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(a.x + e);
        uint32_t h0, l0, h1, l1;
        nr_split_pk(v[0], v[1], h0, l0);
        nr_split_pk(v[2], v[3], h1, l1);
        *reinterpret_cast<uint2*>(a.hi + e) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(a.lo + e) = make_uint2(l0, l1);
    }
}

template <int CPL, int THREADS = CF_THREADS>
__global__ __launch_bounds__(THREADS) void nr_group_front_kernel(NrGroupOf<NrCtmFrontArgs> g) {
    NR_CRITICAL_PATH();
    extern __shared__ __attribute__((aligned(16))) float sx[];
    const int gi = g.find(blockIdx.x);
    nr_ctm_front_body<CPL, THREADS>(g.p[gi], blockIdx.x - g.start[gi], sx);
}

// front + back in one launch for stages without a mask (stage 1 of the step): the back half needs nothing from
// other workgroups then, and the normalised rows it merges are the ones the front half left in LDS
template <int CPL, int THREADS = CF_THREADS>
__global__ __launch_bounds__(THREADS) void nr_group_front_back_kernel(NrGroupOf<NrCtmFrontArgs> gf, NrGroupOf<NrCtmBackArgs> gb) {
    NR_CRITICAL_PATH();
    extern __shared__ __attribute__((aligned(16))) float sx[];
    const int gi = gf.find(blockIdx.x);
    const int b = blockIdx.x - gf.start[gi];
    nr_ctm_front_body<CPL, THREADS>(gf.p[gi], b, sx);
    __threadfence_block();                 // the distances / token weights this workgroup just stored are read back
    __syncthreads();
    nr_ctm_back_body<true, THREADS>(gb.p[gi], b, sx);
}

// second form of the bodies (nr_ctm_bodies.h): C % 256 == 0, 512-thread workgroups (256 for a handful of tokens)
template <int V4, int THREADS>
__global__ __launch_bounds__(THREADS, THREADS / 128) void nr_group_front2_kernel(NrGroupOf<NrCtmFrontArgs> g) {
    NR_CRITICAL_PATH();
    extern __shared__ __attribute__((aligned(16))) float sx[];
    const int gi = g.find(blockIdx.x);
    nr_ctm_front_body2<V4, THREADS>(g.p[gi], blockIdx.x - g.start[gi], sx);
}

// (the 16-cluster / 64-token form keeps a 64-entry distance row per lane: one workgroup per CU, up to 256 registers)
template <int V4, int THREADS, int MAXC, int MAXN>
__global__ __launch_bounds__(THREADS, MAXC <= 4 ? THREADS / 128 : THREADS / 256) void nr_group_front_back2_kernel(NrGroupOf<NrCtmFrontArgs> gf, NrGroupOf<NrCtmBackArgs> gb) {
    NR_CRITICAL_PATH();
    extern __shared__ __attribute__((aligned(16))) float sx[];
    const int gi = gf.find(blockIdx.x);
    const int b = blockIdx.x - gf.start[gi];
    const NrCtmFrontArgs& f = gf.p[gi];
    // the back half's tie-break draws: requested now, in LDS by the time it starts (a round trip less behind the front half)
    if ((int)threadIdx.x < f.N) sx[(size_t)f.N * f.C + (size_t)f.N * f.N + 64 + threadIdx.x] = gb.p[gi].noise[(size_t)b * f.N + threadIdx.x];
    nr_ctm_front_body2<V4, THREADS>(f, b, sx);
    __syncthreads();
    nr_ctm_back_body2<true, THREADS, MAXC, (256 * V4) / THREADS, MAXN>(gb.p[gi], b, sx, sx + (size_t)f.N * f.C, sx + (size_t)f.N * f.C + (size_t)f.N * f.N);
}

template <int THREADS, int MAXC, int CPT>
__global__ __launch_bounds__(THREADS, MAXC <= 4 ? THREADS / 128 : THREADS / 256) void nr_group_back2_kernel(NrGroupOf<NrCtmBackArgs> g, int use_lds) {
    NR_CRITICAL_PATH();
    extern __shared__ __attribute__((aligned(16))) float sxn[];
    const int gi = g.find(blockIdx.x);
    nr_ctm_back_body2<false, THREADS, MAXC, CPT, MAXC <= 4 ? 32 : 64>(g.p[gi], blockIdx.x - g.start[gi], use_lds ? sxn : nullptr, nullptr, nullptr);
}

template <int THREADS = BK_THREADS>
__global__ __launch_bounds__(THREADS) void nr_group_back_kernel(NrGroupOf<NrCtmBackArgs> g, int use_lds) {
    NR_CRITICAL_PATH();
    extern __shared__ __attribute__((aligned(16))) float sxn[];
    const int gi = g.find(blockIdx.x);
    nr_ctm_back_body<false, THREADS>(g.p[gi], blockIdx.x - g.start[gi], use_lds ? sxn : nullptr);
}

__global__ __launch_bounds__(1024) void nr_group_attention_kernel(NrGroupOf<NrAttnArgs> g, int use_lds) {
    NR_CRITICAL_PATH();
    extern __shared__ __attribute__((aligned(16))) float skv[];
    const int gi = g.find(blockIdx.x);
    nr_tc_attention_body(g.p[gi], blockIdx.x - g.start[gi], use_lds ? skv : nullptr);
}

// a workgroup per (sample, pair of heads): see nr_tc_attention_heads_body.  g.start[] counts WORKGROUPS here.
#define NR_ATTN_HG 2
__global__ __launch_bounds__(256) void nr_group_attention_heads_kernel(NrGroupOf<NrAttnArgs> g) {
    NR_CRITICAL_PATH();
    extern __shared__ __attribute__((aligned(16))) float skv[];
    const int gi = g.find(blockIdx.x);
    const int idx = blockIdx.x - g.start[gi], per_sample = g.p[gi].H / NR_ATTN_HG;
    nr_tc_attention_heads_body<NR_ATTN_HG>(g.p[gi], idx / per_sample, idx % per_sample, skv);
}

#ifdef NR_STAMP
extern "C" int nr_debug_front_stamps(unsigned long long* host) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(nr_front_stamps), sizeof(unsigned long long) * 16);
    return 5;
}
extern "C" int nr_debug_back_stamps(unsigned long long* host) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(nr_back_stamps), sizeof(unsigned long long) * 16);
    return 7;
}
#endif

// ---- workspace carve-up --------------------------------------------------------------------------------------
namespace {
struct Carve {
    char* base;
    size_t off;
    template <typename T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

struct StageBuffers {
    uint16_t *cat_hi, *cat_lo, *kvn_hi, *kvn_lo, *qn_hi, *qn_lo, *att_hi, *att_lo;
    float *y, *xn, *score, *tokw, *dist, *smax, *merged_pb, *q, *kv;
    size_t bytes;
};

StageBuffers carve(void* ws, long B, long N, long C, long cnum) {
    Carve c{static_cast<char*>(ws), 0};
    StageBuffers s;
    s.cat_hi = c.take<uint16_t>(B * N * 3 * C);
    s.cat_lo = c.take<uint16_t>(B * N * 3 * C);
    s.y = c.take<float>(B * N * C);
    s.xn = c.take<float>(B * N * C);
    s.kvn_hi = c.take<uint16_t>(B * N * C);
    s.kvn_lo = c.take<uint16_t>(B * N * C);
    s.score = c.take<float>(B * N);
    s.tokw = c.take<float>(B * N);
    s.dist = c.take<float>(B * N * N);
    s.smax = c.take<float>(B);
    s.merged_pb = c.take<float>(B * cnum * C);
    s.qn_hi = c.take<uint16_t>(B * cnum * C);
    s.qn_lo = c.take<uint16_t>(B * cnum * C);
    s.q = c.take<float>(B * cnum * C);
    s.kv = c.take<float>(B * N * 2 * C);
    s.att_hi = c.take<uint16_t>(B * cnum * C);
    s.att_lo = c.take<uint16_t>(B * cnum * C);
    s.bytes = c.off;
    return s;
}
}  // namespace

extern "C" size_t nr_ctm_stage_workspace_bytes(int n_samples, int N, int C, int cluster_num) {
    if (n_samples <= 0 || N <= 0 || C <= 0 || cluster_num <= 0) return 0;
    return carve(nullptr, n_samples, N, C, cluster_num).bytes;
}

// byte offsets inside the stage workspace of what a backward pass needs: y (conv output + residual, pre-LayerNorm),
// xn (LayerNorm output), score (masked tokens: -inf), tokw (exp(score)), merged_pb (cluster means + proj bias), q, kv;
// and smax [n]: every sample's largest pairwise distance, written by the front launch and max-reduced over the samples by
// the back launch (cluster.py:473-475 fills masked columns with the maximum over the WHOLE batch + 1) -- a rank that
// clusters only its own samples puts the all-reduced maximum into smax[0] between the two launches
extern "C" int nr_ctm_stage_workspace_layout(int n_samples, int N, int C, int cluster_num, size_t* offsets) {
    if (n_samples <= 0 || N <= 0 || C <= 0 || cluster_num <= 0 || !offsets) return NR_EINVAL;
    char* const base = reinterpret_cast<char*>(4096);
    const StageBuffers s = carve(base, n_samples, N, C, cluster_num);
    const void* p[8] = {s.y, s.xn, s.score, s.tokw, s.merged_pb, s.q, s.kv, s.smax};
    for (int i = 0; i < 8; ++i) offsets[i] = (size_t)(static_cast<const char*>(p[i]) - base);
    return NR_OK;
}

extern "C" int nr_ctm_stage_workspace_layout2(int n_samples, int N, int C, int cluster_num, size_t* offsets) {
    int rc = nr_ctm_stage_workspace_layout(n_samples, N, C, cluster_num, offsets);
    if (rc != NR_OK) return rc;
    char* const base = reinterpret_cast<char*>(4096);
    const StageBuffers s = carve(base, n_samples, N, C, cluster_num);
    const void* p[6] = {s.kvn_hi, s.kvn_lo, s.qn_hi, s.qn_lo, s.att_hi, s.att_lo};
    for (int i = 0; i < 6; ++i) offsets[8 + i] = (size_t)(static_cast<const char*>(p[i]) - base);
    return NR_OK;
}

// ---- the stage: validate, carve, plan once, launch [first, last) of the plan ----------------------------------------
namespace {
// Every check of a call that needs no device, in the order their statuses are reported: per problem NR_EINVAL before
// NR_EUNSUPPORTED.  pointers = false (nr_ctm_stage_plan): only the scalars, and x_hi / x_lo only as "given or not".
int validate(const NrCtmStageDesc* d, int n, bool pointers) {
    if (!d || n <= 0 || n > NR_CTM_MAX_GROUP) return NR_EINVAL;
    for (int i = 0; i < n; ++i) {
        const NrCtmStageDesc& s = d[i];
        if (pointers && (!s.x || !s.noise || !s.wconv_hi || !s.wconv_lo || !s.ln_w || !s.ln_b || !s.sc_w || !s.sc_b || !s.n1_w || !s.n1_b ||
                         !s.wq_hi || !s.wq_lo || !s.wkv_hi || !s.wkv_lo || !s.wp_hi || !s.wp_lo || !s.proj_bias || !s.workspace || !s.out))
            return NR_EINVAL;
        if (s.n_samples <= 0 || s.N <= 0 || s.k <= 0 || s.k > s.N || s.cnum <= 0 || s.cnum > s.N || s.heads <= 0) return NR_EINVAL;
        if (s.N > 64 || s.C <= 0 || (s.C % 128) != 0 || s.C > 1024 || s.C != s.heads * 64) return NR_EUNSUPPORTED;
        if (s.cnum * (s.C / 128) > 16 * BK_MAXJ) return NR_EUNSUPPORTED;
        if ((size_t)s.N * s.C * sizeof(float) > 150 * 1024) return NR_EUNSUPPORTED;      // the front half keeps a sample's rows in LDS
    }
    for (int i = 0; i < n; ++i)
        if ((d[i].x_hi == nullptr) != (d[i].x_lo == nullptr)) return NR_EINVAL;
    return NR_OK;
}

// What the seven launches of one call have to agree on, decided once (plan_stage) from the validated shapes alone.
struct StagePlan {
    int samples, start[NR_CTM_MAX_GROUP + 1];   // one workgroup per sample in launches 2 and 3: first sample of every problem
    int split_grid;                             // launch 0: 0 = every problem brings x_hi / x_lo, nothing to launch
    bool fusable;                               // no problem carries a mask
    int form;                                   // 1 / 2: first or second form of the two bodies (nr_ctm_bodies.h)
    bool small, few;                            // every C <= 512 (register budget); a handful of tokens per sample
    int front_threads;                          // launch 2: front alone, or front + back in one kernel when back == NR_CTM_BACK_NONE
    size_t front_lds;
    bool front_attr;
    int back, back_form, back_threads, back_use_lds;       // launch 3 (NR_CTM_BACK_*)
    size_t back_lds;
    bool back_attr;
    int kv_launch;                              // 3: the kv GEMM rides beside the back half; 4: with the q GEMM
    int attn_form, attn_grid, attn_threads, attn_use_lds;  // launch 5 (NR_CTM_ATTN_*)
    size_t attn_lds;
    bool attn_attr;
};

int shift_blocks(const NrCtmStageDesc& s) { return (s.n_samples * s.N + NR_SHIFT_ROWS - 1) / NR_SHIFT_ROWS; }
int attn_blocks(const NrCtmStageDesc& s, int form) { return s.n_samples * (form == NR_CTM_ATTN_HEADS ? s.heads / NR_ATTN_HG : 1); }

// Pure host arithmetic: no HIP call, no launch range.  The tuning hooks (NR_TUNE builds only, tools/ab_attn.sh) are read here
// and nowhere else in this file.
StagePlan plan_stage(const NrCtmStageDesc* d, int n) {
    StagePlan p{};
    const bool kv_apart = nr_tune_env("NR_KV_APART") != nullptr, v1 = nr_tune_env("NR_CTM_V1") != nullptr;
    const bool attn_whole = nr_tune_env("NR_ATTN_WHOLE") != nullptr;
    const char* te = nr_tune_env("NR_CTM_THREADS");
    const bool threads512 = te && atoi(te) == 512;
    p.fusable = p.small = true;
    bool c512 = true, n8 = true, few1 = true, rows256 = true, heads_even = true;
    int maxc = 0, maxn = 0, jobs_max = 0;       // jobs: (head, query) pairs of a sample's attention
    size_t rows_lds = 0, front2_lds = 0, kv_lds = 0, kv_heads_lds = 0;       // largest problem's, bytes
    auto upto = [](size_t& m, size_t v) { m = v > m ? v : m; };
    for (int i = 0; i < n; ++i) {
        const NrCtmStageDesc& s = d[i];
        p.start[i] = p.samples;
        p.samples += s.n_samples;
        if (!s.x_hi) p.split_grid += shift_blocks(s);
        p.fusable = p.fusable && s.mask == nullptr;
        p.small = p.small && s.C <= 512;
        c512 = c512 && s.C == 512;
        n8 = n8 && s.N <= 8;
        few1 = few1 && s.N <= 8 && s.cnum * (s.C / 128) <= 4 * BK_MAXJ;
        rows256 = rows256 && (s.N * s.C) % 256 == 0;
        heads_even = heads_even && s.heads % NR_ATTN_HG == 0;
        maxc = s.cnum > maxc ? s.cnum : maxc;
        maxn = s.N > maxn ? s.N : maxn;
        jobs_max = s.heads * s.cnum > jobs_max ? s.heads * s.cnum : jobs_max;
        upto(rows_lds, (size_t)s.N * s.C * sizeof(float));
        upto(front2_lds, nr_ctm_front2_lds_floats(s.N, s.C) * sizeof(float));
        upto(kv_lds, (size_t)s.N * (2 * s.C + 4) * sizeof(float));
        upto(kv_heads_lds, (size_t)s.N * (2 * 64 * NR_ATTN_HG + 4) * sizeof(float));
    }
    for (int i = n; i <= NR_CTM_MAX_GROUP; ++i) p.start[i] = p.samples;

    // The second form of the two bodies: every problem 512 channels wide (the model's width), at most 16 clusters.  Its back half
    // keeps 4 cluster accumulators and a 32-entry distance row per token in registers, or 16 and 64.  NR_CTM_V1=1 keeps the first.
    p.form = (!v1 && c512 && maxc <= 16) ? 2 : 1;
    p.back_form = p.form == 1 ? 0 : (maxc <= 4 && maxn <= 32) ? 4 : 16;
    // Front and back are ONE launch when no problem carries a mask (stage 1 of the step); with a mask the back half needs the
    // maximum distance over ALL samples.  First form, C > 512: sixteen channels per lane of seven per-channel vectors do not fit
    // the 128 registers a 1024-thread workgroup leaves a lane (48 spilled registers, round 3) -- 512-thread workgroups, never fused.
    const bool fused = p.fusable && (p.form == 2 || p.small);
    // a handful of tokens per sample (stage 1 of the step): 256-thread workgroups for the fused kernel
    p.few = p.form == 2 ? (maxc <= 4 && n8) : (p.small && few1);
    if (p.form == 2) {
        p.front_threads = (fused && p.few) ? 256 : 512;
        p.front_lds = front2_lds;
        p.front_attr = p.front_lds > 40 * 1024;
    } else {
        p.front_threads = (fused && p.few) ? 256 : p.small ? CF_THREADS : 512;
        p.front_lds = rows_lds;
        p.front_attr = p.front_lds > 64 * 1024;
    }

    // Launch 3: the back half when it is a launch of its own, with the token rows of a sample in LDS when they fit (second form:
    // while two workgroups still share a CU).  The kv projection needs the front launch alone, like the back half, so it rides in
    // that launch where nr_linear.h takes the pair, and launch 4 is the q projection alone.  NR_KV_APART=1: never.
    p.kv_launch = 4;
    if (fused) {
        p.back = NR_CTM_BACK_NONE;
        p.back_form = 0;
    } else {
        p.back_use_lds = p.form == 2 ? rows_lds <= 56 * 1024 : (rows256 && rows_lds <= 96 * 1024);
        p.back_lds = p.back_use_lds ? rows_lds : 0;
        bool beside = !p.fusable && p.small && !kv_apart;
        for (int i = 0; i < n; ++i) beside = beside && nr_linear_beside_back_fits(d[i].C, true, d[i].N, d[i].C, d[i].cnum, p.back_form);
        p.back = beside ? NR_CTM_BACK_BESIDE_KV : NR_CTM_BACK_ALONE;
        p.back_threads = (beside || p.form == 2 || threads512) ? 512 : BK_THREADS;
        p.back_attr = !beside && p.back_lds > 40 * 1024;
        if (beside) p.kv_launch = 3;
    }

    // Launch 5.  More than a wave's worth of (head, query) jobs per pair of heads: a 256-thread workgroup per (sample, pair of
    // heads) with only those heads' k | v columns in LDS -- several share a CU, and 64-token samples get their k | v rows into LDS
    // at all.  Otherwise one workgroup per sample with up to 128 KB of k | v rows: a wave per job, 8 waves when that covers them.
    // NR_ATTN_WHOLE=1 keeps the whole-sample form (A/B hook).
    if (jobs_max > 8 && !attn_whole && heads_even && kv_heads_lds <= 72 * 1024) {
        p.attn_form = NR_CTM_ATTN_HEADS;
        p.attn_threads = 256;
        p.attn_use_lds = 1;
        p.attn_lds = kv_heads_lds;
    } else {
        p.attn_form = NR_CTM_ATTN_WHOLE;
        p.attn_threads = (jobs_max <= 8 || threads512) ? 512 : 1024;
        p.attn_use_lds = kv_lds <= 128 * 1024;
        p.attn_lds = p.attn_use_lds ? kv_lds : 0;
    }
    p.attn_attr = p.attn_lds > 64 * 1024;
    for (int i = 0; i < n; ++i) p.attn_grid += attn_blocks(d[i], p.attn_form);
    return p;
}

int raise_lds(const void* kernel, size_t lds) { return (int)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }

// ---- the argument groups ----
void kv_problems(const NrCtmStageDesc* d, const StageBuffers* w, int n, NrLinearArgs* p) {
    for (int i = 0; i < n; ++i)
        p[i] = NrLinearArgs{w[i].kvn_hi, w[i].kvn_lo, d[i].wkv_hi, d[i].wkv_lo, d[i].kv_bias, nullptr, w[i].kv, d[i].n_samples * d[i].N, 2 * d[i].C, d[i].C};
}

NrGroupOf<NrCtmFrontArgs> front_args(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan& p) {
    NrGroupOf<NrCtmFrontArgs> g;
    g.n = n;
    for (int i = 0; i <= NR_CTM_MAX_GROUP; ++i) g.start[i] = p.start[i];
    for (int i = 0; i < n; ++i) {
        const NrCtmStageDesc& s = d[i];
        g.p[i] = NrCtmFrontArgs{w[i].y, s.mask, s.ln_w, s.ln_b, s.sc_w, s.sc_b, s.n1_w, s.n1_b, s.eps_ctm, 1.0f / sqrtf((float)s.C),
                                s.N, s.C, w[i].xn, nullptr, w[i].score, w[i].tokw, w[i].dist, w[i].smax, w[i].kvn_hi, w[i].kvn_lo};
    }
    return g;
}

NrGroupOf<NrCtmBackArgs> back_args(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan& p) {
    NrGroupOf<NrCtmBackArgs> g;
    g.n = n;
    for (int i = 0; i <= NR_CTM_MAX_GROUP; ++i) g.start[i] = p.start[i];
    for (int i = 0; i < n; ++i) {
        const NrCtmStageDesc& s = d[i];
        g.p[i] = NrCtmBackArgs{w[i].dist, w[i].smax, s.mask, s.noise, w[i].xn, w[i].tokw, s.n1_w, s.n1_b, s.proj_bias,
                               s.n_samples, s.N, s.C, s.k, s.cnum, s.eps_n1, nullptr, w[i].merged_pb, nullptr, s.assign,
                               w[i].qn_hi, w[i].qn_lo};
    }
    return g;
}

NrGroupOf<NrAttnArgs> attn_args(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan& p) {
    NrGroupOf<NrAttnArgs> g;
    g.n = n;
    int blocks = 0;                          // (start[] counts WORKGROUPS: samples, or (sample, pair of heads))
    for (int i = 0; i < n; ++i) {
        const NrCtmStageDesc& s = d[i];
        g.p[i] = NrAttnArgs{w[i].q, w[i].kv, w[i].score, s.N, s.C, s.cnum, s.heads, 1.0f / sqrtf(64.0f), nullptr, w[i].att_hi, w[i].att_lo};
        g.start[i] = blocks;
        blocks += attn_blocks(s, p.attn_form);
    }
    for (int i = n; i <= NR_CTM_MAX_GROUP; ++i) g.start[i] = blocks;
    return g;
}

// ---- the seven launches, by launch index ----
// 0. the token rows as bf16 pairs [rows, C] -- for the problems that do not bring them along (x_hi / x_lo: written by the
//    previous stage's proj GEMM).  The k=3 convolution reads its neighbour rows in place: no shifted copy.
int launch_split(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan& p, hipStream_t st) {
    if (p.split_grid == 0) return NR_OK;
    NrGroupOf<NrShiftArgs> g;
    g.n = 0;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        if (d[i].x_hi) continue;
        g.p[g.n] = NrShiftArgs{d[i].x, d[i].n_samples * d[i].N, d[i].C, w[i].cat_hi, w[i].cat_lo, 1};       // (N = all rows: see the kernel)
        g.start[g.n++] = total;
        total += shift_blocks(d[i]);
    }
    for (int i = g.n; i <= NR_CTM_MAX_GROUP; ++i) g.start[i] = total;
    hipLaunchKernelGGL(nr_group_shift_kernel, dim3(total), dim3(256), 0, st, g);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// 1. y = x + conv(x)  (k=3 convolution as a [B*N, 3C] x [3C, C] product whose A operand is read in place)
int launch_conv(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan&, hipStream_t st) {
    NrLinearArgs p[NR_CTM_MAX_GROUP];
    for (int i = 0; i < n; ++i) {
        p[i] = NrLinearArgs{d[i].x_hi ? d[i].x_hi : w[i].cat_hi, d[i].x_hi ? d[i].x_lo : w[i].cat_lo, d[i].wconv_hi, d[i].wconv_lo,
                            d[i].conv_bias, d[i].x, w[i].y, d[i].n_samples * d[i].N, d[i].C, 3 * d[i].C};
        p[i].conv_n = d[i].N;
    }
    return nr_linear_group_launch(p, n, st, true);
}

// 2. front (LayerNorm, score, exp, norm1, pairwise distances) -- and, fused, back (launch 3 is empty then)
int launch_front(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan& p, hipStream_t st) {
    const NrGroupOf<NrCtmFrontArgs> gf = front_args(d, w, n, p);
    const NrGroupOf<NrCtmBackArgs> gb = back_args(d, w, n, p);
    const bool fused = p.back == NR_CTM_BACK_NONE;
    const dim3 grid(p.samples), block(p.front_threads);
    const size_t lds = p.front_lds;
    const void* k = p.form == 2 ? (!fused  ? (const void*)nr_group_front2_kernel<2, 512>
                                   : p.few ? (const void*)nr_group_front_back2_kernel<2, 256, 4, 8>
                                           : (const void*)nr_group_front_back2_kernel<2, 512, 16, 64>)
                    : fused     ? (p.few ? (const void*)nr_group_front_back_kernel<8, 256> : (const void*)nr_group_front_back_kernel<8>)
                    : p.small   ? (const void*)nr_group_front_kernel<8>
                                : (const void*)nr_group_front_kernel<CF_MAX_CPL, 512>;
    int rc;
    if (p.front_attr && (rc = raise_lds(k, lds)) != NR_OK) return rc;
    if (p.form == 2) {
        if (!fused) hipLaunchKernelGGL((nr_group_front2_kernel<2, 512>), grid, block, lds, st, gf);
        else if (p.few) hipLaunchKernelGGL((nr_group_front_back2_kernel<2, 256, 4, 8>), grid, block, lds, st, gf, gb);
        else hipLaunchKernelGGL((nr_group_front_back2_kernel<2, 512, 16, 64>), grid, block, lds, st, gf, gb);
    } else if (fused) {
        if (p.few) hipLaunchKernelGGL((nr_group_front_back_kernel<8, 256>), grid, block, lds, st, gf, gb);
        else hipLaunchKernelGGL(nr_group_front_back_kernel<8>, grid, block, lds, st, gf, gb);
    } else {
        if (p.small) hipLaunchKernelGGL(nr_group_front_kernel<8>, grid, block, lds, st, gf);
        else hipLaunchKernelGGL((nr_group_front_kernel<CF_MAX_CPL, 512>), grid, block, lds, st, gf);
    }
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// 3. back (DPC-KNN assignment, weighted cluster means, norm1) as a launch of its own, the kv projection beside it where it fits
int launch_back(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan& p, hipStream_t st) {
    if (p.back == NR_CTM_BACK_NONE) return NR_OK;
    const NrGroupOf<NrCtmBackArgs> gb = back_args(d, w, n, p);
    const size_t lds = p.back_lds;
    const int use_lds = p.back_use_lds;
    int rc;
    if (p.back == NR_CTM_BACK_BESIDE_KV) {
        NrLinearArgs kv[NR_CTM_MAX_GROUP];
        kv_problems(d, w, n, kv);
        rc = nr_linear_group_launch_beside_back(kv, n, gb, lds, use_lds, p.back_form, st);
        return rc == NR_EUNSUPPORTED ? NR_EINVAL : rc;      // planned with the launch's own predicate: a refusal is a bug here
    }
    const dim3 grid(p.samples), block(p.back_threads);
    const void* k = p.back_form == 4    ? (const void*)nr_group_back2_kernel<512, 4, 1>
                    : p.back_form == 16 ? (const void*)nr_group_back2_kernel<512, 16, 1>
#ifdef NR_TUNE
                    : p.back_threads == 512 ? (const void*)nr_group_back_kernel<512>
#endif
                                        : (const void*)nr_group_back_kernel<BK_THREADS>;
    if (p.back_attr && (rc = raise_lds(k, lds)) != NR_OK) return rc;
    if (p.back_form == 4) hipLaunchKernelGGL((nr_group_back2_kernel<512, 4, 1>), grid, block, lds, st, gb, use_lds);
    else if (p.back_form == 16) hipLaunchKernelGGL((nr_group_back2_kernel<512, 16, 1>), grid, block, lds, st, gb, use_lds);
#ifdef NR_TUNE
    else if (p.back_threads == 512) hipLaunchKernelGGL(nr_group_back_kernel<512>, grid, block, lds, st, gb, use_lds);
#endif
    else hipLaunchKernelGGL(nr_group_back_kernel<BK_THREADS>, grid, block, lds, st, gb, use_lds);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// 4. q = norm1(merged) Wq^T (+b), and kv = norm1(xn) Wkv^T (+b) unless it rode in launch 3: one grouped launch
int launch_qkv(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan& p, hipStream_t st) {
    NrLinearArgs lp[2 * NR_CTM_MAX_GROUP];
    int np = 0;
    if (p.kv_launch == 4) {
        kv_problems(d, w, n, lp);
        np = n;
    }
    for (int i = 0; i < n; ++i) {
        const NrCtmStageDesc& s = d[i];
        lp[np++] = NrLinearArgs{w[i].qn_hi, w[i].qn_lo, s.wq_hi, s.wq_lo, s.q_bias, nullptr, w[i].q, s.n_samples * s.cnum, s.C, s.C};
    }
    return nr_linear_group_launch(lp, np, st);
}

// 5. score-biased attention of the merged tokens over the un-merged ones
int launch_attention(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan& p, hipStream_t st) {
    const NrGroupOf<NrAttnArgs> g = attn_args(d, w, n, p);
    const dim3 grid(p.attn_grid), block(p.attn_threads);
    const bool by_heads = p.attn_form == NR_CTM_ATTN_HEADS;
    int rc;
    if (p.attn_attr && (rc = raise_lds(by_heads ? (const void*)nr_group_attention_heads_kernel : (const void*)nr_group_attention_kernel, p.attn_lds)) != NR_OK)
        return rc;
    if (by_heads) hipLaunchKernelGGL(nr_group_attention_heads_kernel, grid, block, p.attn_lds, st, g);
    else hipLaunchKernelGGL(nr_group_attention_kernel, grid, block, p.attn_lds, st, g, p.attn_use_lds);
    NR_LAUNCH_CHECK();
    return NR_OK;
}

// 6. out = merged + proj(att) + proj.bias
int launch_proj(const NrCtmStageDesc* d, const StageBuffers* w, int n, const StagePlan&, hipStream_t st) {
    NrLinearArgs p[NR_CTM_MAX_GROUP];
    for (int i = 0; i < n; ++i) {
        p[i] = NrLinearArgs{w[i].att_hi, w[i].att_lo, d[i].wp_hi, d[i].wp_lo, nullptr, w[i].merged_pb, d[i].out,
                            d[i].n_samples * d[i].cnum, d[i].C, d[i].C};
        p[i].out_hi = d[i].out_hi;              // optional: the output also as a bf16 pair (the next stage's x_hi / x_lo)
        p[i].out_lo = d[i].out_lo;
    }
    return nr_linear_group_launch(p, n, st);
}

using StageLaunch = int (*)(const NrCtmStageDesc*, const StageBuffers*, int, const StagePlan&, hipStream_t);
constexpr StageLaunch stage_launches[NR_CTM_STAGE_LAUNCHES] = {launch_split, launch_conv,      launch_front, launch_back,
                                                               launch_qkv,   launch_attention, launch_proj};
}  // namespace

extern "C" int nr_ctm_stage_plan(const NrCtmStageDesc* d, int n, int32_t* plan) {
    if (!plan) return NR_EINVAL;
    const int rc = validate(d, n, false);
    if (rc != NR_OK) return rc;
    const StagePlan p = plan_stage(d, n);
    plan[NR_CTM_PLAN_SAMPLES] = p.samples;
    for (int i = 0; i < NR_CTM_MAX_GROUP; ++i) plan[NR_CTM_PLAN_START + i] = p.start[i];
    plan[NR_CTM_PLAN_SPLIT_GRID] = p.split_grid;
    plan[NR_CTM_PLAN_FUSABLE] = p.fusable;
    plan[NR_CTM_PLAN_FORM] = p.form;
    plan[NR_CTM_PLAN_FRONT_THREADS] = p.front_threads;
    plan[NR_CTM_PLAN_FRONT_LDS] = (int32_t)p.front_lds;
    plan[NR_CTM_PLAN_FRONT_ATTR] = p.front_attr;
    plan[NR_CTM_PLAN_BACK] = p.back;
    plan[NR_CTM_PLAN_BACK_FORM] = p.back_form;
    plan[NR_CTM_PLAN_BACK_THREADS] = p.back_threads;
    plan[NR_CTM_PLAN_BACK_LDS] = (int32_t)p.back_lds;
    plan[NR_CTM_PLAN_BACK_USE_LDS] = p.back_use_lds;
    plan[NR_CTM_PLAN_BACK_ATTR] = p.back_attr;
    plan[NR_CTM_PLAN_KV_LAUNCH] = p.kv_launch;
    plan[NR_CTM_PLAN_ATTN_FORM] = p.attn_form;
    plan[NR_CTM_PLAN_ATTN_GRID] = p.attn_grid;
    plan[NR_CTM_PLAN_ATTN_THREADS] = p.attn_threads;
    plan[NR_CTM_PLAN_ATTN_LDS] = (int32_t)p.attn_lds;
    plan[NR_CTM_PLAN_ATTN_USE_LDS] = p.attn_use_lds;
    plan[NR_CTM_PLAN_ATTN_ATTR] = p.attn_attr;
    return NR_OK;
}

extern "C" int nr_ctm_stage_fwd(const NrCtmStageDesc* d, int n, void* stream) {
    return nr_ctm_stage_fwd_range(d, n, 0, NR_CTM_STAGE_LAUNCHES, stream);
}

// launches [first, last) of the stage's seven: lets the host interleave them with other work in capture order
extern "C" int nr_ctm_stage_fwd_range(const NrCtmStageDesc* d, int n, int first, int last, void* stream) {
    if (first < 0 || last > NR_CTM_STAGE_LAUNCHES || first >= last) return NR_EINVAL;
    int rc = validate(d, n, true);
    if (rc != NR_OK) return rc;
    StageBuffers w[NR_CTM_MAX_GROUP];
    for (int i = 0; i < n; ++i) w[i] = carve(d[i].workspace, d[i].n_samples, d[i].N, d[i].C, d[i].cnum);
    const StagePlan p = plan_stage(d, n);
    for (int i = first; i < last; ++i)
        if ((rc = stage_launches[i](d, w, n, p, (hipStream_t)stream)) != NR_OK) return rc;
    return NR_OK;
}

