// Multi-tensor BertAdam step (DESIGN.md "BertAdam in the captured step"): the trainer's global gradient clip, the optimizer's
// per-tensor clip, the moment update without bias correction, decoupled weight decay, the warm-up schedule and the upper clamp
// of single entries, over a device-resident table of fp32 tensors, in three launches whatever the number of tensors.
//
//   A  sumsq   : sum of g^2 of every (tensor, chunk) pair into the workspace; a chunk is NR_OPT_CHUNK consecutive elements.
//   B  scalars : one workgroup.  Per tensor (one wave each) its chunk sums are added in double, lanes striding over the chunks,
//                then a fixed butterfly; then, one thread per tensor, the global coefficient c (sum over the tensors in table
//                order), the tensor's own coefficient c_t, its scheduled learning rate (double, rounded to fp32 once) and the
//                increment of its step counter.
//   C  update  : the streaming pass over all chunks: read p, g, m, v; write p, m, v (28 bytes per element); 16-byte accesses
//                for p, m, v when all three are aligned (the gradient as one 16-byte or four dword loads), dword accesses else.
//
// A and C use a grid capped at NR_OPT_MAX_GRID workgroups that strides over the chunks; the chunk -> tensor lookup is a binary
// search over the table's chunk prefix (uniform per workgroup: scalar loads).  Nothing depends on a host value that changes
// from step to step, so the same three launches replay from a graph.  nr_bertadam_step_guarded is the same
// three launches with a device-side decision in B: a step whose sum of squared gradients is not finite changes nothing.  No float atomics and no order that depends on which
// workgroup arrives first: a chunk's sum is formed in one fixed order whether its gradient is 16-byte aligned or not, so the
// result does not depend on alignment either.  The gradient buffers are only read.
//
// Weight EMA: e += (1 - d) (p_new - e) per averaged element, d from a device-resident NrEmaState.  Fused form
// (nr_bertadam_step_ema): the owner of the guard in launch B forms (float)(1 - d) and counts the update, launch C averages the
// chunks it is streaming anyway (36 instead of 28 bytes per element).  Stand-alone form (nr_ema_update): a one-thread launch
// for the state, then a streaming launch over a table of (p, shadow) pairs, 12 bytes per element.  nr_ema_swap exchanges the
// contents of p and shadow.  One __device__ function holds the element's arithmetic, so every form and path gives the same bits.
#include "nr_common.h"
#include "../../include/nr_hip.h"

#define NR_OPT_CHUNK 4096          // elements per chunk: 16 per thread of a 256-thread workgroup, four 16-byte accesses per array
#define NR_OPT_MAX_GRID 2048       // 256 CUs x 8 workgroups: memory-bound grid cap
#define NR_OPT_B_THREADS 1024      // launch B: 16 waves

// the table entry that owns chunk `chunk`: the last one whose chunk0 is <= chunk (entries without elements share their
// successor's chunk0 and are never selected)
template <typename Entry>
__device__ __forceinline__ int nr_opt_find(const Entry* __restrict__ table, int T, int chunk) {
    int lo = 0, hi = T;                      // invariant: table[lo].chunk0 <= chunk, answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid].chunk0 <= chunk) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool nr_opt_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- weight EMA: the state's advance (one thread, ever) and the element ---------------------------------------------------------
// d = warmup ? min(decay, (1 + n) / (10 + n)) : decay with n the updates so far, in double; 1 - d rounded to fp32 once
__device__ __forceinline__ void nr_ema_advance(NrEmaState* __restrict__ st) {
    const int64_t n = st->updates;
    double d = st->decay;
    if (st->warmup != 0) {
        const double w = (1.0 + (double)n) / (10.0 + (double)n);
        d = w < d ? w : d;
    }
    st->omd = (float)(1.0 - d);
    st->updates = n + 1;
}

// roundings spelled out, as in nr_opt_update: the vector path, the dword path, the fused and the stand-alone form agree in bits
__device__ __forceinline__ float nr_ema_elem(float omd, float p, float e) { return fmaf(omd, __fsub_rn(p, e), e); }

__device__ __forceinline__ f32x4_t nr_ema_elem4(float omd, const f32x4_t& p, const f32x4_t& e) {
    f32x4_t r;
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = nr_ema_elem(omd, p[q], e[q]);
    return r;
}

// elements 4 i .. 4 i + 3 of a 4-byte aligned array: one 16-byte access, or four dword accesses
__device__ __forceinline__ f32x4_t nr_opt_load4(const float* __restrict__ x, int i, bool vec) {
    if (vec) return reinterpret_cast<const f32x4_t*>(x)[i];
    const float* q = x + 4 * i;
    return f32x4_t{q[0], q[1], q[2], q[3]};
}

__device__ __forceinline__ void nr_opt_store4(float* __restrict__ x, int i, bool vec, const f32x4_t& val) {
    if (vec) {
        reinterpret_cast<f32x4_t*>(x)[i] = val;
    } else {
        float* q = x + 4 * i;
        q[0] = val[0];
        q[1] = val[1];
        q[2] = val[2];
        q[3] = val[3];
    }
}

// ---- launch A ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nr_bertadam_sumsq_kernel(const NrOptimTensor* __restrict__ table, int T, int n_chunks,
                                                               float* __restrict__ part) {
    __shared__ float wave_sum[4];
    const int tid = threadIdx.x;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int t = nr_opt_find(table, T, chunk);
        const long long e0 = (long long)(chunk - table[t].chunk0) * NR_OPT_CHUNK;
        const long long left = table[t].n - e0;
        const int len = left < NR_OPT_CHUNK ? (int)left : NR_OPT_CHUNK;
        const float* g = table[t].g + e0;
        // thread `tid` owns elements 4 (tid + 256 k) + {0, 1, 2, 3}, k = 0 .. 3, and adds them in that order on both paths
        float s = 0.f;
        if (len == NR_OPT_CHUNK && nr_opt_al16(g)) {
            const f32x4_t* g4 = reinterpret_cast<const f32x4_t*>(g);
            f32x4_t x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = g4[tid + 256 * k];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int j = 0; j < 4; ++j) s = fmaf(x[k][j], x[k][j], s);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * (tid + 256 * k) + j;
                    const float x = e < len ? g[e] : 0.f;
                    s = fmaf(x, x, s);
                }
            }
        }
        s = nr_wave_sum(s);
        if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) part[chunk] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
        __syncthreads();
    }
}

// ---- launch B ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double nr_opt_schedule(int id, double x, double warmup) {
    if (x < warmup) return x / warmup;
    if (id == NR_SCHEDULE_WARMUP_COSINE) return 0.5 * (1.0 + cos(3.141592653589793 * x));
    if (id == NR_SCHEDULE_WARMUP_CONSTANT) return 1.0;
    const double y = (x - 1.0) / (warmup - 1.0);
    return y > 0.0 ? y : 0.0;               // warmup_linear
}

// min(1, limit / (norm + 1e-6)) with a NaN coefficient kept (torch.clamp keeps it)
__device__ __forceinline__ double nr_opt_clip(double limit, double norm) {
    const double c = limit / (norm + 1e-6);
    return c > 1.0 ? 1.0 : c;
}

// What the guarded step adds to launch B.  One thread -- the only writer of the guard and of the ring, ever --
// decides, counts and leaves the step's record; launch C reads guard->skip.
struct NrOptGuardArgs {
    NrStepGuard* guard;
    const float* losses;
    int n_losses;
    NrStepRecord* ring;
    int n_ring;
};

template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(NR_OPT_B_THREADS) void nr_bertadam_scalars_kernel(const NrOptimTensor* __restrict__ table, int T,
                                                                              int n_chunks,
                                                                              const NrOptimGroup* __restrict__ groups,
                                                                              float global_max_norm,
                                                                              const float* __restrict__ part,
                                                                              double* __restrict__ tensor_sq,
                                                                              float* __restrict__ scale, float* __restrict__ lr,
                                                                              NrOptGuardArgs ga, NrEmaState* __restrict__ ema_state) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < T; t += NR_OPT_B_THREADS / 64) {
        const int c0 = table[t].chunk0;
        const int c1 = t + 1 < T ? table[t + 1].chunk0 : n_chunks;
        double s = 0.0;
        for (int c = c0 + lane; c < c1; c += 64) s += (double)part[c];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) tensor_sq[t] = s;
    }
    __threadfence_block();
    __syncthreads();
    double c = 1.0, total = 0.0;
    if (GUARDED || global_max_norm > 0.f) {
        for (int t = 0; t < T; ++t) total += tensor_sq[t];          // table order, the same in every thread
        if (global_max_norm > 0.f) c = nr_opt_clip((double)global_max_norm, sqrt(total));
    }
    // the sum of all squares is finite exactly when no gradient entry is NaN or infinite and no chunk sum overflowed fp32
    const bool bad = GUARDED && !(fabs(total) <= 1.79769313486231570815e308);
    if (GUARDED && threadIdx.x == 0) {
        NrStepGuard* gd = ga.guard;
        const int64_t attempt = gd->attempts;
        gd->attempts = attempt + 1;
        if (bad) {
            const int64_t run = gd->consecutive + 1;
            gd->skipped += 1;
            gd->consecutive = run;
            if (run > gd->max_consecutive) gd->max_consecutive = run;
            gd->last_skipped = attempt;
        } else {
            gd->consecutive = 0;
        }
        gd->skip = bad ? 1 : 0;
        NrStepRecord rec;
        rec.attempt = attempt;
        rec.grad_norm = (float)sqrt(total);
        rec.clip = (float)c;
        rec.skipped = bad ? 1 : 0;
        rec.n_losses = ga.n_losses;
#pragma unroll
        for (int i = 0; i < NR_GUARD_MAX_LOSSES; ++i) rec.losses[i] = i < ga.n_losses ? ga.losses[i] : 0.f;
        ga.ring[attempt & (int64_t)(ga.n_ring - 1)] = rec;
    }
    if (bad) return;                                                // no scale, no lr, no counter moves: launch C returns too
    if (EMA && threadIdx.x == 0) nr_ema_advance(ema_state);         // the guard's owner; a bad step has touched nothing of it
    for (int t = threadIdx.x; t < T; t += NR_OPT_B_THREADS) {
        const NrOptimGroup g = groups[table[t].group];
        double ct = 1.0;
        if (g.max_grad_norm > 0.0) ct = nr_opt_clip(g.max_grad_norm, c * sqrt(tensor_sq[t]));
        scale[t] = (float)(c * ct);
        int32_t* step = table[t].step;
        const int32_t st = *step;
        double rate = g.lr;
        if (g.t_total != -1) rate = g.lr * nr_opt_schedule(g.schedule, (double)st / (double)g.t_total, g.warmup);
        lr[t] = (float)rate;
        *step = st + 1;
    }
}

// ---- launch C ---------------------------------------------------------------------------------------------------------------
struct NrOptCoef {
    float scale, b1, omb1, b2, omb2, e, wd, lr, clamp;
    bool decay, clamped;
};

__device__ __forceinline__ void nr_opt_update(const NrOptCoef& k, float& p, float g, float& m, float& v) {
    // roundings and fused multiply-adds spelled out: the vector and the dword path give the same bits
    const float gh = __fmul_rn(g, k.scale);
    m = fmaf(k.b1, m, __fmul_rn(k.omb1, gh));
    v = fmaf(k.b2, v, __fmul_rn(k.omb2, __fmul_rn(gh, gh)));
    float u = m / __fadd_rn(sqrtf(v), k.e);
    if (k.decay) u = fmaf(k.wd, p, u);
    p = fmaf(-k.lr, u, p);
    if (k.clamped) p = p > k.clamp ? k.clamp : p;                   // a NaN parameter stays NaN, as under torch.clamp_
}

__device__ __forceinline__ void nr_opt_update4(const NrOptCoef& k, f32x4_t& p, const f32x4_t& g, f32x4_t& m, f32x4_t& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float xp = p[q], xm = m[q], xv = v[q];
        nr_opt_update(k, xp, g[q], xm, xv);
        p[q] = xp;
        m[q] = xm;
        v[q] = xv;
    }
}

// elements 4 i .. 4 i + 3 of the gradient: one 16-byte load, or four dword loads when the gradient is not 16-byte aligned
__device__ __forceinline__ f32x4_t nr_opt_load_g4(const float* __restrict__ g, int i, bool vec) {
    if (vec) return reinterpret_cast<const f32x4_t*>(g)[i];
    const float* q = g + 4 * i;
    return f32x4_t{q[0], q[1], q[2], q[3]};
}

// GUARDED: one uniform load of the word launch B has just written; a skipped step touches none of p, m, v, g
// EMA: shadows[t] (NULL: tensor t is not averaged) takes nr_ema_elem of the new p with the 1 - d launch B has just written; a
// shadow joins the 16-byte path when it is aligned, and is read and written as four dwords per lane otherwise, like the gradient
template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(256) void nr_bertadam_update_kernel(const NrOptimTensor* __restrict__ table, int T, int n_chunks,
                                                                const NrOptimGroup* __restrict__ groups,
                                                                const float* __restrict__ scale, const float* __restrict__ lr,
                                                                const NrStepGuard* __restrict__ guard,
                                                                float* const* __restrict__ shadows,
                                                                const NrEmaState* __restrict__ ema_state) {
    if (GUARDED) {
        if (guard->skip != 0) return;
    }
    const int tid = threadIdx.x;
    float omd = 0.f;
    if (EMA) omd = ema_state->omd;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int t = nr_opt_find(table, T, chunk);
        const NrOptimTensor ent = table[t];
        const NrOptimGroup grp = groups[ent.group];
        NrOptCoef k;
        k.scale = scale[t];
        k.lr = lr[t];
        k.b1 = (float)grp.b1;
        k.omb1 = (float)(1.0 - grp.b1);
        k.b2 = (float)grp.b2;
        k.omb2 = (float)(1.0 - grp.b2);
        k.e = (float)grp.e;
        k.wd = (float)grp.weight_decay;
        k.decay = grp.weight_decay > 0.0;
        k.clamp = ent.clamp_max;
        k.clamped = ent.has_clamp != 0;
        const long long e0 = (long long)(chunk - ent.chunk0) * NR_OPT_CHUNK;
        const long long left = ent.n - e0;
        const int len = left < NR_OPT_CHUNK ? (int)left : NR_OPT_CHUNK;
        float* p = ent.p + e0;
        const float* g = ent.g + e0;
        float* m = ent.m + e0;
        float* v = ent.v + e0;
        float* sh = nullptr;                                        // this chunk of the tensor's shadow
        if (EMA) {
            sh = shadows[t];
            if (sh) sh += e0;
        }
        // 16-byte accesses for p, m, v when the three are aligned; the gradient joins them when it is aligned too, and is read
        // as four dwords per lane otherwise (the multi-rank step's gradients are views of one flat buffer at any 4-byte offset,
        // while p, m, v come from the allocator): 24 of the 28 bytes per element stay vector accesses
        if (nr_opt_al16(p) && nr_opt_al16(m) && nr_opt_al16(v)) {
            const int n4 = len >> 2;
            const bool g_vec = nr_opt_al16(g);
            const bool s_vec = EMA && nr_opt_al16(sh);
            f32x4_t* p4 = reinterpret_cast<f32x4_t*>(p);
            f32x4_t* m4 = reinterpret_cast<f32x4_t*>(m);
            f32x4_t* v4 = reinterpret_cast<f32x4_t*>(v);
            if (n4 == NR_OPT_CHUNK / 4) {
                f32x4_t xp[4], xg[4], xm[4], xv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = tid + 256 * j;
                    xp[j] = p4[i];
                    xg[j] = nr_opt_load_g4(g, i, g_vec);
                    xm[j] = m4[i];
                    xv[j] = v4[i];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    nr_opt_update4(k, xp[j], xg[j], xm[j], xv[j]);
                    const int i = tid + 256 * j;
                    p4[i] = xp[j];
                    m4[i] = xm[j];
                    v4[i] = xv[j];
                }
                if (EMA && sh) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = tid + 256 * j;
                        nr_opt_store4(sh, i, s_vec, nr_ema_elem4(omd, xp[j], nr_opt_load4(sh, i, s_vec)));
                    }
                }
            } else {
                for (int i = tid; i < n4; i += 256) {
                    f32x4_t xp = p4[i], xm = m4[i], xv = v4[i];
                    const f32x4_t xg = nr_opt_load_g4(g, i, g_vec);
                    nr_opt_update4(k, xp, xg, xm, xv);
                    p4[i] = xp;
                    m4[i] = xm;
                    v4[i] = xv;
                    if (EMA && sh) nr_opt_store4(sh, i, s_vec, nr_ema_elem4(omd, xp, nr_opt_load4(sh, i, s_vec)));
                }
                const int e = 4 * n4 + tid;                        // at most 3 elements left over
                if (e < len) {
                    float xp = p[e], xm = m[e], xv = v[e];
                    nr_opt_update(k, xp, g[e], xm, xv);
                    p[e] = xp;
                    m[e] = xm;
                    v[e] = xv;
                    if (EMA && sh) sh[e] = nr_ema_elem(omd, xp, sh[e]);
                }
            }
        } else {
            for (int e = tid; e < len; e += 256) {
                float xp = p[e], xm = m[e], xv = v[e];
                nr_opt_update(k, xp, g[e], xm, xv);
                p[e] = xp;
                m[e] = xm;
                v[e] = xv;
                if (EMA && sh) sh[e] = nr_ema_elem(omd, xp, sh[e]);
            }
        }
    }
}

// ---- weight EMA, stand-alone ----------------------------------------------------------------------------------------------------
// A launch of its own: no workgroup of the streaming kernel can then read the state after another has changed it
__global__ void nr_ema_state_kernel(NrEmaState* __restrict__ st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) nr_ema_advance(st);
}

// SWAP: exchange the contents of p and shadow (bit-exact, no state); else shadow = nr_ema_elem(omd, p, shadow), p only read
template <bool SWAP>
__global__ __launch_bounds__(256) void nr_ema_stream_kernel(const NrEmaTensor* __restrict__ table, int T, int n_chunks,
                                                           const NrEmaState* __restrict__ st) {
    const int tid = threadIdx.x;
    float omd = 0.f;
    if (!SWAP) omd = st->omd;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int t = nr_opt_find(table, T, chunk);
        const NrEmaTensor ent = table[t];
        const long long e0 = (long long)(chunk - ent.chunk0) * NR_OPT_CHUNK;
        const long long left = ent.n - e0;
        const int len = left < NR_OPT_CHUNK ? (int)left : NR_OPT_CHUNK;
        float* p = ent.p + e0;
        float* sh = ent.ema + e0;
        if (nr_opt_al16(p) && nr_opt_al16(sh)) {
            const int n4 = len >> 2;
            f32x4_t* p4 = reinterpret_cast<f32x4_t*>(p);
            f32x4_t* s4 = reinterpret_cast<f32x4_t*>(sh);
            if (n4 == NR_OPT_CHUNK / 4) {                           // a whole chunk: all eight 16-byte loads in flight at once
                f32x4_t xp[4], xs[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    xp[j] = p4[tid + 256 * j];
                    xs[j] = s4[tid + 256 * j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (SWAP) {
                        p4[tid + 256 * j] = xs[j];
                        s4[tid + 256 * j] = xp[j];
                    } else {
                        s4[tid + 256 * j] = nr_ema_elem4(omd, xp[j], xs[j]);
                    }
                }
                continue;
            }
            for (int i = tid; i < n4; i += 256) {
                const f32x4_t xp = p4[i], xs = s4[i];
                if (SWAP) {
                    p4[i] = xs;
                    s4[i] = xp;
                } else {
                    s4[i] = nr_ema_elem4(omd, xp, xs);
                }
            }
            const int e = 4 * n4 + tid;                            // at most 3 elements left over
            if (e < len) {
                const float xp = p[e], xs = sh[e];
                if (SWAP) {
                    p[e] = xs;
                    sh[e] = xp;
                } else {
                    sh[e] = nr_ema_elem(omd, xp, xs);
                }
            }
        } else {
            for (int e = tid; e < len; e += 256) {
                const float xp = p[e], xs = sh[e];
                if (SWAP) {
                    p[e] = xs;
                    sh[e] = xp;
                } else {
                    sh[e] = nr_ema_elem(omd, xp, xs);
                }
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
extern "C" int nr_bertadam_plan(NrOptimTensor* entries, int T, const NrOptimGroup* groups, int G, int* n_chunks) {
    if (!n_chunks || T < 0 || G < 0 || (T > 0 && (!entries || !groups))) return NR_EINVAL;
    for (int g = 0; g < G; ++g) {
        const NrOptimGroup& q = groups[g];
        if (q.schedule != NR_SCHEDULE_WARMUP_COSINE && q.schedule != NR_SCHEDULE_WARMUP_CONSTANT &&
            q.schedule != NR_SCHEDULE_WARMUP_LINEAR)
            return NR_EINVAL;
        if (q.t_total < -1 || q.t_total == 0) return NR_EINVAL;
    }
    long long chunks = 0;
    for (int t = 0; t < T; ++t) {
        NrOptimTensor& e = entries[t];
        if (e.n < 0 || e.group < 0 || e.group >= G || !e.step) return NR_EINVAL;
        if (e.n > 0 && (!e.p || !e.g || !e.m || !e.v)) return NR_EINVAL;
        if ((((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v | (uintptr_t)e.step) & 3) != 0) return NR_EINVAL;
        e.chunk0 = (int32_t)chunks;
        chunks += (e.n + NR_OPT_CHUNK - 1) / NR_OPT_CHUNK;
        if (chunks > 0x7fffffffLL) return NR_EUNSUPPORTED;
    }
    *n_chunks = (int)chunks;
    return NR_OK;
}

static size_t nr_opt_round256(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" size_t nr_bertadam_workspace_bytes(int T, int n_chunks) {
    if (T <= 0 || n_chunks < 0) return 0;
    // [tensor_sq: T doubles][scale: T floats][lr: T floats][part: n_chunks floats], each section 256-byte aligned
    return nr_opt_round256((size_t)T * sizeof(double)) + 2 * nr_opt_round256((size_t)T * sizeof(float)) +
           nr_opt_round256((size_t)n_chunks * sizeof(float));
}

static int nr_opt_launch(const NrOptimTensor* table, int T, int n_chunks, const NrOptimGroup* groups, float global_max_norm,
                         void* workspace, const NrOptGuardArgs* ga, float* const* ema, NrEmaState* es, void* stream) {
    char* ws = static_cast<char*>(workspace);
    double* tensor_sq = reinterpret_cast<double*>(ws);
    ws += nr_opt_round256((size_t)T * sizeof(double));
    float* scale = reinterpret_cast<float*>(ws);
    ws += nr_opt_round256((size_t)T * sizeof(float));
    float* lr = reinterpret_cast<float*>(ws);
    ws += nr_opt_round256((size_t)T * sizeof(float));
    float* part = reinterpret_cast<float*>(ws);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(n_chunks < NR_OPT_MAX_GRID ? n_chunks : NR_OPT_MAX_GRID);
    if (grid > 0) {
        hipLaunchKernelGGL(nr_bertadam_sumsq_kernel, dim3(grid), dim3(256), 0, st, table, T, n_chunks, part);
        NR_LAUNCH_CHECK();
    }
    const NrOptGuardArgs gargs = ga ? *ga : NrOptGuardArgs{};
    const NrStepGuard* guard = ga ? ga->guard : nullptr;
#define NR_OPT_LAUNCH_B(GUARDED, EMA)                                                                                          \
    hipLaunchKernelGGL((nr_bertadam_scalars_kernel<GUARDED, EMA>), dim3(1), dim3(NR_OPT_B_THREADS), 0, st, table, T, n_chunks, \
                       groups, global_max_norm, part, tensor_sq, scale, lr, gargs, es)
#define NR_OPT_LAUNCH_C(GUARDED, EMA)                                                                                          \
    hipLaunchKernelGGL((nr_bertadam_update_kernel<GUARDED, EMA>), dim3(grid), dim3(256), 0, st, table, T, n_chunks, groups,    \
                       scale, lr, guard, ema, (const NrEmaState*)es)
    if (ga && ema) NR_OPT_LAUNCH_B(true, true);
    else if (ga) NR_OPT_LAUNCH_B(true, false);
    else if (ema) NR_OPT_LAUNCH_B(false, true);
    else NR_OPT_LAUNCH_B(false, false);
    NR_LAUNCH_CHECK();
    if (grid > 0) {
        if (ga && ema) NR_OPT_LAUNCH_C(true, true);
        else if (ga) NR_OPT_LAUNCH_C(true, false);
        else if (ema) NR_OPT_LAUNCH_C(false, true);
        else NR_OPT_LAUNCH_C(false, false);
        NR_LAUNCH_CHECK();
    }
#undef NR_OPT_LAUNCH_B
#undef NR_OPT_LAUNCH_C
    return NR_OK;
}

extern "C" int nr_bertadam_step(const NrOptimTensor* table, int T, int n_chunks, const NrOptimGroup* groups, int G,
                                float global_max_norm, void* workspace, void* stream) {
    if (T < 0 || n_chunks < 0 || G < 0 || global_max_norm != global_max_norm) return NR_EINVAL;
    if (T == 0) return n_chunks == 0 ? NR_OK : NR_EINVAL;
    if (!table || !groups || !workspace || G == 0 || ((uintptr_t)workspace & 7) != 0) return NR_EINVAL;
    return nr_opt_launch(table, T, n_chunks, groups, global_max_norm, workspace, nullptr, nullptr, nullptr, stream);
}

extern "C" int nr_bertadam_step_guarded(const NrOptimTensor* table, int T, int n_chunks, const NrOptimGroup* groups, int G,
                                        float global_max_norm, void* workspace, NrStepGuard* guard, const float* losses,
                                        int n_losses, NrStepRecord* ring, int n_ring, void* stream) {
    if (T < 0 || n_chunks < 0 || G < 0 || global_max_norm != global_max_norm) return NR_EINVAL;
    if (!guard || !ring || ((uintptr_t)guard & 7) != 0 || ((uintptr_t)ring & 7) != 0) return NR_EINVAL;
    if (n_ring < 1 || n_ring > NR_GUARD_MAX_RING || (n_ring & (n_ring - 1)) != 0) return NR_EINVAL;
    if (n_losses < 0 || n_losses > NR_GUARD_MAX_LOSSES || (n_losses > 0 && (!losses || ((uintptr_t)losses & 3) != 0)))
        return NR_EINVAL;
    if (T == 0) return n_chunks == 0 ? NR_OK : NR_EINVAL;            // nothing to update: no launch, not an attempt
    if (!table || !groups || !workspace || G == 0 || ((uintptr_t)workspace & 7) != 0) return NR_EINVAL;
    const NrOptGuardArgs ga{guard, losses, n_losses, ring, n_ring};
    return nr_opt_launch(table, T, n_chunks, groups, global_max_norm, workspace, &ga, nullptr, nullptr, stream);
}

// ---- weight EMA: host -------------------------------------------------------------------------------------------------------------
extern "C" int nr_bertadam_step_ema(const NrOptimTensor* table, int T, int n_chunks, const NrOptimGroup* groups, int G,
                                    float global_max_norm, void* workspace, NrStepGuard* guard, const float* losses, int n_losses,
                                    NrStepRecord* ring, int n_ring, float* const* ema, NrEmaState* state, void* stream) {
    if (T < 0 || n_chunks < 0 || G < 0 || global_max_norm != global_max_norm) return NR_EINVAL;
    if (!ema || !state || ((uintptr_t)ema & 7) != 0 || ((uintptr_t)state & 7) != 0) return NR_EINVAL;
    if (guard) {
        if (!ring || ((uintptr_t)guard & 7) != 0 || ((uintptr_t)ring & 7) != 0) return NR_EINVAL;
        if (n_ring < 1 || n_ring > NR_GUARD_MAX_RING || (n_ring & (n_ring - 1)) != 0) return NR_EINVAL;
        if (n_losses < 0 || n_losses > NR_GUARD_MAX_LOSSES || (n_losses > 0 && (!losses || ((uintptr_t)losses & 3) != 0)))
            return NR_EINVAL;
    }
    if (T == 0) return n_chunks == 0 ? NR_OK : NR_EINVAL;            // nothing to update: no launch, no update counted
    if (!table || !groups || !workspace || G == 0 || ((uintptr_t)workspace & 7) != 0) return NR_EINVAL;
    const NrOptGuardArgs ga{guard, losses, n_losses, ring, n_ring};
    return nr_opt_launch(table, T, n_chunks, groups, global_max_norm, workspace, guard ? &ga : nullptr, ema, state, stream);
}

extern "C" int nr_ema_plan(NrEmaTensor* entries, int T, const NrEmaState* state, int* n_chunks) {
    if (!n_chunks || !state || T < 0 || (T > 0 && !entries)) return NR_EINVAL;
    if (!(state->decay >= 0.0 && state->decay < 1.0) || state->updates < 0) return NR_EINVAL;       // (a NaN decay fails both)
    long long chunks = 0;
    for (int t = 0; t < T; ++t) {
        NrEmaTensor& e = entries[t];
        if (e.n < 0 || (e.n > 0 && (!e.p || !e.ema))) return NR_EINVAL;
        if ((((uintptr_t)e.p | (uintptr_t)e.ema) & 3) != 0) return NR_EINVAL;
        e.chunk0 = (int32_t)chunks;
        chunks += (e.n + NR_OPT_CHUNK - 1) / NR_OPT_CHUNK;
        if (chunks > 0x7fffffffLL) return NR_EUNSUPPORTED;
    }
    *n_chunks = (int)chunks;
    return NR_OK;
}

extern "C" int nr_ema_update(const NrEmaTensor* table, int T, int n_chunks, NrEmaState* state, void* stream) {
    if (T < 0 || n_chunks < 0 || !state || ((uintptr_t)state & 7) != 0) return NR_EINVAL;
    if (T == 0) return n_chunks == 0 ? NR_OK : NR_EINVAL;            // nothing to average: no launch, no update counted
    if (!table || ((uintptr_t)table & 7) != 0) return NR_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nr_ema_state_kernel, dim3(1), dim3(1), 0, st, state);
    NR_LAUNCH_CHECK();
    const unsigned grid = (unsigned)(n_chunks < NR_OPT_MAX_GRID ? n_chunks : NR_OPT_MAX_GRID);
    if (grid > 0) {
        hipLaunchKernelGGL(nr_ema_stream_kernel<false>, dim3(grid), dim3(256), 0, st, table, T, n_chunks, (const NrEmaState*)state);
        NR_LAUNCH_CHECK();
    }
    return NR_OK;
}

extern "C" int nr_ema_swap(const NrEmaTensor* table, int T, int n_chunks, void* stream) {
    if (T < 0 || n_chunks < 0) return NR_EINVAL;
    if (T == 0) return n_chunks == 0 ? NR_OK : NR_EINVAL;
    if (!table || ((uintptr_t)table & 7) != 0) return NR_EINVAL;
    const unsigned grid = (unsigned)(n_chunks < NR_OPT_MAX_GRID ? n_chunks : NR_OPT_MAX_GRID);
    if (grid > 0) {
        hipLaunchKernelGGL(nr_ema_stream_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, T, n_chunks,
                           (const NrEmaState*)nullptr);
        NR_LAUNCH_CHECK();
    }
    return NR_OK;
}
