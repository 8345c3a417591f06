/* nr_hip.h -- C ABI of libnr_hip.so: the MI355X (gfx950) kernels behind NeighborRetr's
 * similarity / neighbour-weighting / loss head.
 *
 * The reference has no FFI layer: its hot path is a sequence of ATen calls inside two Python
 * modules.  Each entry point below replaces one such sequence; the reference
 * lines it stands in for are cited per function (paths relative to the reference checkout).
 * The binding a maintainer adds on the reference side is a ctypes stub -- see INTEGRATION.md.
 *
 * Conventions (all functions):
 *   - plain device pointers + extents, contiguous row-major, no torch types;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised;
 *   - no allocation inside: scratch comes in through `workspace` arguments whose size the
 *     matching *_workspace_bytes() query returns;
 *   - return value: 0 ok, <0 invalid argument / unsupported shape (NR_E*), >0 a hipError_t;
 *   - never throws, never writes outside the buffers named in the signature.
 */
#ifndef NR_HIP_H
#define NR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever a signature or the layout of a descriptor struct changes (2: NrCtmStageDesc gained x_hi/x_lo/out_hi/out_lo in
 * round 3, nr_stream_create / nr_stream_destroy, NrBankAbsorbDesc in round 4; 3: nr_pack_shard_convert); a binding compares nr_version() with the value it was written for */
#define NR_ABI_VERSION 5

/* precision of the MFMA contractions */
#define NR_PREC_BF16 0   /* one bf16 pass (training path)                                   */
#define NR_PREC_BF16X3 1 /* split-bf16, 3 passes: ~fp32 products (eval / rank-parity path)  */
/* (2 is not a contraction precision: it is the host-level mixed plan, neighborretr_amd/head.py PREC_MIXED) */
#define NR_PREC_F16 3    /* one fp16 pass (v_mfma_f32_16x16x32_f16): the `hi` operand pointers hold IEEE fp16 planes (11 significand
                          * bits; the operands are normalised tokens, |x| <= 1, and scorer weights), the `lo` pointers are ignored and
                          * may be NULL.  Accepted by nr_local_level_fwd / nr_local_level_plan (the register kernel's one-pass forms,
                          * picked exactly as NR_PREC_BF16, on the blocks built for it: 96 x 96 at 24 x 12 tokens, 192 x 384, 256 x 256
                          * at 64 x 64 tokens; NR_EUNSUPPORTED, nothing launched, for every other block and where the shape would run
                          * the LDS kernel -- the plan call answers the same), nr_token_logits_fwd / nr_token_weights_fwd / nr_token_weights_fwd_pair / nr_token_scorer_plan
                          * (as one bf16 pass; nr_token_weights_fwd_group refuses it: NR_EUNSUPPORTED, nothing written).  Every
                          * other entry point with a `prec` argument still returns NR_EINVAL for it (ABI 5: an added value).   */

/* what nr_local_level_fwd writes */
#define NR_OUT_FULL 0   /* S[A,Bv]                                                          */
#define NR_OUT_ROWSUM 1 /* partial[n_col_tiles, A]  : sum over the tile's columns (videos)  */
#define NR_OUT_COLSUM 2 /* partial[n_row_tiles, Bv] : sum over the tile's rows (texts)      */

int nr_version(void);
/* sizeof of one of this header's descriptor structs by name ("NrSplitItem", ...; 0: unknown name): lets a foreign-language
 * binding verify its mirror of the layout at load time. */
size_t nr_struct_size(const char* name);

/* Identity of the HIP stream capture `stream` belongs to (0 = not capturing).  No counterpart in the reference (it launches
 * eagerly, trainer.py:84-110); used by neighborretr_amd/capture_guard.py to validate the step's fork / join topology per
 * capture before handing it to the runtime.  Host-only, no launch, no sync. */
int nr_stream_capture_id(void* stream, unsigned long long* id);

/* A new non-blocking HIP stream (hipStreamCreateWithFlags) / its destruction.  No counterpart in the reference.  The host code
 * forks the step's branches onto streams created for ONE graph capture each (neighborretr_amd/streams.py): a stream object
 * that has taken part in an earlier capture is never handed to a later one.  Host-only. */
int nr_stream_create(void** stream);
int nr_stream_destroy(void* stream);

/* F.normalize (eps 1e-12) + mask multiply + bf16 hi/lo split of a token matrix.
 * Replaces modeling.py:495-496 and the two mask einsums :500-501 (a masked token becomes a zero
 * vector, so every product with it is exactly 0, as in the reference).
 *   x [n_tok,d] f32; mask [n_tok] f32 or NULL; normalize: 1 = L2-normalise rows, 0 = keep scale
 *   hi, lo [n_tok,d] bf16 (lo may be NULL); norm [n_tok] f32 = max(||x||,1e-12) (may be NULL);
 *   colsum_part [nr_prepare_parts(n_tok), d] f32 or NULL: per-workgroup column sums of the
 *   UNMASKED normalised rows (feeds compute_centrality_weights, modeling.py:413-424).        */
int nr_prepare_parts(int n_tok);
int nr_prepare_tokens(const float* x, const float* mask, int n_tok, int d, int normalize,
                      uint16_t* hi, uint16_t* lo, float* norm, float* colsum_part, void* stream);

/* nr_prepare_tokens for TWO token matrices of the same width (the batch's text and video tokens) in one launch. */
int nr_prepare_tokens_pair(const float* x0, const float* mask0, int n_tok0, uint16_t* hi0, uint16_t* lo0, float* norm0,
                           float* colsum_part0, const float* x1, const float* mask1, int n_tok1, uint16_t* hi1, uint16_t* lo1,
                           float* norm1, float* colsum_part1, int d, int normalize, void* stream);

/* nr_prepare_tokens / nr_prepare_tokens_pair that ALSO write an fp16 plane f16 [n_tok,d] of the same normalised, masked values
 * (fp32 -> fp16, nearest even), the operand of the NR_PREC_F16 contractions, in the same pass.  f16 may be NULL (then the call is
 * the plain one); hi, norm and the column sums do not depend on it.  (Additions of ABI 5.) */
int nr_prepare_tokens_f16(const float* x, const float* mask, int n_tok, int d, int normalize, uint16_t* hi, uint16_t* lo,
                          uint16_t* f16, float* norm, float* colsum_part, void* stream);
int nr_prepare_tokens_pair_f16(const float* x0, const float* mask0, int n_tok0, uint16_t* hi0, uint16_t* lo0, uint16_t* f16_0,
                               float* norm0, float* colsum_part0, const float* x1, const float* mask1, int n_tok1, uint16_t* hi1,
                               uint16_t* lo1, uint16_t* f16_1, float* norm1, float* colsum_part1, int d, int normalize, void* stream);

/* plain f32 -> bf16 hi/lo split (MLP weight matrices). */
int nr_split_bf16(const float* x, size_t n, uint16_t* hi, uint16_t* lo, void* stream);
/* plain f32 -> fp16 (nearest even): the NR_PREC_F16 image of a scorer's W1.  (Addition of ABI 5.) */
int nr_split_f16(const float* x, size_t n, uint16_t* f16, void* stream);

/* Token-weight MLP, Linear(d,H)+ReLU+Linear(H,1), on the prepared tokens (modeling.py:148-153,
 * called at :485 and :490).  logit_part[p, tok] holds the contribution of hidden units
 * [128p, 128p+128); the H/128 parts are summed by nr_token_softmax.
 *   tok_hi/lo [n_tok,d] normalised tokens, norm [n_tok] their original norms (row scale),
 *   w1_hi/lo [H,d], b1 [H], w2 [H] f32.                                                       */
int nr_token_logits_fwd(const uint16_t* tok_hi, const uint16_t* tok_lo, const float* norm, int n_tok, int d,
                        const uint16_t* w1_hi, const uint16_t* w1_lo, const float* b1, const float* w2, int H,
                        int prec, float* logit_part, void* stream);

/* Backward of the token-weight MLP's hidden layer, fused (the reference's autograd does this in ~10 element-wise launches on
 * [n_tok, H] tensors behind modeling.py:148-153): recomputes h = norm * (tok W1^T) + b1 like nr_token_logits_fwd and writes
 *   dh = (h > 0) * dl[t] * w2 as bf16 pairs -- transposed into dhT [H, ldT] at columns [t0, t0 + n_tok) (the K = tokens operand
 *   of dW1 = dh^T X; columns up to the next multiple of 64, as far as ldT reaches, are written as zeros: the K padding;
 *   t0 % 8 == 0, ldT % 8 == 0; dhT_lo may be NULL when the weight-gradient GEMM is one-pass) and, when dh_hi/lo are given,
 *   row-major [n_tok, H] (operand of dX = dh W1);
 *   dw2_part / db1_part [nr_token_mlp_bwd_part_rows(n_tok, H, prec, hi_only), H] (hi_only: the call passes dhT_lo = dh_hi =
 *   dh_lo = NULL, which lets the large one-pass sets run a bigger block): partial column sums of dl * relu(h) and of dh;
 *   dl_part [the same number of rows] (may be NULL): partial sums of dl (the gradient of the output bias).
 * dl [n_tok] f32 = gradient of the logits (0 on masked tokens).                                                            */
int nr_token_mlp_bwd_row_tiles(int n_tok);
int nr_token_mlp_bwd_part_rows(int n_tok, int H, int prec, int hi_only);
int nr_token_mlp_bwd_hidden(const uint16_t* tok_hi, const uint16_t* tok_lo, const float* norm, int n_tok, int d,
                            const uint16_t* w1_hi, const uint16_t* w1_lo, const float* b1, const float* w2, int H, int prec,
                            const float* dl, uint16_t* dhT_hi, uint16_t* dhT_lo, int ldT, int t0, uint16_t* dh_hi, uint16_t* dh_lo,
                            float* dw2_part, float* db1_part, float* dl_part, void* stream);

/* masked_fill(-9e15) + softmax over the token axis (modeling.py:486-487 / :491-492).
 *   logit_part [n_parts, n_samples*N]; b2 [1] device; mask [n_samples*N] f32 or NULL;
 *   w [n_samples, N] out; logits [n_samples*N] out or NULL (pre-mask logits, kept for backward) */
int nr_token_softmax(const float* logit_part, int n_parts, const float* b2, const float* mask,
                     int n_samples, int N, float* w, float* logits, void* stream);

/* The two calls above in ONE launch: scorer MLP + masked softmax over each sample's tokens (modeling.py:485-487 /
 * :490-492).  The H/BN column blocks of a row tile add to the tile's counter once their partial logits are visible
 * device-wide; the block that arrives last sums the parts, applies mask and softmax for the tile's samples and resets the
 * counter.  counters [n_counters] u32, zero on entry (the kernel leaves them zero), n_counters >= ceil(n_samples*N / 64);
 * launches that may run concurrently need separate counters.  NR_EUNSUPPORTED when no block shape holds whole samples
 * (N must divide 96 or 192, or 64 / 128 -- the caller then issues the two calls above) or N > 256.                        */
int nr_token_weights_fwd(const uint16_t* tok_hi, const uint16_t* tok_lo, const float* norm, int n_samples, int N, int d,
                         const uint16_t* w1_hi, const uint16_t* w1_lo, const float* b1, const float* w2, const float* b2,
                         int H, int prec, const float* mask, float* logit_part, unsigned int* counters, int n_counters,
                         float* w, float* logits, void* stream);

/* Two nr_token_weights_fwd calls of one precision in ONE launch (round 4: the step's text and video tokens, from a few
 * workgroups per CU on: configs[2] / [3]; smaller sets are faster as two launches).  Fields as the arguments of
 * nr_token_weights_fwd; the two problems need separate `counters`.  NR_EUNSUPPORTED when the two do not run the same block
 * shape (the caller issues them one by one then); results are bit-identical to the single calls.                        */
typedef struct NrTokenWeightsProblem {
    const uint16_t *tok_hi, *tok_lo;
    const float* norm;
    const uint16_t *w1_hi, *w1_lo;
    const float *b1, *w2, *b2, *mask;
    float* logit_part;
    unsigned int* counters;
    float *w, *logits;
    int32_t n_samples, N, d, H, n_counters, reserved;
} NrTokenWeightsProblem;
int nr_token_weights_fwd_pair(const NrTokenWeightsProblem* a, const NrTokenWeightsProblem* b, int prec, void* stream);
/* Up to four nr_token_weights_fwd calls -- the four token sets a step scores: batch text / video (modeling.py:485-492 inside
 * local_level :283-287) and bank video / text (the two bank calls, until_module.py:170-185) -- each in its own precision
 * (precs[i]: NR_PREC_*), in ONE launch of 192 x 256 blocks; split-bf16 sets as three accumulated passes.  NR_EUNSUPPORTED
 * when a set does not fit that block (192 % N, H % 256): issue the sets one by one then.  One-pass sets: bit-identical to
 * their single launch; split-bf16 sets: another summation order (~1e-7 relative).                                          */
int nr_token_weights_fwd_group(const NrTokenWeightsProblem* probs, const int* precs, int n, void* stream);
/* The launch form of ONE scorer call, from the host alone (no device): block rows *bm (64 / 96 / 128 / 192), hidden units *bn
 * (128 on 4 waves, 256 on 8) and ring depth *stages (1 or 2) that nr_token_weights_fwd (N_fused = tokens per sample) or
 * nr_token_logits_fwd (N_fused = 0) will run for n_tok tokens -- the launcher's own picker and ring rule, not a copy.
 * NR_EUNSUPPORTED exactly where nr_token_weights_fwd returns it (no block holds whole samples, N_fused > 256); NR_EINVAL for
 * n_tok <= 0, H % 128, an unknown prec, N_fused < 0, n_tok % N_fused, a null pointer.  The outputs are untouched then. */
int nr_token_scorer_plan(int n_tok, int H, int prec, int N_fused, int* bm, int* bn, int* stages);

/* Fused local_level (modeling.py:499-512): token-token cosine products on MFMA, max-pool over
 * each token axis, weighted sums, (t2v+v2t)/2.  The [A,Bv,Nt,Nv] tensor is never materialised.
 *   t_hi/lo [A*Nt,d], v_hi/lo [Bv*Nv,d] prepared tokens; w_t [A*Nt], w_v [Bv*Nv] token weights;
 *   out per out_mode (see NR_OUT_*).  Optional outputs kept for the backward pass (all or none):
 *   arg_v [A,Bv,Nt] / arg_t [A,Bv,Nv] u8 arg-max indices, pmax [A,Bv,Nt] / qmax [A,Bv,Nv] f32 the
 *   pooled maxima themselves.
 * nr_local_level_tiles reports the tile grid the kernel will use for that shape and precision (sizes of
 * the partial outputs).                                                                            */
int nr_local_level_tiles(int A, int Nt, int Bv, int Nv, int prec, int* n_row_tiles, int* n_col_tiles);
int nr_local_level_fwd(const uint16_t* t_hi, const uint16_t* t_lo, const uint16_t* v_hi, const uint16_t* v_lo,
                       const float* w_t, const float* w_v, int A, int Nt, int Bv, int Nv, int d,
                       int prec, int out_mode, float* out, uint8_t* arg_v, uint8_t* arg_t,
                       float* pmax, float* qmax, void* stream);

/* The launch form of ONE nr_local_level_fwd call, from the host alone (no device, no launch): NR_LLP_WORDS ints computed by the
 * launcher's own selection, tile grid, ring rule and LDS budget, not by a copy of them.
 *   [NR_LLP_KERNEL]     NR_LLP_KERNEL_LDS (nr_sim.hip: the block goes through the LDS) or NR_LLP_KERNEL_REG (nr_sim_reg.hip)
 *   [NR_LLP_BLOCK_ROWS], [NR_LLP_BLOCK_COLS]   the MFMA block in tokens;  [NR_LLP_WAVES]  4 or 8
 *   [NR_LLP_STAGES]     ring depth;  [NR_LLP_KLOOP]  NR_KLOOP_PLAIN, NR_KLOOP_PP (ping-pong) or NR_KLOOP_PP3 (split-bf16 as three
 *                       accumulated passes through the ping-pong loop of the one-pass tile)
 *   [NR_LLP_TEXTS], [NR_LLP_VIDEOS]   whole texts x videos per block: the tiling nr_local_level_tiles reports
 *   [NR_LLP_GRID_COLS], [NR_LLP_GRID_ROWS]   blocks along the videos / the texts
 *   [NR_LLP_PAIR_LANES] LDS kernel: lanes per pair in its last phase (1 .. 64); 0 for the register kernel
 * NR_EINVAL / NR_EUNSUPPORTED exactly where nr_local_level_fwd returns them for these arguments (pointer checks aside);
 * `words` is untouched then. */
#define NR_LLP_KERNEL 0
#define NR_LLP_BLOCK_ROWS 1
#define NR_LLP_BLOCK_COLS 2
#define NR_LLP_WAVES 3
#define NR_LLP_STAGES 4
#define NR_LLP_KLOOP 5
#define NR_LLP_TEXTS 6
#define NR_LLP_VIDEOS 7
#define NR_LLP_GRID_COLS 8
#define NR_LLP_GRID_ROWS 9
#define NR_LLP_PAIR_LANES 10
#define NR_LLP_WORDS 11
#define NR_LLP_KERNEL_LDS 0
#define NR_LLP_KERNEL_REG 1
#define NR_KLOOP_PLAIN 0
#define NR_KLOOP_PP 1
#define NR_KLOOP_PP3 2
int nr_local_level_plan(int A, int Nt, int Bv, int Nv, int d, int prec, int32_t* words);

/* Fused local_level (modeling.py:483-514) of CANDIDATE LISTS: the token-level score of chosen (query, gallery item) pairs
 * instead of a whole rectangle -- the second stage of two-stage retrieval.  No counterpart in the reference, which scores
 * every pair (evaluator.py:21-63).
 *   q_hi/lo [n_q*Nq,d], g_hi/lo [n_g*Ng,d] prepared tokens (nr_prepare_tokens; lo: split-bf16 only); w_q [n_q*Nq], w_g [n_g*Ng]
 *   token weights; cand [n_q,C] int32; out [n_q,C] f32: out[i,c] = 0.5 (sum_t w_q max_v + sum_v w_g max_t) of query i and
 *   item cand[i,c].  The formula is symmetric: queries may be texts or videos.  An entry of cand outside [0, n_g) (the
 *   padding -1 included) gives -inf and is never dereferenced; duplicates are allowed; a fully masked query or item gives
 *   exactly 0.  The score of a pair does not depend on its position in the list or on C (identical pairs: identical bits).
 * NR_EINVAL: a null pointer, a count <= 0, d % 64 != 0, C outside [1, 128], an unknown prec, split-bf16 without lo.
 * NR_EUNSUPPORTED: Nq or Ng > 128, d > 1024.  Both before any launch.                                                  */
int nr_local_level_cand(const uint16_t* q_hi, const uint16_t* q_lo, const uint16_t* g_hi, const uint16_t* g_lo,
                        const float* w_q, const float* w_g, int n_q, int Nq, int n_g, int Ng, int d, int prec,
                        const int32_t* cand, int C, float* out, void* stream);

/* Several fused local_level products of ONE step in a single grid (modeling.py:499-512 is called three times per step:
 * batch x batch, :283-287, and the two memory-bank products of until_module.py:170-185): every product as
 * nr_local_level_fwd would compute it, without arg-max outputs, outputs in the same layout.  A CU picks up the next
 * product's block when its previous block retires instead of paying one dispatch + drain per product.
 * nr_local_level_group_kind: >= 0 if a product can join a group (24 x 12 tokens at sizes where the single launch runs the
 * 192 x 384 bf16 or the 96 x 192 split-bf16 blocks), -1 otherwise; nr_local_level_group returns NR_EUNSUPPORTED then
 * (nothing launched: call nr_local_level_fwd per product).  At most 4 products.                                        */
typedef struct NrLocalLevelProblem {
    const uint16_t *t_hi, *t_lo, *v_hi, *v_lo;   /* prepared tokens, as for nr_local_level_fwd (lo: split-bf16 only) */
    const float *w_t, *w_v;                      /* token weights [A*Nt], [Bv*Nv]                                   */
    float* out;                                  /* per out_mode                                                     */
    int A, Nt, Bv, Nv, d, prec, out_mode;
} NrLocalLevelProblem;
int nr_local_level_group_kind(int A, int Nt, int Bv, int Nv, int d, int prec);
int nr_local_level_group(int n, const NrLocalLevelProblem* problems, void* stream);

/* out[i] = scale * sum_p part[p, i]   (memory-bank centrality, until_module.py:181) */
int nr_reduce_parts(const float* part, int n_parts, int n, float scale, float* out, void* stream);

/* C[M,N] = A[M,K] * B[N,K]^T in exact fp32 (v_mfma_f32_16x16x4_f32): the one-global-token case
 * of global_level (modeling.py:526-537), whose logits are un-normalised and feed Sinkhorn. */
int nr_gemm_nt_f32(const float* a, const float* b, int M, int N, int K, float* c, void* stream);

/* compute_centrality_weights (modeling.py:403-430) from the prepared column sums:
 *   w[i] = exp(scale * <g_i/||g_i||, mean_tok>),  mean_tok = sum_p colsum_part[p,:] / n_tok.
 *   g [B,d] f32 global tokens; w [B]; gnorm [B] out or NULL (kept for backward);
 *   mean_out [d] out or NULL.                                                                */
int nr_centrality_weights(const float* g, int B, int d, const float* colsum_part, int n_parts, int n_tok,
                          float scale, float* w, float* gnorm, float* mean_out, void* stream);

/* Same weights for both modalities in one launch, from the finished token means
 * (mean = nr_reduce_parts(colsum_part, 1/n_tok)).  g_text [B, n_g_text, d], g_video [B, n_g_video, d]:
 *   w[i] = mean_g exp(scale * <g_ig/||g_ig||, mean>).
 * n_g = 1 is the reference's expression (modeling.py:403-430).  n_g > 1 (ActivityNet token counts) has no reference
 * answer -- its loss fails to broadcast [B] * [B,n_g] (until_module.py:321); the mean over the global tokens is this
 * build's documented reduction (config.centrality_multi_token = "mean").
 * gnorm_* [B*n_g] and wtok_* [B*n_g] (per-token norms / weights, kept for backward) out or NULL.     */
int nr_centrality_weights_pair(const float* g_text, const float* g_video, int B, int n_g_text, int n_g_video, int d,
                               const float* mean_text, const float* mean_video, float scale, float* w_text,
                               float* w_video, float* gnorm_text, float* gnorm_video, float* wtok_text,
                               float* wtok_video, void* stream);

/* DPC-KNN cluster assignment of every token (cluster.py:453-509; index-only, no gradient):
 *   x [n_samples,N,C] f32 tokens; mask [n_samples,N] f32 (>0 = valid) or NULL; noise [n_samples,N]
 *   f32 in [0,1) (the reference's torch.rand tie-break draw, cluster.py:483); k nearest neighbours for
 *   the density; cluster_num centres; assign [n_samples,N] i64 out (cluster id in [0,cluster_num)).
 *   N <= 64.  workspace: nr_dpc_workspace_bytes(n_samples, N).                                  */
size_t nr_dpc_workspace_bytes(int n_samples, int N);
int nr_dpc_knn_assign(const float* x, const float* mask, const float* noise, int n_samples, int N, int C, int k,
                      int cluster_num, int64_t* assign, void* workspace, void* stream);

/* Forward pieces of one CTM + TCBlock stage (cluster.py:689-717, :834-888, :938-965) between the
 * library GEMMs (no gradient: the training path keeps these ops on autograd):
 *   nr_shift_concat     x [n_samples,N,C] -> out [n_samples*N, 3C] = (x[n-1] | x[n] | x[n+1]), zero at
 *                       the sample borders: the k=3, padding=1 token convolution becomes one GEMM.
 *   nr_ctm_norm_score   y [n_rows,C] (= x + conv) -> xn = LayerNorm(y), score = xn.sc_w + sc_b (masked
 *                       rows -> -inf, cluster.py:703-705), tokw = exp(score), kvn = norm1(xn).
 *   nr_merge_ln         merge_tokens (cluster.py:512-561): merged [n_samples,cnum,C] weighted cluster
 *                       means, merged_pb = merged + proj_b, qn = norm1(merged).
 *   nr_tc_attention     out [n_samples,cnum,C] = softmax_n(q.k/8 + score[n]) v over H heads of 64;
 *                       q [n_samples,cnum,C], kv [n_samples,N,2C] (k | v), score [n_samples,N].     */
int nr_shift_concat(const float* x, int n_samples, int N, int C, float* out, void* stream);
int nr_ctm_norm_score(const float* y, const float* mask, int n_rows, int C, const float* ln_w, const float* ln_b,
                      const float* sc_w, const float* sc_b, const float* n1_w, const float* n1_b, float eps,
                      float* xn, float* kvn, float* score, float* tokw, void* stream);
int nr_merge_ln(const float* xn, const int64_t* assign, const float* tokw, int n_samples, int N, int C, int cnum,
                const float* n1_w, const float* n1_b, const float* proj_b, float eps, float* merged,
                float* merged_pb, float* qn, void* stream);
int nr_tc_attention(const float* q, const float* kv, const float* score, int n_samples, int N, int C, int cnum,
                    int H, float* out, void* stream);

/* Two-launch form of the same stage pieces, one workgroup per sample (what the step actually runs):
 *   nr_ctm_front = nr_ctm_norm_score + the distance half of nr_dpc_knn_assign
 *                  (dist [n_samples,N,N], smax [n_samples] out); norm1(xn) goes either to kvn (f32) or,
 *                  when kvn_hi/kvn_lo are given, straight to the split-bf16 operand of nr_linear_x3;
 *   nr_ctm_back  = the assignment half of nr_dpc_knn_assign + nr_merge_ln (assign may be NULL).   */
int nr_ctm_front(const float* y, const float* mask, int n_samples, int N, int C, const float* ln_w,
                 const float* ln_b, const float* sc_w, const float* sc_b, const float* n1_w, const float* n1_b,
                 float eps, float* xn, float* kvn, uint16_t* kvn_hi, uint16_t* kvn_lo, float* score, float* tokw,
                 float* dist, float* smax, void* stream);
int nr_ctm_back(const float* dist, const float* smax, const float* mask, const float* noise, const float* xn,
                const float* tokw, int n_samples, int N, int C, int k, int cluster_num, const float* n1_w,
                const float* n1_b, const float* proj_b, float eps, float* merged, float* merged_pb, float* qn,
                int64_t* assign, void* stream);

/* ---- one whole clustering stage for a group of problems ------------------------------------------------
 * The step's form of the stage: CTM.forward (cluster.py:689-717) + TCBlock.forward (:938-965) of up to
 * NR_CTM_MAX_GROUP independent problems -- the text and the video tokens of modeling.py:446-481 -- in
 * seven launches that each carry the workgroups of every problem (conv GEMM, front, back, q+kv GEMMs,
 * attention, proj GEMM, preceded by the bf16 split of the token rows; the k=3 convolution reads the neighbour rows in place).  All GEMMs run split-bf16 (see nr_linear_x3); the
 * w*_hi/lo operands are the bf16 pairs (nr_split_bf16) of: the conv kernel as a [C, 3C] matrix with the
 * three taps side by side (tap k multiplies x[n+k-1]), q.weight [C,C], kv.weight [2C,C], proj.weight [C,C].
 * mask may be NULL (stage 1); conv_bias / q_bias / kv_bias may be NULL; assign (int64 [n_samples,N]) may
 * be NULL.  workspace: nr_ctm_stage_workspace_bytes(n_samples, N, C, cnum) bytes, 256-byte aligned,
 * private to the problem.  out [n_samples, cnum, C] f32.
 * Shapes, checked per problem before anything is launched (NR_EINVAL before NR_EUNSUPPORTED): NR_EINVAL for a NULL required
 * pointer, a count <= 0, k or cnum > N, and -- after every problem passed -- x_hi without x_lo; NR_EUNSUPPORTED for N > 64,
 * C % 128 != 0, C > 1024, C != 64 * heads, cnum * C/128 > 192 and N * C * 4 > 150 KB.  What is launched for the shapes that
 * pass is decided once per call by one host function; nr_ctm_stage_plan (below) returns that decision without a device.  */
#define NR_CTM_MAX_GROUP 4
typedef struct NrCtmStageDesc {
    int32_t n_samples, N, C, k, cnum, heads;
    float eps_ctm, eps_n1;
    const float* x;
    const float* mask;
    const float* noise;
    const uint16_t *wconv_hi, *wconv_lo;
    const float* conv_bias;
    const float *ln_w, *ln_b, *sc_w, *sc_b, *n1_w, *n1_b;
    const uint16_t *wq_hi, *wq_lo;
    const float* q_bias;
    const uint16_t *wkv_hi, *wkv_lo;
    const float* kv_bias;
    const uint16_t *wp_hi, *wp_lo;
    const float* proj_bias;
    void* workspace;
    float* out;
    int64_t* assign;
    /* optional (NULL): x as a bf16 pair [n_samples*N, C] (nr_split_bf16 of x) -- the stage then skips its own split launch;
     * out_hi / out_lo [n_samples*cnum, C]: `out` also written as a bf16 pair by the proj GEMM (chain two stages with them). */
    const uint16_t *x_hi, *x_lo;
    uint16_t *out_hi, *out_lo;
} NrCtmStageDesc;
size_t nr_ctm_stage_workspace_bytes(int n_samples, int N, int C, int cluster_num);
/* What the stage leaves in its workspace for a backward pass (neighborretr_amd/cluster_backward.py): byte offsets of
 *   [0] y [n,N,C] conv output + residual (LayerNorm input)   [1] xn [n,N,C] LayerNorm output   [2] score [n,N] (-inf on
 *   masked tokens)   [3] tokw [n,N] = exp(score)   [4] merged_pb [n,cnum,C] cluster means + proj bias   [5] q [n*cnum,C]
 *   [6] kv [n*N,2C]   [7] smax [n]: per-sample maximum pairwise distance, written by the front launch (launch 2 of
 *   nr_ctm_stage_fwd_range) and max-reduced over the samples by the back launch (3): a caller that clusters only a shard of
 *   the batch stores the maximum over ALL shards in smax[0] between the two (cluster.py:473-475 uses the batch-wide
 *   maximum).  All fp32.  offsets: 8 entries.                                                                          */
int nr_ctm_stage_workspace_layout(int n_samples, int N, int C, int cluster_num, size_t* offsets);
int nr_ctm_stage_fwd(const NrCtmStageDesc* problems, int n_problems, void* stream);
/* Launches [first, last) of the stage's NR_CTM_STAGE_LAUNCHES only (0 shift|split, 1 conv GEMM, 2 front, 3 back,
 * 4 q+kv GEMMs, 5 attention, 6 proj GEMM): a host that captures the step into a HIP graph interleaves them with
 * the launches of an independent branch, because the graph starts its nodes in capture order.            */
#define NR_CTM_STAGE_LAUNCHES 7
int nr_ctm_stage_fwd_range(const NrCtmStageDesc* problems, int n_problems, int first, int last, void* stream);
/* What nr_ctm_stage_fwd_range will launch for these problems, from the host alone (no device, no HIP call): the plan the stage
 * itself launches from, not a copy -- every call validates, plans once and then issues the launches [first, last) of that one
 * plan, so a stage driven whole, launch by launch or in two halves runs the same kernels.  Reads the scalar fields of the
 * descriptors and whether mask, x_hi and x_lo are NULL; no other pointer is looked at or required.  NR_EINVAL / NR_EUNSUPPORTED
 * exactly where nr_ctm_stage_fwd_range returns them for shapes (plan is untouched then):
 *   NR_EINVAL        no problems or more than NR_CTM_MAX_GROUP, a count <= 0, k or cnum > N, x_hi without x_lo, plan NULL
 *   NR_EUNSUPPORTED  N > 64, C % 128, C > 1024, C != 64 * heads, cnum * C/128 > 192 merge jobs, N * C * 4 > 150 KB of LDS
 * plan: NR_CTM_PLAN_WORDS integers.  Every launch is a grid of `..._GRID` workgroups of `..._THREADS` threads with `..._LDS`
 * bytes of dynamic LDS (`..._ATTR`: the launch first raises the kernel's dynamic-LDS limit to that size).                  */
#define NR_CTM_PLAN_WORDS 24
enum {
    NR_CTM_PLAN_SAMPLES = 0,       /* samples of all problems: the grid of launches 2 and 3 and of the whole-sample attention    */
    NR_CTM_PLAN_START = 1,         /* [NR_CTM_MAX_GROUP] first sample of every problem (SAMPLES past the last problem)           */
    NR_CTM_PLAN_SPLIT_GRID = 5,    /* launch 0; 0 = no launch (every problem brings x_hi / x_lo)                                 */
    NR_CTM_PLAN_FUSABLE = 6,       /* no problem carries a mask                                                                  */
    NR_CTM_PLAN_FORM = 7,          /* 1 / 2: first or second form of the front and back bodies (second: every C = 512, cnum <= 16) */
    NR_CTM_PLAN_FRONT_THREADS = 8, /* launch 2: the front half alone, or front + back in one kernel when BACK is ..._BACK_NONE    */
    NR_CTM_PLAN_FRONT_LDS = 9,
    NR_CTM_PLAN_FRONT_ATTR = 10,
    NR_CTM_PLAN_BACK = 11,         /* launch 3: NR_CTM_BACK_*                                                                    */
    NR_CTM_PLAN_BACK_FORM = 12,    /* 0 first form; 4 / 16 second form with accumulators for that many clusters                  */
    NR_CTM_PLAN_BACK_THREADS = 13,
    NR_CTM_PLAN_BACK_LDS = 14,     /* of a back workgroup (beside the kv GEMM the grid takes the larger of this and the tile ring) */
    NR_CTM_PLAN_BACK_USE_LDS = 15, /* the back half keeps the sample's token rows in LDS                                         */
    NR_CTM_PLAN_BACK_ATTR = 16,
    NR_CTM_PLAN_KV_LAUNCH = 17,    /* 3: the kv GEMM rides beside the back half; 4: with the q GEMM                               */
    NR_CTM_PLAN_ATTN_FORM = 18,    /* launch 5: NR_CTM_ATTN_*                                                                    */
    NR_CTM_PLAN_ATTN_GRID = 19,
    NR_CTM_PLAN_ATTN_THREADS = 20,
    NR_CTM_PLAN_ATTN_LDS = 21,
    NR_CTM_PLAN_ATTN_USE_LDS = 22, /* whole-sample form: k | v rows in LDS                                                       */
    NR_CTM_PLAN_ATTN_ATTR = 23
};
enum { NR_CTM_BACK_NONE = 0, NR_CTM_BACK_ALONE = 1, NR_CTM_BACK_BESIDE_KV = 2 };
enum { NR_CTM_ATTN_WHOLE = 0, NR_CTM_ATTN_HEADS = 1 };      /* a workgroup per sample / per (sample, pair of heads) */
int nr_ctm_stage_plan(const NrCtmStageDesc* problems, int n_problems, int32_t* plan);

/* As nr_ctm_stage_workspace_layout, plus the split-bf16 operands the forward GEMMs read and the backward's weight-gradient
 * GEMMs need again: [8] kvn_hi [9] kvn_lo  [n*N, C]  norm1(xn);  [10] qn_hi [11] qn_lo  [n*cnum, C]  norm1(merged);
 * [12] att_hi [13] att_lo  [n*cnum, C]  attention output (input of proj).  offsets: 14 entries.                          */
int nr_ctm_stage_workspace_layout2(int n_samples, int N, int C, int cluster_num, size_t* offsets);

/* ---- backward of the clustering stage (no counterpart in the reference: PyTorch autograd differentiates cluster.py:453-561,
 * 689-717, 834-888 op by op; here the hand-derived backward of neighborretr_amd/cluster_backward.py runs as grouped kernels)
 *
 * nr_split_group: up to NR_SPLIT_MAX matrices in ONE launch.  mode 0: f32 src [rows, cols] -> bf16 hi/lo [rows, ld]
 * (ld >= cols, same 64-column tile count; lo may be NULL); mode 1: the same split written TRANSPOSED [cols, ld], ld >= rows,
 * entries [rows, min(ld, rows rounded up to 64)) zero (K padding of a GEMM operand; hi / lo may point INTO a wider buffer of
 * pitch ld at a 64-aligned column); mode 2: a bf16 PAIR src (hi) / src2 (lo) [rows, cols] -> transposed
 * [cols, ld]; mode 3: f32 src [rows, cols] = token rows in samples of `group` tokens -> the transposed k=3 neighbourhood
 * [3 cols, ld]: row 3 c + s holds src[r + s - 1, c] at column r (zero where r + s - 1 leaves the sample of r, and in the K
 * padding) -- the operand that makes the token-convolution weight gradient (cluster.py:664) come out of its GEMM in the
 * parameter's own [C_out, C_in, 3] order; modes 4 / 5: the two matrix forms of a k=3 convolution kernel W [C_out, C_in, 3] read
 * in place, row-major like mode 0 -- 4: dst[o, s C_in + i] = W[o, i, s] (rows C_out, cols 3 C_in, group C_in), 5: dst[i, s C_out + o]
 * = W[o, i, s] (rows C_in, cols 3 C_out, group C_out), 6: as 5 with the taps reversed, dst[i, s C_out + o] = W[o, i, 2 - s] (the
 * kernel of the TRANSPOSED convolution in nr_linear_group's in-place form).  Used for the per-step re-split of every weight matrix and for the K = token-rows
 * operands of the weight-gradient GEMMs.                                                                                   */
#define NR_SPLIT_MAX 48
typedef struct NrSplitItem {
    const void* src;
    const void* src2;
    uint16_t *hi, *lo;
    int32_t rows, cols, mode, ld;
    int32_t group, pad_;                         /* mode 3: tokens per sample; modes 4 / 5: C_in / C_out */
} NrSplitItem;                                   /* 56 bytes */
int nr_split_group(int n, const NrSplitItem* items, void* stream);

/* nr_colsum_group: dst[c] = scale * sum_r src[r, c] for up to NR_COLSUM_MAX f32 matrices in one launch (bias gradients, sums of
 * per-sample partial parameter gradients); fixed summation order.                                                           */
#define NR_COLSUM_MAX 16
typedef struct NrColsumItem {
    const float* src;
    float* dst;
    int32_t rows, cols;
    float scale;       /* dst = scale * column sums */
    int32_t pad_;
} NrColsumItem;
int nr_colsum_group(int n, const NrColsumItem* items, void* stream);

/* nr_linear_group: up to 8 independent problems Y = X W^T (+bias) (+residual) of nr_linear_x3's kind in one launch (every
 * problem tiled with the same block shape; K % 64 == 0 each).
 *   x_lo == w_lo == NULL in EVERY problem: the one-pass bf16 product of the hi halves (a third of the matrix-core work).
 *   ld > 0: X and W are K-slices of wider row-major matrices with row pitch ld elements (ld >= K, ld % 8 == 0) -- how a
 *   weight-gradient GEMM with a long K (token rows) is cut into several problems whose outputs are added afterwards
 *   (nr_slab_sum_group).  ld == 0: the rows are K long.                                                                     */
typedef struct NrLinearProblem {
    const uint16_t *x_hi, *x_lo, *w_hi, *w_lo;
    const float *bias, *residual;
    float* out;
    int32_t M, N, K, ld;
    int32_t conv_n, pad_;                        /* conv_n > 0: X is the token matrix [M, K/3] of samples of conv_n rows and the
                                                    product the k=3 token convolution read in place: sum_s X[r+s-1] W[:, s K/3..]
                                                    (rows outside r's sample read as zeros); every problem of the launch then is */
} NrLinearProblem;                               /* 80 bytes */
int nr_linear_group(int n, const NrLinearProblem* problems, void* stream);
/* nr_linear_plan: which kernel form a launch of these problems runs, as a pure function (host-only, nothing launched; unit-tested
 * without a GPU; pointers are only compared with NULL).  single = 0: nr_linear_group(n, problems); single = 1: nr_linear_x3 of
 * problems[0] (n == 1).  Returns the status the launch would return (validation included); when that is 0, plan[0..5] =
 * MI, NI, STAGES, WC, conv, one_pass: blocks of 32 MI x 16 WC NI outputs on 2 x WC waves, a STAGES-deep ring of 64-wide K slices,
 * conv = 1 the token convolution read in place, one_pass = 1 the product of the hi halves only.                            */
#define NR_LINEAR_PLAN_WORDS 6
int nr_linear_plan(int n, const NrLinearProblem* problems, int single, int32_t* plan);

/* Score-biased attention backward (cluster.py:868-885) per sample for up to NR_CTM_MAX_GROUP problems: from q [n*cnum,C],
 * kv [n*N,2C] (k | v), score [n,N] and d_att [n*cnum,C] (gradient of the attention output, = upstream x proj.weight) to
 * d_q [n*cnum,C], d_kv [n*N,2C] (both also as bf16 pairs, operands of the next GEMMs) and d_score [n,N] (the gradient
 * reaching the token scores through the attention bias).  N <= 64, C == 64 * heads, heads <= 16.                           */
typedef struct NrCtmAttnBwdDesc {
    int32_t n_samples, N, C, cnum, heads;
    const float *q, *kv, *score, *d_att;
    float *d_q, *d_kv, *d_score;
    uint16_t *dq_hi, *dq_lo, *dkv_hi, *dkv_lo;
} NrCtmAttnBwdDesc;
int nr_ctm_attn_bwd(int n, const NrCtmAttnBwdDesc* problems, void* stream);

/* The middle of the stage, backward, per sample: norm1 backward of the merged rows (d_qn) and of the token rows (d_kvn),
 * the block's residual (g), weighted cluster means (cluster.py:536-556; cluster ids `assign` carry no gradient), score / exp
 * (masked tokens: zero), LayerNorm(ctm) backward.  Writes d_y [n*N,C] (gradient of the conv output), the same as a bf16 pair
 * dy_hi / dy_lo [n*N,C] -- the A operand of the transposed token convolution, which nr_linear_group reads in place
 * (conv_n) -- and partial [n,6,C]: per-sample sums of d norm1.weight, d norm1.bias, d ctm.norm.weight, d ctm.norm.bias,
 * d score.weight, and d score.bias in [.,5,0].  merged_pb = cluster means + proj bias (what the forward keeps).            */
typedef struct NrCtmMidBwdDesc {
    int32_t n_samples, N, C, cnum;
    float eps_ctm, eps_n1;
    const float *d_qn, *d_kvn, *g, *merged_pb, *proj_b, *xn, *y, *tokw, *d_score, *mask, *n1_w, *ln_w, *sc_w;
    const int64_t* assign;
    float* d_y;
    uint16_t *dy_hi, *dy_lo;
    float* partial;
} NrCtmMidBwdDesc;
int nr_ctm_mid_bwd(int n, const NrCtmMidBwdDesc* problems, void* stream);

/* Y[M,N] = X[M,K] W[N,K]^T (+ bias[N]) (+ residual[M,N]) in split-bf16 on the MFMA tile engine: the big
 * fp32 GEMMs of the clustering stage (token convolution cluster.py:664, kv projection :866).
 * x_hi/x_lo [M,K], w_hi/w_lo [N,K] bf16 pairs; out [M,N] f32; K % 64 == 0.
 * nr_shift_concat_split = nr_shift_concat writing the bf16 pair directly.                        */
int nr_linear_x3(const uint16_t* x_hi, const uint16_t* x_lo, const uint16_t* w_hi, const uint16_t* w_lo,
                 const float* bias, const float* residual, int M, int N, int K, float* out, void* stream);
int nr_shift_concat_split(const float* x, int n_samples, int N, int C, uint16_t* hi, uint16_t* lo, void* stream);

/* Log-domain Sinkhorn targets, both directions in one launch (until_module.py:235-266):
 *   tgt_rows = beta*Q(G) + (1-beta)*I,  tgt_cols = beta*Q(G^T) + (1-beta)*I  (each [B,B],
 *   tgt_cols indexed in the transposed frame).  workspace: nr_sinkhorn_workspace_bytes(B).    */
size_t nr_sinkhorn_workspace_bytes(int B);
/* 128 < B <= 1024, B % 64 == 0: nr_sinkhorn_targets runs ONE launch whose B/32 workgroups per direction meet at counter
 * barriers, which needs them resident together.  nr_sinkhorn_cooperative_ok(B): 1 if the current device can hold them (kernel
 * occupancy x CUs of one XCD >= B/32) -- else, and for every other B > 128, the multi-launch form (2 iters + 3 launches) runs.
 * nr_sinkhorn_cooperative_gate: the same decision as a pure function (host-only; unit-tested without a GPU).
 * nr_sinkhorn_targets_multilaunch: the fallback form on its own (B > 128).  Should residency fail at run time all the same,
 * every spin is bounded and BOTH targets come back as NaN in full. */
int nr_sinkhorn_cooperative_ok(int B);
int nr_sinkhorn_cooperative_gate(int B, int blocks_per_cu, int n_cus, int n_xcd);
int nr_sinkhorn_targets_multilaunch(const float* G, int B, float beta, int iters, float* tgt_rows, float* tgt_cols,
                                    void* workspace, void* stream);
int nr_sinkhorn_targets(const float* G, int B, float beta, int iters, float* tgt_rows, float* tgt_cols,
                        void* workspace, void* stream);
/* The same solve emitting the uniform-regularisation ROW TERMS directly (until_module.py:285-289 on those targets):
 *   uniform_rows[dir][i] = -sum_j tgt_ij (T X_ij - LSE_j(T X_ij)),  X = G (dir 0) / G^T (dir 1)   (direction dir at
 * uniform_rows + dir * uniform_dir_stride);
 * write them as rows 1 of rowloss [2,4,B] (uniform_rows = rowloss + B, uniform_dir_stride = 4B) and run
 * nr_row_losses_fwd_no_uniform for the other terms BESIDE this launch.  tgt_rows / tgt_cols may both be NULL.
 * B <= 128, B % 4 == 0 (NR_EUNSUPPORTED otherwise: use nr_sinkhorn_targets + nr_row_losses_fwd).            */
int nr_sinkhorn_uniform_rows(const float* G, int B, float beta, int iters, float temperature, float* uniform_rows,
                             int uniform_dir_stride, float* tgt_rows, float* tgt_cols, void* workspace, void* stream);

/* Row-wise fused losses, both directions (until_module.py:303-328 centrality, :161-211 neighbour,
 * :285-289 uniform CE, :351-357 KL; orchestration modeling.py:329-401).  One wave per
 * (row, direction); direction 1 works on the transposed matrices.
 *   S, G [B,B]; tgt_rows/tgt_cols from nr_sinkhorn_targets; bank_c0 [B] = mean_m local_level(bank_text,
 *   video).T (used by the t2v loss), bank_c1 [B] = mean_m local_level(text, bank_video) (v2t loss);
 *   wc_text / wc_video [B] centrality weights; logit_scale [1] device f32.
 *   rowloss [2,4,B] out (dir, {centrality, uniform, neighbour, kl}, row).
 * nr_loss_finalize reduces rowloss to losses[5] = (total, centrality, uniform, neighbour, kl).  */
int nr_row_losses_fwd(const float* S, const float* G, const float* tgt_rows, const float* tgt_cols,
                      const float* bank_c0, const float* bank_c1, const float* wc_text, const float* wc_video,
                      const float* logit_scale, int B, int K, float temperature, float* rowloss, void* stream);
int nr_loss_finalize(const float* rowloss, int B, float uniform_weight, float neighbor_weight, float kl_weight,
                     float* losses, void* stream);
/* The split tail of the loss-only step as two CONCURRENT launches that finalize themselves (B <= 128, B % 4 == 0):
 *   nr_sinkhorn_uniform_rows_final      Sinkhorn solve + uniform-CE row terms into rowloss[:,1,:]  (2 workgroups)
 *   nr_row_losses_fwd_no_uniform_final  centrality / neighbour / KL row terms into rowloss[:,(0,2,3),:], reading the
 *                                       bank centralities as the PARTIAL sums the fused local_level kernel writes
 *                                       (c0_parts [n_c0,B], c1_parts [n_c1,B], c_j = c_scale * sum_p part[p][j]:
 *                                       until_module.py:181 without a reduction launch)
 * Every workgroup of both launches adds to `counter` (one zero-initialised device word the caller keeps); the one that
 * arrives last -- nr_split_tail_workgroups(B) in all -- reduces rowloss [2,4,B] to losses[5] exactly as
 * nr_loss_finalize does and resets the counter.  Neither launch may be issued without the other.                    */
int nr_split_tail_workgroups(int B);
int nr_sinkhorn_uniform_rows_final(const float* G, int B, float beta, int iters, float temperature, float* rowloss,
                                   uint32_t* counter, float uniform_weight, float neighbor_weight, float kl_weight,
                                   float* losses, void* workspace, void* stream);
int nr_row_losses_fwd_no_uniform_final(const float* S, const float* G, const float* c0_parts, int n_c0,
                                       const float* c1_parts, int n_c1, float c_scale, const float* wc_text,
                                       const float* wc_video, const float* logit_scale, int B, int K, float temperature,
                                       float* rowloss, uint32_t* counter, float uniform_weight, float neighbor_weight,
                                       float kl_weight, float* losses, void* stream);
/* nr_row_losses_fwd_no_uniform_final computing the centrality weights itself (compute_centrality_weights, modeling.py:403-430,
 * ONE global token per sample): g_text / g_video [B,d] global tokens, mean_text / mean_video [d] means of the normalised
 * batch tokens, w_i = exp(centrality_scale * <g_i, mean> / max(|g_i|, 1e-12)) -- the arithmetic of
 * nr_centrality_weights_pair, whose launch this form saves in the loss-only step. */
int nr_row_losses_fwd_no_uniform_final_cw(const float* S, const float* G, const float* c0_parts, int n_c0,
                                          const float* c1_parts, int n_c1, float c_scale, const float* g_text,
                                          const float* g_video, const float* mean_text, const float* mean_video, int d,
                                          float centrality_scale, const float* logit_scale, int B, int K, float temperature,
                                          float* rowloss, uint32_t* counter, float uniform_weight, float neighbor_weight,
                                          float kl_weight, float* losses, void* stream);
/* nr_row_losses_fwd without the uniform term: rowloss[dir][0,2,3][i] only, no dependence on the Sinkhorn targets. */
int nr_row_losses_fwd_no_uniform(const float* S, const float* G, const float* bank_c0, const float* bank_c1,
                                 const float* wc_text, const float* wc_video, const float* logit_scale, int B, int K,
                                 float temperature, float* rowloss, void* stream);

/* Row-slab form of nr_row_losses_fwd for a loss sharded over ranks: the caller owns samples
 * [row0, row0 + n_rows) and holds S_rows = S[row0 : row0+n_rows, :] ([n_rows, B]) and S_cols = S[:, row0 : row0+n_rows]
 * ([B, n_rows]); G, the Sinkhorn targets, the bank centralities and the centrality weights are the full (replicated)
 * ones.  Only the owned rows of rowloss [2,4,B] are written: zero the buffer first, sum it over the ranks
 * (all-reduce), then nr_loss_finalize -- every rank then holds the same five losses.                    */
int nr_row_losses_fwd_slab(const float* S_rows, const float* S_cols, int row0, int n_rows, const float* G,
                           const float* tgt_rows, const float* tgt_cols, const float* bank_c0, const float* bank_c1,
                           const float* wc_text, const float* wc_video, const float* logit_scale, int B, int K,
                           float temperature, float* rowloss, void* stream);

/* Backward of nr_row_losses_fwd_slab (the sharded TRAINING loss, neighborretr_amd/sharded.py): for the rows a rank owns,
 * from upstream g_rowloss [2,4,B] (only the owned rows are read): dS_dir [2,n_rows,B] (direction 0: d S[row0+k, :],
 * direction 1: d S[:, row0+k] as a row), dG_dir [2,n_rows,B] likewise, d_c_rows [2,n_rows,B] (gradient of the bank
 * centrality vector a row's neighbour term read: direction 0 -> bank_c0, 1 -> bank_c1), d_wc / d_ls_rows [2,n_rows].       */
int nr_row_losses_bwd_slab(const float* S_rows, const float* S_cols, int row0, int n_rows, const float* G,
                           const float* tgt_rows, const float* tgt_cols, const float* bank_c0, const float* bank_c1,
                           const float* wc_text, const float* wc_video, const float* logit_scale, int B, int K,
                           float temperature, const float* g_rowloss, float* dS_dir, float* dG_dir, float* d_c_rows,
                           float* d_wc, float* d_ls_rows, void* stream);

/* nr_row_losses_fwd + nr_loss_finalize in one launch: the workgroup that finishes last reduces the row
 * terms (same arithmetic, bit-identical losses).  counter: one zero-initialised device word owned by the
 * caller; the kernel leaves it at zero again.                                                        */
int nr_row_losses_fwd_final(const float* S, const float* G, const float* tgt_rows, const float* tgt_cols,
                            const float* bank_c0, const float* bank_c1, const float* wc_text,
                            const float* wc_video, const float* logit_scale, int B, int K, float temperature,
                            float* rowloss, uint32_t* counter, float uniform_weight, float neighbor_weight,
                            float kl_weight, float* losses, void* stream);

/* Backward of nr_row_losses_fwd: recomputes the row statistics, then differentiates all four
 * terms.  g_rowloss [2,4,B] = d(objective)/d(rowloss) (for the fused objective: the constants of
 * nr_loss_finalize).  Outputs, all in the direction's own frame (direction 1 = transposed):
 *   dS_dir [2,B,B], dG_dir [2,B,B], d_c_rows [2,B,B] (row i's contribution to d bank_c[dir][j];
 *   the caller sums over i), d_wc [2,B], d_ls_rows [2,B] (summed by the caller).               */
int nr_row_losses_bwd(const float* S, const float* G, const float* tgt_rows, const float* tgt_cols,
                      const float* bank_c0, const float* bank_c1, const float* wc_text, const float* wc_video,
                      const float* logit_scale, int B, int K, float temperature, const float* g_rowloss,
                      float* dS_dir, float* dG_dir, float* d_c_rows, float* d_wc, float* d_ls_rows, void* stream);

/* g_rowloss [2,4,B] for nr_row_losses_bwd from the gradients of the five losses nr_loss_finalize returns (device scalars; NULL =
 * that loss has no gradient): coef[term] = (g_total * weight[term] + g_term) * 0.5 / B, the kl term divided by B once more.  One
 * launch in place of a dozen element-wise ones on 5-element tensors at the start of every backward pass.                    */
int nr_rowloss_coef(const float* g_total, const float* g_centrality, const float* g_uniform, const float* g_neighbor,
                    const float* g_kl, float uniform_weight, float neighbor_weight, float kl_weight, int B,
                    float* g_rowloss, void* stream);

/* out[i,j] = a[i,j] + b[j,i]  (folds the direction-1 gradients back into the row-major frame);
 * colsum variant: out[j] = sum_i a[i,j].                                                        */
int nr_add_transposed(const float* a, const float* b, int B, float* out, void* stream);
int nr_colsum(const float* a, int rows, int cols, float* out, void* stream);

/* Backward of nr_local_level_fwd through the stored arg-max indices (max-pool backward = route to
 * the arg-max) for ONE side of the product.
 *   side 0: gradients of the ROW (text) operand: d_x [A*Nt,d], d_w [A*Nt]; one workgroup per text,
 *           looping over the Bv videos.  side 1: the COLUMN (video) operand: d_x [Bv*Nv,d], d_w [Bv*Nv].
 *   dS: upstream gradient; ds_mode 0: dS[A,Bv] full, 1: dS[a,b] = vec[a] (row-mean modes),
 *       2: dS[a,b] = vec[b] (column-mean modes); `ds_scale` multiplies it (1/M for the means).
 *   o_hi/o_lo: prepared tokens of the OTHER operand (lo may be NULL: hi only);
 *   w_self / w_other: token weights of this / the other operand;
 *   d_x may be NULL (weights-only: memory-bank side, whose features get no gradient);
 *   accumulate != 0 adds into d_x / d_w instead of overwriting.
 *   workspace: nr_local_level_bwd_workspace_bytes(...) (chunk partials, reduced in fixed order). */
size_t nr_local_level_bwd_workspace_bytes(int side, int A, int Nt, int Bv, int Nv, int d);
int nr_local_level_bwd(int side, const float* dS, int ds_mode, float ds_scale,
                       const uint16_t* o_hi, const uint16_t* o_lo, const float* w_self, const float* w_other,
                       const uint8_t* arg_v, const uint8_t* arg_t, const float* pmax, const float* qmax,
                       int A, int Nt, int Bv, int Nv, int d, float* d_x, float* d_w, int accumulate,
                       void* workspace, void* stream);

/* The d_x half of nr_local_level_bwd as an MFMA GEMM: 96 x 96 blocks of the (sparse) routing matrix
 *   P[(s,n),(o,m)] = 0.5 dS(s,o) ( w_other[o,m] [scat(s,o,m) == n] + w_self[s,n] [gath(s,o,n) == m] )
 * are generated in LDS from the stored arg-max bytes and multiplied with the other operand's tokens.
 *   oT_hi / oT_lo: the other operand's prepared tokens in the order the kernel reads them (fragment-major, written by
 *   nr_sim_bwd_operand_group; ldk = the tokens they cover, whole slices of 96); oT_lo may be NULL (one pass).
 *   Token counts: multiples of 4 that divide 96 with at most 32 sample pairs per block (24 x 12, 12 x 24, 24 x 24,
 *   16 x 24, 24 x 16), d % 256 == 0 (nr_local_level_bwd_mfma_supported); d_w is not produced --
 *   nr_pool_weight_bwd_group computes it.  workspace: nr_local_level_bwd_mfma_workspace_bytes(...).      */
int nr_local_level_bwd_mfma_supported(int Nt, int Nv, int d);
size_t nr_local_level_bwd_mfma_workspace_bytes(int side, int A, int Nt, int Bv, int Nv, int d);
int nr_local_level_bwd_mfma(int side, const float* dS, int ds_mode, float ds_scale, const uint16_t* oT_hi,
                            const uint16_t* oT_lo, int ldk, const float* w_self, const float* w_other,
                            const uint8_t* arg_v, const uint8_t* arg_t, int A, int Nt, int Bv, int Nv, int d,
                            float* d_x, int accumulate, void* workspace, void* stream);

/* Prepared tokens [n_tok][d] (bf16 hi, optional lo; nr_prepare_tokens) -> fragment-major
 * [slice of 96 tokens][k-step of 32][d / 16][64 lanes][8]: element j of lane (kg, n) of block (slice, ks, dg) is token
 * 96 slice + 32 ks + 8 kg + j, dim 16 dg + n -- one wave load of the backward kernel is then one contiguous KiB.
 * out_hi / out_lo hold ceil(n_tok / 96) * 96 * d elements (tokens past n_tok are written as zeros); out_lo may be NULL.
 * d % 64 == 0, n <= 4 operands per launch.                                                                */
typedef struct NrSimBwdOperand {
    const uint16_t* hi;
    const uint16_t* lo;
    uint16_t* out_hi;
    uint16_t* out_lo;
    int32_t n_tok, d;
} NrSimBwdOperand;                               /* 40 bytes */
int nr_sim_bwd_operand_group(int n, const NrSimBwdOperand* items, void* stream);

/* Several of those products in ONE launch (+ one launch that sums the chunks): the loss step has four -- text and
 * video gradient of the batch x batch product (modeling.py:331) and of the two memory-bank products
 * (modeling.py:339-340).  Items with the same d_x are added together in item order (`accumulate` of the FIRST
 * item of a d_x says whether its previous content is kept).  All items share d and have oT_lo either all set
 * or all NULL.  n <= 4.  Fields as the arguments of nr_local_level_bwd_mfma.                            */
typedef struct NrSimBwdItem {
    const float* dS;
    const uint16_t* oT_hi;
    const uint16_t* oT_lo;
    const float* w_self;
    const float* w_other;
    const uint8_t* arg_v;
    const uint8_t* arg_t;
    float* d_x;
    float ds_scale;
    int32_t side, ds_mode, ldk, A, Nt, Bv, Nv, d, accumulate;
} NrSimBwdItem;                                  /* 104 bytes */
size_t nr_local_level_bwd_group_workspace_bytes(int n, const NrSimBwdItem* items);
int nr_local_level_bwd_group(int n, const NrSimBwdItem* items, void* workspace, size_t workspace_bytes, void* stream);

/* out[i] = (accumulate ? out[i] : 0) + sum over sources k, slabs c < n_slabs[k] of part[k][c * n + i], in that fixed order
 * (bitwise reproducible).  What nr_local_level_bwd_group ends with, exported for the weight-gradient GEMMs that are cut
 * along their long K (token rows) into several nr_linear_group problems.  n % 4 == 0; <= 4 outputs, <= 4 sources each.     */
typedef struct NrSlabSum {
    float* out;
    uint64_t n;
    int32_t accumulate, n_src;
    const float* part[4];
    int32_t n_slabs[4];
} NrSlabSum;                                     /* 72 bytes */
int nr_slab_sum_group(int n, const NrSlabSum* items, void* stream);

/* Gradient of the token weights of the fused product (modeling.py:505-512: the weighted sums of the pooled
 * maxima are linear in the weights):   d_w[s,n] = sum_o 0.5 * ds_scale * dS(s,o) * pooled[s,o,n]
 * summed over up to two products that use the same weights (batch x batch + one bank product).
 *   side 0: s = row sample a, pooled = pmax [A,Bv,N];  side 1: s = column sample b, pooled = qmax [A,Bv,N]
 *   (the arrays nr_local_level_fwd stores with want_arg).  dS / ds_mode / ds_scale as in nr_local_level_bwd.
 *   The sources of a job share the differentiated operand (side 0: same A; side 1: same Bv).  n <= 8 jobs,
 *   one launch, fixed summation order.                                                                */
typedef struct NrPoolWSrc {
    const float* dS;
    const float* pool;
    float ds_scale;
    int32_t ds_mode, A, Bv;
} NrPoolWSrc;                                    /* 32 bytes */
typedef struct NrPoolWJob {
    NrPoolWSrc src[2];
    float* d_w;
    int32_t n_src, side, N, accumulate;
} NrPoolWJob;                                    /* 88 bytes */
int nr_pool_weight_bwd_group(int n, const NrPoolWJob* jobs, void* stream);

/* Backward of F.normalize + mask + the centrality mean (nr_prepare_tokens):
 *   g = mask*d_xn + dmean/n_tok;  dx = (g - xhat <xhat,g>) / ||x||,  xhat = x/||x||.
 *   x [n_tok,d] original features, norm [n_tok], mask [n_tok] or NULL, d_xn [n_tok,d] or NULL,
 *   dmean [d] or NULL.                                                                          */
int nr_normalize_bwd(const float* x, const float* norm, const float* mask, const float* d_xn, const float* dmean,
                     int n_tok, int d, float* dx, void* stream);

/* The short head of the loss backward (everything between nr_row_losses_bwd and the two long chains) in three launches:
 *   nr_rowloss_bwd_finish: dS = dS_dir[0] + dS_dir[1]^T, dG likewise, d_c0 / d_c1 [B] = column sums of d_c_rows[0] / [1],
 *     d_ls [1] = sum of d_ls_rows [2,B]  (fixed order);
 *   nr_centrality_weights_bwd_pair: nr_centrality_weights_bwd for the text and the video global tokens together;
 *   nr_global_logits_bwd: gradient of G = gt gv^T (one global token per sample, modeling.py:333) with the centrality part added:
 *     d_gt [B,d] = dG gv + add_t,  d_gv [B,d] = dG^T gt + add_v   (fp32).                                                  */
int nr_rowloss_bwd_finish(const float* dS_dir, const float* dG_dir, const float* d_c_rows, const float* d_ls_rows, int B,
                          float* dS, float* dG, float* d_c0, float* d_c1, float* d_ls, void* stream);
int nr_centrality_weights_bwd_pair(const float* g_t, const float* gnorm_t, const float* mean_t, const float* w_t, const float* dw_t,
                                   const float* g_v, const float* gnorm_v, const float* mean_v, const float* w_v, const float* dw_v,
                                   int B, int d, float scale, float* dg_t, float* dmean_t, float* dg_v, float* dmean_v, void* stream);
int nr_global_logits_bwd(const float* dG, const float* gt, const float* gv, const float* add_t, const float* add_v, int B, int d,
                         float* d_gt, float* d_gv, void* stream);

/* Backward of nr_token_softmax: dlogit = w * (dw - sum_t w dw) per sample ([n_samples,N]). */
int nr_token_softmax_bwd(const float* w, const float* dw, int n_samples, int N, float* dlogit, void* stream);

/* Backward of nr_centrality_weights:  a_i = dw_i * w_i * scale;
 *   dg_i = a_i * (mean - ghat_i <ghat_i, mean>) / ||g_i||;   dmean = sum_i a_i ghat_i.           */
int nr_centrality_weights_bwd(const float* g, const float* gnorm, const float* mean, const float* w, const float* dw,
                              int B, int d, float scale, float* dg, float* dmean, void* stream);

/* The exchange step's packing (modeling.py:274-280: five all_gathers -> one).  nr_pack_shard copies n <= 8
 * device buffers (srcs / bytes / offsets are HOST arrays) to their offsets inside one packed record;
 * nr_unpack_gathered scatters the [world, record_bytes] all-gather result into n rank-major outputs
 * (dst_k[w*bytes_k + i] = rec_w[offset_k + i]); where u8_to_f32[k] != 0 the piece is bytes_k uint8 values per
 * rank written as fp32 (the masks become the multipliers the kernels read).  One launch each.        */
int nr_pack_shard(int n, const void* const* srcs, const size_t* bytes, const size_t* offsets, void* packed, void* stream);
/* nr_pack_shard with the masks' dtype conversion folded in (the reference gathers its int64 masks as they are,
 * modeling.py:277-278; this build's record carries them as u8): kinds[k] = 0 raw bytes, 1 = int64 elements -> u8,
 * 2 = fp32 elements -> u8 (C truncation, as torch's .to(uint8)); for a converted piece bytes[k] is its ELEMENT count (= the
 * bytes it takes in the record).  kinds == NULL: all raw.  One launch instead of two element-wise ones and the pack. */
int nr_pack_shard_convert(int n, const void* const* srcs, const size_t* bytes, const size_t* offsets, const int* kinds,
                          void* packed, void* stream);
int nr_unpack_gathered(int n, const void* gathered, int world, size_t record_bytes, const size_t* bytes,
                       const size_t* offsets, void* const* dsts, const int* u8_to_f32, void* stream);
/* n <= 12 device-to-device copies (srcs[k] -> dsts[k], bytes[k] each) in one launch.  No counterpart in the reference: the bank
 * copy in front of an overlapped owned step of the step-interleaved job (the prepared shadow, masks and noise counter as the
 * step's loss must see them: neighborretr_amd/modeling.py OwnedSlot). */
int nr_copy_group(int n, const void* const* srcs, void* const* dsts, const size_t* bytes, void* stream);

/* The whole exchange step in one call (SURVEY.md 8b minimum set): nr_pack_shard into `packed` [record_bytes], ONE RCCL
 * all-gather of record_bytes uint8 per rank over xGMI on the caller's communicator (`nccl_comm` = its ncclComm_t),
 * nr_unpack_gathered from `gathered` [world * record_bytes] into the rank-major outputs -- all on `stream`.  RCCL is
 * resolved at run time (the librccl.so.1 already loaded in the process, else the system one): NR_EUNSUPPORTED if there is
 * none, 1000 + ncclResult_t if the collective fails.  The Python host reaches the same collective through
 * torch.distributed (neighborretr_amd/dist.py), whose communicator is not exposed as a raw handle.                      */
int nr_allgather_packed(void* nccl_comm, int world, int n, const void* const* srcs, const size_t* bytes,
                        const size_t* offsets, size_t record_bytes, void* packed, void* gathered, void* const* dsts,
                        const int* u8_to_f32, void* stream);

/* Front of the step in one launch (any part may be switched off with n = 0 / NULL):
 *   out0[i] = (float)mask0[i], out1[i] = (float)mask1[i]   the loader's int64 masks as fp32 multipliers;
 *   logit_scale_exp[0] = exp(logit_scale[0])                modeling.py:289;
 *   noise[0..n_noise) uniform in [0,1)                      the torch.rand draws of cluster.py:483, from a
 *       counter-based generator: rng_state = device uint64[2] {seed, counter}; the kernel advances the
 *       counter, so replays of a captured graph draw fresh numbers;
 *   ring_head (device int32, optional): *ring_head = (*ring_head - ring_advance) mod ring_capacity -- the
 *       memory bank's ring head moves back by the batch this step will push (nr_bank_ring_push reads it).  */
int nr_step_prologue(const int64_t* mask0, int n0, float* out0, const int64_t* mask1, int n1, float* out1,
                     const float* logit_scale, float* logit_scale_exp, uint64_t* rng_state, float* noise,
                     int n_noise, int32_t* ring_head, int ring_advance, int ring_capacity, void* stream);

/* Memory-bank FIFO push (modeling.py:237-249): bank <- cat(batch, bank)[:capacity] done as an
 * in-place shift; rows are `row_bytes` wide.  Requires 0 < n_new; if n_new >= capacity the bank
 * becomes the first `capacity` rows of the batch.  scratch: capacity*row_bytes bytes.          */
int nr_bank_push(void* bank, const void* batch, int capacity, int n_new, size_t row_bytes, void* scratch,
                 void* stream);

/* The same FIFO kept as a ring (logical order L[i] = S[(head+i) mod capacity]): writes the n_new batch
 * rows of up to 12 tensors at rows [head_new, head_new+n_new) mod capacity in one launch.
 * banks / batches / row_bytes are HOST arrays of n_tensors device pointers / row sizes.  head_dev (device
 * int32, optional) overrides head_new: the head then lives on the device, advanced by nr_step_prologue, so that
 * a captured HIP graph pushes to a new place at every replay.                                      */
int nr_bank_ring_push(int n_tensors, void* const* banks, const void* const* batches, const size_t* row_bytes,
                      int capacity, int head_new, const int32_t* head_dev, int n_new, void* stream);

/* A gathered batch straight into the memory bank, ONE launch (step-interleaved multi-rank job: a step whose loss another rank
 * evaluates leaves nothing behind on this rank but the FIFO push of modeling.py:309-310 and the bank's prepared shadow).
 * Reads the RECEIVE buffer of the packed exchange step -- world records of record_bytes bytes, each holding per_rank samples'
 * text tokens f32 [per_rank, Nt, d] at off_text, video tokens at off_video, ids i64 at off_index, masks u8 [per_rank, N] at
 * off_text_mask / off_video_mask (nr_pack_shard's layout) -- and
 *   moves the ring head back by world * per_rank (as nr_step_prologue does) and writes the samples at the new head on:
 *   bank_text [capacity, Nt, d] / bank_video f32, bank_index i64 [capacity], bank_*_mask f32 [capacity, N];
 *   the same rows PREPARED (normalised x mask as bf16 hi / lo + norms: nr_prepare_tokens' arithmetic, bit for bit) into
 *   shadow_* (hi / lo [capacity * N, d], norm [capacity * N]; all six NULL: no shadow kept);
 *   rng_state (optional): the noise stream's step counter advances by one, as a step's nr_step_prologue advances it.
 * counter: nr_bank_absorb_counter_words() zeroed device words (a two-level ticket: one word per group of workgroups, 64 B
 *   apart, and the launch's own), all zero again when the launch ends.
 * world * per_rank >= capacity: the batch's first `capacity` samples become the bank and the head 0 (the reference's
 *   cat(batch, bank)[:capacity], modeling.py:244-249).  d % 256 == 0, d <= 1024. */
typedef struct NrBankAbsorbDesc {
    const void* gathered;
    uint64_t record_bytes, off_text, off_video, off_index, off_text_mask, off_video_mask;
    int32_t world, per_rank, Nt, Nv, d, capacity;
    float *bank_text, *bank_video, *bank_text_mask, *bank_video_mask;
    int64_t* bank_index;
    uint16_t *shadow_text_hi, *shadow_text_lo, *shadow_video_hi, *shadow_video_lo;
    float *shadow_text_norm, *shadow_video_norm;
    int32_t* ring_head;
    uint64_t* rng_state;
    uint32_t* counter;
} NrBankAbsorbDesc;
int nr_bank_absorb_counter_words(void);
int nr_bank_absorb_gathered(const NrBankAbsorbDesc* desc, void* stream);

/* Rank of the diagonal in every row under the reference's tie rule (metrics.py:58-66):
 *   greater[i] = #{j : S[i,j] > S[i,i]},  equal[i] = #{j : S[i,j] == S[i,i]} (includes j=i). */
int nr_diag_ranks(const float* S, int N, int32_t* greater, int32_t* equal, void* stream);

/* Sharded evaluation (evaluator.py:21-63 with the N x N matrix split into row slabs over the ranks; metrics.py:58-66):
 * rank counts from S_slab = S[row0 : row0 + n_rows, :] and the full diagonal diag [N] (gathered by the caller).
 *   greater_rows / equal_rows [n_rows]: text->video counts of the slab's rows (complete);
 *   greater_cols / equal_cols [N]: this slab's PARTIAL video->text counts per column (sum them over the ranks).      */
int nr_slab_ranks(const float* S_slab, int n_rows, int N, int row0, const float* diag, int32_t* greater_rows,
                  int32_t* equal_rows, int32_t* greater_cols, int32_t* equal_cols, void* stream);

/* Multi-sentence retrieval (several captions per video: evaluator.py:114-149,225-262; metrics.py:82-148) from a row slab
 * S_slab = S[row0 : row0 + n_rows, :] of the sentence x video matrix.  group_end [G] (device, int32, increasing): the
 * sentences of video g are the global rows [group_end[g-1], group_end[g]); the last entry is the sentence count and
 * row0 + n_rows must not exceed it (checked by the caller: the array lives on the device).
 *   greater_rows / equal_before_rows [n_rows]: #{j : S[i,j] > S[i,g(i)]} and #{j < g(i) : S[i,j] == S[i,g(i)]}; their sum
 *     is the text->video rank of sentence i (metrics.py:103-106 with a stable sort; NaN scores rank first, as torch.argsort
 *     puts them); greater = -1 marks a sentence whose own score is NaN / infinite: not ranked (metrics.py:108-111);
 *   group_max [G, V]: max over this slab's sentences of video g of S[., j], -inf where the slab has none (NaN scores
 *     ignored): MAX-reduce over the ranks, transpose, and nr_diag_ranks gives the video->text ranks (metrics.py:141-146). */
int nr_group_slab_ranks(const float* S_slab, int n_rows, int V, int row0, const int32_t* group_end, int G,
                        int32_t* greater_rows, int32_t* equal_before_rows, float* group_max, void* stream);

/* Top-k lists for hubness evaluation (k-occurrence, NeighborRetr's project page "Hubness Observation"; the reference has no
 * code for it).  Order of a line: score descending, equal scores by index ascending, -0.0 == +0.0, NaN never selected; a
 * line with fewer than k selectable entries is padded with index -1 / value -inf.  Values are the exact bits of S.
 * 1 <= k <= 128 (else NR_EINVAL before any launch).  Radix select in LDS, no sort; bitwise reproducible.
 *   nr_slab_topk_rows: idx_out / val_out [n_rows, k], one list per row of S_slab [n_rows, N] (indices: columns).
 *   nr_slab_topk_cols: idx_out / val_out [N, k], one list per column over this slab's rows only, indices row0 + i: the
 *     partial lists that nr_topk_merge combines over the ranks. */
int nr_slab_topk_rows(const float* S_slab, int n_rows, int N, int k, int32_t* idx_out, float* val_out, void* stream);
int nr_slab_topk_cols(const float* S_slab, int n_rows, int N, int row0, int k, int32_t* idx_out, float* val_out, void* stream);

/* Merge of n_lists partial lists per item: idx / val [n_lists, n_items, k], each list in the order above with its absent
 * entries (index < 0 or NaN value) last, as the two functions above write them -> idx_out / val_out [n_items, k] in the
 * same order.  Combines column lists of row slabs, or lists of a gallery scored in chunks.  An index found in several lists
 * with equal keys is kept once per list, ordered by list number. */
int nr_topk_merge(int n_lists, const int32_t* idx, const float* val, int n_items, int k, int32_t* idx_out, float* val_out,
                  void* stream);

/* k-occurrence counts of n_q lists idx [n_q, k] over a gallery of n_gallery items: occ[j] = #{q : j in list q},
 * good[j] = #{q : j in list q and gt_begin[q] <= j < gt_end[q]} (int32, zeroed here first).  gt_begin / gt_end [n_q]:
 * query q's ground-truth range (single-sentence sets: [q, q+1); multi-sentence: the group's video, or the video's
 * sentences).  Absent slots (-1) and indices outside the gallery are not counted.  n_q = 0: the zeroed counts. */
int nr_topk_occurrences(const int32_t* idx, int n_q, int k, int n_gallery, const int32_t* gt_begin, const int32_t* gt_end,
                        int32_t* occ, int32_t* good, void* stream);

/* Test-time hubness reduction (IS, DSL, QB-Norm; DESIGN.md "Test-time hubness reduction"; the reference has no code for it,
 * its README and project page compare against it).  Statistics of a line of beta * S, beta finite and > 0 (the product
 * rounded to fp32): (max, sum) with sum = sum of exp(beta x - max) over the non-NaN entries, an entry equal to the max adding
 * exactly 1; lse = max + log(sum), -inf for a line with no entry.  Fixed reduction orders, no float atomics: bitwise
 * reproducible.  n = 0 or L = 0 is allowed; a negative extent, a null pointer, a bad beta or mode: NR_EINVAL before any launch.
 *   nr_hubnorm_row_lse: lse [n] of the rows of S [n, L] (one wave per row).
 *   nr_hubnorm_col_stats: stats [2, L] = (max [L], sum [L]) of the columns of S [n, L]: partial pairs of 64-row blocks in
 *     `workspace` (nr_hubnorm_col_workspace(n, L) bytes, 16-B aligned for the vector path; may be null when n = 0), then
 *     nr_hubnorm_combine in block order.  n = 0: every column (-inf, 0). */
#define NR_HUBNORM_IS 0  /* inverted softmax, in log form: fl(fl(beta s) - c)                                   */
#define NR_HUBNORM_DSL 1 /* dual softmax: s * exp(beta s - c)                                                   */
int nr_hubnorm_row_lse(const float* S, int n, int L, float beta, float* lse, void* stream);
size_t nr_hubnorm_col_workspace(int n, int L);
int nr_hubnorm_col_stats(const float* S, int n, int L, float beta, void* workspace, float* stats, void* stream);

/* Merge of P (max, sum) pairs per item, parts [P, 2, L] (pair p of item c: parts[2p L + c], parts[(2p + 1) L + c]), in
 * index order p = 0, 1, ... -> stats [2, L] and / or lse [L] (either may be null, not both).  Used by nr_hubnorm_col_stats
 * and by the cross-rank merge of gathered column statistics: every rank combines the same bits in rank order. */
int nr_hubnorm_combine(int P, const float* parts, int L, float* stats, float* lse, void* stream);

/* One read of S [n, L] -> T and / or V [n, L] (either may be null, not both).  mode NR_HUBNORM_IS or NR_HUBNORM_DSL.
 *   T[i,j] = f(S[i,j], col_norm[j]) where row_gate[i] != 0, else S[i,j]   (row_gate null: every row; col_norm [L])
 *   V[i,j] = f(S[i,j], row_norm[i]) where col_gate[j] != 0, else S[i,j]   (col_gate null: every column; row_norm [n])
 * is: fl(fl(beta s) - c) without fused multiply-add; dsl: s * expf(beta s - c), the exponent carried to about one rounding. */
int nr_hubnorm_apply(const float* S, int n, int L, float beta, int mode, const float* col_norm, const int32_t* row_gate,
                     float* T, const float* row_norm, const int32_t* col_gate, float* V, void* stream);

/* Query-bank normalisation and re-ranking of CANDIDATE LISTS: the search-time stage of IS / QB-Norm on two-stage retrieval
 * (DESIGN.md "Query-bank normalisation of two-stage retrieval").  The reference has no such path: it has neither candidate
 * lists nor a test-time normalisation.  One launch; fine / cand [n, C] as nr_local_level_cand reads and writes them (the
 * lists in ascending gallery index, so position order is index order); norm [n_gallery] f32 or null, active [n_gallery] int32
 * or null: the gallery's normalisers and activation set, computed once from a query bank.  Per query i:
 *   present   slot p is present iff 0 <= cand[i,p] < n_gallery; an absent slot never forms an address into norm / active,
 *             its out_corr is -inf and it is never selected;
 *   top-1     the present slot with the largest non-NaN fine, ties by lower position, -0.0 == +0.0 (nr_slab_topk_rows' order);
 *   gate      0 when norm is null; 1 when norm is given and active is null (every query); with active: 1 iff a top-1 exists
 *             and active[cand[i,top1]] != 0;
 *   corr      gate = 1: fl(fl(beta fine[i,p]) - norm[cand[i,p]]), no fused multiply-add (NR_HUBNORM_IS); gate = 0: fine[i,p];
 *   output    the top k of corr over the present non-NaN slots, value descending, ties by lower position:
 *             out_idx [n,k] = cand[...], out_val [n,k] = corr[...], missing entries -1 / -inf.
 * out_corr [n,C] and out_gate [n] may be null.  Integer comparisons order the list, no atomics: bitwise reproducible, and a
 * query's output depends on its own line only.
 * NR_EINVAL before any launch: fine, cand, out_idx or out_val null; n, n_gallery or k <= 0; C outside [1, 128]; k > C; active
 * without norm; norm with a beta that is not finite and > 0.                                                            */
int nr_cand_norm_rerank(const float* fine, const int32_t* cand, int n, int C, int n_gallery, const float* norm,
                        const int32_t* active, float beta, int k, int32_t* out_idx, float* out_val, float* out_corr,
                        int32_t* out_gate, void* stream);

/* Inverted-file (IVF) prefilter of two-stage retrieval: the gallery's pooled vectors x [n_items, d] are dealt to
 * n_lists k-means lists and a query scans only the n_probe lists whose centroids it is closest to.  The reference has no such
 * path.  An index is list_offsets [n_lists + 1] int32 (list l = the rows [list_offsets[l], list_offsets[l + 1]), empty lists
 * allowed), list_items [n_items] int32 (the gallery index of every row; ascending inside a list) and rows [n_items, d] =
 * x[list_items].  Device offsets and items are clamped to the index before they form an address.
 *
 * nr_ivf_list_sums (the k-means update): sums [n_lists, d], sums[l] = the members of list l added in list order,
 *   one sequential fp32 addition per component (a float32 loop on the host gives the same bits; an empty list: zeros).  One
 *   workgroup per list, no atomics.  NR_EINVAL before any launch: a null pointer; n_items, n_lists or d <= 0; n_lists > n_items.
 *
 * nr_ivf_scan (the pool scores of a chunk of n queries q [n, d]): probes [n, n_probe] int32 = every query's
 *   lists in probe order (an entry outside [0, n_lists) is an empty list).  The pool of query i = the members of its probed
 *   lists, concatenated in probe order: slot base(i, r) + j holds member j of the list of probe rank r, base = the sizes of the
 *   lists of lower rank.  pool_item [n, stride] int32 = the gallery index, pool_score [n, stride] f32 = q_i . x_item with exactly
 *   the bits nr_gemm_nt_f32 gives that pair (the same K split over four waves, MFMA sequence and combine), pool_len [n] int32 =
 *   the pool's length; slots from pool_len[i] on are not written.  stride >= the sum of the n_probe largest list sizes (slots
 *   past stride are dropped, never written).  The launch is list-major: the caller passes the (query, probe) pairs grouped by
 *   list -- bucket b < n_lists = list b, bucket n_lists = the pairs without a list -- as pair_order [n * n_probe] int32 (pair ids
 *   i * n_probe + r, bucket by bucket, ascending inside a bucket), group_offsets [n_lists + 2] int32 (where each bucket's pairs
 *   start, and their total) and tile_offsets [n_lists + 2] int32 (prefix sums of ceil(bucket size / 16)); one workgroup scores 16
 *   pairs of one bucket against 16 rows of its list.  max_list_size: the host's bound of a list's size (sizes the grid; surplus
 *   workgroups exit).  No float atomics, every output element is written by exactly one workgroup.
 *   NR_EINVAL before any launch: a null pointer; n, n_items, n_lists or d <= 0; n_lists > n_items; d % 16 != 0; n_probe outside
 *   [1, min(n_lists, 128)]; max_list_size outside [0, n_items]; stride < 1.  NR_EUNSUPPORTED: more than 2^31 - 1 query tiles or
 *   a list of more than 16 x 65535 rows.
 *
 * nr_ivf_select (the candidates of every pool line): cand [n, C] int32 = the top C of the pool_len[i] (clamped to
 *   [0, stride]) entries of line i by (score descending, gallery index ascending; -0.0 == +0.0; NaN never taken), emitted in
 *   ASCENDING GALLERY INDEX and padded with -1; score_out [n, C] f32 or null = their scores (the bits of pool_score; -inf at the
 *   padding).  The items of a line must be distinct and >= 0.  One workgroup per line: a radix select on the 64-bit keys
 *   (score key << 32) | ~item; lines of stride <= 16384 keep their keys in LDS, longer ones re-read memory in every pass.  Integer
 *   counts only: bitwise reproducible.  NR_EINVAL before any launch: pool_score, pool_item, pool_len or cand null; n <= 0;
 *   stride < 1; C outside [1, 128].                                                                                          */
int nr_ivf_list_sums(const float* x, const int32_t* list_items, const int32_t* list_offsets, int n_items, int n_lists, int d,
                     float* sums, void* stream);
int nr_ivf_scan(const float* q, int n, const float* rows, const int32_t* list_items, const int32_t* list_offsets, int n_items,
                int n_lists, int d, const int32_t* probes, int n_probe, const int32_t* pair_order, const int32_t* group_offsets,
                const int32_t* tile_offsets, int max_list_size, float* pool_score, int32_t* pool_item, int32_t* pool_len,
                int stride, void* stream);
int nr_ivf_select(const float* pool_score, const int32_t* pool_item, const int32_t* pool_len, int n, int stride, int C,
                  int32_t* cand, float* score_out, void* stream);

/* Test-time Sinkhorn normalisation (DESIGN.md "Test-time Sinkhorn normalisation"): the log-domain iteration of the reference's
 * uniform regularisation (until_module.py:223-266; :248-250 is the order of the two half-steps) on a test similarity slab
 * S [n, L] instead of the batch's logits.  a[i,j] = fl(beta S[i,j]), beta finite and > 0; log_mu [n], log_nu [L]: the log
 * marginals, as vectors; u [n], v [L]: the potentials (start: 0).  Statistics are the (max, sum) pairs of nr_hubnorm_*: NaN
 * entries are skipped, an entry equal to the max adds exactly 1, fixed reduction orders, no float atomics: bitwise reproducible.
 * A line whose LSE is not finite (no entry, only -inf, a +inf entry) gets potential 0.  n = 0 or L = 0 is allowed; a negative
 * extent, a null pointer or a bad beta: NR_EINVAL before any launch.  Each entry point is one launch unless said.
 *   nr_sinknorm_row (until_module.py:249): u[i] = log_mu[i] - LSE_j(fl(a[i,j] + v[j])), one wave per row.
 *   nr_sinknorm_col_stats (until_module.py:250, first part): (max, sum) pairs of fl(a[i,j] + u[i]) down the columns, per block
 *     of 64 rows, into `workspace` (nr_hubnorm_col_workspace(n, L) bytes: [ceil(n / 64), 2, L] floats, 16-B aligned for the
 *     vector path; may be null when n = 0).  stats non-null: a second launch merges them in block order into stats [2, L]
 *     (what a rank contributes to the cross-rank gather; n = 0: every column (-inf, 0)).  stats null: the pairs stay in the
 *     workspace for nr_sinknorm_finish_cols (one rank: no launch in between).
 *   nr_sinknorm_finish_cols (until_module.py:250, second part): v[j] = log_nu[j] - lse of P pairs per column, parts [P, 2, L],
 *     merged in index order (the workspace's blocks, or the gathered ranks' stats in rank order).
 *   nr_sinknorm_apply (until_module.py:253-257, in the log domain): T[i,j] = fl(fl(a[i,j] + u[i]) + v[j]), no fused
 *     multiply-add; one read of S, one write of T.  NaN stays NaN.
 *   nr_sinknorm_row_err: err[i] = |exp(LSE_j(T[i,j]) - log_mu[i]) - 1| with T as nr_sinknorm_apply gives it (not stored), 0 for
 *     a row whose LSE is not finite: how far the rows are from their marginal after the last column half-step. */
int nr_sinknorm_row(const float* S, int n, int L, float beta, const float* v, const float* log_mu, float* u, void* stream);
int nr_sinknorm_col_stats(const float* S, int n, int L, float beta, const float* u, void* workspace, float* stats,
                          void* stream);
int nr_sinknorm_finish_cols(int P, const float* parts, int L, const float* log_nu, float* v, void* stream);
int nr_sinknorm_apply(const float* S, int n, int L, float beta, const float* u, const float* v, float* T, void* stream);
int nr_sinknorm_row_err(const float* S, int n, int L, float beta, const float* u, const float* v, const float* log_mu,
                        float* err, void* stream);

/* Local scaling (CSLS, NICDM, LS; DESIGN.md "Local scaling"; the reference has no code for it, its project page argues from
 * these neighbourhoods): every score of S [n, L] (cosine scale, d = 1 - s the distance) is rescaled by statistics of its row's and
 * its column's top-k lists, as nr_slab_topk_rows / nr_slab_topk_cols / nr_topk_merge write them.  Statistics of a list with c
 * present entries (index >= 0):
 *   mean = fl(fl(sum of the c present values, added one by one in list order starting from the first) / fl(c)),
 *   kth  = the c-th present value;   c = 0: both NaN.  Infinities follow IEEE.
 * Scores, fp32, every operation rounded once (no fused multiply-add), EPS = 2^-20, max(x, .) keeps a NaN x:
 *   csls:  T[i,j] = fl(fl(2 s - mean_row[i]) - mean_col[j])
 *   nicdm: d = max(fl(1 - s), 0), a[i] = max(fl(1 - mean_row[i]), EPS), b[j] = max(fl(1 - mean_col[j]), EPS);
 *          T[i,j] = -fl(d / fl(sqrt(fl(a b))))
 *   ls:    a[i] = max(fl(1 - kth_row[i]), EPS), b[j] likewise;  T[i,j] = -fl(fl(d d) / fl(a b))   (the log of exp(-d^2 / a b))
 * A NaN s gives a NaN T, a NaN statistic a NaN line.  No scratch, no float atomics, bitwise reproducible.  A null pointer, a
 * negative extent, k outside [1, 128] or an unknown mode: NR_EINVAL before any launch; n = 0 or L = 0: NR_OK, no launch.
 *   nr_localscale_stats: lists idx / val [n, k] -> mean [n], kth [n] (one thread per list).
 *   nr_localscale_apply: one read of S, one write of T; row_stat [n] / col_stat [L] are the means (csls, nicdm) or the k-th
 *     values (ls).  16-byte accesses when L % 4 == 0 and S, T, col_stat are 16-byte aligned, a scalar path otherwise. */
#define NR_LOCALSCALE_CSLS 0
#define NR_LOCALSCALE_NICDM 1
#define NR_LOCALSCALE_LS 2
int nr_localscale_stats(const int32_t* idx, const float* val, int n, int k, float* mean, float* kth, void* stream);
int nr_localscale_apply(const float* S, int n, int L, int mode, const float* row_stat, const float* col_stat, float* T,
                        void* stream);

/* Local scaling and re-ranking of CANDIDATE LISTS: the search-time stage of CSLS / NICDM / LS on two-stage retrieval (DESIGN.md
 * "Local scaling of two-stage retrieval"; added at ABI version 5 as nr_cand_norm_rerank was).  The reference has no such path.
 * One launch; fine / cand [n, C] as nr_cand_norm_rerank takes them (the lists in ascending gallery index); g_stat [n_gallery] f32:
 * the gallery items' neighbourhood statistic against a query bank, computed once (the means for csls / nicdm, the k-th values for
 * ls: nr_localscale_stats).  Per query i:
 *   present   slot p is present iff 0 <= cand[i,p] < n_gallery; an absent slot never forms an address into g_stat, its out_corr
 *             is -inf and it is never selected; selectable = present and not NaN; every order is value descending, ties by lower
 *             position, -0.0 == +0.0 (nr_slab_topk_rows' order);
 *   q stat    the top-ls_k list of the selectable RAW scores, c <= ls_k entries: q_mean = fl(fl(sum of the c values, added one
 *             by one in list order starting from the first) / fl(c)), q_kth = the c-th value; c = 0: both NaN -- the statistics of
 *             nr_localscale_stats on that list: the query's neighbourhood in the gallery, taken among its candidates;
 *   corr      T(fine[i,p], row, col) of nr_localscale_apply's formulas (every operation rounded once, no fused multiply-add,
 *             EPS = 2^-20, a NaN statistic gives NaN) with the query's statistic (q_mean; q_kth for ls) and g_stat[cand[i,p]]:
 *             query_is_row = 1: (row, col) = (query, item) -- text queries on a video gallery; 0: (item, query);
 *   output    the top k of corr over the present non-NaN slots: out_idx [n,k] = cand[...], out_val [n,k] = corr[...], missing
 *             entries -1 / -inf.
 * out_corr [n,C] and out_qstat [n,2] = (q_mean, q_kth) may be null.  Integer comparisons order both lists, the sum has one fixed
 * order, no atomics: bitwise reproducible, and a query's output depends on its own line only.
 * NR_EINVAL before any launch: fine, cand, g_stat, out_idx or out_val null; n, n_gallery or k <= 0; C outside [1, 128]; k > C;
 * ls_k outside [1, C]; an unknown mode; query_is_row not 0 or 1.                                                          */
int nr_cand_localscale_rerank(const float* fine, const int32_t* cand, int n, int C, int n_gallery, const float* g_stat, int mode,
                              int ls_k, int query_is_row, int k, int32_t* out_idx, float* out_val, float* out_corr,
                              float* out_qstat, void* stream);

/* Mutual proximity (emp, gauss; DESIGN.md "Mutual proximity"; Schnitzer et al., JMLR 2012; the reference has no code for it): every
 * score s = S[i,j] of S [n, L] becomes the probability that it beats the scores of its row's reference line and of its column's
 * reference line, in the independent form MP_I = P_row P_col.  A line X has c(X) = #{x in X : x is not NaN} entries.
 *   emp:   r2(s, X) = 2 #{x in X : x < s} + #{x in X : x == s}   (IEEE compares: NaN is neither, -0 == +0)
 *          p = fl(fl(r2) / fl(2 c))   (c = 0: 0 / 0 = NaN);   T[i,j] = fl(p_row p_col);   a NaN s gives a NaN T.
 *          Counts are exact integers: a line must hold fewer than 2^23 entries (2 c < 2^24), a longer one is NR_EINVAL.
 *   gauss: mean and population sd (divide by c) of every line over its non-NaN entries, accumulated in fp64 in two passes and a fixed
 *          order, delivered as fp32; c = 0: both NaN; c = 1: sd = 0; infinities follow IEEE (sd NaN).  EPS = 2^-20, max(x, .) keeps
 *          a NaN x, every operation rounded once (no fused multiply-add):
 *          z = fl(fl(s - mean) / max(sd, EPS));   Q(z) = fl(0.5 erfcf(fl(z fl(1 / sqrt 2))))   (the line's upper tail at s)
 *          T[i,j] = -fl(fl(Q_r + Q_c) - fl(Q_r Q_c))   (= MP_I - 1: the same ranking, full relative precision at the top)
 * No scratch, no float atomics, no hand-off between workgroups; the same inputs give the same bits.  A null pointer, a negative extent,
 * `accumulate` outside {0, 1} or a line too long for exact counts: NR_EINVAL before any launch; nothing to do: NR_OK, no launch.
 *   nr_mp_row_counts: r2[i,j] = r2(S[i,j], R[i,:]), R [n, Lr].  One wave per (row, 1024 columns), 16 scores per lane; the reference
 *     row is staged through LDS 1024 floats at a time and read as a broadcast.
 *   nr_mp_col_counts: c2[i,j] (+)= r2(S[i,j], Q[:,j]), Q [m, L]; accumulate 0 overwrites, 1 adds to what is there (the host feeds
 *     the reference rows in blocks; integers: any blocking gives the same result).  Lanes own consecutive columns, a wave 16 rows.
 *     Q may be null when m = 0.
 *   nr_mp_line_counts: row_cnt[i] = c(R[i,:]) and / or col_cnt[j] = c(Q[:,j]) of this slab of Q (either output may be null, not
 *     both; the input of a null output is not read).
 *   nr_mp_emp_apply: one read of S, r2, c2, one write of T.  16-byte accesses when L % 4 == 0 and S, r2, c2, col_cnt, T are
 *     16-byte aligned, a scalar path otherwise.
 *   nr_mp_row_moments: mean [n], sd [n] of the rows of R [n, Lr], one wave per row.
 *   nr_mp_col_moments: parts [3, L] fp64 = (count, mean, M2) of the columns of this slab Q [m, L] (count 0: mean = M2 = 0).
 *   nr_mp_moments_combine: P triples per column, parts [P, 3, L], merged by Chan's update in index order -> mean [L], sd [L]
 *     (every rank combines the same bits in rank order).
 *   nr_mp_gauss_apply: one read of S, one write of T; the alignment rule of nr_mp_emp_apply over S, col_mean, col_sd, T. */
int nr_mp_row_counts(const float* S, int n, int L, const float* R, int Lr, int32_t* r2, void* stream);
int nr_mp_col_counts(const float* S, int n, int L, const float* Q, int m, int32_t* c2, int accumulate, void* stream);
int nr_mp_line_counts(const float* R, int n, int Lr, int32_t* row_cnt, const float* Q, int m, int L, int32_t* col_cnt,
                      void* stream);
int nr_mp_emp_apply(const float* S, int n, int L, const int32_t* r2, const int32_t* c2, const int32_t* row_cnt,
                    const int32_t* col_cnt, float* T, void* stream);
int nr_mp_row_moments(const float* R, int n, int Lr, float* mean, float* sd, void* stream);
int nr_mp_col_moments(const float* Q, int m, int L, double* parts, void* stream);
int nr_mp_moments_combine(int P, const double* parts, int L, float* mean, float* sd, void* stream);
int nr_mp_gauss_apply(const float* S, int n, int L, const float* row_mean, const float* row_sd, const float* col_mean,
                      const float* col_sd, float* T, void* stream);

/* Mutual proximity and re-ranking of CANDIDATE LISTS: the search-time stage of emp / gauss on two-stage retrieval (DESIGN.md
 * "Mutual proximity of two-stage retrieval"; added at ABI version 5 as nr_cand_norm_rerank was).  The reference has no such path.
 * One launch; fine / cand [n, C] as nr_cand_norm_rerank takes them (the lists in ascending gallery index).  Computed once per
 * gallery against a query bank of M items: g_line [n_gallery, M] f32, item-major, item g's M bank scores; g_cnt [n_gallery] i32 =
 * c(g_line[g,:]) (nr_mp_line_counts); g_mean / g_sd [n_gallery] f32 its moments (nr_mp_row_moments, or nr_mp_col_moments +
 * nr_mp_moments_combine).  Per query i:
 *   present   slot p is present iff 0 <= cand[i,p] < n_gallery; an absent slot never forms an address into g_line, g_cnt, g_mean
 *             or g_sd, its out_corr is -inf and it is never selected; selectable = present and not NaN; every order is value
 *             descending, ties by lower position, -0.0 == +0.0 (nr_slab_topk_rows' order);
 *   q line    the selectable slots' RAW scores, c_q of them; q_mean, q_sd = their mean and population sd, accumulated in fp64 in
 *             position order (the sum, then the squared distances from the fp64 mean), delivered as fp32; c_q = 0: both NaN;
 *   corr      with s = fine[i,p], g = cand[i,p], the formulas of nr_mp_emp_apply / nr_mp_gauss_apply (MP_I = P_query P_item; every
 *             operation rounded once, EPS = 2^-20, the same erfcf):
 *             emp:   fl(fl(fl(r2(s, q line)) / fl(2 c_q)) fl(fl(r2(s, g_line[g,:])) / fl(2 g_cnt[g])));  a NaN s gives NaN, an
 *                    item whose line is all NaN 0 / 0 = NaN;
 *             gauss: -fl(fl(Q_q + Q_g) - fl(Q_q Q_g)),  Q_q the upper tail of (q_mean, q_sd) at s, Q_g that of (g_mean[g], g_sd[g]);
 *   output    the top k of corr over the present slots whose corr is not NaN: out_idx [n,k] = cand[...], out_val [n,k] = corr[...],
 *             missing entries -1 / -inf.
 * out_corr [n,C] and out_qstat [n,3] = (fl(c_q), q_mean, q_sd), written in both modes, may be null.  Integer counts and comparisons,
 * the fp64 sums in one fixed order, no atomics: bitwise reproducible, and a query's output depends on its own line only.
 * NR_EINVAL before any launch: fine, cand, out_idx or out_val null; n, n_gallery or k <= 0; C outside [1, 128]; k > C; an unknown
 * mode; emp with g_line or g_cnt null or M outside [1, 2^23); gauss with g_mean or g_sd null (a mode reads its own arrays only). */
#define NR_MUTUALPROX_EMP 0
#define NR_MUTUALPROX_GAUSS 1
int nr_cand_mutualprox_rerank(const float* fine, const int32_t* cand, int n, int C, int n_gallery, int mode, const float* g_line,
                              const int32_t* g_cnt, int M, const float* g_mean, const float* g_sd, int k, int32_t* out_idx,
                              float* out_val, float* out_corr, float* out_qstat, void* stream);

/* Bootstrap of rank statistics (DESIGN.md "Bootstrap confidence intervals"; Efron 1979; the reference has no code for it): n_boot
 * resamples of U units (queries; the videos of a multi-sentence set) drawn with replacement, for V = 1 or 2 rankings over the same
 * units (ranks_b NULL: V = 1, unit_end_b and E_b are ignored).  Ranking v: ranks_v [E_v] int32, 0-based, 0 <= r < 2^30; unit_end_v [U]
 * int32 = index of the LAST entry of unit u (non-decreasing, unit_end_v[U-1] = E_v - 1, the unit before unit 0 ends at -1, a unit
 * may be empty).  Draws are counter-based:  SM64(seed, c) = the (c+1)-th output of SplitMix64 seeded with `seed`,
 *   z = seed + (c + 1) 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) 0x94D049BB133111EB;  z ^= z >> 31
 *   u(b, t) = ((SM64(seed, (b << 32) | t) >> 32) * U) >> 32,   t in [0, U);   both rankings of a call use the same u(b, t).
 * out [n_boot, V, 4 + K] int64, exact integers: for resample b0 + i and ranking v, over the multiset of entries of its U drawn units,
 *   (n, sum, med_lo, med_hi, hits[0..K-1]):  the entry count, the sum of ranks, the order statistics at sorted positions (n-1)/2 and
 *   n/2 (both -1 when n = 0), hits[k] = #{r < cuts[k]}.  cuts [K] is HOST memory: K strictly increasing positive cut-offs.
 * One workgroup per resample; the order statistics by a radix select on the rank value (LDS histograms of 1024 bins, at most three
 * passes), the draws recomputed in every pass.  No global atomics, no scratch: the result depends on (seed, b, inputs) alone, whatever
 * the grid and the split of the resamples over calls.  A resample must hold fewer than 2^32 entries (U times the largest unit < 2^32
 * guarantees it).  NR_EINVAL before any launch: U outside [1, 2^24], K outside [1, 8], cuts not positive and increasing, E < 0,
 * b0 < 0, n_boot < 0, b0 + n_boot > 2^31 - 1, a null required pointer; n_boot = 0: NR_OK, no launch. */
int nr_bootstrap_rank_stats(const int32_t* ranks_a, const int32_t* unit_end_a, int E_a, const int32_t* ranks_b,
                            const int32_t* unit_end_b, int E_b, int U, const int32_t* cuts, int K, uint64_t seed, int b0, int n_boot,
                            int64_t* out, void* stream);

/* Ranks of every relevant (sentence, video) pair from a row slab (DESIGN.md "Rank-aware IR metrics"; the reference has no code for
 * it).  M_slab [n_rows, V] = rows [row0, row0 + n_rows) of the n_total x V matrix being ranked (rows: sentences, columns: videos);
 * group_end [V] DEVICE int32: video g owns the rows [group_end[g-1], group_end[g]) (nr_group_slab_ranks's convention; increasing,
 * group_end[0] > 0, group_end[V-1] = n_total; the kernels stay in bounds whatever it holds, the caller checks it); pair s = (row s, column g(s));
 * own [n_total] DEVICE fp32 = M[s, g(s)], gathered by the caller.  Entry x at index i of a line is AHEAD of pair s when x > own[s], or
 * x == own[s] and i is lower than the pair's own index on that line (IEEE compares: -0.0 == +0.0, a NaN entry is never ahead).  A
 * pair whose own[s] is NaN or infinite is unranked.
 *   row_rank [n_rows]   = entries of row row0 + i ahead of its pair (index: the column, own index g(s)): the complete text->video
 *                         rank, 0-based; -1 when unranked.  May be NULL.
 *   col_ahead [n_total] = THIS SLAB's rows ahead of pair s in column g(s) (index: the global row, own index s); 0 when unranked.
 *                         Overwritten, not accumulated: the sum over the slabs of a split is the video->text rank of sentence s among
 *                         all sentences.  May be NULL.
 * Row side: one wave per row, one pass.  Column side: a workgroup per 64 pairs, own[s] in registers, its four waves stream
 * interleaved rows of column g(s) past it (element stride V) and add their counts in LDS.  Integers only, no atomics, one writer
 * per output: a function of the inputs alone.
 * NR_EINVAL before any launch: a null required pointer, a negative extent, V < 1, row0 + n_rows > n_total.  n_rows = 0: NR_OK,
 * col_ahead is zeroed, M_slab may be NULL. */
int nr_pair_ranks(const float* M_slab, int n_rows, int V, int row0, int n_total, const int32_t* group_end, const float* own,
                  int32_t* row_rank, int32_t* col_ahead, void* stream);

/* Bootstrap of per-unit sums (DESIGN.md "Rank-aware IR metrics"): values [U, Q] int64 row-major, U in [1, 2^24], Q in [1, 16];
 *   out[i, q] = sum over t < U of values[u(b0 + i, t), q],   out [n_boot, Q] int64,
 * with exactly the draws u(b, t) of nr_bootstrap_rank_stats: resample b is the same multiset of units in both entry points.  One
 * workgroup per resample, int64 sums in registers, combined by wave shuffles and through LDS; nothing is stored per resample, no
 * global atomics: the result depends on (seed, b, inputs) alone.  The caller keeps U max|value| below 2^62.  NR_EINVAL before any
 * launch: U or Q out of range, b0 < 0, n_boot < 0, b0 + n_boot > 2^31 - 1, a null pointer; n_boot = 0: NR_OK, no launch. */
int nr_bootstrap_unit_sums(const int64_t* values, int U, int Q, uint64_t seed, int b0, int n_boot, int64_t* out, void* stream);

/* Paired permutation test of rank statistics (DESIGN.md "Paired permutation tests"; Fisher's randomisation test as used for retrieval
 * metrics, Smucker et al. 2007; the reference has no code for it): two rankings A and B over the same U units, with the conventions of
 * nr_bootstrap_rank_stats (ranks_x [E_x] int32, 0 <= r < 2^30; unit_end_x [U] int32 = index of the LAST entry of unit u,
 * non-decreasing, a unit may be empty, E_a != E_b allowed).  Swap bits, counter-based with the SplitMix64 above:
 *   s(p, u) = SM64(seed ^ 0x7065726D74657374, (p << 32) | u) >> 63,   u in [0, U);   the salt keeps the stream apart from the draws of
 *   the bootstrap at equal seeds; the identity labelling is not one of the draws.
 * In permutation p side X takes unit u's entries from A when s = 0 and from B when s = 1; side Y takes the other ranking's entries.
 * out [n_perm, 2, 4 + K] int64, exact integers: for permutation p0 + i and side (X, Y), over the multiset of its entries,
 *   (n, sum, med_lo, med_hi, hits[0..K-1]):  the entry count, the sum of ranks, the order statistics at sorted positions (n-1)/2 and
 *   n/2 (both -1 when n = 0), hits[k] = #{r < cuts[k]}.  cuts [K] is HOST memory: K strictly increasing positive cut-offs.
 *   n_X + n_Y = E_a + E_b, and the same for the sum and the hits.
 * One workgroup per permutation, its threads stride over u: unit_end and the entries are read coalesced.  The order statistics by a
 * radix select on the rank value (LDS histograms of 1024 bins, LDS atomics, at most three passes), the swap bits recomputed in every
 * pass.  No global atomics, no scratch: the result depends on (seed, p, inputs) alone, whatever the grid and the split over p0.
 * NR_EINVAL before any launch: U outside [1, 2^24], K outside [1, 8], cuts not positive and increasing, E < 0, p0 < 0, n_perm < 0,
 * p0 + n_perm > 2^31 - 1, a null pointer; n_perm = 0: NR_OK, no launch. */
int nr_permtest_rank_stats(const int32_t* ranks_a, const int32_t* unit_end_a, int E_a, const int32_t* ranks_b,
                           const int32_t* unit_end_b, int E_b, int U, const int32_t* cuts, int K, uint64_t seed, int p0, int n_perm,
                           int64_t* out, void* stream);

/* Paired permutation test of per-unit sums (DESIGN.md "Paired permutation tests"): values_a, values_b [U, Q] int64 row-major, U in
 * [1, 2^24], Q in [1, 16];
 *   out[i, q] = sum over u < U of (s(p0 + i, u) ? values_b : values_a)[u, q],   out [n_perm, Q] int64,
 * side X with exactly the swap bits s(p, u) of nr_permtest_rank_stats; side Y is total_a + total_b - X, which the caller takes.  One
 * workgroup per permutation, rows read coalesced, int64 sums in registers, combined by wave shuffles and through LDS; no global
 * atomics: the result depends on (seed, p, inputs) alone.  The caller keeps U max|value| below 2^62 for either input.  NR_EINVAL
 * before any launch: U or Q out of range, p0 < 0, n_perm < 0, p0 + n_perm > 2^31 - 1, a null pointer; n_perm = 0: NR_OK, no launch. */
int nr_permtest_unit_sums(const int64_t* values_a, const int64_t* values_b, int U, int Q, uint64_t seed, int p0, int n_perm,
                          int64_t* out, void* stream);

/* Paired permutation test of hubness (DESIGN.md "Permutation test of hubness"): two rankings A and B as top-k lists idx_a, idx_b
 * [n_lists, k] int32 over the same queries and one gallery of n_gallery items, exactly as nr_slab_topk_rows / nr_topk_merge write them
 * (absent slots -1; indices outside [0, n_gallery) are not counted; a list holds an item at most once); gt_begin / gt_end [n_lists]: the
 * ground-truth gallery range of every list (nr_topk_occurrences's convention, one pair of arrays for both rankings); unit_end [U] int32
 * = index of the LAST list of unit u (nr_bootstrap_rank_stats's convention: non-decreasing, the unit before unit 0 ends at -1, a unit
 * may be empty, unit_end[U-1] = n_lists - 1); occ_ab / good_ab [n_gallery] int32 = the sums over A and B of nr_topk_occurrences's occ
 * and good.  With exactly the swap bits s(p, u) of nr_permtest_rank_stats, side X takes unit u's lists from A when s = 0 and from B
 * when s = 1, side Y the other ranking's.  With N[j] = the side's lists that hold j and GN[j] = those whose range holds j,
 *   out [n_perm, 2 (X, Y), 9] int64, exact integers:  S1 = sum N, S2 = sum N^2, S3 = sum N^3, anti = #{N = 0}, hubs = #{N G > 2 S1},
 *   hub_occ = sum of N over the hubs, bad_hubs = #{hub and N - GN > GN}, good = sum GN, max N;   X + Y = A + B in S1 and good.
 * One workgroup of 256 threads per permutation: side X's counters in LDS by integer LDS atomics, one 32-bit word per item (N low,
 * GN high: n_lists < 65 536), side Y as occ_ab - N_X; a wave reads consecutive words of idx, the unit of a word found by shuffles and
 * its swap bit recomputed; two sweeps over the items; int64 reductions by wave shuffles and through LDS.  Dynamic LDS 4 n_gallery + 576
 * bytes (above 64 KB the kernel's limit is raised first).  No global atomics, no float atomics, no scratch, no hand-off between
 * workgroups: the result depends on (seed, p, inputs) alone, whatever the grid and the split over p0.  The kernel stays in bounds
 * whatever unit_end and idx hold; the caller checks them.
 * NR_EINVAL before any launch: U outside [1, 2^24], k outside [1, 128], n_lists < 0, n_gallery < 1, p0 < 0, n_perm < 0,
 * p0 + n_perm > 2^31 - 1, a null pointer.  NR_EUNSUPPORTED before any launch: n_gallery > 32 768 or n_lists >= 65 536.
 * n_perm = 0: NR_OK, no launch. */
int nr_permtest_hubness(const int32_t* idx_a, const int32_t* idx_b, int n_lists, int k, const int32_t* unit_end, int U, int n_gallery,
                        const int32_t* gt_begin, const int32_t* gt_end, const int32_t* occ_ab, const int32_t* good_ab, uint64_t seed,
                        int p0, int n_perm, int64_t* out, void* stream);

/* Multi-tensor BertAdam step (models/optimization.py:76-211 with the trainer's clip and clamp around it, trainer.py:104-119;
 * DESIGN.md "BertAdam in the captured step").  fp32 tensors only.  Per step, for every table entry t with group q:
 *   c    = min(1, global_max_norm / (sqrt(sum_t ||g_t||^2) + 1e-6))             (global_max_norm <= 0: c = 1)
 *   c_t  = min(1, q.max_grad_norm / (c ||g_t|| + 1e-6))                          (q.max_grad_norm <= 0: c_t = 1)
 *   gh   = g c c_t;  m = b1 m + (1 - b1) gh;  v = b2 v + (1 - b2) gh^2;  u = m / (sqrt(v) + e) [+ weight_decay p if > 0]
 *   lr_t = q.lr * schedule(*step / t_total, warmup), *step read BEFORE its increment (q.t_total == -1: lr_t = q.lr),
 *          evaluated in double and rounded to fp32 once
 *   p   -= lr_t u;  p = min(p, clamp_max) where has_clamp;  *step += 1.          No bias correction; g is never written.
 * Three launches whatever T is (chunk sums of g^2; one workgroup of scalars; the update), every reduction in a fixed order, no
 * float atomics: same inputs, same bits, launched eagerly or replayed from a graph.  Non-finite gradients propagate as the
 * formulas give (nr_bertadam_step_guarded below is the form that skips such a step on the device instead).  `table` and
 * `groups` are DEVICE arrays; nothing the launches read comes from the host after the call. */
#define NR_SCHEDULE_WARMUP_COSINE 0   /* x / warmup if x < warmup else 0.5 (1 + cos(pi x))                  */
#define NR_SCHEDULE_WARMUP_CONSTANT 1 /* ... else 1                                                         */
#define NR_SCHEDULE_WARMUP_LINEAR 2   /* ... else max((x - 1) / (warmup - 1), 0)                            */
typedef struct {
    float* p;          /* parameter, n elements, 4-byte aligned (16-byte aligned p, g, m, v take the vector path)     */
    const float* g;    /* gradient                                                                                     */
    float* m;          /* first moment  (next_m)                                                                       */
    float* v;          /* second moment (next_v)                                                                       */
    int32_t* step;     /* the tensor's step counter (device)                                                           */
    int64_t n;
    int32_t group;     /* index into groups                                                                            */
    int32_t chunk0;    /* first chunk of this tensor: written by nr_bertadam_plan                                      */
    int32_t has_clamp; /* != 0: p = min(p, clamp_max) after the update                                                 */
    float clamp_max;
} NrOptimTensor; /* 64 bytes */
typedef struct {
    double lr, weight_decay, b1, b2, e, max_grad_norm, warmup;
    int64_t t_total;   /* -1: constant learning rate                                                                   */
    int32_t schedule;  /* NR_SCHEDULE_*                                                                                */
    int32_t pad_;
} NrOptimGroup; /* 72 bytes */

/* Host-only: validates the HOST copies of the table and the groups before they are uploaded (null pointers, misaligned
 * pointers, negative counts, group indices out of range, bad schedule ids, t_total 0 or < -1: NR_EINVAL), writes every
 * entry's chunk0 and returns the number of chunks in *n_chunks. */
int nr_bertadam_plan(NrOptimTensor* entries, int T, const NrOptimGroup* groups, int G, int* n_chunks);
size_t nr_bertadam_workspace_bytes(int T, int n_chunks);
/* The three launches.  table [T] / groups [G]: device copies of what nr_bertadam_plan checked; workspace:
 * nr_bertadam_workspace_bytes(T, n_chunks) bytes, 8-byte aligned.  NR_EINVAL before any launch for null pointers, negative
 * counts, a NaN global_max_norm. */
int nr_bertadam_step(const NrOptimTensor* table, int T, int n_chunks, const NrOptimGroup* groups, int G, float global_max_norm,
                     void* workspace, void* stream);

/* The guarded step (DESIGN.md "Non-finite step guard"): the same three launches, the same workspace
 * (nr_bertadam_workspace_bytes: the word launch C tests lives in NrStepGuard, not in the workspace), and for finite gradients the
 * same bits in p, m, v, the counters and the learning rates as nr_bertadam_step.  Launch B always forms
 * total = sum_t ||g_t||^2 in table order (with a global limit: the very sum c is made from) and calls the step BAD when total is
 * not finite: a NaN or an infinite gradient entry anywhere, or a finite entry so large that the fp32 sum of squares of its
 * 4096-element chunk overflows (|g| >= 2^64 always does) -- the last is treated as non-finite on purpose: such a step has no
 * usable norm.  A bad step writes nothing to p, m, v, leaves every step counter where it was (the schedule does not move) and sets
 * guard->skip = 1 (0 on a good step; written on every execution).  One thread of launch B is the only writer of *guard and of
 * the ring, with plain stores and no atomics; launches on one stream are ordered, so there is one writer at a time.  Per
 * execution it adds one attempt to the guard and writes
 *   ring[attempts_before & (n_ring - 1)] = {attempt, (float)sqrt(total), (float)c, skipped, n_losses, losses[0 .. n_losses), 0 ...}
 * (losses: optional DEVICE floats, copied bit for bit, read when launch B runs).  The caller zeroes *guard and the ring once, with
 * last_skipped = -1, and reads them back whenever it likes; nothing here synchronises.
 * NR_EINVAL before any launch: what nr_bertadam_step refuses, a null or misaligned (8 bytes) guard or ring, n_ring not a power of
 * two in [1, NR_GUARD_MAX_RING], n_losses outside [0, NR_GUARD_MAX_LOSSES], losses NULL with n_losses > 0.  T = 0: NR_OK, no
 * launch, no attempt counted. */
#define NR_GUARD_MAX_LOSSES 8
#define NR_GUARD_MAX_RING 4096
typedef struct {
    int64_t attempts;        /* executions of the guarded step                                                         */
    int64_t skipped;         /* of those, bad ones                                                                     */
    int64_t consecutive;     /* length of the run of bad steps that is open now (0 after a good step)                  */
    int64_t max_consecutive; /* longest such run so far                                                                */
    int64_t last_skipped;    /* attempt index of the last bad step, -1: none yet                                       */
    int32_t skip;            /* the last execution's decision, read by launch C                                        */
    int32_t pad_;
} NrStepGuard; /* 48 bytes */
typedef struct {
    int64_t attempt;         /* 0-based index of the execution                                                         */
    float grad_norm;         /* (float)sqrt(total): the global gradient norm before any clip; NaN / Inf on a bad step  */
    float clip;              /* (float)c, 1 without a global limit                                                     */
    int32_t skipped;
    int32_t n_losses;
    float losses[NR_GUARD_MAX_LOSSES];
} NrStepRecord; /* 56 bytes */
int nr_bertadam_step_guarded(const NrOptimTensor* table, int T, int n_chunks, const NrOptimGroup* groups, int G,
                             float global_max_norm, void* workspace, NrStepGuard* guard, const float* losses, int n_losses,
                             NrStepRecord* ring, int n_ring, void* stream);

/* Exponential moving average of the weights (DESIGN.md "Weight EMA").  Per averaged element, AFTER the parameter's update of the
 * same step, with n = state->updates (the updates that have happened before this one):
 *   d   = warmup ? min(decay, (1 + n) / (10 + n)) : decay      in double
 *   omd = (float)(1.0 - d)                                     rounded once
 *   e   = fmaf(omd, p_new - e, e)                              fp32, the difference rounded; e is the fp32 shadow
 *   state->updates = n + 1
 * One device function holds the element's arithmetic: the fused and the stand-alone form, 16-byte and dword accesses give the same
 * bits.  No float atomics, nothing read from the host after a call: every form replays from a graph. */
typedef struct {
    double decay;      /* in [0, 1)                                                                                    */
    int64_t updates;   /* good updates so far                                                                          */
    int32_t warmup;    /* != 0: the decay ramps up as (1 + n) / (10 + n) until it reaches `decay`                      */
    float omd;         /* (float)(1 - d) of the last update, written on every good update                              */
} NrEmaState; /* 24 bytes */
typedef struct {
    float* p;          /* parameter, n elements, 4-byte aligned (16-byte aligned p and ema take the vector path)       */
    float* ema;        /* its shadow                                                                                   */
    int64_t n;
    int32_t chunk0;    /* first chunk of this tensor: written by nr_ema_plan                                           */
    int32_t pad_;
} NrEmaTensor; /* 32 bytes */
/* nr_bertadam_step_guarded's arguments (guard == NULL: the unguarded step, ring and losses are ignored) plus `ema`, a DEVICE
 * array of T pointers parallel to `table` (NULL entry: that tensor is not averaged), and the DEVICE state.  The same three
 * launches and workspace: in launch B the thread that owns the guard forms omd and counts the update (on a bad step it touches
 * nothing of *state and no shadow moves), launch C averages the chunks it is streaming.  p, m, v, the counters and the learning
 * rates get the bits nr_bertadam_step / _guarded give.  NR_EINVAL before any launch: what those refuse, a null or misaligned
 * (8 bytes) ema or state.  T = 0: NR_OK, no launch, no update counted. */
int nr_bertadam_step_ema(const NrOptimTensor* table, int T, int n_chunks, const NrOptimGroup* groups, int G, float global_max_norm,
                         void* workspace, NrStepGuard* guard, const float* losses, int n_losses, NrStepRecord* ring, int n_ring,
                         float* const* ema, NrEmaState* state, void* stream);
/* Host-only: validates the HOST copies of a stand-alone table and of the state (null or misaligned pointers, negative counts, a
 * decay outside [0, 1) or NaN: NR_EINVAL), writes every entry's chunk0 and returns the number of chunks in *n_chunks. */
int nr_ema_plan(NrEmaTensor* entries, int T, const NrEmaState* state, int* n_chunks);
/* Stand-alone update of every tensor of the DEVICE table: a one-thread launch that forms omd and counts the update, then the
 * streaming launch (12 bytes per element).  NR_EINVAL before any launch for null or misaligned (8 bytes) table or state and
 * negative counts.  T = 0: NR_OK, no launch, no update counted. */
int nr_ema_update(const NrEmaTensor* table, int T, int n_chunks, NrEmaState* state, void* stream);
/* Exchanges the contents of p and ema of every table entry in place: one launch, no state, bit-exact. */
int nr_ema_swap(const NrEmaTensor* table, int T, int n_chunks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NR_HIP_H */
