"""Orchestration of the HIP kernels for one step of the NeighborRetr loss head: which launches a step issues, in which order,
on which streams.

The step is the fused equivalent of the reference's `_compute_losses` (NeighborRetr/models/modeling.py:314-360); the
token-clustering stage comes in as global tokens or as a `join` that produces them:

    prepare (normalise+mask+bf16 split)  x4     modeling.py:495-496, :500-501
    token scorer MLP + masked softmax    x4     modeling.py:485-492
    fused local_level  BxB / BxM / MxB          modeling.py:499-512, :389-390
    global logits G (exact fp32 MFMA)           modeling.py:516-539
    Sinkhorn targets (both directions)          until_module.py:235-266
    centrality weights                          modeling.py:403-430
    row losses + finalize                       until_module.py:56-211, :285-289, :303-359

What is here, in the order a step passes through it:

    precision_plan / backward_plan   which contraction precision each product runs in
    head_plan -> HeadPlan            shapes, precisions after the `keep` demotion, who reads the lo planes, split tail or not; the
                                     refusals of both forwards (pure host code)
    local_steps / bank_steps         the local branch and one memory-bank chain, generators of one launch per step
    _interleave / _run_branches      the clustering against the local branch: interleaved in capture order, joined from another
                                     stream, or on one stream
    _split_tail / _joined_tail       logits -> Sinkhorn -> row losses, self-finalizing (loss-only, B <= 128) or joined
    head_forward                     plan, branches, tail, saved state
    head_forward_sharded             the loss-only step with the products sharded over the ranks (same plan, own launches)

The differentiable entry points (`head_losses`, the autograd Functions) live in functional.py and backward.py; they call
`head_forward(keep=True)`.  Nothing here falls back to eager PyTorch for the forward math.
"""
from collections import namedtuple
from typing import NamedTuple

import torch

from . import hip, ops
from .capture_guard import record_event, wait_event, wait_stream

MLP_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias")


class ScorerWeights:
    """bf16 hi/lo split of one token-scorer MLP (re-split whenever the parameters change)."""

    def __init__(self, w1, b1, w2, b2, want_lo=True):
        self.w1_hi, self.w1_lo = ops.split_bf16(w1.detach(), want_lo)
        self.b1 = b1.detach().float().contiguous()
        self.w2 = w2.detach().float().reshape(-1).contiguous()
        self.b2 = b2.detach().float().reshape(1).contiguous()
        self._w1 = w1.detach()
        self._w1t = None
        self._w1_f16 = None

    @property
    def w1_f16(self):
        """fp16 image of W1 (the hip.PREC_F16 operand): built on first use per version, cached with the bf16 halves."""
        if self._w1_f16 is None:
            self._w1_f16 = ops.split_f16(self._w1)
        return self._w1_f16

    def w1_transposed(self):
        """bf16 pair of W1^T [d, H]: the operand of dX = dh W1 in the scorer's backward (built on first use per version)."""
        if self._w1t is None:
            from .cluster_fused import split_group
            H, d = self._w1.shape
            hi = torch.empty((d, H), dtype=torch.int16, device=self._w1.device)
            lo = torch.empty((d, H), dtype=torch.int16, device=self._w1.device)
            split_group([(self._w1.float().contiguous(), None, hi, lo, H, d, 1, H)])
            self._w1t = (hi, lo)
        return self._w1t


def _scorer_operands(sw, prec):
    """(W1 operand, its lo half or None) of a scorer for a contraction precision."""
    return (sw.w1_f16, None) if int(prec) == hip.PREC_F16 else (sw.w1_hi, sw.w1_lo)


def token_weights(prep, mask, sw, n, N, prec, want_logits=False, scale_override=None):
    p = prep if scale_override is None else prep._replace(norm=scale_override)
    if int(prec) == hip.PREC_F16 and p.f16 is None and p.lo is not None:
        # tokens prepared as a bf16 pair only, handed the training plan's scorer precision: they run the split passes they
        # carry (what that plan ran before it had fp16 planes; no less exact)
        prec = hip.PREC_BF16X3
    w1_a, w1_b = _scorer_operands(sw, prec)
    return ops.token_weights(p, w1_a, w1_b, sw.b1, sw.w2, sw.b2, mask, n, N, prec, want_logits)


def similarity_matrix(text_feat, video_feat, text_mask, video_mask, sw_t, sw_v, prec=hip.PREC_BF16X3):
    """local_level forward only (eval path): [A,Nt,d] x [Bv,Nv,d] -> S [A,Bv]."""
    A, Nt, _ = text_feat.shape
    Bv, Nv, _ = video_feat.shape
    lo, f16 = prec == hip.PREC_BF16X3, prec == hip.PREC_F16
    pt = ops.prepare_tokens(text_feat, text_mask, want_lo=lo, want_f16=f16)
    pv = ops.prepare_tokens(video_feat, video_mask, want_lo=lo, want_f16=f16)
    w_t, _ = token_weights(pt, text_mask, sw_t, A, Nt, prec)
    w_v, _ = token_weights(pv, video_mask, sw_v, Bv, Nv, prec)
    S, _ = ops.local_level(pt, pv, w_t, w_v, A, Nt, Bv, Nv, prec)
    return S


def global_logits(gt, gv, sw_t1=None, sw_v1=None, keep=False):
    """global_level (modeling.py:516-539).  One global token per sample: an exact-fp32 GEMM.
    Several tokens (ActivityNet token counts): the fused kernel on un-normalised tokens, split-bf16.
    keep=True: returns (G, saved) with what the backward of the multi-token form needs (None for one token)."""
    B, Ngt, d = gt.shape
    Ngv = gv.shape[1]
    if Ngt == 1 and Ngv == 1:
        G = ops.gemm_nt_f32(gt.reshape(B, d), gv.reshape(gv.shape[0], d))
        return (G, None) if keep else G
    pt = ops.prepare_tokens(gt, None, normalize=False)
    pv = ops.prepare_tokens(gv, None, normalize=False)
    ones_t = torch.ones_like(pt.norm)
    ones_v = torch.ones_like(pv.norm)
    w_t, _ = token_weights(pt, None, sw_t1, B, Ngt, hip.PREC_BF16X3, scale_override=ones_t)
    w_v, _ = token_weights(pv, None, sw_v1, gv.shape[0], Ngv, hip.PREC_BF16X3, scale_override=ones_v)
    G, aux = ops.local_level(pt, pv, w_t, w_v, B, Ngt, gv.shape[0], Ngv, hip.PREC_BF16X3, hip.OUT_FULL, keep)
    return (G, dict(pt=pt, pv=pv, w_t=w_t, w_v=w_v, aux=aux)) if keep else G


def _check_global_tokens(gt, gv, hp):
    """More than one global token per sample (ActivityNet token counts: 64 -> 11 -> 3 text, 64 -> 16 -> 6 video
    tokens): the reference's centrality term multiplies [B] by [B,G] and raises (until_module.py:321), so there is
    no reference answer.  config.centrality_multi_token = "raise" (default) mirrors that; "mean" runs the step with
    w_i = mean over the sample's global tokens of the reference's per-token weight."""
    if gt.shape[1] == 1 and gv.shape[1] == 1:
        return
    mode = hp.get("centrality_multi_token", "raise")
    if mode == "mean":
        return
    if mode != "raise":
        raise ValueError(f"centrality_multi_token={mode!r}: expected 'raise' or 'mean'")
    raise RuntimeError(f"{gt.shape[1]} / {gv.shape[1]} global tokens per sample: the reference's centrality term fails to "
                       "broadcast at this shape (until_module.py:321); set config.centrality_multi_token='mean' to run "
                       "with the documented reduction (parity unpinned for that one term)")


PREC_MIXED = 2   # host-level plan: split-bf16 where logit_scale amplifies the error, bf16 elsewhere


def precision_plan(prec, shape=None):
    """(batch x batch similarity, batch-token scorer, memory-bank paths) kernel precisions.

    The centrality term feeds S*logit_scale (x100) into a log-softmax, so single-pass bf16 error on
    the B x B similarity (~1.5e-4) shows up as ~2e-3 on that loss at small B: bf16's 8 significand bits are
    too few for the batch side.  The mixed plan runs the B x B product and the batch scorers in ONE fp16
    pass (11 bits; the operands are normalised tokens and scorer weights: |dL| <= 2.5e-4 on the probe of
    tools/prec_probe_f16.py, profiles/f16_prec_probe.txt) and the two memory-bank products -- whose outputs
    are only consumed as means over M entries -- and the bank-side scorer in one bf16 pass.

    This is the plan of the LOSS-ONLY step; a forward kept for the backward (head_forward(keep=True), the sharded training
    node) runs backward_plan, i.e. split-bf16 on the batch side, because the gradients need the finer S (see head_plan).

    shape = (B, Nt, Nv, d, H): the fp16 precision is returned only where the host-side plan calls
    (hip.local_level_plan / hip.token_scorer_plan) say an fp16 form is built for that launch; a launch without
    one stays split-bf16, as the whole batch side was before.  Without a shape: the plan's constants."""
    if prec == PREC_MIXED:
        p_bb = p_mlp = hip.PREC_F16
        if shape is not None:
            B, Nt, Nv, d, H = (int(v) for v in shape)
            if hip.local_level_plan(B, Nt, B, Nv, d, hip.PREC_F16) is None:
                p_bb = hip.PREC_BF16X3
            if (hip.token_scorer_plan(B * Nt, H, hip.PREC_F16, 0) is None
                    or hip.token_scorer_plan(B * Nv, H, hip.PREC_F16, 0) is None):
                p_mlp = hip.PREC_BF16X3
        return p_bb, p_mlp, hip.PREC_BF16
    return prec, prec, prec


def backward_plan(prec):
    """precision_plan of a step that is differentiated, forward and backward: split-bf16 wherever the loss-only step runs one
    fp16 pass (the backward kernels know the bf16 pair only, and the gradients need the finer forward: head_plan)."""
    return tuple(backward_prec(p) for p in precision_plan(prec))


def backward_prec(p):
    return hip.PREC_BF16X3 if int(p) == hip.PREC_F16 else p


# The step issues the two bank products as two launches (nr_sim_pair_kernel, one launch for both, makes the step slower:
# docs/LAB_NOTEBOOK.md); bench.py's roofline reads this name.
PAIR_BANK_PRODUCTS = False
# Loss-only step: the batch's text and video scorers as one launch (nr_token_weights_fwd_pair) from this many tokens in the smaller
# set on (a few workgroups per CU): configs[3] 517 -> 530 steps/s, configs[2] 424 -> 427; at configs[1] (3072 + 1536 tokens: one
# workgroup per CU) the two launches one after the other are faster, 3725 vs 3605
PAIR_BATCH_SCORERS_FROM = 8192


class HeadPlan(NamedTuple):
    """The decisions of one step, taken once from shapes and arguments (head_plan)."""
    B: int
    Nt: int
    Nv: int
    d: int
    M: int
    K: int
    p_bb: int            # precisions of the B x B product, the batch scorers, the bank paths -- after the `keep` demotion
    p_mlp: int
    p_bank: int
    f16_b: bool          # the batch is prepared with an fp16 plane
    lo_b: bool           # ... with a bf16 lo plane
    lo_k: bool           # the bank is prepared with a lo plane
    split_tail: bool
    keep: bool
    b: int               # sharded form: rows of this rank's slabs, and the first of them (B, 0 otherwise)
    r0: int


def head_plan(text_shape, Nv, bank_rows, H, K, prec, keep=False, prepared_out=False, side_streams=False, global_tokens=True,
              shard=None):
    """HeadPlan of a step, or the refusal of its arguments.  text_shape = (B, Nt, d); bank_rows = rows of the (text, video) bank;
    H = the scorers' hidden width; prepared_out: the caller takes the batch's prepared tokens; side_streams: bank streams AND a
    local stream are given; global_tokens: gt / gv or a join that produces them; shard = (rank, world) for head_forward_sharded."""
    B, Nt, d = (int(v) for v in text_shape)
    Nv, M, K = int(Nv), int(bank_rows[1]), int(K)
    rank, world = shard if shard is not None else (0, 1)
    if B % world:
        raise ValueError("the gathered batch must divide over the ranks")
    if K > B:
        raise ValueError(f"num_neighbors={K} > batch={B}" + ("" if shard is not None else
                         ": the reference raises IndexError here (until_module.py:119-123)"))
    if shard is None and (M == 0 or bank_rows[0] != M):
        raise ValueError("empty or inconsistent memory bank")
    if not global_tokens:
        raise ValueError("gt / gv missing and no join callable to produce them")
    p_bb, p_mlp, p_bank = precision_plan(prec, (B, Nt, Nv, d, H))
    if keep:
        # A forward that will be differentiated keeps the batch side split-bf16: with one fp16 pass the losses hold (|dL| <= 3e-4)
        # but the gradients do not -- d/d logit_scale is a sum of cancelling terms in S, and against the reference's autograd it
        # moved from < 2e-3 to 6.4e-3 relative at c1_b16, the row sums of the text gradient to 1.7e-2 (bars 2e-3 / 5e-3,
        # tests/test_head_gpu.py::test_backward_matches_reference).  The loss-only step has no such reader.
        p_bb, p_mlp = backward_prec(p_bb), backward_prec(p_mlp)
    b = B // world
    if shard is not None and p_bb == hip.PREC_F16 and (hip.local_level_plan(b, Nt, B, Nv, d, p_bb) is None
                                                       or hip.local_level_plan(B, Nt, b, Nv, d, p_bb) is None):
        # (the slabs are b x B and B x b products: the fp16 form must exist for both, or both stay split-bf16)
        p_bb = hip.PREC_BF16X3
    f16_b = hip.PREC_F16 in (p_bb, p_mlp)
    # who reads the batch's lo plane: the backward (keep), a split-bf16 launch, and -- on the fp16 plan -- the memory bank's
    # prepared shadow, which takes the batch's hi / lo / norm rows at the push (prepared_out)
    lo_b = keep or hip.PREC_BF16X3 in (p_bb, p_mlp, p_bank) or (f16_b and bool(prepared_out))
    lo_k = keep or p_bank == hip.PREC_BF16X3
    # Loss-only step at B <= 128 ("split tail", _split_tail): the bank centralities stay PARTIAL sums (the row-loss kernel adds
    # them up itself: two reduction launches less per step)
    split_tail = (not keep) and bool(side_streams) and B <= 128 and B % 4 == 0
    return HeadPlan(B, Nt, Nv, d, M, K, p_bb, p_mlp, p_bank, f16_b, lo_b, lo_k, split_tail, bool(keep), b, rank * b)


def _masks_f32(*masks):
    """masks as fp32 once (the loaders hand over int64); the kernels read them as multipliers"""
    return tuple(m if m.dtype == torch.float32 else m.float() for m in masks)


def _keep_alive(tensors, *streams):
    """record_stream on every given stream for every CUDA tensor of `tensors` (None and host entries skipped): memory that was
    allocated on one stream and is read on another must not go back to its own stream's free list before that read."""
    for t_ in tensors:
        if torch.is_tensor(t_) and t_.is_cuda:
            for st_ in streams:
                t_.record_stream(st_)


# What the launches of one step share: their inputs, `chains` (the arguments of the two bank chains), `L` (dict: the local
# branch's results by name) and `early` (list: the results of the chains that ran early, on the local stream)
_Step = namedtuple("_Step", "text_feat video_feat text_mask video_mask sw_t sw_v chains local_stream bank_early pipeline L early")


def local_steps(plan, st):
    """The local branch, one kernel launch per step (a generator, so that it can be interleaved launch by launch with the
    clustering: _run_branches); its results land in st.L."""
    L, B, Nt, Nv, keep = st.L, plan.B, plan.Nt, plan.Nv, plan.keep
    L["pt"], L["pv"] = pt_, pv_ = ops.prepare_tokens_pair(st.text_feat, st.text_mask, st.video_feat, st.video_mask, want_lo=plan.lo_b,
                                                          want_colsum=True, want_f16=plan.f16_b)
    yield
    if not keep and B * min(Nt, Nv) >= PAIR_BATCH_SCORERS_FROM:
        # the text and the video scorer in one grid; bit-identical to the two launches
        (L["w_t"], L["lg_t"]), (L["w_v"], L["lg_v"]) = ops.token_weights_pair(
            [(pt_, *_scorer_operands(st.sw_t, plan.p_mlp), st.sw_t.b1, st.sw_t.w2, st.sw_t.b2, st.text_mask, B, Nt),
             (pv_, *_scorer_operands(st.sw_v, plan.p_mlp), st.sw_v.b1, st.sw_v.w2, st.sw_v.b2, st.video_mask, B, Nv)], plan.p_mlp)
        yield
    else:
        L["w_t"], L["lg_t"] = token_weights(pt_, st.text_mask, st.sw_t, B, Nt, plan.p_mlp, keep)
        yield
        L["w_v"], L["lg_v"] = token_weights(pv_, st.video_mask, st.sw_v, B, Nv, plan.p_mlp, keep)
        yield
    L["S"], L["aux0"] = ops.local_level(pt_, pv_, L["w_t"], L["w_v"], B, Nt, B, Nv, plan.p_bb, hip.OUT_FULL, keep)
    yield
    # mean of the (unmasked) normalised tokens for the centrality weights, both in one launch
    L["mean_t"], L["mean_v"] = ops.colsum_pair(pt_.colsum, 1.0 / pt_.n_tok, pv_.colsum, 1.0 / pv_.n_tok)
    yield
    # `bank_early` chains (0..2) run right behind the batch products, i.e. beside the clustering; the rest is
    # forked after the join (beside the Sinkhorn solve)
    if st.local_stream is not None:
        for i in range(min(st.bank_early, 2)):
            st.early[i] = yield from bank_steps(plan, st, *st.chains[i])


def after_previous_push(pipeline):
    """Pipelined steps: whatever reads the memory bank waits for the PREVIOUS step's push (on the stream it runs on)."""
    if pipeline is not None and pipeline.prev_push_done is not None:
        wait_event(torch.cuda.current_stream(), pipeline.prev_push_done)
    if pipeline is not None and pipeline.prev_tail_done is not None:
        # ... and for the previous step's ROW LOSSES.  No data flows along this edge.  It is there because of how the ROCm 7.2
        # runtime orders a graph's nodes: a node nothing depends on (the row-loss launch is the last of its step) is put at the
        # END of the graph's hardware queues -- the row losses of all ten steps of a pipelined graph ran one after the other
        # when everything else was done, 24 of every 298 us with 32 workgroups on the chip; with a dependent it is started
        # before that dependent.  The bank chain starts ~150 us after the previous solve: nothing waits in practice
        # (profiles/r04_step_timeline_pipelined.txt: 3350-3480 -> 3490-3560 steps/s, A/B per box).
        wait_event(torch.cuda.current_stream(), pipeline.prev_tail_done)
        pipeline.prev_tail_done = None


def bank_steps(plan, st, feat, mask, prepared, sw, n_tok, out):
    """One memory-bank chain: prepare (unless the bank's prepared shadow is given), scorer, the product with the batch and,
    outside the split tail, the mean over the M entries.  Returns (prepared, weights, logits, aux, centrality)."""
    L, B, Nt, Nv, M, keep = st.L, plan.B, plan.Nt, plan.Nv, plan.M, plan.keep
    after_previous_push(st.pipeline)
    pb = prepared
    if pb is None:
        pb = ops.prepare_tokens(feat, mask, want_lo=plan.lo_k)
        yield
    w_b, lg_b = token_weights(pb, mask, sw, M, n_tok, plan.p_bank, keep)
    yield
    if out == hip.OUT_ROWSUM:
        part, aux = ops.local_level(L["pt"], pb, L["w_t"], w_b, B, Nt, M, Nv, plan.p_bank, out, keep)
    else:
        part, aux = ops.local_level(pb, L["pv"], w_b, L["w_v"], M, Nt, B, Nv, plan.p_bank, out, keep)
    yield
    if plan.split_tail:
        return pb, w_b, lg_b, aux, part
    c = ops.reduce_parts(part, 1.0 / M)
    yield
    return pb, w_b, lg_b, aux, c


def exhaust(gen):
    """Runs a step generator to its end; returns its return value."""
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            return stop.value


def bank_chain(plan, st, i):
    """Chain i, unless it already ran early on the local stream."""
    return st.early[i] or exhaust(bank_steps(plan, st, *st.chains[i]))


def _interleave(clu, loc, capture_order, on_local):
    """Drives the generators `clu` (this stream) and `loc` (inside on_local()) in turns: `capture_order` =
    [(clustering launches, local launches), ...] per turn, the last pair repeating; once one side has run out the other runs to
    its end.  Returns what `clu` returned."""
    loc_alive, clu_alive = True, True
    produced = None
    turn = 0
    while loc_alive or clu_alive:
        n_clu, n_loc = capture_order[min(turn, len(capture_order) - 1)]
        turn += 1
        if clu_alive:
            try:
                for _ in range(n_clu if loc_alive else 1 << 30):
                    next(clu)
            except StopIteration as stop:
                produced, clu_alive = stop.value, False
        if loc_alive:
            with on_local():
                try:
                    for _ in range(n_loc if clu_alive else 1 << 30):
                        next(loc)
                except StopIteration:
                    loc_alive = False
    return produced


def _run_branches(plan, st, gt, gv, join, capture_order, cur):
    """The clustering (`join`, when it produces the global tokens) and the local branch, in one of three orders.  -> (gt, gv)."""
    local_stream = st.local_stream
    stepwise_join = join is not None and hasattr(join, "__next__")
    produced = None
    if local_stream is not None and stepwise_join:
        # A captured HIP graph starts its nodes in CAPTURE ORDER: a node on another queue does not start before
        # the nodes captured ahead of it have started (profiled step: a branch captured after 7 clustering nodes
        # began 120 us late and ended up the critical path).  So the two branches are captured interleaved:
        # `capture_order` = [(clustering launches, local launches), ...] per turn, the last pair repeating.
        wait_stream(local_stream, cur)
        produced = _interleave(join, local_steps(plan, st), capture_order, lambda: torch.cuda.stream(local_stream))
    elif local_stream is not None:
        # `join`: one callable run right before gt / gv are needed (may return them) -- here ahead of the local branch, which
        # goes to the other stream
        wait_stream(local_stream, cur)
        if join is not None:
            produced = join()
        with torch.cuda.stream(local_stream):
            exhaust(local_steps(plan, st))
    else:
        # one stream: the local branch, then the join; generators are run through
        exhaust(local_steps(plan, st))
        if join is not None:
            produced = exhaust(join) if stepwise_join else join()
    return produced if produced is not None else (gt, gv)


# What either tail leaves: chain_t / chain_v are the bank chains' (prepared, weights, logits, aux, centrality)
_Tail = namedtuple("_Tail", "G g_saved tgt_r tgt_c c0 c1 wc_t wc_v cw_aux chain_t chain_v rowloss losses")


def _split_tail(plan, st, hp, gt, gv, gt2, gv2, ls, logit_scale, sw_t1, sw_v1, bank_streams, bank_push, slot, cur):
    """Loss-only step at B <= 128 ("split tail"): the global logits and the Sinkhorn solve depend on the clustering
    alone, so they follow it on THIS stream without waiting for the local branch; the Sinkhorn kernel emits the
    uniform-CE row terms itself, and everything that needs the local branch (leftover bank chains, bank push,
    centrality weights, the row-loss kernel with its top-K) gathers on a side stream.  The two tail kernels finalize
    themselves (whichever workgroup finishes last reduces the row terms to the five losses), so the critical path
    is prologue -> clustering -> logits -> Sinkhorn, with neither a finalize launch nor the push behind it."""
    B, M, K, L, pipeline, local_stream = plan.B, plan.M, plan.K, st.L, st.pipeline, st.local_stream
    pt, pv, S, mean_t, mean_v = L["pt"], L["pv"], L["S"], L["mean_t"], L["mean_v"]
    tail = pipeline.tail_stream if pipeline is not None else None
    G = global_logits(gt, gv, sw_t1, sw_v1)
    g_ready = record_event(cur)
    rowloss = torch.empty((2, 4, B), dtype=torch.float32, device=G.device)
    losses = torch.empty((5,), dtype=torch.float32, device=G.device)
    counter = ops.split_tail_counter(G.device, slot)
    wts = (hp["uniform_weight"], hp["neighbor_weight"], hp["kl_weight"])
    # The two self-finalizing launches share `counter`; only the one that finishes last resets it.  If anything raises
    # between them (the push callable, an NR_E* status), the word would stay non-zero and every later step would finalize
    # on incomplete row terms without an error: zero it before passing the exception on.
    try:
        if tail is not None:
            wait_stream(tail, cur)
            with torch.cuda.stream(tail):
                ops.sinkhorn_uniform_rows_final(G, hp["beta"], hp["temperature"], rowloss, counter, *wts, losses, 50)
            _keep_alive((G, rowloss, losses), tail)
        else:
            ops.sinkhorn_uniform_rows_final(G, hp["beta"], hp["temperature"], rowloss, counter, *wts, losses, 50)
        side, side2 = bank_streams[0], bank_streams[1]
        push_stream = bank_streams[2] if len(bank_streams) > 2 else None
        wait_stream(side, local_stream)
        wait_stream(side2, local_stream)
        with torch.cuda.stream(side2):
            chain_t = bank_chain(plan, st, 1)
        with torch.cuda.stream(side):
            chain_v = bank_chain(plan, st, 0)
            c0, c1 = chain_t[4], chain_v[4]
            wait_stream(side, side2)
            if bank_push is not None:
                # both bank products have read the bank (and its prepared shadow): the batch may take the oldest rows'
                # place -- on a stream of its own, beside the centrality weights and the row losses.  (A stream that
                # has already been joined must not be forked again inside one capture: putting the push back on
                # `side2` after `wait_stream(side, side2)` made the ROCm 7.2 runtime segfault at capture time.)
                pst = push_stream if push_stream is not None else side
                if push_stream is not None:
                    wait_stream(push_stream, side)
                with torch.cuda.stream(pst):
                    _keep_alive((pt.hi, pt.norm, pv.hi, pv.norm, pt.lo, pv.lo), pst)
                    with torch.no_grad():
                        bank_push()
            wait_event(side, g_ready)
            if gt2.shape[1] == 1 and gv2.shape[1] == 1 and gt2.shape[0] == B and gv2.shape[0] == B:
                # one global token per sample: the row-loss launch computes the centrality weights itself (one launch less
                # on the chain that the next step's bank reads wait for)
                wc_t = wc_v = cw_aux = None
                ops.row_losses_no_uniform_final_cw(S, G, c0, c1, 1.0 / M, gt2.view(B, -1), gv2.view(B, -1), mean_t, mean_v,
                                                   hp["centrality_scale"], ls, K, hp["temperature"], rowloss, counter, *wts, losses)
            else:
                wc_t, wc_v, cw_aux = ops.centrality_weights_pair(gt2, gv2, mean_t, mean_v, hp["centrality_scale"], plan.keep)
                ops.row_losses_no_uniform_final(S, G, c0, c1, 1.0 / M, wc_t, wc_v, ls, K, hp["temperature"], rowloss, counter,
                                                *wts, losses)
            if pipeline is not None:
                pipeline.tail_done = record_event(side)
    except BaseException:
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize(G.device)
            counter.zero_()
        else:
            ops.forget_split_tail_counter(G.device, slot)   # an aborted capture: the next step takes a fresh zeroed word
        raise
    pushed_aside = (push_stream,) if (push_stream is not None and bank_push is not None) else ()
    if pipeline is not None:
        # everything this step allocated stays referenced until the capture ends (StepPipeline.own): its forked streams are
        # not joined here, and the next step allocates on this stream right away
        pipeline.own(L, st.early, gt, gv, gt2, gv2, ls, G, rowloss, losses, c0, c1, wc_t, wc_v, cw_aux, chain_t, chain_v,
                     st.text_mask, st.video_mask, *(c[1] for c in st.chains))
        pipeline.pending += [tail, side, *pushed_aside]
        # Nothing is joined into this stream, which goes straight on to the NEXT step: whatever was allocated on it and is
        # still read by this step's forked streams must not go back to its free list when this function returns
        _keep_alive((gt2, gv2, gt, gv, ls, logit_scale, st.text_mask, st.video_mask, G, rowloss, losses),
                    tail, side, side2, local_stream, *pushed_aside)
    else:
        wait_stream(cur, side)
        if push_stream is not None:
            wait_stream(cur, push_stream)
    # (wc_t / wc_v None: the centrality weights were computed inside the row-loss launch)
    _keep_alive((S, mean_t, mean_v, L["w_t"], L["w_v"], pt.hi, pv.hi, c0, c1, wc_t, wc_v, G, rowloss, losses), cur, side)
    _keep_alive((pt.lo, pv.lo, pt.norm, pv.norm), cur)
    return _Tail(G, None, None, None, c0, c1, wc_t, wc_v, cw_aux, chain_t, chain_v, rowloss, losses)


def _joined_tail(plan, st, hp, gt, gv, gt2, gv2, ls, sw_t1, sw_v1, bank_streams, cur):
    """The critical path after the join is global logits -> Sinkhorn -> row losses: captured FIRST.  The logits and the solve
    need the global tokens only, so this stream joins the local branch (whose tail, with the bank chains run early, is
    the last bank product) BEHIND the solve, not in front of it.  What is left of the bank chains and the centrality
    weights feed only the row-loss kernel; with `bank_streams` they are forked from the join point (an event recorded
    before the Sinkhorn launch) and run beside the solve."""
    L, keep, local_stream = st.L, plan.keep, st.local_stream
    S, mean_t, mean_v = L["S"], L["mean_t"], L["mean_v"]
    fork = record_event(cur) if bank_streams is not None else None
    G, g_saved = global_logits(gt, gv, sw_t1, sw_v1, keep=True) if keep else (global_logits(gt, gv, sw_t1, sw_v1), None)
    tgt_r, tgt_c = ops.sinkhorn_targets(G, hp["beta"], 50)
    if local_stream is not None:
        wait_stream(cur, local_stream)
        _keep_alive((S, mean_t, mean_v, L["w_t"], L["w_v"], L["pt"].hi, L["pv"].hi), cur)
    if bank_streams is not None:
        for st_ in bank_streams:
            wait_event(st_, fork)
            if local_stream is not None:
                wait_stream(st_, local_stream)       # (their launches read the local branch's tokens / weights / means)
        with torch.cuda.stream(bank_streams[1]):
            chain_t = bank_chain(plan, st, 1)
        with torch.cuda.stream(bank_streams[0]):
            chain_v = bank_chain(plan, st, 0)
            wc_t, wc_v, cw_aux = ops.centrality_weights_pair(gt2, gv2, mean_t, mean_v, hp["centrality_scale"], keep)
        for st_ in bank_streams:
            wait_stream(cur, st_)
        _keep_alive((chain_t[4], chain_v[4], wc_t, wc_v) + ((chain_t[0].hi, chain_v[0].hi, chain_t[1], chain_v[1]) if keep else ()), cur)
    else:
        chain_v = bank_chain(plan, st, 0)
        chain_t = bank_chain(plan, st, 1)
        wc_t, wc_v, cw_aux = ops.centrality_weights_pair(gt2, gv2, mean_t, mean_v, hp["centrality_scale"], keep)
    c0, c1 = chain_t[4], chain_v[4]
    rowloss, losses = ops.row_losses_final(S, G, tgt_r, tgt_c, c0, c1, wc_t, wc_v, ls, plan.K, hp["temperature"],
                                           hp["uniform_weight"], hp["neighbor_weight"], hp["kl_weight"])
    return _Tail(G, g_saved, tgt_r, tgt_c, c0, c1, wc_t, wc_v, cw_aux, chain_t, chain_v, rowloss, losses)


def head_forward(text_feat, video_feat, text_mask, video_mask, mb_feat_t, mb_feat_v, mb_mask_t, mb_mask_v,
                 gt, gv, sw_t, sw_v, hp, logit_scale, prec=hip.PREC_BF16, keep=False, sw_t1=None, sw_v1=None, join=None,
                 bank_streams=None, local_stream=None, bank_early=0,
                 capture_order=((7, 5), (7, 1 << 30)), bank_prepared=None, prepared_out=None, bank_push=None, slot=0,
                 pipeline=None):
    """Forward of the head.  Returns (losses[5] device tensor, saved-state dict or None).

    `join`: optional callable run right before the first use of gt / gv.  Either the caller produces the
    global tokens on side streams while the local branch runs here and joins those streams in it, or --
    with gt = gv = None -- `join` runs the token clustering on the current stream and returns (gt, gv), while
    the local branch (prepare, scorer, B x B product) runs on `local_stream`; if `join` is a GENERATOR that
    issues one launch per next() and returns (gt, gv), its launches are interleaved with the local branch's.
    `bank_streams`: optional pair of side streams for the two memory-bank chains (see below).
    `bank_prepared`: optional (text, video) ops.Prepared of the bank (its persistent normalised bf16 shadow): the
    two bank prepare launches are skipped.  `prepared_out`: optional dict that receives the batch's prepared
    tokens ("pt", "pv") -- what the bank shadow is extended with at the push.
    `bank_push`: optional callable that pushes the batch into the memory bank (modeling.py:309-310).  The split tail
    calls it on its side stream as soon as both bank products have read the bank -- beside the Sinkhorn solve instead
    of behind it on the critical path; the other paths leave it to the caller.
    `pipeline` (split tail only; modeling.StepPipeline): consecutive steps captured overlapped.  The Sinkhorn solve then runs
    on `pipeline.tail_stream` (forked from this stream behind the logits) and NOTHING is joined back here: the streams still
    at work when this function returns -- solve, row losses, bank push -- are appended to `pipeline.pending`, to be joined
    into the capture's origin stream by whoever captures the steps (every join of a capture goes into its origin:
    capture_guard).  This stream is then free for the next step's prologue and clustering while this step's tail runs."""
    plan = head_plan(text_feat.shape, video_feat.shape[1], (mb_feat_t.shape[0], mb_feat_v.shape[0]), sw_t.b1.numel(),
                     hp["num_neighbors"], prec, keep, prepared_out is not None,
                     bank_streams is not None and local_stream is not None, gt is not None or join is not None)
    text_mask, video_mask, mb_mask_t, mb_mask_v = _masks_f32(text_mask, video_mask, mb_mask_t, mb_mask_v)
    cur = torch.cuda.current_stream()
    # The two bank chains, in the order they start early:
    #   text x bank-video, row mean     -> centrality of text j  (used by the v2t neighbour loss)
    #   bank-text x video, column mean  -> centrality of video j (used by the t2v neighbour loss)
    pb_t, pb_v = bank_prepared if bank_prepared is not None else (None, None)
    chains = ((mb_feat_v, mb_mask_v, pb_v, sw_v, plan.Nv, hip.OUT_ROWSUM),
              (mb_feat_t, mb_mask_t, pb_t, sw_t, plan.Nt, hip.OUT_COLSUM))
    st = _Step(text_feat, video_feat, text_mask, video_mask, sw_t, sw_v, chains, local_stream, bank_early, pipeline, {}, [None, None])
    gt, gv = _run_branches(plan, st, gt, gv, join, capture_order, cur)
    L = st.L
    if prepared_out is not None:
        prepared_out["pt"], prepared_out["pv"] = L["pt"], L["pv"]
    _check_global_tokens(gt, gv, hp)
    gt2 = gt.float().contiguous()                  # [B, G, d]: G = 1 at the MSR-VTT token counts
    gv2 = gv.float().contiguous()
    ls = logit_scale.detach().float().reshape(1).contiguous()
    if plan.split_tail:
        t = _split_tail(plan, st, hp, gt, gv, gt2, gv2, ls, logit_scale, sw_t1, sw_v1, bank_streams, bank_push, slot, cur)
    else:
        t = _joined_tail(plan, st, hp, gt, gv, gt2, gv2, ls, sw_t1, sw_v1, bank_streams, cur)
    saved = None
    if keep:
        (pbt, w_bt, lg_bt, aux2, _), (pbv, w_bv, lg_bv, aux1, _) = t.chain_t, t.chain_v
        saved = dict(pt=L["pt"], pv=L["pv"], pbt=pbt, pbv=pbv, w_t=L["w_t"], w_v=L["w_v"], w_bt=w_bt, w_bv=w_bv,
                     lg_t=L["lg_t"], lg_v=L["lg_v"], lg_bt=lg_bt, lg_bv=lg_bv,
                     aux=(L["aux0"], aux1, aux2), S=L["S"], G=t.G, tgt_r=t.tgt_r, tgt_c=t.tgt_c,
                     c0=t.c0, c1=t.c1, wc_t=t.wc_t, wc_v=t.wc_v, cw_aux=t.cw_aux, mean_t=L["mean_t"], mean_v=L["mean_v"],
                     ls=ls, gt2=gt2, gv2=gv2, g_saved=t.g_saved)
    return t.losses, saved


def _rows(prep, first, count):
    """Rows [first, first + count) of a Prepared token set (contiguous views)."""
    return ops.Prepared(prep.hi[first:first + count], prep.lo[first:first + count] if prep.lo is not None else None,
                        prep.norm[first:first + count], None, count, prep.d,
                        prep.f16[first:first + count] if prep.f16 is not None else None)


def head_forward_sharded(text_feat, video_feat, text_mask, video_mask, mb_feat_t, mb_feat_v, mb_mask_t, mb_mask_v,
                         gt, gv, sw_t, sw_v, hp, logit_scale, prec, rank, world, bank_prepared=None, prepared_out=None,
                         sw_t1=None, sw_v1=None, join=None, local_stream=None):
    """Loss-only forward with the similarity and bank work SHARDED over `world` ranks: rank r owns the
    samples [r*b, (r+1)*b) of the gathered batch and computes the two slabs of S it needs for its rows of either
    direction (2/W of the batch x batch product), its slice of both bank centrality vectors (1/W of the bank
    products) and its rows of the row losses.  Exchanged: the centrality slices (one all-gather of 2b floats) and
    the row terms (one all-reduce of 8B floats); the token scorers, the global logits and the Sinkhorn solve are
    small and stay replicated.  Returns the same [5] losses on every rank as head_forward.

    `join` (gt = gv = None): callable that produces the global tokens -- the rank's share of the clustering plus the
    all-gather of the [b, c, d] tokens -- on the CURRENT stream, while the local branch (prepare, scorers, the four
    products) runs on `local_stream`; the global logits and the Sinkhorn solve follow the clustering without waiting for
    the local branch.  Both collectives of this function are issued on the current stream, in program order, so that
    every rank enqueues the same sequence whatever its streams do.  No host synchronisation anywhere: with the "nccl"
    backend (RCCL) the whole sharded step captures into ONE HIP graph (tools/rccl_capture_probe.py,
    profiles/r03_rccl_capture.txt)."""
    from . import comm
    plan = head_plan(text_feat.shape, video_feat.shape[1], (mb_feat_t.shape[0], mb_feat_v.shape[0]), sw_t.b1.numel(),
                     hp["num_neighbors"], prec, prepared_out=prepared_out is not None,
                     global_tokens=gt is not None or join is not None, shard=(rank, world))
    B, Nt, Nv, M, K, b, r0 = plan.B, plan.Nt, plan.Nv, plan.M, plan.K, plan.b, plan.r0
    p_bb, p_mlp, p_bank = plan.p_bb, plan.p_mlp, plan.p_bank
    text_mask, video_mask, mb_mask_t, mb_mask_v = _masks_f32(text_mask, video_mask, mb_mask_t, mb_mask_v)
    L = {}

    def local_branch():
        pt, pv = ops.prepare_tokens_pair(text_feat, text_mask, video_feat, video_mask, want_lo=plan.lo_b, want_colsum=True,
                                         want_f16=plan.f16_b)
        w_t, _ = token_weights(pt, text_mask, sw_t, B, Nt, p_mlp)
        w_v, _ = token_weights(pv, video_mask, sw_v, B, Nv, p_mlp)
        if prepared_out is not None:
            prepared_out["pt"], prepared_out["pv"] = pt, pv
        pt_r, pv_r = _rows(pt, r0 * Nt, b * Nt), _rows(pv, r0 * Nv, b * Nv)
        w_t_r, w_v_r = w_t[r0:r0 + b].contiguous(), w_v[r0:r0 + b].contiguous()
        L["S_rows"], _ = ops.local_level(pt_r, pv, w_t_r, w_v, b, Nt, B, Nv, p_bb, hip.OUT_FULL)          # S[r0:r0+b, :]
        L["S_cols"], _ = ops.local_level(pt, pv_r, w_t, w_v_r, B, Nt, b, Nv, p_bb, hip.OUT_FULL)          # S[:, r0:r0+b]
        if bank_prepared is not None:
            pbt, pbv = bank_prepared
        else:
            pbt = ops.prepare_tokens(mb_feat_t, mb_mask_t, want_lo=plan.lo_k)
            pbv = ops.prepare_tokens(mb_feat_v, mb_mask_v, want_lo=plan.lo_k)
        w_bt, _ = token_weights(pbt, mb_mask_t, sw_t, M, Nt, p_bank)
        w_bv, _ = token_weights(pbv, mb_mask_v, sw_v, M, Nv, p_bank)
        p1, _ = ops.local_level(pt_r, pbv, w_t_r, w_bv, b, Nt, M, Nv, p_bank, hip.OUT_ROWSUM)
        p0, _ = ops.local_level(pbt, pv_r, w_bt, w_v_r, M, Nt, b, Nv, p_bank, hip.OUT_COLSUM)
        L["mine"] = torch.stack((ops.reduce_parts(p0, 1.0 / M), ops.reduce_parts(p1, 1.0 / M)))          # [2, b]
        L["mean_t"], L["mean_v"] = ops.colsum_pair(pt.colsum, 1.0 / pt.n_tok, pv.colsum, 1.0 / pv.n_tok)
        L["keep"] = (pt, pv, w_t, w_v, pbt, pbv, w_bt, w_bv, pt_r, pv_r, w_t_r, w_v_r)                       # alive until the join

    cur = torch.cuda.current_stream()
    two = local_stream is not None and join is not None
    if two:
        wait_stream(local_stream, cur)
        with torch.cuda.stream(local_stream):
            local_branch()
    if join is not None:
        gt, gv = join()
    if not two:
        local_branch()
    _check_global_tokens(gt, gv, hp)
    gt2 = gt.float().contiguous()
    gv2 = gv.float().contiguous()
    G = global_logits(gt, gv, sw_t1, sw_v1)
    tgt_r, tgt_c = ops.sinkhorn_targets(G, hp["beta"], 50)
    if two:
        wait_stream(cur, local_stream)
        # (the batch's prepared tokens: the bank push -- caller, this stream -- reads them)
        _keep_alive([L["S_rows"], L["S_cols"], L["mine"], L["mean_t"], L["mean_v"]]
                    + [t_ for prep in L["keep"][:2] for t_ in (prep.hi, prep.lo, prep.norm)], cur)
    mine = L["mine"]
    everyone = torch.empty((world, 2, b), dtype=torch.float32, device=mine.device)
    comm.all_gather_into_tensor(everyone.view(-1), mine.view(-1))
    c0 = everyone[:, 0, :].reshape(B).contiguous()
    c1 = everyone[:, 1, :].reshape(B).contiguous()
    wc_t, wc_v, _ = ops.centrality_weights_pair(gt2, gv2, L["mean_t"], L["mean_v"], hp["centrality_scale"], False)
    ls = logit_scale.detach().float().reshape(1).contiguous()
    rowloss = ops.row_losses_slab(L["S_rows"], L["S_cols"], r0, G, tgt_r, tgt_c, c0, c1, wc_t, wc_v, ls, K, hp["temperature"])
    comm.all_reduce(rowloss)                       # every row was written by exactly one rank, zeros elsewhere
    return ops.loss_finalize(rowloss, hp["uniform_weight"], hp["neighbor_weight"], hp["kl_weight"])
