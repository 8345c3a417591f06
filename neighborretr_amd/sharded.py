"""The loss of the TRAINING step sharded over the ranks (reference sketch: AllGather2, until_module.py:391-412).

The reference replicates: after the all-gather every rank evaluates the full B x B problem plus both B x M bank
products, and gradients need no reduction because every rank differentiates the whole loss.  At global B = 1024
(BASELINE configs[2]) that is 677 GF per step repeated W times.  Here rank r owns the samples [r b, (r+1) b):

  heavy, on the HIP kernels, ONE autograd node (ShardedLocalFn: the grouped kernels of the replicated training step --
  one prepare launch per token set, fused scorer + softmax, nr_local_level_bwd_group / nr_pool_weight_bwd_group for the
  four products' gradients, the fused scorer backward -- 30 forward+backward launches instead of four LocalLevelFn nodes):
      S[r-slab, :]  = local_level(text_r, video_all)        [b, B]     rows of the text->video direction
      S[:, r-slab]  = local_level(text_all, video_r)        [B, b]     rows of the video->text direction
      text_r x bank-video [b, M],  bank-text x video_r [M, b]          1/W of both bank products -> centrality slices
  sharded by samples as well: the token clustering of the rank's b samples (fused HIP forward, hand-derived backward).  Its
      masked stage uses the maximum distance over the WHOLE gathered batch (cluster.py:473-475): the ranks all-reduce that
      one number per modality between the stage's front and back kernels; the [b, d] global tokens are all-gathered
  row-local, on the HIP row-loss kernels (SlabRowLossFn: nr_row_losses_fwd_slab / nr_row_losses_bwd_slab -- the same per-row
      code as the replicated loss): the four loss terms of the rank's 2 b rows (until_module.py:56-359);
  light, replicated, ONE more node (ShardedGlobalFn): global logits G = gt gv^T (exact-fp32 MFMA), Sinkhorn targets (no
      gradient), centrality weights, the slab row terms -- nr_gemm_nt_f32, nr_centrality_weights_pair, nr_row_losses_fwd_slab
      forward; nr_row_losses_bwd_slab, nr_centrality_weights_bwd_pair, nr_global_logits_bwd backward.
      (tests/slab_terms_torch.py restates the row terms in torch ops: the cross-check of tests/test_sharded_gpu.py.)

Each rank's L_r is ITS rows' share of every term, so sum_r L_r = L (the reference's loss).  Cross-rank values enter
through differentiable collectives whose backward is the matching reduction (all-gather <-> reduce-scatter(sum),
all-reduce <-> all-reduce), so every rank's autograd graph yields dL_r/dtheta and dL_r/dX for ALL gathered samples.
DDP averages parameter gradients over ranks, so L_r is differentiated as W L_r (`_ScaleGrad`): mean_r(W dL_r) = dL,
the reference's effective gradient; the exchange step's backward then AVERAGES the feature gradients over the ranks
(dist.PackedAllGather with args.shard_loss: reduce-scatter / W), which gives every rank dL/dX of its own samples.
Returned values are the FULL losses on every rank (one all-reduce of five numbers), with the partial gradient attached.
"""
import torch

from . import comm, ops
from .functional import local_level_sim
from .head import _masks_f32, _rows


class _GatherCat(torch.autograd.Function):
    """all-gather + cat on dim 0; backward: every rank's gradient of the gathered tensor summed, this rank's slice."""

    @staticmethod
    def forward(ctx, x, rank, world):
        ctx.rank, ctx.world, ctx.n = rank, world, x.shape[0]
        x = x.contiguous()
        out = torch.empty((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        comm.all_gather_into_tensor(out, x)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        if comm.backend() == "gloo":                          # no reduce_scatter in gloo
            g = g.clone()
            comm.all_reduce(g)
            return g[ctx.rank * ctx.n:(ctx.rank + 1) * ctx.n], None, None
        out = torch.empty((ctx.n,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
        comm.reduce_scatter_tensor(out, g)
        return out, None, None


class _AllReduceSum(torch.autograd.Function):
    """y = sum over ranks of x (every rank gets y); backward: sum over ranks of the upstream gradients."""

    @staticmethod
    def forward(ctx, x):
        y = x.clone()
        comm.all_reduce(y)
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        comm.all_reduce(g)
        return g


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


class SlabRowLossFn(torch.autograd.Function):
    """This rank's share of the four loss terms -- its rows of either direction, from the two slabs of S it owns -- on the HIP
    row-loss kernels (nr_row_losses_fwd_slab / nr_row_losses_bwd_slab: the same per-row code as the replicated loss, top-K
    by wave arg-max rounds, ties to the lowest column).  Returns the PARTIAL [5] losses (total, centrality, uniform,
    neighbour, kl) of the rank's rows, normalised like the full loss (sum over ranks = the reference's values)."""

    @staticmethod
    def forward(ctx, S_rows, S_cols, G, tgt_r, tgt_c, c0, c1, wc_text, wc_video, logit_scale, hp, row0):
        args = [t.detach().float().contiguous() for t in (S_rows, S_cols, G, tgt_r, tgt_c, c0, c1, wc_text, wc_video)]
        ls = logit_scale.detach().float().reshape(1).contiguous()
        K, T = int(hp["num_neighbors"]), float(hp["temperature"])
        rowloss = ops.row_losses_slab(args[0], args[1], row0, *args[2:], ls, K, T)
        ctx.save_for_backward(*args, ls)
        ctx.hp, ctx.row0 = dict(hp), int(row0)
        return ops.loss_finalize(rowloss, hp["uniform_weight"], hp["neighbor_weight"], hp["kl_weight"])

    @staticmethod
    def backward(ctx, g):
        from .backward import coef_rowloss
        S_rows, S_cols, G, tgt_r, tgt_c, c0, c1, wc_text, wc_video, ls = ctx.saved_tensors
        hp, r0 = ctx.hp, ctx.row0
        n, B = S_rows.shape
        coef = coef_rowloss(g.float().contiguous(), hp, B)
        dS, dG_dir, dC, dwc, dls = ops.row_losses_bwd_slab(S_rows, S_cols, r0, G, tgt_r, tgt_c, c0, c1, wc_text, wc_video, ls,
                                                           int(hp["num_neighbors"]), float(hp["temperature"]), coef)
        dG = torch.zeros_like(G)
        dG[r0:r0 + n] += dG_dir[0]                       # direction 0 read rows of G, direction 1 columns
        dG[:, r0:r0 + n] += dG_dir[1].t()
        d_wt, d_wv = torch.zeros_like(wc_text), torch.zeros_like(wc_video)
        d_wt[r0:r0 + n], d_wv[r0:r0 + n] = dwc[0], dwc[1]
        return (dS[0], dS[1].t().contiguous(), dG, None, None, dC[0].sum(0), dC[1].sum(0), d_wt, d_wv,
                dls.sum().reshape(1), None, None)


class ShardedLocalFn(torch.autograd.Function):
    """The token side of rank r's share of the loss: from the gathered features to its two slabs of S, its slices of the two
    bank centrality vectors and the means of the normalised tokens (modeling.py:483-514 x4, :403-424).  Forward and backward on
    the grouped HIP kernels of the replicated training step (backward._local_backward is the B x B form of the same)."""

    @staticmethod
    def forward(ctx, model, masks, r0, b, text_feat, video_feat, mb_feat_t, mb_feat_v, w1t, b1t, w2t, b2t, w1v, b1v, w2v, b2v):
        from . import head, hip
        text_mask, video_mask, mb_mask_t, mb_mask_v = masks
        B, Nt, d = text_feat.shape
        Nv, M = video_feat.shape[1], mb_feat_v.shape[0]
        prec = model._prec()
        sw_t, sw_v = model.scorer_weights("text_weight_fc"), model.scorer_weights("video_weight_fc")
        p_bb, p_mlp, p_bank = head.backward_plan(prec)          # a differentiated forward: split-bf16 on the batch side (head_forward)
        tf, vf = text_feat.detach(), video_feat.detach()
        pt, pv = ops.prepare_tokens_pair(tf, text_mask, vf, video_mask, want_lo=True, want_colsum=True)
        pbt, pbv = ops.prepare_tokens_pair(mb_feat_t, mb_mask_t, mb_feat_v, mb_mask_v, want_lo=True)
        w_t, _ = head.token_weights(pt, text_mask, sw_t, B, Nt, p_mlp)
        w_v, _ = head.token_weights(pv, video_mask, sw_v, B, Nv, p_mlp)
        w_bt, _ = head.token_weights(pbt, mb_mask_t, sw_t, M, Nt, p_bank)
        w_bv, _ = head.token_weights(pbv, mb_mask_v, sw_v, M, Nv, p_bank)
        pt_r, pv_r = _rows(pt, r0 * Nt, b * Nt), _rows(pv, r0 * Nv, b * Nv)
        w_t_r, w_v_r = w_t[r0:r0 + b].contiguous(), w_v[r0:r0 + b].contiguous()
        S_rows, aux_r = ops.local_level(pt_r, pv, w_t_r, w_v, b, Nt, B, Nv, p_bb, hip.OUT_FULL, True)         # S[r0:r0+b, :]
        S_cols, aux_c = ops.local_level(pt, pv_r, w_t, w_v_r, B, Nt, b, Nv, p_bb, hip.OUT_FULL, True)         # S[:, r0:r0+b]
        p1, aux1 = ops.local_level(pt_r, pbv, w_t_r, w_bv, b, Nt, M, Nv, p_bank, hip.OUT_ROWSUM, True)        # text_r x bank-video
        p0, aux2 = ops.local_level(pbt, pv_r, w_bt, w_v_r, M, Nt, b, Nv, p_bank, hip.OUT_COLSUM, True)        # bank-text x video_r
        c1_mine, c0_mine = ops.reduce_parts(p1, 1.0 / M), ops.reduce_parts(p0, 1.0 / M)
        mean_t, mean_v = ops.colsum_pair(pt.colsum, 1.0 / pt.n_tok, pv.colsum, 1.0 / pv.n_tok)
        ctx.st = dict(pt=pt, pv=pv, pbt=pbt, pbv=pbv, pt_r=pt_r, pv_r=pv_r, w_t=w_t, w_v=w_v, w_bt=w_bt, w_bv=w_bv, w_t_r=w_t_r,
                      w_v_r=w_v_r, aux=(aux_r, aux_c, aux1, aux2), masks=masks, r0=int(r0), b=int(b), exact=prec == hip.PREC_BF16X3,
                      plan=(p_bb, p_mlp, p_bank), model=model)
        ctx.save_for_backward(text_feat, video_feat, mb_feat_t, mb_feat_v)
        ctx.set_materialize_grads(False)
        return S_rows, S_cols, c1_mine, c0_mine, mean_t, mean_v

    @staticmethod
    def backward(ctx, dS_rows, dS_cols, d_c1, d_c0, dmean_t, dmean_v):
        from .backward import token_tail
        st = ctx.st
        if st is None:
            raise RuntimeError("ShardedLocalFn: backward a second time (its saved state is released by the first)")
        feats = ctx.saved_tensors
        text_mask, video_mask, _, _ = st["masks"]
        Nt, Nv, M = feats[0].shape[1], feats[1].shape[1], feats[3].shape[0]
        B, r0, b = feats[0].shape[0], st["r0"], st["b"]
        aux_r, aux_c, aux1, aux2 = st["aux"]
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=feats[0].device)       # noqa: E731 -- a slab that brought no gradient
        dS_rows = z(b, B) if dS_rows is None else dS_rows.float().contiguous()
        dS_cols = z(B, b) if dS_cols is None else dS_cols.float().contiguous()
        d_c1 = z(b) if d_c1 is None else d_c1.float().contiguous()
        d_c0 = z(b) if d_c0 is None else d_c0.float().contiguous()
        # ---- the four products, each stated once (ops.sim_backward derives the two d_x launches and the six weight sums; the sharded
        # loss has no scalar-walk form).  A gradient that only a row range of the tokens receives (the rank's b texts / videos) is
        # accumulated in a buffer of its own and added to the full one afterwards.
        t, v, bt, bv = (ops.TokenSet(st[p], st[w]) for p, w in (("pt", "w_t"), ("pv", "w_v"), ("pbt", "w_bt"), ("pbv", "w_bv")))
        t_r, v_r = ops.TokenSet(st["pt_r"], st["w_t_r"]), ops.TokenSet(st["pv_r"], st["w_v_r"])
        Pc = ops.SimProduct(t, v_r, dS_cols, 0, 1.0, aux_c)
        Pr = ops.SimProduct(t_r, v, dS_rows, 0, 1.0, aux_r)
        P1 = ops.SimProduct(t_r, bv, d_c1, 1, 1.0 / M, aux1)
        P2 = ops.SimProduct(bt, v_r, d_c0, 2, 1.0 / M, aux2)
        (d_tn, d_wt), (d_tn_r, d_wt_r), (d_vn, d_wv), (d_vn_r, d_wv_r), g_bv, g_bt = ops.sim_backward(
            [ops.SimTarget(t, [Pc]), ops.SimTarget(t_r, [Pr, P1]), ops.SimTarget(v, [Pr]), ops.SimTarget(v_r, [Pc, P2]),
             ops.SimTarget(bv, [P1], False), ops.SimTarget(bt, [P2], False)], use_lo=st["exact"], fallback=False)
        d_tn[r0 * Nt:(r0 + b) * Nt] += d_tn_r
        d_vn[r0 * Nv:(r0 + b) * Nv] += d_vn_r
        d_wt[r0 * Nt:(r0 + b) * Nt] += d_wt_r
        d_wv[r0 * Nv:(r0 + b) * Nv] += d_wv_r
        d_text, d_video, scorer = token_tail((t, v, bt, bv), feats, (text_mask, video_mask), ((d_tn, d_wt), (d_vn, d_wv), g_bt, g_bv),
                                             (dmean_t, dmean_v), st["plan"], st["model"])
        ctx.st = None
        return (None, None, None, None, d_text, d_video, None, None, *scorer)


class ShardedGlobalFn(torch.autograd.Function):
    """The rest of rank r's share: global logits, Sinkhorn targets, centrality weights and the four row terms of its 2 b rows
    (modeling.py:403-444, until_module.py:56-359) -> the PARTIAL [5] losses (sum over ranks = the reference's values).  Forward
    and backward on the HIP kernels (the slab forms of backward._global_backward)."""

    @staticmethod
    def forward(ctx, hp, r0, S_rows, S_cols, c0, c1, mean_t, mean_v, gt, gv, logit_scale):
        b, B = S_rows.shape
        args = [t.detach().float().contiguous() for t in (S_rows, S_cols, c0, c1, mean_t, mean_v, gt, gv)]
        S_rows, S_cols, c0, c1, mean_t, mean_v, gt2, gv2 = args
        ls = logit_scale.detach().float().reshape(1).contiguous()
        G = ops.gemm_nt_f32(gt2, gv2)
        tgt_r, tgt_c = ops.sinkhorn_targets(G, hp["beta"], 50)
        wc_t, wc_v, cw_aux = ops.centrality_weights_pair(gt2, gv2, mean_t, mean_v, hp["centrality_scale"], True)
        K, T = int(hp["num_neighbors"]), float(hp["temperature"])
        rowloss = ops.row_losses_slab(S_rows, S_cols, r0, G, tgt_r, tgt_c, c0, c1, wc_t, wc_v, ls, K, T)
        ctx.save_for_backward(S_rows, S_cols, c0, c1, mean_t, mean_v, gt2, gv2, ls, G, tgt_r, tgt_c, wc_t, wc_v, *cw_aux)
        ctx.hp, ctx.r0, ctx.shapes = dict(hp), int(r0), (gt.shape, gv.shape)
        return ops.loss_finalize(rowloss, hp["uniform_weight"], hp["neighbor_weight"], hp["kl_weight"])

    @staticmethod
    def backward(ctx, g):
        from .backward import coef_rowloss
        S_rows, S_cols, c0, c1, mean_t, mean_v, gt2, gv2, ls, G, tgt_r, tgt_c, wc_t, wc_v, gn_t, gn_v, wtok_t, wtok_v = ctx.saved_tensors
        hp, r0 = ctx.hp, ctx.r0
        b, B = S_rows.shape
        coef = coef_rowloss(g.float().contiguous(), hp, B)
        dS, dG_dir, dC, dwc, dls = ops.row_losses_bwd_slab(S_rows, S_cols, r0, G, tgt_r, tgt_c, c0, c1, wc_t, wc_v, ls,
                                                           int(hp["num_neighbors"]), float(hp["temperature"]), coef)
        dG = torch.zeros_like(G)
        dG[r0:r0 + b] += dG_dir[0]                       # direction 0 read rows of G, direction 1 columns
        dG[:, r0:r0 + b] += dG_dir[1].t()
        dw_t, dw_v = torch.zeros_like(wc_t), torch.zeros_like(wc_v)
        dw_t[r0:r0 + b], dw_v[r0:r0 + b] = dwc[0], dwc[1]
        dg_t, dmean_t, dg_v, dmean_v = ops.centrality_weights_bwd_pair(gt2, gn_t, mean_t, wtok_t, dw_t, gv2, gn_v, mean_v, wtok_v, dw_v,
                                                                       hp["centrality_scale"])
        d_gt, d_gv = ops.global_logits_bwd(dG, gt2, gv2, dg_t, dg_v)
        return (None, None, dS[0], dS[1].t().contiguous(), dC[0].sum(0), dC[1].sum(0), dmean_t, dmean_v,
                d_gt.reshape(ctx.shapes[0]), d_gv.reshape(ctx.shapes[1]), dls.sum().reshape(()))


def sharded_training_losses(model, text_feat, video_feat, text_mask, video_mask, mb_feat_t, mb_feat_v, mb_mask_t, mb_mask_v,
                            hp, logit_scale, rank, world, noise=None):
    """-> [5] tensor (total, centrality, uniform, neighbour, kl): full values, this rank's share of the gradient (x W)."""
    B, Nt, d = text_feat.shape
    M = mb_feat_v.shape[0]
    K, T = int(hp["num_neighbors"]), float(hp["temperature"])
    if B % world:
        raise ValueError("the gathered batch must divide over the ranks")
    if K > B:
        raise ValueError(f"num_neighbors={K} > batch={B}")
    b, r0 = B // world, rank * (B // world)
    sl = slice(r0, r0 + b)
    text_mask, video_mask, mb_mask_t, mb_mask_v = _masks_f32(text_mask, video_mask, mb_mask_t, mb_mask_v)
    # ---- token clustering: every rank clusters ITS samples (fused forward + hand-derived backward; the batch-wide maximum
    # distance of the masked stage is exchanged inside, modeling._merge_sharded) and the global tokens are gathered with a
    # differentiable all-gather: d gt of a rank's samples = the sum of every rank's W dL_r / d gt, so the clustering
    # parameters receive W x (the contribution of this rank's samples) and DDP's mean over the ranks is the full gradient.
    # `model.shard_clustering = False`: the replicated form (every rank differentiates the whole clustering).
    if model.shard_clustering and text_feat.is_cuda and model._grouped_stages_supported(text_feat, video_feat):
        gt_l, gv_l = model._merge_sharded(text_feat, video_feat, text_mask, video_mask, noise or {}, rank, world)
        if gt_l.shape[1] != 1 or gv_l.shape[1] != 1:
            raise RuntimeError("the sharded training loss covers one global token per sample (until_module.py:321)")
        gg = _GatherCat.apply(torch.stack((gt_l.reshape(b, d).float(), gv_l.reshape(b, d).float()), 1), rank, world)   # [B, 2, d]
        gt, gv = gg[:, 0], gg[:, 1]
    else:
        gt, gv = model.merge_global_features(text_feat, video_feat, text_mask, video_mask, noise)
        if gt.shape[1] != 1 or gv.shape[1] != 1:
            raise RuntimeError("the sharded training loss covers one global token per sample (until_module.py:321)")
        gt, gv = gt.reshape(B, d).float(), gv.reshape(B, d).float()
    # ---- the rank's slabs of S, its slices of the bank centralities and the token means: one node on the grouped HIP kernels
    from .functional import _mlp_params
    S_rows, S_cols, c1_mine, c0_mine, mean_t, mean_v = ShardedLocalFn.apply(
        model, (text_mask, video_mask, mb_mask_t, mb_mask_v), r0, b, text_feat, video_feat, mb_feat_t, mb_feat_v,
        *_mlp_params(model, "text_weight_fc"), *_mlp_params(model, "video_weight_fc"))
    cc = _GatherCat.apply(torch.stack((c0_mine, c1_mine), 1), rank, world)       # [B, 2]: one collective for both vectors
    c0, c1 = cc[:, 0], cc[:, 1]          # video / text centralities (used by the t2v / v2t neighbour loss, modeling.py:393-398)
    # ---- global logits, Sinkhorn targets (no gradient), centrality weights, the four terms on this rank's rows: one node
    part = ShardedGlobalFn.apply(hp, r0, S_rows, S_cols, c0, c1, mean_t, mean_v, gt, gv, logit_scale.reshape(()).float())
    full = part.detach().clone()
    comm.all_reduce(full)                                                              # the reference's (full) values
    # value: full;  gradient: W x this rank's share (DDP's mean over ranks then yields the full-loss gradient)
    return full + (_ScaleGrad.apply(part, float(world)) - part.detach())
