"""Evaluation of the retrieval head with the N x N similarity SHARDED over the ranks.

Reference: training/evaluator.py -- every rank gathers all test features (5 all_gathers, :173-177), scatters them back
into dataset order (:180-189), then EVERY rank computes the whole N x N matrix in 64 x 64 tiles with a device-to-host
copy per tile (:21-63) and ranks it with a NumPy sort (utils/metrics.py:58-66).

Here: one packed all-gather (neighborretr_amd.dist) + one index scatter; rank r then runs the fused local_level kernel
(split-bf16: rank-exact) on ITS row slab only -- texts [r n/W, (r+1) n/W) against all videos, 1/W of the work --, counts
the text->video ranks of its rows and its partial video->text column counts on the GPU (nr_slab_ranks), and three tiny
collectives (diagonal N floats, row counts 2n ints, column counts 2N ints) give every rank the same R@K as the
reference's sort.  Nothing but 4N integers ever leaves the device.
"""
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import comm

from . import ops
from .metrics import RetrievalMetrics


def _world(args):
    return int(getattr(args, "world_size", 1))


def rank_sample_indices(n, world, rank):
    """Dataset indices rank `rank` extracts features for: rank, rank + W, ... PADDED to ceil(n / W) entries by wrapping around
    to the start of the dataset -- torch's DistributedSampler(shuffle=False), which the reference's test loader uses
    (dataloaders/data_dataloaders.py).  Every rank therefore hands the SAME number of rows to the packed all-gather (ranks
    issuing a collective with different byte counts hang RCCL); the duplicates overwrite identical rows in dataset_order."""
    import math
    per = math.ceil(n / world)
    return (torch.arange(rank, rank + per * world, world) % n)[:per]


def gather_eval_features(text_feat, video_feat, idx, text_mask, video_mask, args):
    """evaluator.py:173-189: gather every rank's cached features and put them back into dataset order (`idx` = dataset
    index of every local sample; duplicates from a padded last batch overwrite each other with identical rows), trimmed to
    idx.max() + 1.  -> (text_feat, video_feat, text_mask, video_mask) in dataset order, identical on every rank."""
    from .dist import packed_allgather
    with torch.no_grad():
        tf, vf, ix, tm, vm = packed_allgather(text_feat, video_feat, idx, text_mask, video_mask, args)
    return dataset_order(tf, vf, ix, tm, vm)


def dataset_order(text_feat, video_feat, idx, text_mask, video_mask):
    """evaluator.py:180-189: row idx[k] of every output <- row k of the input (later duplicates win), trimmed to
    idx.max() + 1; positions no sample maps to stay zero."""
    with torch.no_grad():
        idx = idx.reshape(-1).long()
        n = int(idx.max().item()) + 1
        out = []
        for t in (text_feat, video_feat, text_mask, video_mask):
            dst = torch.zeros((max(n, t.shape[0]),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            dst.index_copy_(0, idx, t)
            out.append(dst[:n].contiguous())
    return tuple(out)


def slab_bounds(n, world, rank):
    """Rows [r0, r1) of rank `rank`: slabs differ by at most one row."""
    base, extra = divmod(n, world)
    r0 = rank * base + min(rank, extra)
    return r0, r0 + base + (1 if rank < extra else 0)


def slab_rows(n, world, rank):
    """The number of rows of rank `rank`'s slab."""
    r0, r1 = slab_bounds(n, world, rank)
    return r1 - r0


def _gathered_rows(mine, n_rows, W):
    """[K, width] of this rank (row r0 + i at column i, width = ceil(n_rows / W): slabs differ by at most one row, padded to the
    largest) -> [K, n_rows] of every rank's rows: one padded all-gather, every rank's real rows cut back out."""
    K, width = mine.shape
    if W == 1:
        return mine[:, :n_rows].contiguous()
    allv = torch.empty((W, K, width), dtype=mine.dtype, device=mine.device)
    comm.all_gather_into_tensor(allv.view(-1), mine.reshape(-1))
    return torch.cat([allv[r, :, :slab_rows(n_rows, W, r)] for r in range(W)], dim=1).contiguous()


def _slab_similarity(model, text_feat, video_feat, text_mask, video_mask, r0, r1, chunk=256):
    """Rows [r0, r1) of the text x video similarity, on the rank-exact (split-bf16) path of the fused kernel."""
    old = model.precision
    model.precision = "bf16x3"
    try:
        with torch.no_grad():
            rows = []
            for lo in range(r0, r1, chunk):                 # [chunk, N] pieces keep the kernel's outputs small
                hi = min(lo + chunk, r1)
                S, _ = model.get_similarity_logits(text_feat[lo:hi], video_feat, text_mask[lo:hi], video_mask, shaped=True)
                rows.append(S)
            if rows:
                return torch.cat(rows, 0)
            return torch.empty((0, video_feat.shape[0]), dtype=torch.float32, device=text_feat.device)
    finally:
        model.precision = old


def sharded_retrieval_ranks(model, text_feat, video_feat, text_mask, video_mask, args, chunk=256):
    """-> (greater_t2v, equal_t2v, greater_v2t, equal_v2t), int64 numpy arrays of length N, identical on every rank:
    for text i the number of videos scoring above / equal to its own video (metrics.py:58-66 on S), and for video j the
    number of texts scoring above / equal to its own text (the same on S.T)."""
    S_slab, N, _, W, rank, _ = _eval_slab(model, text_feat, video_feat, text_mask, video_mask, args, None, chunk)
    return _ranks_from_slab(S_slab, N, W, rank)


def _ranks_from_slab(S_slab, N, W, rank):
    """sharded_retrieval_ranks from this rank's slab S[r0:r1, :] (three collectives)."""
    r0, r1 = slab_bounds(N, W, rank)
    dev = S_slab.device
    n = r1 - r0
    width = -(-N // W)
    mine = torch.full((1, width), float("nan"), dtype=torch.float32, device=dev)      # the diagonal of the whole matrix: this slab's part
    if n:
        mine[0, :n] = S_slab[torch.arange(n, device=dev), torch.arange(r0, r1, device=dev)]
    diag = _gathered_rows(mine, N, W)[0]
    if n:
        g_rows, e_rows, g_cols, e_cols = ops.slab_ranks(S_slab, r0, diag)
    else:
        z = lambda k: torch.zeros((k,), dtype=torch.int32, device=dev)      # noqa: E731
        g_rows, e_rows, g_cols, e_cols = z(0), z(0), z(N), z(N)
    cols = torch.stack((g_cols, e_cols))
    rows_pad = torch.zeros((2, width), dtype=torch.int32, device=dev)
    rows_pad[0, :n], rows_pad[1, :n] = g_rows, e_rows
    if W > 1:
        comm.all_reduce(cols)                              # partial column counts -> complete
    rows = _gathered_rows(rows_pad, N, W).cpu().numpy()
    cols = cols.cpu().numpy()
    return rows[0].astype(np.int64), rows[1].astype(np.int64), cols[0].astype(np.int64), cols[1].astype(np.int64)


def _multi_sentence_ranks(S_slab, ends, Ns, V, W, rank):
    """(ranks [Ns] int32 on the device: every sentence's rank of its own video, < 0 where it is not ranked; gmax [V, V]: every
    caption group's best score against every video), the same on every rank (two collectives)."""
    dev = S_slab.device
    group_end = torch.from_numpy(ends.astype(np.int32)).to(dev)
    r0, r1 = slab_bounds(Ns, W, rank)
    n = r1 - r0
    mine = torch.zeros((1, -(-Ns // W)), dtype=torch.int32, device=dev)
    if n:
        greater, equal_before, gmax = ops.group_slab_ranks(S_slab, r0, group_end)
        mine[0, :n] = torch.where(greater < 0, greater, greater + equal_before)
    else:
        gmax = torch.full((V, V), float("-inf"), dtype=torch.float32, device=dev)
    if W > 1:
        comm.all_reduce(gmax, op="max")
    return _gathered_rows(mine, Ns, W)[0], gmax


# ---- top-k lists and hubness (DESIGN.md "Top-k lists and hubness") ------------------------------------------------------
# Rank r scores only its slab of rows, as above.  Text->video (row) lists are complete on the rank that owns the row;
# video->text (column) lists are partial per slab: one all-gather of every rank's [N, k] partial lists and nr_topk_merge
# give every rank the same complete lists.  k-occurrences of the rows: each rank counts its own rows, one int32 all-reduce
# sums them.  Only integers and the selected scores cross the ranks; the N x N matrix never leaves its slabs.

def _group_ends(cut_off_points, Ns, V):
    ends = np.asarray(cut_off_points, dtype=np.int64) + 1
    if len(ends) != V or (np.diff(ends) <= 0).any() or ends[0] <= 0 or ends[-1] != Ns:
        raise ValueError(f"cut_off_points must give {V} non-empty, increasing sentence groups ending at {Ns - 1}")
    return ends


def _ground_truth(n_rows, n_cols, ends, dev):
    """(row_begin, row_end [n_rows], col_begin, col_end [n_cols]) int32 on `dev`: the ground-truth range of every row query
    (over the columns) and of every column query (over the rows).  ends = None: item i's ground truth is item i; otherwise
    ends[g] = one past the last sentence (row) of video (column) g."""
    if ends is None:
        r, c = np.arange(n_rows), np.arange(n_cols)
        rb, re_, cb, ce = r, r + 1, c, c + 1
    else:
        rb = np.searchsorted(ends, np.arange(n_rows), side="right")          # the group of sentence s
        re_ = rb + 1
        cb, ce = np.concatenate(([0], ends[:-1])), ends
    return tuple(torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev) for a in (rb, re_, cb, ce))


def _slab_row_lists(S_slab, k, n_cols):
    if S_slab.shape[0]:
        return ops.slab_topk_rows(S_slab, k)
    dev = S_slab.device
    return torch.empty((0, k), dtype=torch.int32, device=dev), torch.empty((0, k), dtype=torch.float32, device=dev)


def _column_lists(S_slab, n_rows, n_cols, k, W, rank):
    """Complete column lists [n_cols, k] on every rank: this slab's partial lists, one all-gather, nr_topk_merge."""
    r0, r1 = slab_bounds(n_rows, W, rank)
    dev = S_slab.device
    if r1 > r0:
        ci, cv = ops.slab_topk_cols(S_slab, r0, k)
    else:
        ci = torch.full((n_cols, k), -1, dtype=torch.int32, device=dev)
        cv = torch.full((n_cols, k), float("-inf"), dtype=torch.float32, device=dev)
    if W == 1:
        return ci, cv
    part = torch.stack((ci, cv.view(torch.int32)))                   # scores travel as their int32 bits
    allp = torch.empty((W, 2, n_cols, k), dtype=torch.int32, device=dev)
    comm.all_gather_into_tensor(allp.view(-1), part.view(-1))
    return ops.topk_merge(allp[:, 0].contiguous(), allp[:, 1].contiguous().view(torch.float32))


def _topk_from_slab(S_slab, n_rows, n_cols, k, W, rank):
    r0, r1 = slab_bounds(n_rows, W, rank)
    dev = S_slab.device
    ri, rv = _slab_row_lists(S_slab, k, n_cols)
    if W > 1:                                                        # every rank's row lists: indices and score bits, transposed
        mine = torch.zeros((2 * k, -(-n_rows // W)), dtype=torch.int32, device=dev)
        mine[:k, :r1 - r0], mine[k:, :r1 - r0] = ri.T, rv.view(torch.int32).T
        rows = _gathered_rows(mine, n_rows, W)
        ri, rv = rows[:k].T.contiguous(), rows[k:].T.contiguous().view(torch.float32)
    ci, cv = _column_lists(S_slab, n_rows, n_cols, k, W, rank)
    return ri, rv, ci, cv


def _lists_entry(idx, unit_end, gt_begin, gt_end):
    """What a "hubness" entry carries of its top-k lists under "lists" (hubness_test): the lists, their resampling units and their
    ground-truth ranges, as NumPy arrays."""
    return {"idx": idx.cpu().numpy().astype(np.int32), "unit_end": np.asarray(unit_end, dtype=np.int64),
            "gt_begin": gt_begin.cpu().numpy().astype(np.int32), "gt_end": gt_end.cpu().numpy().astype(np.int32)}


def _gathered_row_lists(ri, n_rows, W, rank):
    """Every rank's row lists [n_rows, k] int32 from this rank's ri: the indices travel transposed, as in _topk_from_slab."""
    if W == 1:
        return ri
    r0, r1 = slab_bounds(n_rows, W, rank)
    k = ri.shape[1]
    mine = torch.zeros((k, -(-n_rows // W)), dtype=torch.int32, device=ri.device)
    mine[:, :r1 - r0] = ri.T
    return _gathered_rows(mine, n_rows, W).T.contiguous()


def _row_hubness(S_slab, n_rows, n_cols, k, W, rank, ends, lists=False):
    """Hubness of the row (text -> video) lists: each rank counts its rows, one int32 all-reduce.  lists: the entry also carries
    every rank's row lists (one more all-gather); their unit is the query, in a multi-sentence set the video."""
    r0, r1 = slab_bounds(n_rows, W, rank)
    rb, re_, _, _ = _ground_truth(n_rows, n_cols, ends, S_slab.device)
    ri, _ = _slab_row_lists(S_slab, k, n_cols)
    occ_t = torch.stack(ops.topk_occurrences(ri, n_cols, rb[r0:r1], re_[r0:r1]))
    if W > 1:
        comm.all_reduce(occ_t)                                        # the ranks' row counts -> the whole matrix's
    occ_t = occ_t.cpu().numpy()
    hub = RetrievalMetrics.hubness_from_occurrences(occ_t[0], occ_t[1], k, n_rows)
    if lists:
        unit_end = np.arange(n_rows) if ends is None else np.asarray(ends, dtype=np.int64) - 1
        hub["lists"] = _lists_entry(_gathered_row_lists(ri, n_rows, W, rank), unit_end, rb, re_)
    return hub


def _col_hubness(S_slab, n_rows, n_cols, k, W, rank, ends, lists=False):
    """Hubness of the column (video -> text) lists: partial lists, one all-gather, merge (_column_lists).  lists: the entry also
    carries them (complete on every rank already); their unit is the video."""
    _, _, cb, ce = _ground_truth(n_rows, n_cols, ends, S_slab.device)
    ci, _ = _column_lists(S_slab, n_rows, n_cols, k, W, rank)
    occ_v = torch.stack(ops.topk_occurrences(ci, n_rows, cb, ce)).cpu().numpy()
    hub = RetrievalMetrics.hubness_from_occurrences(occ_v[0], occ_v[1], k, n_cols)
    if lists:
        hub["lists"] = _lists_entry(ci, np.arange(n_cols), cb, ce)
    return hub


def _hubness_from_slab(S_slab, n_rows, n_cols, k, W, rank, ends, lists=False):
    return (_row_hubness(S_slab, n_rows, n_cols, k, W, rank, ends, lists),
            _col_hubness(S_slab, n_rows, n_cols, k, W, rank, ends, lists))


def _check_hubness_k(hubness_k):
    """hubness_k as an int: 0 or None for no hubness entry, else a list length ops._check_k accepts."""
    hubness_k = int(hubness_k or 0)
    if hubness_k:
        ops._check_k(hubness_k)
    return hubness_k


class EvalSlab(NamedTuple):
    """This rank's rows of the text (sentence) x video similarity and where they sit: S [r1 - r0, n_cols] for the rows
    slab_bounds(n_rows, W, rank); ends = None for a single-sentence set, else one past the last sentence of every video."""
    S: torch.Tensor
    n_rows: int
    n_cols: int
    W: int
    rank: int
    ends: Optional[np.ndarray]


def _eval_slab(model, text_feat, video_feat, text_mask, video_mask, args, cut_off_points, chunk):
    """The EvalSlab of this rank (it unpacks as S_slab, n_rows, n_cols, W, rank, ends)."""
    W = _world(args)
    rank = comm.get_rank() if W > 1 else 0
    n_rows, n_cols = text_feat.shape[0], video_feat.shape[0]
    if cut_off_points is None:
        if n_cols != n_rows:
            raise ValueError("single-sentence retrieval: one text per video expected")
        ends = None
    else:
        ends = _group_ends(cut_off_points, n_rows, n_cols)
    r0, r1 = slab_bounds(n_rows, W, rank)
    S_slab = _slab_similarity(model, text_feat, video_feat, text_mask, video_mask, r0, r1, chunk)
    return EvalSlab(S_slab, n_rows, n_cols, W, rank, ends)


def sharded_topk(model, text_feat, video_feat, text_mask, video_mask, k, args, cut_off_points=None, chunk=256):
    """-> (t2v_idx [Nt,k] int32, t2v_val [Nt,k] fp32, v2t_idx [V,k], v2t_val [V,k]) on the device, identical on every rank:
    the top-k videos of every text (sentence) and the top-k texts of every video, scores descending, ties by lower index,
    NaN never selected, padded with -1 / -inf; values are the exact bits of the rank-exact similarity."""
    S_slab, n_rows, n_cols, W, rank, _ = _eval_slab(model, text_feat, video_feat, text_mask, video_mask, args, cut_off_points, chunk)
    ops._check_k(k)
    return _topk_from_slab(S_slab, n_rows, n_cols, int(k), W, rank)


def sharded_hubness(model, text_feat, video_feat, text_mask, video_mask, args, k=15, cut_off_points=None, chunk=256):
    """-> (t2v_hub, v2t_hub): RetrievalMetrics.hubness_from_occurrences of the text->video and video->text top-k lists,
    identical on every rank.  Multi-sentence sets (cut_off_points as in sharded_multi_sentence_metrics): a sentence's ground
    truth is its video, a video's every sentence of its group."""
    S_slab, n_rows, n_cols, W, rank, ends = _eval_slab(model, text_feat, video_feat, text_mask, video_mask, args, cut_off_points,
                                                       chunk)
    ops._check_k(k)
    return _hubness_from_slab(S_slab, n_rows, n_cols, int(k), W, rank, ends)


# ---- test-time hubness reduction: IS, DSL, QB-Norm (DESIGN.md "Test-time hubness reduction") -------------------------------
# T (text -> video, rows are the queries) and V (video -> text, columns are the queries) are normalised copies of this rank's
# slab of S.  The column normalisers of T come from the ranks' partial (max, sum) pairs: one all-gather of [W, 2, N] fp32 and a
# combine in rank order, so every rank holds the same bits.  V's row normalisers are rank-local.  QB-Norm replaces the test
# queries by a querybank (the memory bank) and normalises only the queries whose top-1 lies in the bank's activation set.

TEST_NORM_MODES = ("is", "dsl", "qbnorm", "sinkhorn", "qbsinkhorn")
TEST_NORM_LABELS = {"is": "IS", "dsl": "DSL", "qbnorm": "QB-Norm", "sinkhorn": "Sinkhorn", "qbsinkhorn": "QB-Sinkhorn"}
SINKHORN_MODES = ("sinkhorn", "qbsinkhorn")                 # the iterated modes (DESIGN.md "Test-time Sinkhorn normalisation")
BANK_MODES = ("qbnorm", "qbsinkhorn")                       # the modes that need a querybank


def test_norm_label(mode, beta, n_iter=None):
    """The tag of the log lines of the normalised metrics, e.g. "[IS b=20]"; the iterated modes: "[Sinkhorn b=20 it=50]"."""
    if mode in SINKHORN_MODES and n_iter is not None:
        return f"[{TEST_NORM_LABELS[mode]} b={beta:g} it={int(n_iter)}]"
    return f"[{TEST_NORM_LABELS[mode]} b={beta:g}]"


def _check_n_iter(n_iter):
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or int(n_iter) < 1:
        raise ValueError(f"test_norm iterations must be an integer >= 1, got {n_iter!r}")
    return int(n_iter)


def _check_test_norm(mode, beta, qb_k, hubness_k):
    if mode not in TEST_NORM_MODES:
        raise ValueError(f"test_norm mode must be one of {TEST_NORM_MODES}, got {mode!r}")
    beta = ops._check_beta(beta)
    qb_k = ops._check_k(qb_k)
    return beta, qb_k, _check_hubness_k(hubness_k)


def _querybank(model, querybank, dev):
    """(text_feat, text_mask, video_feat, video_mask) of the querybank on `dev`: `querybank` as such a tuple, or None for the
    model's memory bank (mb_feat_t / mb_mask_t / mb_feat_v / mb_mask_v)."""
    if querybank is None:
        bank = (model.mb_feat_t, model.mb_mask_t, model.mb_feat_v, model.mb_mask_v)
    else:
        bank = tuple(querybank)
        if len(bank) != 4:
            raise ValueError("querybank must be (text_feat, text_mask, video_feat, video_mask)")
    if bank[0].dim() != 3 or bank[2].dim() != 3 or bank[0].shape[0] == 0 or bank[2].shape[0] == 0:
        raise ValueError("qbnorm needs a querybank and the model's memory bank is empty: call load_memory_bank(...) before "
                         "evaluating, or pass querybank=(text_feat, text_mask, video_feat, video_mask)")
    tf, tm, vf, vm = bank
    return tf.to(dev).float(), tm.to(dev).float(), vf.to(dev).float(), vm.to(dev).float()


def _bank_slabs(model, text_feat, video_feat, text_mask, video_mask, bank, W, rank, chunk=256):
    """(Qt_slab, Qv_slab) of this rank: bank texts slab_bounds(M, W, rank) x every test video, and this rank's test texts x every
    bank video, on the rank-exact path of S."""
    btf, btm, bvf, bvm = bank
    q0, q1 = slab_bounds(btf.shape[0], W, rank)
    r0, r1 = slab_bounds(text_feat.shape[0], W, rank)
    Qt = _slab_similarity(model, btf, video_feat, btm, video_mask, q0, q1, chunk)
    Qv = _slab_similarity(model, text_feat, bvf, text_mask, bvm, r0, r1, chunk)
    return Qt, Qv


def _check_bank_slabs(Qt, Qv, S_slab, n_cols, n_bank_texts, W, rank):
    """The shapes _bank_slabs gives rank `rank`: its bank texts x every test video, its test texts x every bank video."""
    q = slab_rows(int(n_bank_texts), W, rank)
    if Qt.shape[0] != q or Qt.shape[1] != n_cols or Qv.shape[0] != S_slab.shape[0]:
        raise ValueError(f"bank slabs of rank {rank} must be [{q}, {n_cols}] and [{S_slab.shape[0]}, bank videos], got "
                         f"{tuple(Qt.shape)} and {tuple(Qv.shape)}")


def _gathered_lse(stats, W):
    """This rank's column pairs [2, L] -> lse [L] over every rank's rows: one all-gather, combine in rank order."""
    if W > 1:
        allp = torch.empty((W,) + tuple(stats.shape), dtype=torch.float32, device=stats.device)
        comm.all_gather_into_tensor(allp.view(-1), stats.reshape(-1))
    else:
        allp = stats[None]
    return ops.hubnorm_combine(allp)


def _activated(idx, n_gallery):
    """bool [n_gallery]: the items that appear in some list of idx [n_q, k] (absent slots -1 ignored), as int32 counts."""
    dev = idx.device
    none = torch.zeros((idx.shape[0],), dtype=torch.int32, device=dev)
    occ, _ = ops.topk_occurrences(idx, n_gallery, none, none)
    return occ


def _gate(top1, active):
    """int32 [n_q]: 1 where the query's top-1 (idx [n_q, 1], -1 = none) is an active item."""
    i = top1[:, 0].long()
    return ((i >= 0) & active[i.clamp(min=0)]).to(torch.int32)


def _normalised_from_slab(S_slab, n_rows, n_cols, W, rank, mode, beta, bank_slabs=None, qb_k=1):
    """(T_slab, V_slab) of this rank's slab S[r0:r1] (rows: texts / sentences, columns: videos).  qbnorm: bank_slabs =
    (Qt_slab, Qv_slab) as _bank_slabs scores them."""
    if mode in ("is", "dsl"):
        c_v = _gathered_lse(ops.hubnorm_col_stats(S_slab, beta), W)
        c_t = ops.hubnorm_row_lse(S_slab, beta)
        return ops.hubnorm_apply(S_slab, beta, mode, col_norm=c_v, row_norm=c_t)
    Qt, Qv = bank_slabs
    n_bank_v = Qv.shape[1]
    c_v = _gathered_lse(ops.hubnorm_col_stats(Qt, beta), W)
    c_t = ops.hubnorm_row_lse(Qv, beta)
    # A_v: videos in the top-qb_k list of some bank text (this rank's bank rows, one int32 all-reduce)
    occ_v = _activated(_slab_row_lists(Qt, qb_k, n_cols)[0], n_cols)
    if W > 1:
        comm.all_reduce(occ_v)
    # A_t: test texts in the top-qb_k list of some bank video (partial column lists of Qv, merged)
    occ_t = _activated(_column_lists(Qv, n_rows, n_bank_v, qb_k, W, rank)[0], n_rows)
    row_gate = _gate(_slab_row_lists(S_slab, 1, n_cols)[0], occ_v > 0)
    col_gate = _gate(_column_lists(S_slab, n_rows, n_cols, 1, W, rank)[0], occ_t > 0)
    return ops.hubnorm_apply(S_slab, beta, "is", col_norm=c_v, row_gate=row_gate, row_norm=c_t, col_gate=col_gate)


# ---- test-time Sinkhorn normalisation (DESIGN.md "Test-time Sinkhorn normalisation") -------------------------------------------
# The reference's log-domain Sinkhorn (until_module.py:223-266) on the test similarity: n_iter times a row half-step (rank-local:
# every rank holds the whole v) and a column half-step (the ranks' [2, L] partial pairs, one all-gather, combined in rank order:
# every rank holds the same bits of v).  The slab never leaves its rank.

def _log_marginals(n_rows, n_cols, ends, dev):
    """(log_mu [n_rows], log_nu [n_cols]) fp32 on `dev`: every row the same mass; every column the same mass, or (ends: one past
    the last sentence of every video) the share of the rows it owns."""
    log_mu = np.full((n_rows,), -np.log(float(n_rows)) if n_rows else 0.0)
    if ends is None:
        log_nu = np.full((n_cols,), -np.log(float(n_cols)) if n_cols else 0.0)
    else:
        sizes = np.diff(np.concatenate(([0], np.asarray(ends, dtype=np.int64)))).astype(np.float64)
        log_nu = np.log(sizes / float(n_rows))
    return tuple(torch.from_numpy(a.astype(np.float32)).to(dev) for a in (log_mu, log_nu))


def _sinkhorn_potentials(A_slab, beta, log_mu, log_nu, n_iter, W):
    """(u, v, marginal_err) of the slab A [rows of this rank, L]: n_iter iterations from u = v = 0 with the log marginals log_mu
    (of THIS rank's rows) and log_nu [L].  u [rows] is rank-local, v [L] and marginal_err (float: the largest
    |row mass / mu - 1| after the last iteration, over every rank's rows that take part) are the same on every rank.  One
    all-gather of 8L bytes per iteration and one max all-reduce of 4 bytes at the end."""
    A_slab = ops._slab_2d(A_slab)
    n, L = A_slab.shape
    dev = A_slab.device
    u = torch.zeros((n,), dtype=torch.float32, device=dev)
    v = torch.zeros((L,), dtype=torch.float32, device=dev)
    ws = ops.sinknorm_workspace(n, L, dev)
    allp = torch.empty((W, 2, L), dtype=torch.float32, device=dev) if W > 1 else None
    for _ in range(n_iter):
        ops.sinknorm_row(A_slab, beta, v, log_mu, out=u)
        if W > 1:
            stats = ops.sinknorm_col_stats(A_slab, beta, u, ws)
            comm.all_gather_into_tensor(allp.view(-1), stats.view(-1))
            ops.sinknorm_finish_cols(allp, log_nu, out=v)
        else:                                               # one rank: the blocks' pairs are finished straight from the workspace
            ops.sinknorm_finish_cols(ops.sinknorm_col_stats(A_slab, beta, u, ws, want_stats=False), log_nu, out=v)
    err = torch.zeros((1,), dtype=torch.float32, device=dev)
    if n and L:
        err = ops.sinknorm_row_err(A_slab, beta, u, v, log_mu).max().reshape(1)
    if W > 1:
        comm.all_reduce(err, op="max")
    return u, v, float(err.item())


def _sinkhorn_from_slab(S_slab, n_rows, n_cols, W, rank, mode, beta, n_iter, ends=None, bank_slabs=None, n_bank_texts=None):
    """(T_slab, V_slab, info) of this rank's slab.  sinkhorn: ONE output, V_slab is T_slab (text->video ranks its rows,
    video->text its columns).  qbsinkhorn: bank_slabs = (Qt_slab, Qv_slab) as _bank_slabs scores them, n_bank_texts = the
    bank's text count M (Qt_slab holds the rows slab_bounds(M, W, rank)); T takes the column
    potentials of Qt, V the row potentials of Qv (the `is` apply with col_norm = -v_t, row_norm = -u_v).  info: "iters" and
    "marginal_err" (qbsinkhorn: of Qt and of Qv)."""
    dev = S_slab.device
    r0, r1 = slab_bounds(n_rows, W, rank)
    if mode == "sinkhorn":
        log_mu, log_nu = _log_marginals(n_rows, n_cols, ends, dev)
        u, v, err = _sinkhorn_potentials(S_slab, beta, log_mu[r0:r1].contiguous(), log_nu, n_iter, W)
        T = ops.sinknorm_apply(S_slab, beta, u, v)
        return T, T, dict(iters=n_iter, marginal_err=(err, err))
    Qt, Qv = bank_slabs
    M_t, M_v = int(n_bank_texts), Qv.shape[1]
    q0, q1 = slab_bounds(M_t, W, rank)
    if Qt.shape[0] != q1 - q0:
        raise ValueError(f"Qt_slab must hold the {q1 - q0} bank rows of rank {rank}, got {Qt.shape[0]}")
    mu_t, nu_t = _log_marginals(M_t, n_cols, None, dev)
    _, v_t, err_t = _sinkhorn_potentials(Qt, beta, mu_t[q0:q1].contiguous(), nu_t, n_iter, W)
    mu_v, nu_v = _log_marginals(n_rows, M_v, None, dev)
    u_v, _, err_v = _sinkhorn_potentials(Qv, beta, mu_v[r0:r1].contiguous(), nu_v, n_iter, W)
    T, V = ops.hubnorm_apply(S_slab, beta, "is", col_norm=-v_t, row_norm=-u_v)
    return T, V, dict(iters=n_iter, marginal_err=(err_t, err_v))


def _metrics_and_units(T_slab, V_slab, n_rows, n_cols, W, rank, ends):
    """(t2v, v2t, units): text->video ranks from the rows of T, video->text from the columns of V (multi-sentence sets: the group
    ranks of T, the group max of V; V_slab is T_slab: both directions from one pass), and the two directions' resampling units
    (entries, unit_end, median) of the bootstrap (_query_units / _video_units)."""
    if ends is None:
        gt, et, gv, ev = _ranks_from_slab(T_slab, n_rows, W, rank)
        if V_slab is not T_slab:
            _, _, gv, ev = _ranks_from_slab(V_slab, n_rows, W, rank)
        units = _query_units(gt, et), _query_units(gv, ev)
        t2v, v2t = (RetrievalMetrics.metrics_from_ranks(u[0]) for u in units)
        return t2v, v2t, units
    ranks, gmax = _multi_sentence_ranks(T_slab, ends, n_rows, n_cols, W, rank)
    if V_slab is not T_slab:
        _, gmax = _multi_sentence_ranks(V_slab, ends, n_rows, n_cols, W, rank)
    t2v = RetrievalMetrics.multi_sentence_metrics_from_ranks(ranks[ranks >= 0])      # < 0: own score NaN / inf, not ranked
    gv, ev = (x.cpu().numpy() for x in ops.diag_ranks(gmax.T.contiguous()))          # [video, caption group], metrics.py:146-148
    video_units = _query_units(gv, ev)
    return t2v, RetrievalMetrics.metrics_from_ranks(video_units[0]), (_video_units(ranks, ends), video_units)


def _metrics_from_normalised(T_slab, V_slab, n_rows, n_cols, W, rank, ends, hubness_k, units=None, lists=False):
    """(t2v, v2t) of _metrics_and_units, and with hubness_k the hubness of T's row lists and V's column lists (lists: each entry
    with its "lists").  units: a list that receives the two directions' resampling units."""
    t2v, v2t, u = _metrics_and_units(T_slab, V_slab, n_rows, n_cols, W, rank, ends)
    if units is not None:
        units.extend(u)
    if hubness_k and V_slab is T_slab:
        t2v["hubness"], v2t["hubness"] = _hubness_from_slab(T_slab, n_rows, n_cols, hubness_k, W, rank, ends, lists)
    elif hubness_k:
        t2v["hubness"] = _row_hubness(T_slab, n_rows, n_cols, hubness_k, W, rank, ends, lists)
        v2t["hubness"] = _col_hubness(V_slab, n_rows, n_cols, hubness_k, W, rank, ends, lists)
    return t2v, v2t


# ---- bootstrap confidence intervals (DESIGN.md "Bootstrap confidence intervals") ------------------------------------------------------
# The queries are resampled with replacement, n_boot times, on the GPU (nr_bootstrap_rank_stats): percentile intervals for every
# reported metric and, for a correction, a paired bootstrap (the same draws) of "corrected minus raw".  The unit of resampling is the
# query (its equal[i] tied entries stay together); in a multi-sentence set it is the VIDEO in both directions, since the sentences
# of one video are not independent.  Every rank holds the same rank vectors and computes every resample itself: no collective.

BOOTSTRAP_MAX = 1 << 20
BOOTSTRAP_CUTS = (1, 5, 10, 50)


def _check_bootstrap(bootstrap, seed=0, level=0.95):
    """None for bootstrap = 0, else (n_boot, seed, level); an integer in [0, 2^20], a seed in [0, 2^64 - 1), a level in (0, 1)."""
    if isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer)) or not 0 <= int(bootstrap) <= BOOTSTRAP_MAX:
        raise ValueError(f"bootstrap must be an integer in [0, 2^20], got {bootstrap!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64) - 1:
        raise ValueError(f"bootstrap_seed must be an integer in [0, 2^64 - 1), got {seed!r}")
    if isinstance(level, bool) or not isinstance(level, (int, float, np.floating)) or not 0.0 < float(level) < 1.0:
        raise ValueError(f"bootstrap_level must lie in (0, 1), got {level!r}")
    return (int(bootstrap), int(seed), float(level)) if int(bootstrap) else None


def _query_units(greater, equal):
    """(entries, unit_end, median) of a direction ranked by counts: entries = ranks_from_counts (the `ind` its metrics come from),
    query i owns its equal[i] consecutive entries; the median is np.median's."""
    equal = np.asarray(equal, dtype=np.int64)
    return RetrievalMetrics.ranks_from_counts(greater, equal), np.cumsum(equal) - 1, "mid"


def _video_units(ranks, ends):
    """Multi-sentence text->video units: video g owns its ranked sentences (an unranked one, rank < 0, is dropped: a video may be
    left empty); ends[g] = one past its last sentence; the median is torch.median's (the lower one)."""
    ranks = ranks.cpu().numpy().astype(np.int64)
    kept = np.cumsum(ranks >= 0)
    return ranks[ranks >= 0], kept[np.asarray(ends, dtype=np.int64) - 1] - 1, "low"


def _dev32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _rank_bootstrap(units, other, boot, seed, dev):
    """(stats, paired): the ops.bootstrap_rank_stats rows of `units` = (entries, unit_end, median) and, with `other`, of both from
    ONE launch (the same draws) next to the paired summary of units minus other; paired is None without other."""
    n_boot, _, level = boot
    rankings = tuple(units[:2]) + (() if other is None else tuple(other[:2]))
    stats = ops.bootstrap_rank_stats(*(_dev32(x, dev) for x in rankings), cuts=BOOTSTRAP_CUTS, seed=seed, b0=0, n_boot=n_boot)
    stats = stats.cpu().numpy()
    if other is None:
        return stats, None
    paired = RetrievalMetrics.paired_bootstrap_summary(stats[:, 0], stats[:, 1], BOOTSTRAP_CUTS, units[0], other[0], level, units[2])
    return stats, dict(paired, seed=seed)


def _bootstrap_direction(units, boot, seed, dev, raw_units=None):
    """{"bootstrap": summary of `units`} and, with raw_units, "bootstrap_vs_raw": the paired summary of units minus raw_units from ONE
    launch (the same draws); summaries carry the units they resampled ("entries", "unit_end")."""
    entries, unit_end, median = units
    stats, paired = _rank_bootstrap(units, raw_units, boot, seed, dev)
    out = {"bootstrap": RetrievalMetrics.bootstrap_summary(stats[:, 0], BOOTSTRAP_CUTS, entries, boot[2], median)}
    out["bootstrap"].update(seed=seed, entries=np.asarray(entries, dtype=np.int64), unit_end=np.asarray(unit_end, dtype=np.int64))
    if paired is not None:
        out["bootstrap_vs_raw"] = paired
    return out


def _add_bootstrap(t2v, v2t, units, boot, dev, raw_units=None):
    """Adds the bootstrap entries to the two directions' dictionaries: seed for text->video, seed + 1 for video->text."""
    if not boot:
        return
    for side, metrics in enumerate((t2v, v2t)):
        metrics.update(_bootstrap_direction(units[side], boot, boot[1] + side, dev, None if raw_units is None else raw_units[side]))


# ---- local scaling: CSLS, NICDM, LS (DESIGN.md "Local scaling") ---------------------------------------------------------------------
# Every score is rescaled by statistics of its text's and its video's k-nearest neighbourhoods: a text's neighbourhood is its
# top-k videos (a rank-local row list), a video's its top-k texts (the column lists, complete on every rank after the one
# all-gather and merge of _column_lists).  ONE output T: its rows rank text->video, its columns video->text.  The lists hold the
# exact bits of S and their sums have a fixed order, so T has the same bits whatever the world size.

LOCAL_SCALING_MODES = ("csls", "nicdm", "ls")
LOCAL_SCALING_LABELS = {"csls": "CSLS", "nicdm": "NICDM", "ls": "LS"}


def local_scaling_label(mode, k, bank=False):
    """The tag of the log lines of the locally scaled metrics: "[CSLS k=10]", with a querybank "[QB-NICDM k=10]"."""
    return f"[{'QB-' if bank else ''}{LOCAL_SCALING_LABELS[mode]} k={int(k)}]"


def _check_local_scaling(mode, k, hubness_k=0):
    if mode not in LOCAL_SCALING_MODES:
        raise ValueError(f"local_scaling mode must be one of {LOCAL_SCALING_MODES}, got {mode!r}")
    if isinstance(k, bool) or int(k) != k:
        raise ValueError(f"local_scaling k must be an integer in [1, 128], got {k!r}")
    k = ops._check_k(k)
    return k, _check_hubness_k(hubness_k)


def _local_scaling_stats(S_slab, n_rows, n_cols, W, rank, mode, k, bank_slabs=None, n_bank_texts=None):
    """(row_stat [rows of this rank], col_stat [n_cols]) of `mode`: the neighbourhood means (csls, nicdm) or k-th values (ls).
    Rows from this rank's lists of S (bank: of Qv), columns from the merged lists of S over n_rows (bank: of Qt over the bank's
    n_bank_texts rows); col_stat is the same bits on every rank."""
    if bank_slabs is None:
        ri, rv = _slab_row_lists(S_slab, k, n_cols)
        ci, cv = _column_lists(S_slab, n_rows, n_cols, k, W, rank)
    else:
        Qt, Qv = bank_slabs
        _check_bank_slabs(Qt, Qv, S_slab, n_cols, n_bank_texts, W, rank)
        ri, rv = _slab_row_lists(Qv, k, Qv.shape[1])
        ci, cv = _column_lists(Qt, int(n_bank_texts), n_cols, k, W, rank)
    which = 1 if mode == "ls" else 0
    return ops.localscale_stats(ri, rv)[which], ops.localscale_stats(ci, cv)[which]


def _local_scaled_from_slab(S_slab, n_rows, n_cols, W, rank, mode, k, bank_slabs=None, n_bank_texts=None):
    """T_slab of this rank's slab S[r0:r1] (rows: texts / sentences, columns: videos).  bank_slabs = (Qt_slab, Qv_slab) as
    _bank_slabs scores them and n_bank_texts = the bank's text count: the neighbourhoods are taken in the querybank."""
    row_stat, col_stat = _local_scaling_stats(S_slab, n_rows, n_cols, W, rank, mode, k, bank_slabs, n_bank_texts)
    return ops.localscale_apply(S_slab, mode, row_stat, col_stat)


# ---- mutual proximity: emp, gauss (DESIGN.md "Mutual proximity") ---------------------------------------------------------------------
# Every score becomes the probability that it beats its row's line and its column's line (the independent form P_row P_col).  A
# row's line is rank-local (S_slab, or Qv_slab with a querybank).  A column's line spans the ranks: every rank needs every rank's
# rows of the column source (S, or Qt over the bank's rows), gathered in blocks of MP_GATHER_ROWS rows per rank and fed to the
# accumulating count kernel (emp), or one all-gather of the ranks' [3, L] fp64 (count, mean, M2) triples (gauss).  ONE output T:
# its rows rank text->video, its columns video->text.  emp is integer counts and two divisions: the same bits whatever the split.

MUTUAL_PROXIMITY_MODES = ("emp", "gauss")
MP_GATHER_ROWS = 256            # B: rows per rank and collective of the column source; the gather buffer is W B L floats


def mutual_proximity_label(mode, bank=False):
    """The tag of the log lines of the mutual-proximity metrics: "[MP-emp]", with a querybank "[QB-MP-gauss]"."""
    if mode not in MUTUAL_PROXIMITY_MODES:
        raise ValueError(f"mutual_proximity mode must be one of {MUTUAL_PROXIMITY_MODES}, got {mode!r}")
    return f"[{'QB-' if bank else ''}MP-{mode}]"


def _check_mutual_proximity(mode, hubness_k=0):
    if mode not in MUTUAL_PROXIMITY_MODES:
        raise ValueError(f"mutual_proximity mode must be one of {MUTUAL_PROXIMITY_MODES}, got {mode!r}")
    return _check_hubness_k(hubness_k)


def _mp_column_counts(S_slab, src_slab, n_src, W, rank):
    """(c2 [rows of this rank, L], col_cnt [L]) int32: the doubled rank of every score of S_slab in its column of the source
    (src_slab: this rank's rows slab_bounds(n_src, W, rank) of it) over EVERY rank's rows, and the columns' non-NaN counts.
    ceil(ceil(n_src / W) / B) all-gathers of B rows per rank and one int32 all-reduce; W = 1: no collective."""
    dev = S_slab.device
    L = S_slab.shape[1]
    mine = src_slab.shape[0]
    _, col_cnt = ops.mp_line_counts(Q=src_slab)
    if W == 1:
        return ops.mp_col_counts(S_slab, src_slab), col_cnt
    comm.all_reduce(col_cnt)
    B = MP_GATHER_ROWS
    c2 = torch.zeros(tuple(S_slab.shape), dtype=torch.int32, device=dev)
    block = torch.empty((B, L), dtype=torch.float32, device=dev)
    allb = torch.empty((W, B, L), dtype=torch.float32, device=dev)
    for b0 in range(0, -(-n_src // W), B):
        have = max(0, min(B, mine - b0))
        if have:
            block[:have] = src_slab[b0:b0 + have]
        if have < B:
            block[have:].fill_(float("nan"))                          # the padding of a short block (never counted: see below)
        comm.all_gather_into_tensor(allb.view(-1), block.view(-1))
        for r in range(W):                                            # only the rows rank r really holds
            real = max(0, min(B, slab_rows(n_src, W, r) - b0))
            if real:
                ops.mp_col_counts(S_slab, allb[r, :real], out=c2)
    return c2, col_cnt


def _mp_column_moments(src_slab, W):
    """(mean, sd) [L] fp32 of the columns of the source over every rank's rows: this rank's (count, mean, M2) triples, one
    all-gather, Chan's update in rank order (the same bits on every rank)."""
    parts = ops.mp_col_moments(src_slab)
    if W > 1:
        allp = torch.empty((W,) + tuple(parts.shape), dtype=torch.float64, device=parts.device)
        comm.all_gather_into_tensor(allp.view(-1), parts.view(-1))
    else:
        allp = parts[None]
    return ops.mp_moments_combine(allp)


def _mutual_proximity_from_slab(S_slab, n_rows, n_cols, W, rank, mode, bank_slabs=None, n_bank_texts=None):
    """T_slab of this rank's slab S[r0:r1] (rows: texts / sentences, columns: videos).  bank_slabs = (Qt_slab, Qv_slab) as
    _bank_slabs scores them and n_bank_texts = the bank's text count: the reference lines are taken in the querybank."""
    S_slab = ops._slab_2d(S_slab)
    if bank_slabs is None:
        row_src, col_src, n_src = S_slab, S_slab, n_rows
    else:
        Qt, Qv = bank_slabs
        _check_bank_slabs(Qt, Qv, S_slab, n_cols, n_bank_texts, W, rank)
        row_src, col_src, n_src = ops._slab_2d(Qv), ops._slab_2d(Qt), int(n_bank_texts)
    if max(n_src, row_src.shape[1]) >= ops.hip.MP_LINE_MAX:
        raise ValueError(f"mutual proximity: a reference line of {max(n_src, row_src.shape[1])} entries is too long for exact counts")
    if mode == "emp":
        row_cnt, _ = ops.mp_line_counts(R=row_src)
        r2 = ops.mp_row_counts(S_slab, row_src)
        c2, col_cnt = _mp_column_counts(S_slab, col_src, n_src, W, rank)
        return ops.mp_emp_apply(S_slab, r2, c2, row_cnt, col_cnt)
    row_mean, row_sd = ops.mp_row_moments(row_src)
    col_mean, col_sd = _mp_column_moments(col_src, W)
    return ops.mp_gauss_apply(S_slab, row_mean, row_sd, col_mean, col_sd)


# ---- rank-aware IR metrics: MRR, mAP, nDCG@10, R-precision (DESIGN.md "Rank-aware IR metrics") ------------------------------------
# R@K ranks only the best caption of a video; these metrics need the rank of EVERY relevant (sentence, video) pair in both
# directions.  Pair s is (row s, column g(s)).  rt[s] (text->video) is row-local.  rv[s] (video->text: the rank of sentence s among
# all sentences in the column of its video) is a column count against the pair's own score, which lives on another rank's slab:
# the own scores are gathered first (4 n_total bytes), every rank counts its rows ahead of every pair (nr_pair_ranks), and one
# int32 SUM all-reduce (4 n_total bytes) completes the counts.  rt travels like the multi-sentence ranks: one int32 all-gather.

def _check_ir(ir):
    """ir as a bool: the flag of the public functions (--ir_metrics {0,1})."""
    if isinstance(ir, (bool, np.bool_)):
        return bool(ir)
    if isinstance(ir, (int, np.integer)) and int(ir) in (0, 1):
        return bool(ir)
    raise ValueError(f"ir_metrics must be 0 or 1, got {ir!r}")


def _pair_ends(n_rows, n_cols, ends):
    """group_end of the pairs as int64 numpy: ends, or 1 .. N for a single-sentence set."""
    if ends is None:
        if n_rows != n_cols:
            raise ValueError("single-sentence retrieval: one text per video expected")
        return np.arange(1, n_rows + 1, dtype=np.int64)
    return np.asarray(ends, dtype=np.int64)


def _pair_ranks_from_slab(T_slab, V_slab, n_rows, n_cols, W, rank, ends):
    """(rt, rv, ranked): int64 numpy [n_rows] each, identical on every rank.  rt[s] = the text->video rank of pair s from the rows
    of T, rv[s] = its video->text rank among all sentences from the columns of V (each against its OWN matrix's scores), -1 where
    the pair is unranked in that matrix; ranked = (rt >= 0) & (rv >= 0).  V_slab is T_slab: one kernel call gives both.  Three
    collectives: the own scores (padded all-gather), rt (int32 all-gather), rv (int32 SUM all-reduce of the slabs' parts)."""
    dev = T_slab.device
    pair_ends = _pair_ends(n_rows, n_cols, ends)
    group_end = torch.from_numpy(pair_ends.astype(np.int32)).to(dev)
    r0, r1 = slab_bounds(n_rows, W, rank)
    n = r1 - r0
    width = -(-n_rows // W)
    slabs = (T_slab,) if V_slab is T_slab else (T_slab, V_slab)
    slabs = tuple(ops._slab_2d(M) for M in slabs)
    mine = torch.full((len(slabs), width), float("nan"), dtype=torch.float32, device=dev)
    if n:
        cols = torch.from_numpy(np.searchsorted(pair_ends, np.arange(r0, r1), side="right")).to(dev)
        rows = torch.arange(n, device=dev)
        for k, M in enumerate(slabs):
            mine[k, :n] = M[rows, cols]
    own = _gathered_rows(mine, n_rows, W)
    row_rank, col_ahead = ops.pair_ranks(slabs[0], r0, group_end, own[0].contiguous(), want_col=len(slabs) == 1)
    if len(slabs) == 2:
        _, col_ahead = ops.pair_ranks(slabs[1], r0, group_end, own[1].contiguous(), want_row=False)
    if W > 1:
        comm.all_reduce(col_ahead)                                        # the slabs' parts -> the whole column's count
    rt_mine = torch.full((1, width), -1, dtype=torch.int32, device=dev)
    rt_mine[0, :n] = row_rank
    rt = _gathered_rows(rt_mine, n_rows, W)[0].cpu().numpy().astype(np.int64)
    own_v = own[-1].cpu().numpy()
    rv = np.where(np.isfinite(own_v), col_ahead.cpu().numpy().astype(np.int64), -1)
    return rt, rv, (rt >= 0) & (rv >= 0)


def _column_bootstrap(columns, other, boot, seed, dev):
    """(sums, paired): the ops.bootstrap_unit_sums rows of the IR `columns` and, with `other`, of both rankings' columns from ONE
    launch next to the paired summary of columns minus other; paired is None without other."""
    n_boot, _, level = boot
    both = columns if other is None else np.concatenate([columns, other], axis=1)
    sums = ops.bootstrap_unit_sums(torch.from_numpy(np.ascontiguousarray(both)).to(dev), seed=seed, b0=0, n_boot=n_boot).cpu().numpy()
    return sums, None if other is None else dict(RetrievalMetrics.ir_paired_bootstrap_summary(sums, columns, other, level), seed=seed)


def _ir_bootstrap(columns, boot, seed, dev, raw_columns=None):
    """{"bootstrap": summary of `columns`} and, with raw_columns, "bootstrap_vs_raw": both rankings' columns in ONE launch."""
    sums, paired = _column_bootstrap(columns, raw_columns, boot, seed, dev)
    out = {"bootstrap": RetrievalMetrics.ir_bootstrap_summary(sums[:, :columns.shape[1]], columns, boot[2])}
    out["bootstrap"].update(seed=seed, columns=columns)
    if paired is not None:
        out["bootstrap_vs_raw"] = paired
    return out


def _ir_from_slab(T_slab, V_slab, n_rows, n_cols, W, rank, ends, boot=None, raw_columns=None):
    """((text->video "ir", video->text "ir"), columns): the IR dictionaries of RetrievalMetrics.ir_from_ranks -- text->video: every
    sentence a query, from the rows of T; video->text: every video a query over its sentences, from the columns of V -- and the two
    directions' bootstrap columns (ir_unit_columns; the unit of a multi-sentence set is the video in both directions).  boot: each
    gains "bootstrap" (seed for text->video, seed + 1 for video->text) and, with raw_columns, "bootstrap_vs_raw"."""
    rt, rv, _ = _pair_ranks_from_slab(T_slab, V_slab, n_rows, n_cols, W, rank, ends)
    groups = None if ends is None else np.asarray(ends, dtype=np.int64)
    out = RetrievalMetrics.ir_from_ranks(rt), RetrievalMetrics.ir_from_ranks(rv, groups)
    columns = RetrievalMetrics.ir_unit_columns(rt, None, groups), RetrievalMetrics.ir_unit_columns(rv, groups)
    if boot:
        for side in range(2):
            out[side].update(_ir_bootstrap(columns[side], boot, boot[1] + side, T_slab.device,
                                           None if raw_columns is None else raw_columns[side]))
    return out, columns


def _add_ir(t2v, v2t, T_slab, V_slab, n_rows, n_cols, W, rank, ends, boot, raw_columns=None):
    """Puts "ir" into the two directions' dictionaries -> the bootstrap columns (a correction pairs with them)."""
    (t2v["ir"], v2t["ir"]), columns = _ir_from_slab(T_slab, V_slab, n_rows, n_cols, W, rank, ends, boot, raw_columns)
    return columns


def sharded_ir_metrics(model, text_feat, video_feat, text_mask, video_mask, args, cut_off_points=None, bootstrap=0, bootstrap_seed=0,
                       bootstrap_level=0.95, chunk=256):
    """(text->video, video->text) IR dictionaries of the raw similarity, identical on every rank: MRR, mAP, nDCG10, RPrec (x 100),
    n_queries, n_unranked and the rank of every relevant pair ("ranks": rt resp. rv, -1 where unranked).  cut_off_points as in
    sharded_multi_sentence_metrics; None: a single-sentence set.  bootstrap > 0: each gains "bootstrap"."""
    boot = _check_bootstrap(bootstrap, bootstrap_seed, bootstrap_level)
    S_slab, n_rows, n_cols, W, rank, ends = _eval_slab(model, text_feat, video_feat, text_mask, video_mask, args, cut_off_points, chunk)
    return _ir_from_slab(S_slab, S_slab, n_rows, n_cols, W, rank, ends, boot)[0]


# ---- paired permutation tests (DESIGN.md "Paired permutation tests") --------------------------------------------------------------------
# Is the corrected ranking (or model A) significantly better than the raw one (model B)?  The two rankings' entries are swapped unit
# by unit, n_perm times, on the GPU (nr_permtest_rank_stats, nr_permtest_unit_sums); the host compares every relabelling's difference
# with the observed one in exact integers.  Units as in the bootstrap.  Every rank holds the same integers and computes every
# permutation itself: no collective.

PERMUTATION_MAX = 1 << 20
CORRECTION_KEYS = ("test_norm", "local_scaling", "mutual_proximity")


def _check_permutation(permutation, seed=0):
    """None for permutation = 0, else (n_perm, seed); an integer in [0, 2^20], a seed in [0, 2^64 - 1)."""
    if isinstance(permutation, bool) or not isinstance(permutation, (int, np.integer)) or not 0 <= int(permutation) <= PERMUTATION_MAX:
        raise ValueError(f"permutation must be an integer in [0, 2^20], got {permutation!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64) - 1:
        raise ValueError(f"permutation_seed must be an integer in [0, 2^64 - 1), got {seed!r}")
    return (int(permutation), int(seed)) if int(permutation) else None


def _units_entry(units):
    """What a direction's dictionary carries of its resampling units under "units"."""
    entries, unit_end, median = units
    return {"entries": np.asarray(entries, dtype=np.int64), "unit_end": np.asarray(unit_end, dtype=np.int64), "median": median}


def _check_comparable(a, b, what="permutation test"):
    """Refuses two dictionaries whose "units" (and, where both carry "ir", whose IR "columns") do not pair up."""
    for name, m in (("a", a), ("b", b)):
        if "units" not in m:
            raise ValueError(f"{what}: result {name} carries no units: evaluate it with permutation > 0")
    ua, ub = a["units"], b["units"]
    if len(ua["unit_end"]) != len(ub["unit_end"]):
        raise ValueError(f"{what}: the two rankings have {len(ua['unit_end'])} and {len(ub['unit_end'])} units")
    if ua["median"] != ub["median"]:
        raise ValueError(f"{what}: the two rankings take different medians ({ua['median']!r}, {ub['median']!r})")
    if "ir" in a and "ir" in b:
        if "columns" not in a["ir"] or "columns" not in b["ir"]:
            raise ValueError(f"{what}: an \"ir\" entry carries no columns: evaluate it with permutation > 0")
        ca, cb = np.asarray(a["ir"]["columns"]), np.asarray(b["ir"]["columns"])
        if ca.shape != cb.shape or ca.ndim != 2 or ca.shape[0] != len(ua["unit_end"]):
            raise ValueError(f"{what}: the two rankings' IR columns are {ca.shape} and {cb.shape} over {len(ua['unit_end'])} units")
    if _has_lists(a) and _has_lists(b):
        ha, hb = a["hubness"], b["hubness"]
        la, lb = ha["lists"], hb["lists"]
        if ha["k"] != hb["k"] or la["idx"].shape != lb["idx"].shape:
            raise ValueError(f"{what}: the two rankings' top-k lists are {la['idx'].shape} (k = {ha['k']}) and {lb['idx'].shape} "
                             f"(k = {hb['k']})")
        if ha["n_gallery"] != hb["n_gallery"]:
            raise ValueError(f"{what}: the two rankings' galleries hold {ha['n_gallery']} and {hb['n_gallery']} items")
        if any(not np.array_equal(la[key], lb[key]) for key in ("unit_end", "gt_begin", "gt_end")):
            raise ValueError(f"{what}: the two rankings' top-k lists have different units or ground-truth ranges")


def _has_lists(m):
    return "hubness" in m and "lists" in m["hubness"]


def _check_hubness_test(hubness_test, hubness_k=0, perm=None, n_rows=None, n_cols=None):
    """hubness_test as a bool (--hubness_test {0,1}); with it hubness_k and permutation must be set and, once the sizes are known,
    both directions' galleries must fit nr_permtest_hubness (the limit of the lists lies above that of the gallery)."""
    if isinstance(hubness_test, (bool, np.bool_)) or (isinstance(hubness_test, (int, np.integer)) and int(hubness_test) in (0, 1)):
        hubness_test = bool(hubness_test)
    else:
        raise ValueError(f"hubness_test must be 0 or 1, got {hubness_test!r}")
    if hubness_test and (not hubness_k or perm is None):
        raise ValueError("hubness_test needs hubness_k > 0 (the top-k lists it relabels) and permutation > 0 (how many relabellings)")
    if hubness_test and n_rows is not None:
        if max(n_rows, n_cols) > ops.hip.HUBPERM_MAX_GALLERY:
            raise ValueError(f"hubness_test: a gallery of {max(n_rows, n_cols)} items is above the limit of {ops.hip.HUBPERM_MAX_GALLERY}")
    return hubness_test


def _hubness_permutation(hub, other, n_perm, seed, dev):
    """RetrievalMetrics.hubness_permutation_summary of the "hubness" entry `hub` minus `other` (both with "lists" over the same
    units): the two rankings' occurrence counts and one launch of the relabellings."""
    la, lb = hub["lists"], other["lists"]
    stats = ops.permtest_hubness(_dev32(la["idx"], dev), _dev32(lb["idx"], dev), _dev32(la["unit_end"], dev), hub["n_gallery"],
                                 _dev32(la["gt_begin"], dev), _dev32(la["gt_end"], dev), seed=seed, p0=0, n_perm=n_perm).cpu().numpy()
    moments = (RetrievalMetrics.hubness_moments(h["occurrence"], h["good_occurrence"]) for h in (hub, other))
    return RetrievalMetrics.hubness_permutation_summary(stats, *moments, hub["n_gallery"], seed)


def _permutation_of_units(units, other, n_perm, seed, dev):
    """RetrievalMetrics.permutation_summary of `units` minus `other` (two "units" entries over the same units): one launch."""
    stats = ops.permtest_rank_stats(_dev32(units["entries"], dev), _dev32(units["unit_end"], dev), _dev32(other["entries"], dev),
                                    _dev32(other["unit_end"], dev), cuts=BOOTSTRAP_CUTS, seed=seed, p0=0, n_perm=n_perm).cpu().numpy()
    return RetrievalMetrics.permutation_summary(stats, BOOTSTRAP_CUTS, units["entries"], other["entries"], units["median"], seed)


def _permutation_of_columns(columns, other, n_perm, seed, dev):
    """RetrievalMetrics.ir_permutation_summary of the IR columns `columns` minus `other` [U, 5]: one launch."""
    columns, other = np.asarray(columns, dtype=np.int64), np.asarray(other, dtype=np.int64)
    sums = ops.permtest_unit_sums(torch.from_numpy(np.ascontiguousarray(columns)).to(dev),
                                  torch.from_numpy(np.ascontiguousarray(other)).to(dev), seed=seed, p0=0, n_perm=n_perm).cpu().numpy()
    return RetrievalMetrics.ir_permutation_summary(sums, columns, other, seed)


def _compare_direction(a, b, side, perm, boot, dev):
    """One direction (or one correction's sub-dictionary) of compare_evaluations: "permutation", with boot "bootstrap", and the same
    under "ir" when both carry it."""
    n_perm, seed = perm
    out = {"permutation": _permutation_of_units(a["units"], b["units"], n_perm, seed + side, dev)}
    ir = "ir" in a and "ir" in b
    if ir:
        out["ir"] = {"permutation": _permutation_of_columns(a["ir"]["columns"], b["ir"]["columns"], n_perm, seed + side, dev)}
    if _has_lists(a) and _has_lists(b):
        out["hubness"] = {"k": a["hubness"]["k"], "permutation": _hubness_permutation(a["hubness"], b["hubness"], n_perm, seed + side, dev)}
    if boot:
        ua, ub = ((u["entries"], u["unit_end"], u["median"]) for u in (a["units"], b["units"]))
        out["bootstrap"] = _rank_bootstrap(ua, ub, boot, boot[1] + side, dev)[1]
        if ir:
            out["ir"]["bootstrap"] = _column_bootstrap(a["ir"]["columns"], b["ir"]["columns"], boot, boot[1] + side, dev)[1]
    return out


def compare_evaluations(a, b, permutation, permutation_seed=0, bootstrap=0, bootstrap_seed=0, bootstrap_level=0.95, device="cuda"):
    """Is evaluation a better than evaluation b on this test set?  a, b: the (text->video, video->text) results of two
    sharded_evaluation calls with permutation > 0 (two checkpoints, or two settings, scored on the SAME test set).  ->
    (text->video, video->text) comparison dictionaries of "a minus b": "permutation" (RetrievalMetrics.permutation_summary; seed for
    text->video, seed + 1 for video->text); with bootstrap > 0 "bootstrap" (paired_bootstrap_summary on the draws of the bootstrap);
    the same two under "ir" when both results carry "ir", ["hubness"]["permutation"] (hubness_permutation_summary) when both carry
    their top-k lists (hubness_test), and all of it under a correction's key when both carry the same one.
    ValueError when the units, the median kind or the column layout of the two results differ."""
    perm = _check_permutation(permutation, permutation_seed)
    if perm is None:
        raise ValueError("compare_evaluations needs permutation > 0: there is nothing else to compare with")
    boot = _check_bootstrap(bootstrap, bootstrap_seed, bootstrap_level)
    for side in range(2):                                   # everything is checked before the first launch
        _check_comparable(a[side], b[side], "compare_evaluations")
        for key in CORRECTION_KEYS:
            if key in a[side] and key in b[side]:
                _check_comparable(a[side][key], b[side][key], "compare_evaluations")
    out = []
    for side in range(2):
        cmp = _compare_direction(a[side], b[side], side, perm, boot, device)
        for key in CORRECTION_KEYS:
            if key in a[side] and key in b[side]:
                cmp[key] = _compare_direction(a[side][key], b[side][key], side, perm, boot, device)
        out.append(cmp)
    return tuple(out)


def _carry_units(t2v, v2t, units, columns=None):
    """Puts "units" into the two directions' dictionaries and, with the IR columns, "columns" into their "ir" entries."""
    for side, m in enumerate((t2v, v2t)):
        m["units"] = _units_entry(units[side])
        if columns is not None:
            m["ir"]["columns"] = columns[side]


def _add_permutation(nt, nv, units, raw_units, perm, dev, columns=None, raw_columns=None):
    """Puts "permutation_vs_raw" into a correction's two dictionaries (corrected minus raw: seed for text->video, seed + 1 for
    video->text), and with the IR columns into their "ir" entries too."""
    n_perm, seed = perm
    for side, m in enumerate((nt, nv)):
        m["permutation_vs_raw"] = _permutation_of_units(_units_entry(units[side]), _units_entry(raw_units[side]), n_perm, seed + side, dev)
        if columns is not None:
            m["ir"]["permutation_vs_raw"] = _permutation_of_columns(columns[side], raw_columns[side], n_perm, seed + side, dev)


# ---- the evaluation: one slab, one driver, an optional correction (DESIGN.md "The evaluation driver") ---------------------------------
# Every metric dictionary comes from sharded_evaluation: ONE scoring of this rank's slab, the raw dictionaries, then the corrected
# ones under the correction's key.  A correction is a value: what its entry says, whether it needs a querybank, and the call that
# turns the slab into (T, V).  Every rank issues the same collectives in the same order; the order below is part of the contract.

class Correction(NamedTuple):
    """One test-time correction of the similarity.  apply(slab, bank_slabs, n_bank_texts) -> (T_slab, V_slab, info): T's rows rank
    text->video, V's columns video->text (V_slab is T_slab for the one-output corrections); info holds "iters" and "marginal_err"
    (text->video, video->text) for the iterated modes and is empty otherwise."""
    key: str                     # the dictionary entry: "test_norm" | "local_scaling" | "mutual_proximity"
    label: str                   # the tag of its log lines
    needs_bank: bool             # scored against a querybank (bank_slabs, n_bank_texts) instead of the test set alone
    entry: dict                  # the fields written into each direction's corrected dictionary
    apply: Callable


def test_norm_correction(mode, beta=20.0, qb_k=1, n_iter=50):
    """IS, DSL, QB-Norm (DESIGN.md "Test-time hubness reduction"); Sinkhorn, QB-Sinkhorn with n_iter iterations (DESIGN.md
    "Test-time Sinkhorn normalisation")."""
    beta, qb_k, _ = _check_test_norm(mode, beta, qb_k, 0)
    n_iter = _check_n_iter(n_iter)
    entry = dict(mode=mode, beta=beta)
    if mode == "qbnorm":
        entry["qb_k"] = qb_k

    def apply(slab, bank_slabs, n_bank_texts):
        S, n_rows, n_cols, W, rank, ends = slab
        if mode in SINKHORN_MODES:
            return _sinkhorn_from_slab(S, n_rows, n_cols, W, rank, mode, beta, n_iter, ends, bank_slabs, n_bank_texts)
        return _normalised_from_slab(S, n_rows, n_cols, W, rank, mode, beta, bank_slabs, qb_k) + ({},)
    return Correction("test_norm", test_norm_label(mode, beta, n_iter), mode in BANK_MODES, entry, apply)


def local_scaling_correction(mode, k=10, bank=False):
    """CSLS, NICDM, LS with neighbourhoods of k items, taken in the querybank with `bank` (DESIGN.md "Local scaling")."""
    k, _ = _check_local_scaling(mode, k)

    def apply(slab, bank_slabs, n_bank_texts):
        T = _local_scaled_from_slab(slab.S, slab.n_rows, slab.n_cols, slab.W, slab.rank, mode, k, bank_slabs, n_bank_texts)
        return T, T, {}
    return Correction("local_scaling", local_scaling_label(mode, k, bank), bool(bank), dict(mode=mode, k=k, bank=bool(bank)), apply)


def mutual_proximity_correction(mode, bank=False):
    """emp, gauss, the reference lines taken in the querybank with `bank` (DESIGN.md "Mutual proximity")."""
    _check_mutual_proximity(mode)

    def apply(slab, bank_slabs, n_bank_texts):
        T = _mutual_proximity_from_slab(slab.S, slab.n_rows, slab.n_cols, slab.W, slab.rank, mode, bank_slabs, n_bank_texts)
        return T, T, {}
    return Correction("mutual_proximity", mutual_proximity_label(mode, bank), bool(bank), dict(mode=mode, bank=bool(bank)), apply)


def _apply_correction(model, text_feat, video_feat, text_mask, video_mask, slab, correction, querybank, chunk):
    """correction.apply on this rank's slab; the one place where the querybank's slabs are scored."""
    bank_slabs, n_bank_texts = None, None
    if correction.needs_bank:
        bank = _querybank(model, querybank, slab.S.device)
        bank_slabs = _bank_slabs(model, text_feat, video_feat, text_mask, video_mask, bank, slab.W, slab.rank, chunk)
        n_bank_texts = bank[0].shape[0]
    return correction.apply(slab, bank_slabs, n_bank_texts)


def _corrected_entry(metrics, correction, info, side):
    """The corrected dictionary of one direction (side 0: text->video, 1: video->text) with the correction's fields."""
    metrics.update(correction.entry)
    if info:
        metrics.update(iters=info["iters"], marginal_err=info["marginal_err"][side])
    return metrics


def sharded_evaluation(model, text_feat, video_feat, text_mask, video_mask, args, correction=None, hubness_k=0, cut_off_points=None,
                       chunk=256, querybank=None, bootstrap=0, bootstrap_seed=0, bootstrap_level=0.95, ir=False, permutation=0,
                       permutation_seed=0, hubness_test=False):
    """-> (text->video, video->text) metric dictionaries, identical on every rank, from ONE scoring of this rank's slab: R@K as
    RetrievalMetrics.compute_metrics(S) / (S.T) would give them (cut_off_points: the multi-sentence metrics, see
    sharded_multi_sentence_metrics).  hubness_k: each with a "hubness" entry (sharded_hubness).  ir: an "ir" entry (DESIGN.md
    "Rank-aware IR metrics").  bootstrap > 0: a "bootstrap" entry, also inside "ir" (DESIGN.md "Bootstrap confidence intervals").
    correction: each with one more entry correction.key, the same dictionary of the corrected scores with correction.entry's
    fields; its bootstrap entries are "bootstrap" and "bootstrap_vs_raw" (paired with the raw ranking on the same draws).
    querybank: (text_feat, text_mask, video_feat, video_mask) for a correction that needs one; None: the model's memory bank.
    permutation > 0 (DESIGN.md "Paired permutation tests"): every dictionary, the correction's too, also carries its resampling
    "units" (entries, unit_end, median) and its "ir" entry its "columns" -- what compare_evaluations reads --, and the correction's
    dictionary and its "ir" entry gain "permutation_vs_raw", the paired permutation test of corrected minus raw.
    hubness_test (DESIGN.md "Permutation test of hubness"; needs hubness_k > 0 and permutation > 0): every "hubness" entry, the
    correction's too, also carries its top-k "lists" (idx, unit_end, gt_begin, gt_end; the row lists of a sharded run cost one more
    all-gather), and the correction's "hubness" entry gains "permutation_vs_raw", the test of corrected minus raw hubness."""
    boot = _check_bootstrap(bootstrap, bootstrap_seed, bootstrap_level)
    perm = _check_permutation(permutation, permutation_seed)
    ir = _check_ir(ir)
    hubness_k = _check_hubness_k(hubness_k)
    hubness_test = _check_hubness_test(hubness_test, hubness_k, perm, text_feat.shape[0], video_feat.shape[0])
    if correction is not None and correction.needs_bank:
        _querybank(model, querybank, text_feat.device)                 # an empty bank fails before any scoring
    slab = _eval_slab(model, text_feat, video_feat, text_mask, video_mask, args, cut_off_points, chunk)
    S_slab, n_rows, n_cols, W, rank, ends = slab
    dev = S_slab.device
    t2v, v2t, raw_units = _metrics_and_units(S_slab, S_slab, n_rows, n_cols, W, rank, ends)
    if hubness_k:
        t2v["hubness"], v2t["hubness"] = _hubness_from_slab(S_slab, n_rows, n_cols, hubness_k, W, rank, ends, hubness_test)
    raw_columns = _add_ir(t2v, v2t, S_slab, S_slab, n_rows, n_cols, W, rank, ends, boot) if ir else None
    _add_bootstrap(t2v, v2t, raw_units, boot, dev)
    if perm:
        _carry_units(t2v, v2t, raw_units, raw_columns)
    if correction is None:
        return t2v, v2t
    T, V, info = _apply_correction(model, text_feat, video_feat, text_mask, video_mask, slab, correction, querybank, chunk)
    del S_slab, slab                       # the raw slab, the largest buffer of the evaluation, goes before the corrected metrics
    units = []
    nt, nv = _metrics_from_normalised(T, V, n_rows, n_cols, W, rank, ends, hubness_k, units, hubness_test)
    _add_bootstrap(nt, nv, units, boot, dev, raw_units)
    columns = _add_ir(nt, nv, T, V, n_rows, n_cols, W, rank, ends, boot, raw_columns) if ir else None
    if perm:
        _carry_units(nt, nv, units, columns)
        _add_permutation(nt, nv, units, raw_units, perm, dev, columns, raw_columns)
    if hubness_test:
        for side, (m, raw) in enumerate(((nt, t2v), (nv, v2t))):
            m["hubness"]["permutation_vs_raw"] = _hubness_permutation(m["hubness"], raw["hubness"], perm[0], perm[1] + side, dev)
    t2v[correction.key] = _corrected_entry(nt, correction, info, 0)
    v2t[correction.key] = _corrected_entry(nv, correction, info, 1)
    return t2v, v2t


def _corrected_slabs(model, text_feat, video_feat, text_mask, video_mask, args, correction, querybank, cut_off_points, chunk):
    """(slab, T_slab, V_slab, info): this rank's slab and its corrected copies, nothing else computed."""
    if correction.needs_bank:
        _querybank(model, querybank, text_feat.device)                 # an empty bank fails before any scoring
    slab = _eval_slab(model, text_feat, video_feat, text_mask, video_mask, args, cut_off_points, chunk)
    return (slab,) + _apply_correction(model, text_feat, video_feat, text_mask, video_mask, slab, correction, querybank, chunk)


def _corrected_metrics(model, text_feat, video_feat, text_mask, video_mask, args, correction, querybank, hubness_k, cut_off_points,
                       chunk):
    """The corrected dictionaries alone: what sharded_evaluation puts under correction.key, without bootstrap and ir."""
    hubness_k = _check_hubness_k(hubness_k)
    slab, T, V, info = _corrected_slabs(model, text_feat, video_feat, text_mask, video_mask, args, correction, querybank,
                                        cut_off_points, chunk)
    t2v, v2t = _metrics_from_normalised(T, V, slab.n_rows, slab.n_cols, slab.W, slab.rank, slab.ends, hubness_k)
    return _corrected_entry(t2v, correction, info, 0), _corrected_entry(v2t, correction, info, 1)


def sharded_metrics(model, text_feat, video_feat, text_mask, video_mask, args, bootstrap=0, bootstrap_seed=0, bootstrap_level=0.95,
                    ir=False, permutation=0, permutation_seed=0):
    """(text->video metrics, video->text metrics) as RetrievalMetrics.compute_metrics(S) / (S.T) would give them.  bootstrap > 0:
    each with a "bootstrap" entry (DESIGN.md "Bootstrap confidence intervals").  ir: each with an "ir" entry (DESIGN.md "Rank-aware
    IR metrics")."""
    return sharded_evaluation(model, text_feat, video_feat, text_mask, video_mask, args, bootstrap=bootstrap,
                              bootstrap_seed=bootstrap_seed, bootstrap_level=bootstrap_level, ir=ir, permutation=permutation,
                              permutation_seed=permutation_seed)


def sharded_multi_sentence_metrics(model, text_feat, video_feat, text_mask, video_mask, cut_off_points, args, chunk=256, bootstrap=0,
                                   bootstrap_seed=0, bootstrap_level=0.95, ir=False, permutation=0, permutation_seed=0):
    """Several captions per video (evaluator.py:114-149 features, :225-262 metrics): text_feat [Ns,...] holds every
    sentence in dataset order, video_feat [V,...] one entry per video, cut_off_points[g] = index of the LAST sentence of
    video g (the dataset's cut_off_points minus one, evaluator.py:98).  -> (text->video, video->text) metric dictionaries.

    The reference pads the Ns x V matrix to [V, max_sentences, V] with -inf on the host and ranks it with two argsorts
    (metrics.py:82-126) and a max over the padded axis (:128-148).  Here rank r scores its slab of sentence rows, one
    launch (nr_group_slab_ranks) gives every row's rank and the slab's per-video best scores, and a MAX all-reduce of
    the V x V best-score matrix + an all-gather of the Ns ranks complete them; no padded tensor exists.  bootstrap > 0: each
    dictionary gains a "bootstrap" entry that resamples VIDEOS (DESIGN.md "Bootstrap confidence intervals").  ir: each gains an "ir"
    entry (DESIGN.md "Rank-aware IR metrics")."""
    return sharded_evaluation(model, text_feat, video_feat, text_mask, video_mask, args, cut_off_points=cut_off_points, chunk=chunk,
                              bootstrap=bootstrap, bootstrap_seed=bootstrap_seed, bootstrap_level=bootstrap_level, ir=ir,
                              permutation=permutation, permutation_seed=permutation_seed)


def sharded_metrics_with_hubness(model, text_feat, video_feat, text_mask, video_mask, args, k, cut_off_points=None, chunk=256,
                                 bootstrap=0, bootstrap_seed=0, bootstrap_level=0.95, ir=False, permutation=0, permutation_seed=0):
    """sharded_evaluation with a "hubness" entry of the top-k lists in each dictionary."""
    return sharded_evaluation(model, text_feat, video_feat, text_mask, video_mask, args, hubness_k=ops._check_k(k),
                              cut_off_points=cut_off_points, chunk=chunk, bootstrap=bootstrap, bootstrap_seed=bootstrap_seed,
                              bootstrap_level=bootstrap_level, ir=ir, permutation=permutation, permutation_seed=permutation_seed)


def sharded_normalised_slabs(model, text_feat, video_feat, text_mask, video_mask, args, mode, beta=20.0, querybank=None, qb_k=1,
                             cut_off_points=None, chunk=256, n_iter=50):
    """-> (T_slab, V_slab) fp32 [r1 - r0, V] of this rank's rows [r0, r1) = slab_bounds(n_texts, W, rank): the text->video
    scores (rows are the queries) and the video->text scores (columns are the queries) after test_norm_correction(mode, beta,
    qb_k, n_iter) ("sinkhorn" has ONE output, V_slab is T_slab).  querybank: (text_feat, text_mask, video_feat, video_mask) of
    the qbnorm / qbsinkhorn querybank; None: the model's memory bank (load_memory_bank)."""
    return _corrected_slabs(model, text_feat, video_feat, text_mask, video_mask, args, test_norm_correction(mode, beta, qb_k, n_iter),
                            querybank, cut_off_points, chunk)[1:3]


def sharded_normalised_metrics(model, text_feat, video_feat, text_mask, video_mask, args, mode, beta=20.0, querybank=None, qb_k=1,
                               hubness_k=0, cut_off_points=None, chunk=256, n_iter=50):
    """(text->video, video->text) metric dictionaries of the normalised scores (sharded_normalised_slabs), identical on every
    rank, each with "mode" and "beta" (and "qb_k" for qbnorm; "iters" and "marginal_err" for sinkhorn / qbsinkhorn) and, with
    hubness_k, a "hubness" entry (sharded_hubness's summary of T's row lists / V's column lists)."""
    return _corrected_metrics(model, text_feat, video_feat, text_mask, video_mask, args, test_norm_correction(mode, beta, qb_k, n_iter),
                              querybank, hubness_k, cut_off_points, chunk)


def sharded_metrics_with_test_norm(model, text_feat, video_feat, text_mask, video_mask, args, mode, beta=20.0, querybank=None,
                                   qb_k=1, hubness_k=0, cut_off_points=None, chunk=256, n_iter=50, bootstrap=0, bootstrap_seed=0,
                                   bootstrap_level=0.95, ir=False, permutation=0, permutation_seed=0):
    """sharded_evaluation with test_norm_correction(mode, beta, qb_k, n_iter): the raw dictionaries, each with one more entry
    "test_norm" = sharded_normalised_metrics."""
    return sharded_evaluation(model, text_feat, video_feat, text_mask, video_mask, args, test_norm_correction(mode, beta, qb_k, n_iter),
                              hubness_k, cut_off_points, chunk, querybank, bootstrap, bootstrap_seed, bootstrap_level, ir,
                              permutation, permutation_seed)


def sharded_local_scaled_slab(model, text_feat, video_feat, text_mask, video_mask, args, mode, k=10, bank=False, querybank=None,
                              cut_off_points=None, chunk=256):
    """-> T_slab fp32 [r1 - r0, V] of this rank's rows [r0, r1) = slab_bounds(n_texts, W, rank): the scores after
    local_scaling_correction(mode, k, bank).  Rows rank text->video, columns video->text.  querybank: (text_feat, text_mask,
    video_feat, video_mask) for `bank`; None: the model's memory bank (load_memory_bank)."""
    return _corrected_slabs(model, text_feat, video_feat, text_mask, video_mask, args, local_scaling_correction(mode, k, bank),
                            querybank, cut_off_points, chunk)[1]


def sharded_local_scaled_metrics(model, text_feat, video_feat, text_mask, video_mask, args, mode, k=10, bank=False, querybank=None,
                                 hubness_k=0, cut_off_points=None, chunk=256):
    """(text->video, video->text) metric dictionaries of the locally scaled scores (sharded_local_scaled_slab), identical on
    every rank, each with "mode", "k" and "bank" and, with hubness_k, a "hubness" entry (T's row lists / column lists)."""
    return _corrected_metrics(model, text_feat, video_feat, text_mask, video_mask, args, local_scaling_correction(mode, k, bank),
                              querybank, hubness_k, cut_off_points, chunk)


def sharded_metrics_with_local_scaling(model, text_feat, video_feat, text_mask, video_mask, args, mode, k=10, bank=False,
                                       querybank=None, hubness_k=0, cut_off_points=None, chunk=256, bootstrap=0, bootstrap_seed=0,
                                       bootstrap_level=0.95, ir=False, permutation=0, permutation_seed=0):
    """sharded_evaluation with local_scaling_correction(mode, k, bank): the raw dictionaries, each with one more entry
    "local_scaling" = sharded_local_scaled_metrics."""
    return sharded_evaluation(model, text_feat, video_feat, text_mask, video_mask, args, local_scaling_correction(mode, k, bank),
                              hubness_k, cut_off_points, chunk, querybank, bootstrap, bootstrap_seed, bootstrap_level, ir,
                              permutation, permutation_seed)


def sharded_mutual_proximity_slab(model, text_feat, video_feat, text_mask, video_mask, args, mode, bank=False, querybank=None,
                                  cut_off_points=None, chunk=256):
    """-> T_slab fp32 [r1 - r0, V] of this rank's rows [r0, r1) = slab_bounds(n_texts, W, rank): the scores after
    mutual_proximity_correction(mode, bank).  Rows rank text->video, columns video->text.  querybank: (text_feat, text_mask,
    video_feat, video_mask) for `bank`; None: the model's memory bank (load_memory_bank)."""
    return _corrected_slabs(model, text_feat, video_feat, text_mask, video_mask, args, mutual_proximity_correction(mode, bank),
                            querybank, cut_off_points, chunk)[1]


def sharded_mutual_proximity_metrics(model, text_feat, video_feat, text_mask, video_mask, args, mode, bank=False, querybank=None,
                                     hubness_k=0, cut_off_points=None, chunk=256):
    """(text->video, video->text) metric dictionaries of the mutual-proximity scores (sharded_mutual_proximity_slab), identical on
    every rank, each with "mode" and "bank" and, with hubness_k, a "hubness" entry (T's row lists / column lists)."""
    return _corrected_metrics(model, text_feat, video_feat, text_mask, video_mask, args, mutual_proximity_correction(mode, bank),
                              querybank, hubness_k, cut_off_points, chunk)


def sharded_metrics_with_mutual_proximity(model, text_feat, video_feat, text_mask, video_mask, args, mode, bank=False,
                                          querybank=None, hubness_k=0, cut_off_points=None, chunk=256, bootstrap=0,
                                          bootstrap_seed=0, bootstrap_level=0.95, ir=False, permutation=0, permutation_seed=0):
    """sharded_evaluation with mutual_proximity_correction(mode, bank): the raw dictionaries, each with one more entry
    "mutual_proximity" = sharded_mutual_proximity_metrics."""
    return sharded_evaluation(model, text_feat, video_feat, text_mask, video_mask, args, mutual_proximity_correction(mode, bank),
                              hubness_k, cut_off_points, chunk, querybank, bootstrap, bootstrap_seed, bootstrap_level, ir,
                              permutation, permutation_seed)


def correction_from_args(args, model):
    """What the command-line flags ask of the evaluation -> (correction or None, the keyword arguments of sharded_evaluation:
    hubness_k, the bootstrap triple, ir and, when asked for, permutation with its seed and hubness_test), everything checked before
    any work: the values, that at most one correction is chosen, that a permutation test has something to compare (a correction,
    args.compare_model, or the weight average of args.ema_decay), and that a correction that needs a querybank finds the model's memory bank filled."""
    kw = dict(bootstrap=getattr(args, "bootstrap", 0) or 0, bootstrap_seed=getattr(args, "bootstrap_seed", 0) or 0,
              bootstrap_level=getattr(args, "bootstrap_level", 0.95))
    _check_bootstrap(kw["bootstrap"], kw["bootstrap_seed"], kw["bootstrap_level"])
    kw["ir"] = _check_ir(getattr(args, "ir_metrics", 0) or 0)
    perm = _check_permutation(getattr(args, "permutation", 0) or 0, getattr(args, "permutation_seed", 0) or 0)
    test_norm = getattr(args, "test_norm", None) or "none"
    local_scaling = getattr(args, "local_scaling", None) or "none"
    mutual_proximity = getattr(args, "mutual_proximity", None) or "none"
    if mutual_proximity != "none" and (test_norm != "none" or local_scaling != "none"):
        raise ValueError("mutual_proximity, local_scaling and test_norm are separate corrections: choose one of them")
    if local_scaling != "none" and test_norm != "none":
        raise ValueError("local_scaling and test_norm are separate corrections: choose one of them")
    correction = None
    if test_norm != "none":
        correction = test_norm_correction(test_norm, getattr(args, "test_norm_beta", 20.0), getattr(args, "qb_k", 1),
                                          getattr(args, "test_norm_iters", 50))
    elif local_scaling != "none":
        correction = local_scaling_correction(local_scaling, getattr(args, "local_scaling_k", 10),
                                              bool(int(getattr(args, "local_scaling_bank", 0) or 0)))
    elif mutual_proximity != "none":
        correction = mutual_proximity_correction(mutual_proximity, bool(int(getattr(args, "mutual_proximity_bank", 0) or 0)))
    kw["hubness_k"] = _check_hubness_k(getattr(args, "hubness_k", 0))
    if perm is not None:
        if correction is None and not getattr(args, "compare_model", None) and not getattr(args, "ema_decay", 0):
            raise ValueError("permutation needs a correction (test_norm, local_scaling, mutual_proximity) or compare_model or "
                             "ema_decay: there is nothing to compare")
        kw.update(permutation=perm[0], permutation_seed=perm[1])
    if _check_hubness_test(getattr(args, "hubness_test", 0) or 0, kw["hubness_k"], perm):
        kw["hubness_test"] = True
    if correction is not None and correction.needs_bank:
        _querybank(model, None, model.mb_feat_t.device)         # checked where it lies: nothing is copied
    return correction, kw


# ---- two-stage retrieval: pooled prefilter, gathered token re-ranking (DESIGN.md "Two-stage retrieval") ----------------------------
# Rank r searches the queries slab_bounds(n_queries, W, r) of each direction against a GalleryIndex every rank prepares in full
# (search.py); the [n, C] candidate lists and their fine scores are gathered like the top-k lists (_gathered_rows: indices and
# score bits, transposed), one collective per direction, and every rank counts the same numbers on the host.  No n x N buffer.

RERANK_CUTS = (1, 5, 10, 50)


def two_stage_label(n_candidates):
    """The tag of the log lines of the two-stage metrics: "[two-stage C=64]"."""
    return f"[two-stage C={int(n_candidates)}]"


def rerank_top_from_args(args):
    """args.rerank_top as an int: 0 (off) or 1..128, checked before any work."""
    from .search import check_candidates
    top = getattr(args, "rerank_top", 0)
    top = 0 if top is None else top
    try:
        return check_candidates(top, allow_zero=True)
    except ValueError:
        raise ValueError(f"rerank_top must be an integer in [0, 128] (0 = off), got {top!r}") from None


def two_stage_counts(cand, fine, gt):
    """(found [n] bool, greater [n], equal [n] int64) of candidate lists cand [n, C] (-1 = absent) with scores fine [n, C] and one
    ground-truth item gt[i] per query: whether gt[i] is a candidate, how many candidates score above it and how many equal it
    (itself included); 0 where it is not found."""
    cand, fine, gt = np.asarray(cand), np.asarray(fine), np.asarray(gt).reshape(-1, 1)
    hit = (cand == gt) & (cand >= 0)
    found = hit.any(1)
    own = np.where(found, np.where(hit, fine, -np.inf).max(1), np.nan)[:, None]
    valid = cand >= 0
    greater = (valid & (fine > own)).sum(1).astype(np.int64)
    equal = (valid & (fine == own)).sum(1).astype(np.int64)
    return found, np.where(found, greater, 0), np.where(found, equal, 0)


def two_stage_metrics(found, greater, equal, n_candidates):
    """The dictionary of one direction from its per-query counts: R@K over all queries (a missed query fails at every K; None
    where K > C), cand_recall, n_candidates, cols (the ranks of the found queries, ranks_from_counts) and, when every query was
    found, MR / MedianR / MeanR."""
    found = np.asarray(found, dtype=bool)
    ind = RetrievalMetrics.ranks_from_counts(np.asarray(greater)[found], np.asarray(equal)[found])
    return _two_stage_dict(ind, int((~found).sum()), len(found), n_candidates)


def _two_stage_dict(ind, n_missed, n_queries, C):
    total = len(ind) + n_missed
    m = {f"R{K}": (float(np.sum(ind < K)) * 100 / total if K <= C and total else None) for K in RERANK_CUTS}
    m["cand_recall"] = float(n_queries - n_missed) * 100 / n_queries if n_queries else 0.0
    m["n_candidates"] = int(C)
    m["cols"] = [int(i) for i in ind]
    if n_missed == 0 and len(ind):
        m["MR"] = m["MedianR"] = float(np.median(ind)) + 1
        m["MeanR"] = float(np.mean(ind)) + 1
    return m


def two_stage_multi_sentence_metrics(cand_t, fine_t, cand_v, fine_v, ends, n_candidates):
    """(t2v, v2t) of a multi-sentence set; ends[g] = one past the last sentence of video g.  t2v: sentence s is ranked among its
    candidate videos, its own video's rank = the candidates scoring above it plus the equal ones at lower indices (the stable
    order of the exhaustive rule; the lists are in ascending index).  v2t: video j's candidate sentences are reduced to group
    scores (the maximum per video group); found = group j has a candidate; greater / equal count the groups present."""
    ends = np.asarray(ends, dtype=np.int64)
    cand_t, fine_t, cand_v, fine_v = (np.asarray(a) for a in (cand_t, fine_t, cand_v, fine_v))
    C = int(n_candidates)
    Ns, V = cand_t.shape[0], cand_v.shape[0]
    group = np.searchsorted(ends, np.arange(Ns), side="right")
    hit = (cand_t == group[:, None]) & (cand_t >= 0)
    found = hit.any(1)
    own = np.where(found, np.where(hit, fine_t, -np.inf).max(1), np.nan)[:, None]
    valid = cand_t >= 0
    ranks = (valid & (fine_t > own)).sum(1) + (valid & (fine_t == own) & (cand_t < group[:, None])).sum(1)
    ranks = ranks[found].astype(np.int64)
    t2v = {f"R{K}": (float(np.sum(ranks < K)) * 100 / Ns if K <= C else None) for K in RERANK_CUTS}
    t2v.update(cand_recall=float(found.sum()) * 100 / Ns, n_candidates=C, cols=[int(r) for r in ranks])
    if found.all():
        t2v["MedianR"] = t2v["MR"] = float(np.sort(ranks + 1)[(len(ranks) - 1) // 2])       # torch.median: the lower middle element
        t2v["MeanR"] = float(np.mean(ranks + 1))
        t2v["Std_Rank"] = float(np.std(ranks + 1))
    f_v, g_v, e_v = np.zeros(V, dtype=bool), np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
    for j in range(V):
        ok = cand_v[j] >= 0
        gmax = np.full(V, -np.inf)
        present = np.zeros(V, dtype=bool)
        gj = np.searchsorted(ends, cand_v[j][ok], side="right")
        np.maximum.at(gmax, gj, fine_v[j][ok])
        present[gj] = True
        if present[j]:
            f_v[j], g_v[j], e_v[j] = True, int((present & (gmax > gmax[j])).sum()), int((present & (gmax == gmax[j])).sum())
    return t2v, two_stage_metrics(f_v, g_v, e_v, C)


def two_stage_norm_label(n_candidates, mode, beta, qb_k=1):
    """The tag of the log lines of the normalised two-stage metrics: "[two-stage C=64 QB-Norm b=20 k=1]", "[two-stage C=64 IS b=20]"."""
    tail = f" k={int(qb_k)}" if mode == "qbnorm" else ""
    return f"[two-stage C={int(n_candidates)} {TEST_NORM_LABELS[mode]} b={beta:g}{tail}]"


def _rerank_mode_from_args(args, flag, check, choices):
    """args.<flag> -> None (unset or "none") or the mode, which search's `check` accepts."""
    mode = getattr(args, flag, None) or "none"
    if mode == "none":
        return None
    try:
        return check(mode)
    except ValueError:
        raise ValueError(f"{flag} must be {choices}, got {mode!r}") from None


def rerank_norm_from_args(args, model):
    """args.rerank_norm -> None or the keyword arguments of two_stage_evaluation (norm, beta, qb_k), checked before any work: the
    mode, that rerank_top asks for candidates, beta (test_norm_beta), qb_k and that the model's memory bank is filled."""
    from .search import check_norm
    mode = _rerank_mode_from_args(args, "rerank_norm", check_norm, "'is' or 'qbnorm'")
    if mode is None:
        return None
    if rerank_top_from_args(args) < 1:
        raise ValueError("rerank_norm normalises candidate lists: it needs rerank_top >= 1")
    kw = dict(norm=mode, beta=ops._check_beta(getattr(args, "test_norm_beta", 20.0)), qb_k=ops._check_k(getattr(args, "qb_k", 1)))
    _querybank(model, None, model.mb_feat_t.device)             # checked where it lies: nothing is copied
    return kw


def two_stage_local_scaling_label(n_candidates, mode, k):
    """The tag of the log lines of the locally scaled two-stage metrics: "[two-stage C=64 QB-CSLS k=10]"."""
    return f"[two-stage C={int(n_candidates)} QB-{LOCAL_SCALING_LABELS[mode]} k={int(k)}]"


def rerank_local_scaling_from_args(args, model):
    """args.rerank_local_scaling / rerank_local_scaling_k -> None or the keyword arguments of two_stage_evaluation (local_scaling,
    local_scaling_k), checked before any work: the mode, K, that it does not meet rerank_norm, that rerank_top asks for at least K
    candidates and that the model's memory bank is filled.  Independent of the exhaustive flags."""
    from .search import check_local_scaling, check_local_scaling_k
    mode = _rerank_mode_from_args(args, "rerank_local_scaling", check_local_scaling, "'csls', 'nicdm' or 'ls'")
    if mode is None:
        return None
    k = getattr(args, "rerank_local_scaling_k", 10)
    try:
        k = check_local_scaling_k(k)
    except ValueError:
        raise ValueError(f"rerank_local_scaling_k must be an integer in [1, 128], got {k!r}") from None
    if (getattr(args, "rerank_norm", None) or "none") != "none":
        raise ValueError("rerank_local_scaling and rerank_norm both correct the candidate scores: choose one")
    if rerank_top_from_args(args) < k:
        raise ValueError(f"rerank_local_scaling takes a query's neighbourhood among its candidates: it needs rerank_top >= "
                         f"rerank_local_scaling_k = {k}")
    _querybank(model, None, model.mb_feat_t.device)             # checked where it lies: nothing is copied
    return dict(local_scaling=mode, local_scaling_k=k)


def two_stage_mutual_proximity_label(n_candidates, mode):
    """The tag of the log lines of the two-stage metrics under mutual proximity: "[two-stage C=64 QB-MP-emp]"."""
    return f"[two-stage C={int(n_candidates)} QB-MP-{mode}]"


def rerank_mutual_proximity_from_args(args, model):
    """args.rerank_mutual_proximity -> None or the keyword arguments of two_stage_evaluation (mutual_proximity), checked before any
    work: the mode, that it meets neither rerank_norm nor rerank_local_scaling, that rerank_top asks for candidates and that the
    model's memory bank is filled.  Independent of the exhaustive flags."""
    from .search import check_mutual_proximity
    mode = _rerank_mode_from_args(args, "rerank_mutual_proximity", check_mutual_proximity, "'emp' or 'gauss'")
    if mode is None:
        return None
    for other in ("rerank_norm", "rerank_local_scaling"):
        if (getattr(args, other, None) or "none") != "none":
            raise ValueError(f"rerank_mutual_proximity and {other} both correct the candidate scores: choose one")
    if rerank_top_from_args(args) < 1:
        raise ValueError("rerank_mutual_proximity corrects candidate lists: it needs rerank_top >= 1")
    _querybank(model, None, model.mb_feat_t.device)             # checked where it lies: nothing is copied
    return dict(mutual_proximity=mode)


def two_stage_ivf_label(n_candidates, n_lists, nprobe):
    """The tag of the log lines of two-stage retrieval behind the inverted-file prefilter: "[two-stage C=64 IVF L=128 P=8]"."""
    return f"[two-stage C={int(n_candidates)} IVF L={int(n_lists)} P={int(nprobe)}]"


def rerank_ivf_from_args(args):
    """args.rerank_lists / rerank_probe / rerank_ivf_iters / rerank_ivf_seed -> None (rerank_lists = 0: off) or the keyword
    arguments of two_stage_evaluation (n_lists, nprobe, ivf_iters, ivf_seed), checked before any work: that rerank_top asks for
    candidates, rerank_lists >= 1, rerank_probe in [1, min(rerank_lists, 128)], rerank_ivf_iters >= 0 and an integer seed.  That
    the galleries hold at least rerank_lists items is checked by two_stage_evaluation, which knows their sizes."""
    from .search import check_ivf_build, check_nprobe
    lists = getattr(args, "rerank_lists", 0)
    if lists is None or (lists == 0 and not isinstance(lists, bool)):
        return None
    if rerank_top_from_args(args) < 1:
        raise ValueError("rerank_lists restricts the prefilter of two-stage retrieval: it needs rerank_top >= 1")
    iters, seed = getattr(args, "rerank_ivf_iters", 10), getattr(args, "rerank_ivf_seed", 0)
    try:
        lists, iters, seed = check_ivf_build(lists, iters, seed, 1 << 31)
    except ValueError as e:
        raise ValueError(f"rerank_lists / rerank_ivf_iters / rerank_ivf_seed: {e}") from None
    try:
        probe = check_nprobe(getattr(args, "rerank_probe", 0), lists)
    except ValueError:
        raise ValueError(f"rerank_probe must be an integer in [1, min(rerank_lists, 128) = {min(lists, 128)}], got "
                         f"{getattr(args, 'rerank_probe', 0)!r}") from None
    return dict(n_lists=lists, nprobe=probe, ivf_iters=iters, ivf_seed=seed)


def _pack_rows(tensors, width):
    """This rank's m rows of any number of 32-bit tensors, [m] or [m, w], int32 or fp32 -> (mine [sum of w, width] int32 for
    _gathered_rows: tensor after tensor, transposed, row i at column i, fp32 as its bits, zero past column m; spec: every
    tensor's (w, dtype, dim)).  The spec does not depend on m: it is the same on every rank, one with no rows included."""
    m = tensors[0].shape[0]
    spec = [(1 if t.dim() == 1 else t.shape[1], t.dtype, t.dim()) for t in tensors]
    mine = torch.zeros((sum(w for w, _, _ in spec), width), dtype=torch.int32, device=tensors[0].device)
    mine[:, :m] = torch.cat([t.reshape(m, w).view(torch.int32).T for t, (w, _, _) in zip(tensors, spec)], 0)
    return mine, spec


def _unpack_rows(rows, spec):
    """The inverse of _pack_rows on the gathered rows [sum of w, n]: the tensors [n] / [n, w] of every rank's rows, bit for bit."""
    out = [part.T.contiguous().view(dtype) for part, (_, dtype, _) in zip(torch.split(rows, [w for w, _, _ in spec]), spec)]
    return tuple(t[:, 0].contiguous() if dim == 1 else t for t, (_, _, dim) in zip(out, spec))


def _two_stage_lists(index, q_feat, q_mask, C, W, rank, chunk, norm=None, nprobe=None, local_scaling=None, mutual_proximity=None):
    """(cand [n, C] int32, fine [n, C] fp32) on the device, the same on every rank: this rank's queries searched, one gather.
    norm: (cand, fine, corr [n, C] fp32, gate [n] int32); local_scaling (never with norm): (cand, fine, corr [n, C] fp32, qstat
    [n, 2] fp32); mutual_proximity (never with either): (cand, fine, corr [n, C] fp32, qstat [n, 3] fp32); nprobe: the candidates
    of the index's inverted file, and as the last element stats [n, 3] int32 (GalleryIndex.candidates, ivf_stats).  Whatever
    `candidates` returns travels in that one gather, in its order."""
    n = q_feat.shape[0]
    r0, r1 = slab_bounds(n, W, rank)
    out = index.candidates(q_feat[r0:r1], q_mask[r0:r1], C, chunk, norm=norm, nprobe=nprobe, ivf_stats=nprobe is not None,
                           local_scaling=local_scaling, mutual_proximity=mutual_proximity)
    if W > 1:
        mine, spec = _pack_rows(out, -(-n // W))
        out = _unpack_rows(_gathered_rows(mine, n, W), spec)
    return out


class _TwoStageCorrection(NamedTuple):
    """What two_stage_evaluation needs to know of the one correction of the candidate scores (norm, local_scaling or
    mutual_proximity)."""
    key: str                    # the corrected dictionary's key in the raw one
    label: str                  # its log tag
    attach: Callable            # (index, bank items, their mask): the index-time statistics
    fields: Callable            # (the direction's extra result of `candidates`, its number of queries) -> the fields it gains


def _two_stage_hubness(cand, score, K, n_gallery, gt_begin, gt_end):
    """Hubness of the top-K lists of gathered candidate scores (the same on every rank): nr_cand_norm_rerank without a
    normaliser orders them, nr_topk_occurrences counts them."""
    idx, _, _, _ = ops.cand_norm_rerank(score, cand, n_gallery, K, want_corr=False)
    occ = torch.stack(ops.topk_occurrences(idx, n_gallery, gt_begin, gt_end)).cpu().numpy()
    return RetrievalMetrics.hubness_from_occurrences(occ[0], occ[1], K, cand.shape[0])


def two_stage_evaluation(model, text_feat, video_feat, text_mask, video_mask, args, n_candidates, cut_off_points=None, chunk=256,
                         norm=None, beta=20.0, qb_k=1, querybank=None, hubness_k=0, n_lists=0, nprobe=0, ivf_iters=10, ivf_seed=0,
                         local_scaling=None, local_scaling_k=10, mutual_proximity=None):
    """-> (t2v, v2t) of two-stage retrieval with n_candidates (1..128) candidates per query, identical on every rank: R1 / R5 /
    R10 / R50 (None where K > C), cand_recall (percent of the queries whose ground truth is among their candidates),
    n_candidates, cols, and MR / MedianR / MeanR only when every query was found.  Every argument is checked before any work.

    norm "is" | "qbnorm" (DESIGN.md 6.15): the candidate scores are also normalised against a querybank (`querybank` as in
    sharded_evaluation, None: the model's memory bank; the video index takes its texts, the text index its videos) with
    inverse temperature beta and, for qbnorm, the activation lists' length qb_k.  Each direction gains ["normalised"]: the same
    fields computed from the corrected scores, `gated` (percent of the queries normalised) and `label`.  hubness_k = K, 1 <= K
    <= n_candidates: the raw and the normalised dictionary each gain ["hubness"] of the top-K of their candidate scores.

    n_lists = L >= 1 with nprobe = P in [1, min(L, 128)] (0: off): both galleries get an inverted file of L lists
    (build_ivf with ivf_iters rounds and ivf_seed, on every rank, deterministic) and every figure above is that of the candidates
    taken from each query's P probed lists.  Each direction gains n_lists, nprobe, pool_mean (the mean pool length / the gallery's
    size) and ivf_overlap (the mean share of the exact prefilter's candidates that the inverted file's lists kept; the exact
    lists are computed for this figure only).  The per-query counts travel in the direction's one gather.

    local_scaling "csls" | "nicdm" | "ls" with local_scaling_k = K in [1, n_candidates] (not with norm): the
    candidate scores are also locally scaled -- every gallery item's neighbourhood of K is taken in the querybank (as for norm),
    a query's among its own candidates.  Each direction gains ["local_scaled"]: the raw dictionary's fields computed from the
    corrected scores, `mode`, `k` and `label`, and with hubness_k its ["hubness"].  corr and the queries' statistics travel in the
    direction's one gather.

    mutual_proximity "emp" | "gauss" (not with norm or local_scaling): the candidate scores are also replaced by
    their mutual proximity -- every gallery item's line is taken in the querybank (as for norm), a query's among its own
    candidates.  Each direction gains ["mutual_proximity"]: the raw dictionary's fields computed from the corrected scores, `mode`
    and `label`, and with hubness_k its ["hubness"].  corr and the queries' statistics travel in the direction's one gather."""
    from .search import (GalleryIndex, check_candidates, check_chunk, check_corrections, check_ivf_build, check_local_scaling_k,
                         check_nprobe)
    C, chunk = check_candidates(n_candidates), check_chunk(chunk)
    norm, local_scaling, mutual_proximity = check_corrections(norm, local_scaling, mutual_proximity)
    if local_scaling is not None:
        local_scaling_k = check_local_scaling_k(local_scaling_k)
        if local_scaling_k > C:
            raise ValueError(f"local_scaling_k must lie in [1, n_candidates = {C}], got {local_scaling_k}")
    hubness_k = _check_hubness_k(hubness_k)
    if hubness_k > C:
        raise ValueError(f"hubness_k must lie in [1, n_candidates = {C}], got {hubness_k}")
    if norm is not None:
        beta, qb_k = ops._check_beta(beta), ops._check_k(qb_k)
    for feat, mask, what in ((text_feat, text_mask, "text"), (video_feat, video_mask, "video")):
        if not torch.is_tensor(feat) or feat.dim() != 3 or not torch.is_tensor(mask) or tuple(mask.shape) != tuple(feat.shape[:2]):
            raise ValueError(f"{what} features must be [n, tokens, d] with a mask [n, tokens]")
    n_rows, n_cols = text_feat.shape[0], video_feat.shape[0]
    if n_rows < 1 or n_cols < 1:
        raise ValueError("two-stage evaluation needs at least one text and one video")
    if cut_off_points is None:
        if n_cols != n_rows:
            raise ValueError("single-sentence retrieval: one text per video expected")
        ends = None
    else:
        ends = _group_ends(cut_off_points, n_rows, n_cols)
    if isinstance(n_lists, bool) or not isinstance(n_lists, int) or n_lists < 0:
        raise ValueError(f"n_lists must be an integer >= 0 (0 = the exact prefilter), got {n_lists!r}")
    if n_lists:
        try:
            n_lists, ivf_iters, ivf_seed = check_ivf_build(n_lists, ivf_iters, ivf_seed, min(n_rows, n_cols))
        except ValueError as e:
            raise ValueError(f"{e} (n_lists / ivf_iters / ivf_seed of {n_rows} texts and {n_cols} videos)") from None
        nprobe = check_nprobe(nprobe, n_lists)
    elif nprobe not in (0, None) or isinstance(nprobe, bool):
        raise ValueError(f"nprobe={nprobe!r} needs an inverted file: give n_lists >= 1")
    else:
        nprobe = None
    corrects = norm is not None or local_scaling is not None or mutual_proximity is not None
    bank = _querybank(model, querybank, text_feat.device) if corrects else None
    W = _world(args)
    rank = comm.get_rank() if W > 1 else 0
    text_mask, video_mask = text_mask.float(), video_mask.float()
    index_v, index_t = GalleryIndex(model, video_feat, video_mask, "video"), GalleryIndex(model, text_feat, text_mask, "text")
    corrected = None
    if norm is not None:
        corrected = _TwoStageCorrection("normalised", two_stage_norm_label(C, norm, beta, qb_k),
                                        lambda index, feat, mask: index.attach_querybank(feat, mask, beta, qb_k, chunk),
                                        lambda gate, n: dict(gated=float(int(gate.sum())) * 100 / n))
    if local_scaling is not None:
        corrected = _TwoStageCorrection("local_scaled", two_stage_local_scaling_label(C, local_scaling, local_scaling_k),
                                        lambda index, feat, mask: index.attach_localscale(feat, mask, local_scaling_k, chunk),
                                        lambda qstat, n: dict(mode=local_scaling, k=local_scaling_k))
    if mutual_proximity is not None:
        corrected = _TwoStageCorrection("mutual_proximity", two_stage_mutual_proximity_label(C, mutual_proximity),
                                        lambda index, feat, mask: index.attach_mutualprox(feat, mask, chunk),
                                        lambda qstat, n: dict(mode=mutual_proximity))
    if corrected is not None:
        corrected.attach(index_v, bank[0], bank[1])
        corrected.attach(index_t, bank[2], bank[3])
    if nprobe is not None:
        index_v.build_ivf(n_lists, ivf_iters, ivf_seed, chunk)
        index_t.build_ivf(n_lists, ivf_iters, ivf_seed, chunk)
    lists_t = _two_stage_lists(index_v, text_feat, text_mask, C, W, rank, chunk, norm, nprobe, local_scaling, mutual_proximity)
    lists_v = _two_stage_lists(index_t, video_feat, video_mask, C, W, rank, chunk, norm, nprobe, local_scaling, mutual_proximity)
    cand_t, cand_v = lists_t[0].cpu().numpy(), lists_v[0].cpu().numpy()

    def metrics(score_t, score_v):
        score_t, score_v = score_t.cpu().numpy(), score_v.cpu().numpy()
        if ends is not None:
            return two_stage_multi_sentence_metrics(cand_t, score_t, cand_v, score_v, ends, C)
        gt = np.arange(n_rows)
        return (two_stage_metrics(*two_stage_counts(cand_t, score_t, gt), C), two_stage_metrics(*two_stage_counts(cand_v, score_v, gt), C))

    def add_hubness(m_t, m_v, score_t, score_v):
        rb, re_, cb, ce = _ground_truth(n_rows, n_cols, ends, score_t.device)
        m_t["hubness"] = _two_stage_hubness(lists_t[0], score_t, hubness_k, n_cols, rb, re_)
        m_v["hubness"] = _two_stage_hubness(lists_v[0], score_v, hubness_k, n_rows, cb, ce)

    t2v, v2t = metrics(lists_t[1], lists_v[1])
    if hubness_k:
        add_hubness(t2v, v2t, lists_t[1], lists_v[1])
    if corrected is not None:
        nt, nv = metrics(lists_t[2], lists_v[2])
        if hubness_k:
            add_hubness(nt, nv, lists_t[2], lists_v[2])
        for m, n, extra, raw in ((nt, n_rows, lists_t[3], t2v), (nv, n_cols, lists_v[3], v2t)):
            m.update(corrected.fields(extra, n), label=corrected.label)
            raw[corrected.key] = m
    if nprobe is not None:
        for m, lists, n_gallery in ((t2v, lists_t, n_cols), (v2t, lists_v, n_rows)):
            stats = lists[-1].cpu().numpy().astype(np.float64)                  # pool length, kept, the exact prefilter's count
            share = np.where(stats[:, 2] > 0, stats[:, 1] / np.maximum(stats[:, 2], 1), 1.0)
            m.update(n_lists=n_lists, nprobe=nprobe, pool_mean=float(stats[:, 0].mean()) / n_gallery, ivf_overlap=float(share.mean()))
    return t2v, v2t
