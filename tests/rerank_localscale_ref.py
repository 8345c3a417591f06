"""Plain-loop restatement of the local scaling of two-stage retrieval, so that the tests do not compare the
code under test with itself.

  cand_localscale_rerank   the rule of nr_cand_localscale_rerank in NumPy float32: present slots, the query's top-ls_k list of its
                           raw scores and localscale_ref.line_stats on it, the corrected scores localscale_ref.scores (every
                           operation rounded once) with the query as the row or as the column, the final order; dtype=np.float64
                           gives the formulas in fp64 on the same float32 inputs (the statistics stay the float32 ones)
  rerank                   the final order alone, on given corrected scores
"""
import numpy as np

import localscale_ref as L
from rerank_norm_ref import _order, _selectable, same_bits      # noqa: F401  (same_bits: for the tests)

F = np.float32


def query_list(fine_line, cand_line, n_gallery, ls_k):
    """(idx [ls_k], val [ls_k] f32) of one line: its selectable slots in list order, the first ls_k; -1 / -inf where it has fewer."""
    C = len(cand_line)
    slots = _order(fine_line, [p for p in range(C) if 0 <= cand_line[p] < n_gallery and _selectable(fine_line[p])])[:ls_k]
    idx, val = np.full(ls_k, -1, dtype=np.int64), np.full(ls_k, -np.inf, dtype=F)
    for e, p in enumerate(slots):
        idx[e], val[e] = cand_line[p], fine_line[p]
    return idx, val


def query_stats(fine, cand, n_gallery, ls_k):
    """qstat [n, 2] f32 = (mean, kth) of every line's top-ls_k list: localscale_ref.line_stats."""
    fine, cand = np.asarray(fine, dtype=F), np.asarray(cand)
    lists = [query_list(fine[i], cand[i], n_gallery, ls_k) for i in range(len(cand))]
    mean, kth = L.line_stats(np.stack([i for i, _ in lists]), np.stack([v for _, v in lists]))
    return np.stack([mean, kth], axis=1)


def rerank(corr, cand, n_gallery, k):
    """(idx [n, k] int32, val [n, k] f32): the top k of corr over the present non-NaN slots, ties by lower position."""
    corr, cand = np.asarray(corr, dtype=F), np.asarray(cand)
    n, C = cand.shape
    idx = np.full((n, k), -1, dtype=np.int32)
    val = np.full((n, k), -np.inf, dtype=F)
    for i in range(n):
        slots = [p for p in range(C) if 0 <= cand[i, p] < n_gallery and _selectable(corr[i, p])]
        for s, p in enumerate(_order(corr[i], slots)[:k]):
            idx[i, s], val[i, s] = cand[i, p], corr[i, p]
    return idx, val


def corrected(fine, cand, n_gallery, g_stat, mode, qstat, query_is_row, dtype=np.float32):
    """corr [n, C] of `dtype`: localscale_ref.scores slot by slot on (fine, the query's statistic, g_stat[cand]); absent -inf."""
    fine, cand, g_stat = np.asarray(fine, dtype=F), np.asarray(cand), np.asarray(g_stat, dtype=F)
    qstat = np.asarray(qstat, dtype=F)
    n, C = cand.shape
    corr = np.full((n, C), -np.inf, dtype=dtype)
    which = 1 if mode == "ls" else 0
    for i in range(n):
        present = [p for p in range(C) if 0 <= cand[i, p] < n_gallery]
        if not present:
            continue
        s, gs, qs = fine[i, present], g_stat[cand[i, present]], qstat[i, which:which + 1]
        if query_is_row:                                         # one row (the query), the line's items as columns
            corr[i, present] = L.scores(s[None, :], mode, qs, gs, dtype)[0]
        else:                                                    # the line's items as rows, one column (the query)
            corr[i, present] = L.scores(s[:, None], mode, gs, qs, dtype)[:, 0]
    return corr


def cand_localscale_rerank(fine, cand, n_gallery, k, g_stat, mode, ls_k, query_is_row, dtype=np.float32):
    """(idx [n, k] int32, val [n, k] f32, corr [n, C] dtype, qstat [n, 2] f32)."""
    qstat = query_stats(fine, cand, n_gallery, ls_k)
    corr = corrected(fine, cand, n_gallery, g_stat, mode, qstat, query_is_row, dtype)
    idx, val = rerank(corr.astype(F), cand, n_gallery, k)
    return idx, val, corr, qstat
