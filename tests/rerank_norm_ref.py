"""Plain-loop restatements of the query-bank normalisation of two-stage retrieval, so that the tests do not
compare the code under test with itself.

  cand_norm_rerank   the rule of nr_cand_norm_rerank in NumPy float32, bit for bit: present slots, top-1, gate, corrected scores
                     fl(fl(beta fine) - norm[cand]) (two float32 operations, no fused multiply-add), the final order
  lse / activation   the index-time statistics in fp64: the log-sum-exp of the float32 products beta * x over the non-NaN
                     entries of a line, and the items found in the top-qb_k list of some bank item
  topk / hubness     the top-K lists of candidate scores and their k-occurrence counts
"""
import math

import numpy as np


def _selectable(x):
    return not math.isnan(float(x))


def _order(scores, slots):
    """The slots in list order: score descending (float comparison: -0.0 == +0.0), equal scores by lower position."""
    return sorted(slots, key=lambda p: (-float(scores[p]), p))


def cand_norm_rerank(fine, cand, n_gallery, k, norm=None, active=None, beta=20.0):
    """(idx [n, k] int32, val [n, k] f32, corr [n, C] f32, gate [n] int32)."""
    fine, cand = np.asarray(fine, dtype=np.float32), np.asarray(cand)
    n, C = cand.shape
    idx = np.full((n, k), -1, dtype=np.int32)
    val = np.full((n, k), -np.inf, dtype=np.float32)
    corr = np.full((n, C), -np.inf, dtype=np.float32)
    gate = np.zeros((n,), dtype=np.int32)
    b = np.float32(beta)
    for i in range(n):
        present = [p for p in range(C) if 0 <= cand[i, p] < n_gallery]
        first = _order(fine[i], [p for p in present if _selectable(fine[i, p])])[:1]
        if norm is not None:
            gate[i] = 1 if active is None else int(bool(first) and active[cand[i, first[0]]] != 0)
        for p in present:
            if gate[i]:
                with np.errstate(invalid="ignore", over="ignore"):
                    corr[i, p] = np.float32(b * fine[i, p]) - np.float32(norm[cand[i, p]])
            else:
                corr[i, p] = fine[i, p]
        for s, p in enumerate(_order(corr[i], [p for p in present if _selectable(corr[i, p])])[:k]):
            idx[i, s], val[i, s] = cand[i, p], corr[i, p]
    return idx, val, corr, gate


def same_bits(a, b):
    """Equal float32 bit patterns; a NaN matches any NaN (its payload is not part of any rule here)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def lse(Q, beta, axis):
    """fp64 log-sum-exp of the float32 products beta * Q along `axis` over the non-NaN entries; -inf when none is left."""
    Q = np.asarray(Q, dtype=np.float32)
    lines = Q.T if axis == 0 else Q
    out = np.full((lines.shape[0],), -np.inf)
    for j, line in enumerate(lines):
        x = [float(np.float32(beta) * v) for v in line if not math.isnan(float(v))]
        if not x:
            continue
        m = max(x)
        if math.isinf(m):
            out[j] = m
            continue
        out[j] = m + math.log(sum(1.0 if v == m else math.exp(v - m) for v in x))
    return out


def topk(scores, cand, n_gallery, k):
    """idx [n, k]: the top k of candidate scores over the present non-NaN slots (the order above), -1 pad."""
    return cand_norm_rerank(scores, cand, n_gallery, k)[0]


def activation(Q, qb_k, axis):
    """bool [n_gallery]: gallery items in the top-qb_k list of some bank item.  axis 1: the bank items are the rows of Q
    [M, n_gallery]; axis 0: they are the columns of Q [n_gallery, M]."""
    Q = np.asarray(Q, dtype=np.float32)
    lines = Q if axis == 1 else Q.T
    act = np.zeros((lines.shape[1],), dtype=bool)
    for line in lines:
        for p in _order(line, [p for p in range(len(line)) if _selectable(line[p])])[:qb_k]:
            act[p] = True
    return act


def occurrences(idx, n_gallery, gt_begin, gt_end):
    """(occ, good) [n_gallery] int64 of lists idx [n_q, k]; query q's ground truth is [gt_begin[q], gt_end[q])."""
    occ, good = np.zeros(n_gallery, dtype=np.int64), np.zeros(n_gallery, dtype=np.int64)
    for q, row in enumerate(np.asarray(idx)):
        for j in row:
            if 0 <= j < n_gallery:
                occ[j] += 1
                good[j] += int(gt_begin[q] <= j < gt_end[q])
    return occ, good


def ground_truth(n_rows, n_cols, ends=None):
    """(row_begin, row_end, col_begin, col_end): item i <-> item i, or (ends[g] = one past the last sentence of video g) a
    sentence's video and a video's sentences."""
    if ends is None:
        r, c = np.arange(n_rows), np.arange(n_cols)
        return r, r + 1, c, c + 1
    group = np.asarray([next(g for g, e in enumerate(ends) if s < e) for s in range(n_rows)])
    begin = np.concatenate(([0], np.asarray(ends)[:-1]))
    return group, group + 1, begin, np.asarray(ends)
