"""NumPy restatement of the top-k / k-occurrence / hubness definitions (DESIGN.md "Top-k lists and hubness").  The reference
has no hubness code, so this file stands in for it: a plain lexsort per line, no cleverness.

Order of a line: score descending, equal scores by index ascending (-0.0 == +0.0: they compare equal), NaN never selected;
lines with fewer than k non-NaN entries are padded with index -1 / value -inf."""
import numpy as np


def topk_lists(S, k, index0=0):
    """(idx [n,k] int32, val [n,k] fp32): the top-k list of every row of S [n,N]; indices index0 + column."""
    S = np.asarray(S, dtype=np.float32)
    n, N = S.shape
    idx = np.full((n, k), -1, dtype=np.int32)
    val = np.full((n, k), -np.inf, dtype=np.float32)
    for i in range(n):
        keep = np.flatnonzero(~np.isnan(S[i]))
        order = keep[np.lexsort((keep, -S[i, keep].astype(np.float64)))][:k]
        idx[i, :len(order)] = order + index0
        val[i, :len(order)] = S[i, order]
    return idx, val


def occurrences(idx, n_gallery, gt_begin, gt_end):
    """(N_k, GN_k) int64 [n_gallery] of the lists idx [n_q,k]; query q's ground truth is [gt_begin[q], gt_end[q])."""
    occ = np.zeros(n_gallery, dtype=np.int64)
    good = np.zeros(n_gallery, dtype=np.int64)
    for q, row in enumerate(np.asarray(idx)):
        for j in row:
            if 0 <= j < n_gallery:
                occ[j] += 1
                good[j] += int(gt_begin[q] <= j < gt_end[q])
    return occ, good


def ground_truth(n_rows, n_cols, cut_off_points=None):
    """(row_begin, row_end, col_begin, col_end): single-sentence sets item i <-> item i; multi-sentence sets (cut_off_points[g] =
    last sentence of video g): a sentence's ground truth is its video, a video's every sentence of its group."""
    if cut_off_points is None:
        r, c = np.arange(n_rows), np.arange(n_cols)
        return r, r + 1, c, c + 1
    ends = np.asarray(cut_off_points, dtype=np.int64) + 1
    group = np.searchsorted(ends, np.arange(n_rows), side="right")
    return group, group + 1, np.concatenate(([0], ends[:-1])), ends


def summary(occ, good):
    """The hubness summary of one direction, straight from the definitions."""
    occ, good = np.asarray(occ, dtype=np.int64), np.asarray(good, dtype=np.int64)
    n = len(occ)
    total = occ.sum()
    mu = total / n
    std = np.std(occ.astype(np.float64))
    skew = float(np.mean((occ - mu) ** 3) / std ** 3) if std > 0 else 0.0
    hubs = occ > 2 * mu
    bad = occ - good
    return {
        "mu": mu,
        "skewness": skew,
        "anti_hub_pct": 100.0 * np.sum(occ == 0) / n,
        "hub_pct": 100.0 * np.sum(hubs) / n,
        "hub_occurrence_pct": 100.0 * occ[hubs].sum() / total if total else 0.0,
        "bad_hub_pct": 100.0 * np.sum(hubs & (bad > good)) / n,
        "good_occurrence_pct": 100.0 * good.sum() / total if total else 0.0,
        "max_occurrence": int(occ.max()),
    }


def hubness(S, k, cut_off_points=None):
    """Both directions of the full matrix S [rows = texts / sentences, cols = videos] -> (t2v, v2t), each a dict of
    (idx, val, occ, good, summary)."""
    S = np.asarray(S, dtype=np.float32)
    n_rows, n_cols = S.shape
    rb, re_, cb, ce = ground_truth(n_rows, n_cols, cut_off_points)
    out = []
    for M, n_gal, b, e in ((S, n_cols, rb, re_), (S.T, n_rows, cb, ce)):
        idx, val = topk_lists(M, k)
        occ, good = occurrences(idx, n_gal, b, e)
        out.append(dict(idx=idx, val=val, occ=occ, good=good, summary=summary(occ, good)))
    return tuple(out)
