"""NumPy restatements of the inverted-file prefilter of two-stage retrieval (neighborretr_amd/search.py build_ivf / ivf_candidates,
csrc/nr_ivf.hip), written from the definitions, not from the kernels.  Everything here is exact: integer keys and
float32 additions in a stated order.

  index    x [N, d] float32 (unit or zero rows), L lists.  Initial centroids x[perm[:L]].  ASSIGN: item g goes to argmax_l c_l . x_g
           by the order of 6.1 (score descending, ties to the LOWER list; a zero vector ties everywhere and goes to list 0; a row
           without a selectable score goes to list 0).  UPDATE: the members of a list are added in ascending gallery index, one
           float32 addition per component, and normalised; an EMPTY list, or one whose sum is the zero vector, keeps its centroid.
           STORAGE: list_offsets [L + 1], list_items [N] (ascending inside a list, lists in order).
  search   PROBES of a query: the top P of its centroid scores by the same order.  POOL: the members of the probed lists,
           concatenated in probe order (a probe of -1 is an empty list).  CANDIDATES: the top C of the pool by (score descending,
           gallery index ascending; -0.0 == +0.0; NaN never taken), then sorted by ascending gallery index, padded with -1.
  consequence 1 (masked_exact): the candidates equal what the exact prefilter selects from the query's coarse row with every entry
           outside the pool set to -inf -- the top C by (score descending, index ascending), where an entry that is -inf BECAUSE it
           is outside the pool is dropped (a cosine is never -inf), sorted by index, padded with -1.
"""
import numpy as np


def score_key(x):
    """The order-preserving uint32 key of float32 scores (nr_order_key of csrc/nr_common.h): NaN -> 0, both zeros one key."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(x)] = 0
    return key


def top_order(scores, k):
    """The first k indices of one line by (score descending, index ascending), NaN never taken; -1 where the line has fewer."""
    key = score_key(scores).astype(np.int64)
    order = [int(i) for i in np.lexsort((np.arange(len(key)), -key)) if key[i] != 0][:k]
    return np.asarray(order + [-1] * (k - len(order)), dtype=np.int32)


def assign(scores):
    """scores [N, L] -> the list of every item: the top-1 of its line, list 0 when the line has no selectable score."""
    return np.asarray([max(int(top_order(row, 1)[0]), 0) for row in np.asarray(scores, dtype=np.float32)], dtype=np.int32)


def layout(lists, L):
    """(list_items [N] int32, list_offsets [L + 1] int32): the members of list 0 in ascending index, then list 1's, ..."""
    lists = np.asarray(lists)
    items = np.argsort(lists, kind="stable").astype(np.int32)
    return items, np.searchsorted(lists[items], np.arange(L + 1)).astype(np.int32)


def list_sums(x, items, offsets):
    """sums [L, d] float32: the members of every list added in list order, one float32 addition per component."""
    x = np.asarray(x, dtype=np.float32)
    sums = np.zeros((len(offsets) - 1, x.shape[1]), dtype=np.float32)
    for l in range(len(offsets) - 1):
        for g in items[offsets[l]:offsets[l + 1]]:
            sums[l] = sums[l] + x[g]
    return sums


def update(centroids, sums, offsets, normalised):
    """The centroids after an update: `normalised` [L, d] where the list has members and a non-zero sum, else the previous one."""
    keep = (np.diff(offsets) == 0) | np.all(sums == 0, axis=1)
    return np.where(keep[:, None], centroids, normalised).astype(np.float32)


def pool(probes, items, offsets):
    """One query's pool: (pool_item int32, base [P] int32) -- the members of the probed lists in probe order and where each
    probed list starts in the pool (a probe outside [0, L) is an empty list)."""
    L = len(offsets) - 1
    parts, base, at = [], [], 0
    for p in probes:
        base.append(at)
        if 0 <= p < L:
            parts.append(items[offsets[p]:offsets[p + 1]])
            at += int(offsets[p + 1] - offsets[p])
    return (np.concatenate(parts).astype(np.int32) if parts else np.zeros((0,), dtype=np.int32)), np.asarray(base, dtype=np.int32)


def select(scores, items, length, C):
    """(cand [C] int32, score [C] float32) of one pool line: the top C of its first `length` entries by (score descending,
    gallery index ascending), NaN never taken; then in ascending gallery index, padded with -1 / -inf."""
    scores, items = np.asarray(scores, dtype=np.float32)[:length], np.asarray(items)[:length]
    key = score_key(scores).astype(np.int64)
    order = [i for i in np.lexsort((items, -key)) if key[i] != 0][:C]
    order = sorted(order, key=lambda i: items[i])
    pad = C - len(order)
    return (np.asarray([items[i] for i in order] + [-1] * pad, dtype=np.int32),
            np.asarray([scores[i] for i in order] + [-np.inf] * pad, dtype=np.float32))


def masked_exact(coarse_row, pool_items, C):
    """Consequence 1 for one query: the exact prefilter on its coarse row with the entries outside the pool at -inf."""
    row = np.full(len(coarse_row), -np.inf, dtype=np.float32)
    inside = np.zeros(len(coarse_row), dtype=bool)
    inside[pool_items] = True
    row[inside] = np.asarray(coarse_row, dtype=np.float32)[inside]
    picked = sorted(int(i) for i in top_order(row, C) if i >= 0 and inside[i])
    return np.asarray(picked + [-1] * (C - len(picked)), dtype=np.int32)


def overlap(exact, ivf):
    """The mean share of the exact prefilter's candidates (rows of `exact`, -1 = absent) that the rows of `ivf` kept; a query
    whose exact list is empty counts 1."""
    shares = []
    for e, c in zip(np.asarray(exact), np.asarray(ivf)):
        e = e[e >= 0]
        shares.append(len(set(e.tolist()) & set(c[c >= 0].tolist())) / len(e) if len(e) else 1.0)
    return float(np.mean(shares))
