"""Restatement of the rank-aware IR metrics (DESIGN.md "Rank-aware IR metrics"), the yardstick of nr_pair_ranks,
nr_bootstrap_unit_sums and RetrievalMetrics.ir_from_ranks: plain loops over the definition, fp64, nothing shared with the product.

Rows are sentences, columns videos; video g owns the rows [group_end[g-1], group_end[g]); pair s is (row s, column g(s)) and
own[s] = M[s, g(s)].  Entry x at index i of a line is ahead of pair s when x > own[s], or x == own[s] and i is lower than the pair's
own index on that line (IEEE compares).  A pair whose own score is NaN or infinite is unranked (-1)."""
import math

import numpy as np

import bootstrap_ref as B

METRICS = ("MRR", "mAP", "nDCG10", "RPrec")
ONE = 1 << 32


def groups_of(group_end):
    """g(s) for every row: int64 [n_total]."""
    ends = np.asarray(group_end, dtype=np.int64)
    return np.searchsorted(ends, np.arange(int(ends[-1]) if len(ends) else 0), side="right")


def _ahead(line, own, own_index):
    """Entries of `line` ahead of a pair with score `own` at index `own_index`."""
    x = np.asarray(line, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return int(np.sum((x > own) | ((x == own) & (np.arange(len(x)) < own_index))))


def pair_ranks(M, group_end):
    """(rt, rv) int64 [n_total] of the whole matrix M [n_total, V]: the text->video rank of every pair along its row and its
    video->text rank among all sentences along its column; -1 where the pair is unranked."""
    M = np.asarray(M, dtype=np.float32)
    g = groups_of(group_end)
    n_total = len(g)
    assert M.shape[0] == n_total and M.shape[1] == len(group_end)
    rt = np.full((n_total,), -1, dtype=np.int64)
    rv = np.full((n_total,), -1, dtype=np.int64)
    for s in range(n_total):
        own = M[s, g[s]]
        if not np.isfinite(own):
            continue
        rt[s] = _ahead(M[s, :], own, g[s])
        rv[s] = _ahead(M[:, g[s]], own, s)
    return rt, rv


def slab_parts(M, group_end, row0, n_rows):
    """(row_rank [n_rows], col_ahead [n_total]) of the slab M[row0 : row0 + n_rows] as nr_pair_ranks defines them: the slab's rows
    ahead of every pair in its column (0 where unranked)."""
    M = np.asarray(M, dtype=np.float32)
    g = groups_of(group_end)
    rt, _ = pair_ranks(M, group_end)
    col = np.zeros((len(g),), dtype=np.int64)
    for s in range(len(g)):
        own = M[s, g[s]]
        if np.isfinite(own):
            col[s] = _ahead(M[row0:row0 + n_rows, g[s]], own, s - row0)
    return rt[row0:row0 + n_rows], col


def dcg10(ranked):
    """sum over the ranks below 10 of 1 / log2(r + 2)."""
    return sum(1.0 / math.log2(int(x) + 2) for x in sorted(ranked) if x < 10)


def idcg10(m):
    """The DCG of m relevant items at the ranks 0 .. min(m, 10) - 1."""
    return sum(1.0 / math.log2(k + 1) for k in range(1, min(m, 10) + 1))


def query(ranked):
    """(RR, AP, nDCG10, RPrec) of one query from the ranks of its ranked relevant items (m >= 1, distinct)."""
    r = sorted(int(x) for x in ranked)
    m = len(r)
    assert m >= 1 and all(a < b for a, b in zip(r, r[1:])) and r[0] >= 0
    rr = 1.0 / (r[0] + 1)
    ap = sum((k + 1) / (x + 1) for k, x in enumerate(r)) / m
    return rr, ap, dcg10(r) / idcg10(m), sum(1 for x in r if x < m) / m


def queries(ranks, group_end=None):
    """[(slot, (RR, AP, nDCG10, RPrec))] of every query with a ranked pair.  group_end None: every pair is a query (m = 1)."""
    ranks = [int(x) for x in np.asarray(ranks).reshape(-1)]
    if group_end is None:
        return [(s, query([r])) for s, r in enumerate(ranks) if r >= 0]
    out, begin = [], 0
    for g, end in enumerate(int(e) for e in group_end):
        kept = [r for r in ranks[begin:end] if r >= 0]
        begin = end
        if kept:
            out.append((g, query(kept)))
    return out


def ir(ranks, group_end=None):
    """The reported dictionary: means over the queries x 100, n_queries, n_unranked, ranks."""
    q = queries(ranks, group_end)
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    out = {name: (100.0 * sum(v[i] for _, v in q) / len(q) if q else float("nan")) for i, name in enumerate(METRICS)}
    out.update(n_queries=len(q), n_unranked=int(np.sum(ranks < 0)), ranks=np.where(ranks < 0, -1, ranks))
    return out


def unit_columns(ranks, group_end=None, unit_end=None):
    """int64 [U, 5]: per unit the query count and the sums of int(rint(x 2^32)) for RR, AP, nDCG10, RPrec over its queries.  The
    unit is the query slot; with unit_end (group_end None) unit u owns the slots [unit_end[u-1], unit_end[u])."""
    n_slots = len(np.asarray(ranks).reshape(-1)) if group_end is None else len(group_end)
    slots = np.zeros((n_slots, 5), dtype=np.int64)
    for slot, v in queries(ranks, group_end):
        slots[slot] = [1] + [int(np.rint(x * ONE)) for x in v]
    if unit_end is None:
        return slots
    assert group_end is None
    out, begin = np.zeros((len(unit_end), 5), dtype=np.int64), 0
    for u, end in enumerate(int(e) for e in unit_end):
        out[u] = slots[begin:end].sum(axis=0)
        begin = end
    return out


def unit_sums(values, seed=0, b0=0, n_boot=1000):
    """int64 [n_boot, Q]: out[i] = sum of the rows values[u(b0 + i, t)], t < U, with the draws of the rank bootstrap."""
    values = np.asarray(values, dtype=np.int64)
    U = values.shape[0]
    return np.stack([values[B.draws(seed, b0 + i, U)].sum(axis=0) for i in range(n_boot)]) if n_boot else values[:0].copy()


def resampled(sums):
    """{metric: fp64 values of the resamples with count > 0}, from rows (count, RR, AP, nDCG10, RPrec sums)."""
    sums = np.asarray(sums, dtype=np.int64)
    keep = sums[:, 0] > 0
    return {name: 100.0 * sums[keep, 1 + i] / (float(ONE) * sums[keep, 0]) for i, name in enumerate(METRICS)}
