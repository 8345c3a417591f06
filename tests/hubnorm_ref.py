"""NumPy restatement of the test-time hubness corrections IS, DSL and QB-Norm (DESIGN.md "Test-time hubness reduction").  The
reference has no code for them, so this file stands in for it: the definitions written out plainly, in fp64, with float32
where the definitions say so (the product beta * x, and the whole IS formula).

S [rows = texts / sentences, columns = videos].  T: text->video scores, its rows are the queries; V: video->text scores, its
columns are the queries."""
import numpy as np

import hubness_ref as H


def beta_x(X, beta):
    """fl(beta * x) in float32, as fp64."""
    return (np.float32(beta) * np.asarray(X, dtype=np.float32)).astype(np.float64)


def lse(X, beta, axis):
    """Log-sum-exp of beta * X along `axis` over the non-NaN entries: max + log(sum exp(beta x - max)), an entry equal to the
    max adding exactly 1; -inf when no entry is left."""
    B = beta_x(X, beta)
    ok = ~np.isnan(B)
    m = np.max(np.where(ok, B, -np.inf), axis=axis, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(B == m, 0.0, B - m)
        s = np.sum(np.where(ok, np.exp(d), 0.0), axis=axis)
    m = np.squeeze(m, axis=axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, m + np.log(np.where(s > 0, s, 1.0)), -np.inf)


def is_scores(S, beta, c, axis):
    """IS in log form, float32 bit for bit: fl(fl(beta s) - c), c per column (axis 0: T) or per row (axis 1: V)."""
    b = np.float32(beta) * np.asarray(S, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    return (b - (c[None, :] if axis == 0 else c[:, None])).astype(np.float32)


def dsl_scores(S, beta, c, axis):
    """DSL in fp64: s * exp(beta s - c)."""
    S64 = np.asarray(S, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return S64 * np.exp(float(np.float32(beta)) * S64 - (c[None, :] if axis == 0 else c[:, None]))


def activation(Q, qb_k, n_gallery):
    """bool [n_gallery]: the items in the top-qb_k list of some line of Q [n_bank, n_gallery]."""
    idx, _ = H.topk_lists(Q, qb_k)
    act = np.zeros(n_gallery, dtype=bool)
    act[idx[idx >= 0]] = True
    return act


def gates(S, Qt, Qv, qb_k):
    """(row_gate [n_rows], col_gate [n_cols]) of QB-Norm: a text query is normalised when the top-1 of its row of S is in A_v
    (videos in the top-qb_k list of some bank text, Qt [M, n_cols]); a video query when the top-1 of its column of S is in
    A_t (test texts in the top-qb_k list of some bank video, Qv [n_rows, M])."""
    S = np.asarray(S, dtype=np.float32)
    a_v = activation(Qt, qb_k, S.shape[1])
    a_t = activation(np.asarray(Qv, dtype=np.float32).T, qb_k, S.shape[0])
    r1, _ = H.topk_lists(S, 1)
    c1, _ = H.topk_lists(S.T, 1)
    row_gate = (r1[:, 0] >= 0) & a_v[np.maximum(r1[:, 0], 0)]
    col_gate = (c1[:, 0] >= 0) & a_t[np.maximum(c1[:, 0], 0)]
    return row_gate, col_gate


def normalise(S, mode, beta, Qt=None, Qv=None, qb_k=1, c_v=None, c_t=None):
    """(T, V) of the whole matrix S.  is / dsl: the querybank is S itself; qbnorm: Qt = sim(bank texts, test videos), Qv =
    sim(test texts, bank videos).  c_v / c_t override the normalisers (e.g. with the GPU's own)."""
    S = np.asarray(S, dtype=np.float32)
    if mode in ("is", "dsl"):
        Qt, Qv = S, S
    c_v = lse(Qt, beta, 0) if c_v is None else c_v
    c_t = lse(Qv, beta, 1) if c_t is None else c_t
    if mode == "dsl":
        return dsl_scores(S, beta, c_v, 0), dsl_scores(S, beta, c_t, 1)
    T, V = is_scores(S, beta, c_v, 0), is_scores(S, beta, c_t, 1)
    if mode == "qbnorm":
        row_gate, col_gate = gates(S, Qt, Qv, qb_k)
        T = np.where(row_gate[:, None], T, S)
        V = np.where(col_gate[None, :], V, S)
    return T, V


def single_ranks(M):
    """0-based ranks of the diagonal in every row of M (nr_slab_ranks's rule: scores above it, then one rank per entry equal
    to it, rows in order)."""
    M = np.asarray(M)
    d = np.diag(M)[:, None]
    greater = np.sum(M > d, axis=1)
    equal = np.sum(M == d, axis=1)
    return np.concatenate([np.arange(g, g + e) for g, e in zip(greater, equal)]).astype(np.int64)


def group_ranks(T, cut_off_points):
    """Multi-sentence text->video: 0-based rank of every sentence's own video in its row of T -- scores above it, NaN scores,
    and equal scores at lower video indices ahead of it; sentences whose own score is not finite are not ranked."""
    T = np.asarray(T)
    ends = np.asarray(cut_off_points, dtype=np.int64) + 1
    group = np.searchsorted(ends, np.arange(T.shape[0]), side="right")
    out = []
    for s, g in enumerate(group):
        own = T[s, g]
        if not np.isfinite(own):
            continue
        j = np.arange(T.shape[1])
        out.append(int(np.sum((T[s] > own) | np.isnan(T[s]) | ((T[s] == own) & (j < g)))))
    return np.asarray(out, dtype=np.int64)


def group_max(V, cut_off_points):
    """[video, caption group]: the best score any sentence of group g reaches in column j of V (NaN never wins)."""
    V = np.nan_to_num(np.asarray(V, dtype=np.float64), nan=-np.inf)
    ends = np.asarray(cut_off_points, dtype=np.int64) + 1
    starts = np.concatenate(([0], ends[:-1]))
    return np.stack([V[a:b].max(axis=0) for a, b in zip(starts, ends)]).T


def recall(ranks, k):
    return 100.0 * np.sum(np.asarray(ranks) < k) / len(ranks)
