"""Plain-loop restatement of the mutual proximity of two-stage retrieval, so that the tests do not compare the
code under test with itself.

  query_stats             qstat [n, 3] f32 = (c_q, mean, sd) of every line's selectable slots: the raw scores added up in fp64 in
                          position order, then the squared distances from the fp64 mean (population sd); c_q = 0: NaN
  query_counts            r2 of every slot's score in the query's own line (the selectable slots; a slot counts itself as equal)
  item_counts             r2 of every present slot's score in its item's bank line g_line[cand]
  emp_corr / gauss_corr   the corrected lines: mutualprox_ref.emp_scores / mutualprox_ref.tail slot by slot, absent slots -inf;
                          float32 (every operation rounded once) or fp64 on the same float32 inputs
  rerank                  the final order (rerank_localscale_ref.rerank): the present slots whose score is not NaN, value
                          descending, ties by lower position
  item_lines              what attach_mutualprox stores, from the bank product
  planted_hub             the input of the planted-hub tests
"""
import numpy as np

import mutualprox_ref as MP
from rerank_localscale_ref import rerank                        # noqa: F401  (for the tests)
from rerank_norm_ref import _selectable, same_bits              # noqa: F401

F = np.float32
MODES = ("emp", "gauss")


def _present(cand_line, n_gallery):
    return [p for p in range(len(cand_line)) if 0 <= cand_line[p] < n_gallery]


def _line(fine_line, cand_line, n_gallery):
    """The positions of the query's line: present and not NaN, in position order."""
    return [p for p in _present(cand_line, n_gallery) if _selectable(fine_line[p])]


def query_stats(fine, cand, n_gallery):
    fine, cand = np.asarray(fine, dtype=F), np.asarray(cand)
    out = np.full((len(cand), 3), np.nan, dtype=F)
    with np.errstate(all="ignore"):
        for i in range(len(cand)):
            xs = [np.float64(fine[i, p]) for p in _line(fine[i], cand[i], n_gallery)]
            c = len(xs)
            out[i, 0] = c
            if c == 0:
                continue
            total = np.float64(0.0)
            for x in xs:
                total = total + x
            mean = total / np.float64(c)
            m2 = np.float64(0.0)
            for x in xs:
                m2 = m2 + (x - mean) * (x - mean)
            out[i, 1], out[i, 2] = F(mean), F(np.sqrt(m2 / np.float64(c)))
    return out


def _r2(s, xs):
    """2 #{x < s} + #{x == s} with IEEE compares, in a plain loop."""
    less = equal = 0
    for x in xs:
        less += int(x < s)
        equal += int(x == s)
    return 2 * less + equal


def query_counts(fine, cand, n_gallery):
    """r2_q [n, C] int64; 0 at the slots that are absent (their score never enters a formula)."""
    fine, cand = np.asarray(fine, dtype=F), np.asarray(cand)
    out = np.zeros(cand.shape, dtype=np.int64)
    for i in range(len(cand)):
        xs = [fine[i, p] for p in _line(fine[i], cand[i], n_gallery)]
        for p in _present(cand[i], n_gallery):
            out[i, p] = _r2(fine[i, p], xs)
    return out


def item_counts(fine, cand, n_gallery, g_line):
    """r2_g [n, C] int64 against g_line [n_gallery, M]; 0 at the absent slots: no line is looked up for them."""
    fine, cand, g_line = np.asarray(fine, dtype=F), np.asarray(cand), np.asarray(g_line, dtype=F)
    out = np.zeros(cand.shape, dtype=np.int64)
    for i in range(len(cand)):
        for p in _present(cand[i], n_gallery):
            out[i, p] = _r2(fine[i, p], g_line[cand[i, p]])
    return out


def emp_corr(fine, cand, n_gallery, g_line, dtype=np.float32):
    """corr [n, C]: fl(fl(r2_q / 2 c_q) fl(r2_g / 2 c_g)), NaN where the score is, -inf where the slot is absent."""
    fine, cand, g_line = np.asarray(fine, dtype=F), np.asarray(cand), np.asarray(g_line, dtype=F)
    n, C = cand.shape
    r2q, r2g = query_counts(fine, cand, n_gallery), item_counts(fine, cand, n_gallery, g_line)
    g_cnt = MP.line_counts(g_line, 1)
    corr = np.full((n, C), -np.inf, dtype=dtype)
    for i in range(n):
        present = _present(cand[i], n_gallery)
        if not present:
            continue
        c_q = len(_line(fine[i], cand[i], n_gallery))
        corr[i, present] = MP.emp_scores(fine[i, present][None, :], r2q[i, present][None, :], r2g[i, present][None, :], [c_q],
                                         g_cnt[cand[i, present]], dtype)[0]
    return corr


def gauss_corr(fine, cand, n_gallery, qstat, g_mean, g_sd, dtype=np.float32):
    """corr [n, C]: -((Q_q + Q_g) - Q_q Q_g) from the query's (mean, sd) = qstat[:, 1:3] and the items' moments."""
    fine, cand, qstat = np.asarray(fine, dtype=F), np.asarray(cand), np.asarray(qstat, dtype=F)
    g_mean, g_sd = np.asarray(g_mean, dtype=F), np.asarray(g_sd, dtype=F)
    n, C = cand.shape
    corr = np.full((n, C), -np.inf, dtype=dtype)
    for i in range(n):
        present = _present(cand[i], n_gallery)
        if not present:
            continue
        s, g = fine[i, present], cand[i, present]
        a = MP.tail(s, np.full(len(s), qstat[i, 1], dtype=F), np.full(len(s), qstat[i, 2], dtype=F), dtype)
        b = MP.tail(s, g_mean[g], g_sd[g], dtype)
        with np.errstate(all="ignore"):
            corr[i, present] = -((a + b).astype(dtype) - (a * b).astype(dtype)).astype(dtype)
    return corr


def item_lines(Q, side):
    """(g_line [N, M] f32, g_cnt [N] int64, g_mean [N], g_sd [N] f32) from the bank product in the evaluator's orientation: Qt
    [M, N] for a video gallery, Qv [N, M] for a text gallery."""
    Q = np.asarray(Q, dtype=F)
    g_line = np.ascontiguousarray(Q.T) if side == "video" else Q
    mean, sd = MP.moments(g_line, 1)
    return g_line, MP.line_counts(g_line, 1), mean, sd


def cand_mutualprox_rerank(fine, cand, n_gallery, k, mode, g_line, dtype=np.float32, qstat=None):
    """(idx [n, k] int32, val [n, k] f32, corr [n, C] dtype, qstat [n, 3] f32); qstat: the query moments gauss is to use (default:
    the restatement's own)."""
    own = query_stats(fine, cand, n_gallery)
    if mode == "emp":
        corr = emp_corr(fine, cand, n_gallery, g_line, dtype)
    elif mode == "gauss":
        mean, sd = MP.moments(np.asarray(g_line, dtype=F), 1)
        corr = gauss_corr(fine, cand, n_gallery, own if qstat is None else qstat, mean, sd, dtype)
    else:
        raise ValueError(mode)
    idx, val = rerank(corr.astype(F), cand, n_gallery, k)
    return idx, val, corr, own


def moments_close(got, want, rtol=1e-6):
    """qstat-like moments agree: NaN and infinities in the same places with the same signs, the finite ones within rtol."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    inf = np.isinf(want)
    if not np.array_equal(np.isinf(got), inf) or not np.array_equal(got[inf], want[inf]):
        return False
    ok = np.isfinite(want)
    return bool(np.all(np.abs(got[ok] - want[ok]) <= rtol * np.abs(want[ok])))


def top1_occurrences(idx, n_gallery):
    occ = np.zeros(n_gallery, dtype=np.int64)
    for j in np.asarray(idx)[:, 0]:
        if 0 <= j < n_gallery:
            occ[j] += 1
    return occ


HUB, HUB_GALLERY, HUB_C, HUB_M, HUB_SEED = 5, 37, 8, 20, 11


def planted_hub(seed=HUB_SEED, n_gallery=HUB_GALLERY, C=HUB_C, M=HUB_M, hub=HUB):
    """(cand [n, C] int32, fine [n, C] f32, g_line [n_gallery, M] f32, own [n]): one query per item but the hub.  The hub scores
    about 0.6 against every query and against every bank item, a query's own item 0.55, everything else about 0.1.  Raw, the hub is
    every query's top-1.  Under gauss the hub's score is ordinary in the hub's own bank line (upper tail about 1/2) while the own
    item's is far out in its line (upper tail about 0): the own item wins."""
    rng = np.random.default_rng(seed)
    own = np.asarray([i for i in range(n_gallery) if i != hub])
    n = len(own)
    cand = np.zeros((n, C), dtype=np.int32)
    fine = np.zeros((n, C), dtype=F)
    for i, item in enumerate(own):
        others = rng.choice([j for j in range(n_gallery) if j not in (hub, item)], C - 2, replace=False)
        cand[i] = np.sort(np.concatenate(([hub, item], others)))
        fine[i] = np.where(cand[i] == hub, 0.6 + 0.01 * rng.standard_normal(C),
                           np.where(cand[i] == item, 0.55, 0.1 + 0.02 * rng.standard_normal(C))).astype(F)
    g_line = (0.1 + 0.02 * rng.standard_normal((n_gallery, M))).astype(F)
    g_line[hub] = (0.6 + 0.02 * rng.standard_normal(M)).astype(F)
    return cand, fine, g_line, own
