"""Restatement of the paired permutation test (DESIGN.md "Paired permutation tests"), the yardstick of nr_permtest_rank_stats,
nr_permtest_unit_sums and the summaries of RetrievalMetrics: NumPy for the containers, Python ints for the arithmetic, plain loops.
It shares nothing with the product."""
from fractions import Fraction

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SALT = 0x7065726D74657374
DEFAULT_CUTS = (1, 5, 10, 50)
IR_METRICS = ("MRR", "mAP", "nDCG10", "RPrec")
IR_ONE = 1 << 32


def sm64(seed, c):
    """SM64(seed, c): the (c + 1)-th output of SplitMix64 seeded with `seed`, in Python ints modulo 2^64."""
    z = (int(seed) + (int(c) + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def swap_bit(seed, p, u):
    """s(p, u) = SM64(seed ^ salt, (p << 32) | u) >> 63."""
    return sm64((int(seed) & MASK) ^ SALT, (int(p) << 32) | int(u)) >> 63


def swap_bits(seed, p, U):
    return [swap_bit(seed, p, u) for u in range(U)]


def _units(ranks, unit_end):
    """The list of every unit's entries."""
    ranks = [int(r) for r in np.asarray(ranks).reshape(-1)]
    end = [int(e) + 1 for e in np.asarray(unit_end).reshape(-1)]
    begin = [0] + end[:-1]
    assert all(e >= b for b, e in zip(begin, end)) and end[-1] == len(ranks)
    return [ranks[b:e] for b, e in zip(begin, end)]


def entry_stats(r, cuts=DEFAULT_CUTS):
    """[n, sum, med_lo, med_hi, hits...] of a multiset of ranks, Python ints."""
    r = sorted(int(x) for x in r)
    n = len(r)
    med = [r[(n - 1) // 2], r[n // 2]] if n else [-1, -1]
    return [n, sum(r)] + med + [sum(1 for x in r if x < c) for c in cuts]


def rank_stats(ranks_a, unit_end_a, ranks_b, unit_end_b, cuts=DEFAULT_CUTS, seed=0, p0=0, n_perm=1000):
    """int64 [n_perm, 2, 4 + K]: the statistics of the sides X, Y of permutations p0 .. p0 + n_perm - 1."""
    ua, ub = _units(ranks_a, unit_end_a), _units(ranks_b, unit_end_b)
    U = len(ua)
    assert len(ub) == U
    out = np.zeros((n_perm, 2, 4 + len(cuts)), dtype=np.int64)
    for i in range(n_perm):
        x, y = [], []
        for u in range(U):
            s = swap_bit(seed, p0 + i, u)
            x += ub[u] if s else ua[u]
            y += ua[u] if s else ub[u]
        out[i, 0], out[i, 1] = entry_stats(x, cuts), entry_stats(y, cuts)
    return out


def unit_sums(values_a, values_b, seed=0, p0=0, n_perm=1000):
    """int64 [n_perm, Q]: side X of the per-unit sums."""
    va, vb = np.asarray(values_a, dtype=np.int64), np.asarray(values_b, dtype=np.int64)
    U, Q = va.shape
    assert vb.shape == (U, Q)
    out = np.zeros((n_perm, Q), dtype=np.int64)
    for i in range(n_perm):
        acc = [0] * Q
        for u in range(U):
            row = vb[u] if swap_bit(seed, p0 + i, u) else va[u]
            for q in range(Q):
                acc[q] += int(row[q])
        out[i] = acc
    return out


# ---- the summaries: every comparison on cross-multiplied integers --------------------------------------------------------------------
def _rank_ratios(row, cuts, median):
    """{metric: (numerator, denominator > 0)} of one row (n, sum, med_lo, med_hi, hits...) with n > 0, Python ints.  The factor 100
    of R@K is kept; the "+ 1" of the two rank metrics cancels in every difference and is left out."""
    n = int(row[0])
    out = {f"R{c}": (100 * int(row[4 + k]), n) for k, c in enumerate(cuts)}
    out["MedianR"] = (int(row[2]) + int(row[3]) if median == "mid" else 2 * int(row[2]), 2)
    out["MeanR"] = (int(row[1]), n)
    return out


def _difference(x, y):
    """x - y of two ratios as (numerator, denominator > 0)."""
    return x[0] * y[1] - y[0] * x[1], x[1] * y[1]


def _p_values(d0, ds, n_perm, n_empty, seed):
    """The summary from the observed differences d0 {metric: (num, den)} and the permutations' ds (a list of such dictionaries):
    d >= d0 is num * den0 >= num0 * den, since every denominator is positive."""
    kept = len(ds)
    out = {"n_perm": n_perm, "n_empty": n_empty, "kept": kept, "seed": seed}
    for name, (n0, m0) in d0.items():
        two = ge = le = 0
        for d in ds:
            n, m = d[name]
            left, right = n * m0, n0 * m
            two += abs(left) >= abs(right)
            ge += left >= right
            le += left <= right
        out[name] = {"diff": float(Fraction(n0, m0)), "p_two": (1 + two) / (1 + kept), "p_ge": (1 + ge) / (1 + kept),
                     "p_le": (1 + le) / (1 + kept)}
    return out


def permutation_summary(stats, cuts, entries_a, entries_b, median="mid", seed=0):
    """The summary of a minus b from stats [n_perm, 2, 4 + K] (rank_stats) and the two un-permuted entry lists (both non-empty)."""
    fa = _rank_ratios(entry_stats(entries_a, cuts), cuts, median)
    fb = _rank_ratios(entry_stats(entries_b, cuts), cuts, median)
    d0 = {k: _difference(fa[k], fb[k]) for k in fa}
    ds, empty = [], 0
    for row in np.asarray(stats).tolist():
        if row[0][0] == 0 or row[1][0] == 0:
            empty += 1
            continue
        x, y = _rank_ratios(row[0], cuts, median), _rank_ratios(row[1], cuts, median)
        ds.append({k: _difference(x[k], y[k]) for k in x})
    out = _p_values(d0, ds, len(stats), empty, seed)
    out["median"] = median
    return out


def _ir_ratios(row):
    return {name: (100 * int(row[1 + i]), IR_ONE * int(row[0])) for i, name in enumerate(IR_METRICS)}


def ir_permutation_summary(sums_x, columns_a, columns_b, seed=0):
    """The summary of a minus b from sums_x [n_perm, 5] (unit_sums of the two column sets) and the columns [U, 5] themselves."""
    ta = [sum(int(v) for v in col) for col in np.asarray(columns_a).T]
    tb = [sum(int(v) for v in col) for col in np.asarray(columns_b).T]
    fa, fb = _ir_ratios(ta), _ir_ratios(tb)
    d0 = {k: _difference(fa[k], fb[k]) for k in fa}
    ds, empty = [], 0
    for x in np.asarray(sums_x).tolist():
        y = [a + b - v for a, b, v in zip(ta, tb, x)]
        if x[0] == 0 or y[0] == 0:
            empty += 1
            continue
        fx, fy = _ir_ratios(x), _ir_ratios(y)
        ds.append({k: _difference(fx[k], fy[k]) for k in fx})
    return _p_values(d0, ds, len(sums_x), empty, seed)


# ---- all permutations at once, for units of exactly one entry each (the calibration runs on it) -------------------------------------
def swap_matrix(seed, p0, n_perm, U):
    """s(p, u) for p in [p0, p0 + n_perm), u in [0, U): int64 [n_perm, U], uint64 wrap-around in NumPy."""
    c = (np.arange(p0, p0 + n_perm, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(U, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        z = np.uint64((int(seed) & MASK) ^ SALT) + (c + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(63)).astype(np.int64)


def single_entry_stats(ranks_a, ranks_b, cuts=DEFAULT_CUTS, seed=0, p0=0, n_perm=1000):
    """rank_stats [n_perm, 2, 4 + K] for two rankings whose units hold exactly one entry each."""
    a, b = np.asarray(ranks_a, dtype=np.int64).reshape(-1), np.asarray(ranks_b, dtype=np.int64).reshape(-1)
    U = len(a)
    assert len(b) == U
    s = swap_matrix(seed, p0, n_perm, U) == 1
    out = []
    for r in (np.where(s, b[None, :], a[None, :]), np.where(s, a[None, :], b[None, :])):
        r = np.sort(r, axis=1)
        cols = [np.full(n_perm, U), r.sum(1), r[:, (U - 1) // 2], r[:, U // 2]] + [(r < c).sum(1) for c in cuts]
        out.append(np.stack(cols, axis=1))
    return np.stack(out, axis=1).astype(np.int64)
