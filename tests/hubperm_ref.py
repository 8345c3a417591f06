"""Restatement of the paired permutation test of hubness (DESIGN.md "Permutation test of hubness"), the yardstick of
nr_permtest_hubness and of RetrievalMetrics.hubness_moments / hubness_permutation_summary: NumPy for the containers, Python ints for the
arithmetic, plain loops.  It shares nothing with the product (the swap bits are restated here too; a test holds them to permtest_ref)."""
import math

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SALT = 0x7065726D74657374
SLOTS = ("S1", "S2", "S3", "anti", "hubs", "hub_occ", "bad_hubs", "good", "max")
RATIONAL = ("anti_hub_pct", "hub_pct", "bad_hub_pct", "hub_occurrence_pct", "good_occurrence_pct", "max_occurrence")
METRICS = ("skewness",) + RATIONAL


def sm64(seed, c):
    """SM64(seed, c): the (c + 1)-th output of SplitMix64 seeded with `seed`, in Python ints modulo 2^64."""
    z = (int(seed) + (int(c) + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def swap_bit(seed, p, u):
    """s(p, u) = SM64(seed ^ salt, (p << 32) | u) >> 63."""
    return sm64((int(seed) & MASK) ^ SALT, (int(p) << 32) | int(u)) >> 63


def unit_of_list(unit_end, n_lists):
    """The unit of every list: unit u owns the lists unit_end[u - 1] + 1 .. unit_end[u]."""
    end = [int(e) for e in np.asarray(unit_end).reshape(-1)]
    assert end and end[-1] == n_lists - 1 and all(b >= a for a, b in zip([-1] + end[:-1], end))
    unit, u = [], 0
    for q in range(n_lists):
        while end[u] < q:
            u += 1
        unit.append(u)
    return unit


def counts(lists, n_gallery, gt_begin, gt_end):
    """(N, GN) as lists of Python ints: N[j] = the lists that hold j, GN[j] = those whose ground-truth range holds j.  Absent slots
    (-1) and indices outside [0, n_gallery) are not counted."""
    N, GN = [0] * n_gallery, [0] * n_gallery
    for q, row in enumerate(lists):
        for j in row:
            j = int(j)
            if 0 <= j < n_gallery:
                N[j] += 1
                if int(gt_begin[q]) <= j < int(gt_end[q]):
                    GN[j] += 1
    return N, GN


def moments(N, GN):
    """The nine integers of one side from its counters."""
    G = len(N)
    S1 = sum(N)
    hubs = [j for j in range(G) if N[j] * G > 2 * S1]
    return [S1, sum(n * n for n in N), sum(n * n * n for n in N), sum(1 for n in N if n == 0), len(hubs), sum(N[j] for j in hubs),
            sum(1 for j in hubs if N[j] - GN[j] > GN[j]), sum(GN), max(N)]


def hubness_stats(idx_a, idx_b, unit_end, n_gallery, gt_begin, gt_end, seed=0, p0=0, n_perm=1000):
    """int64 [n_perm, 2, 9]: the integers of the sides X, Y of permutations p0 .. p0 + n_perm - 1."""
    a, b = np.asarray(idx_a), np.asarray(idx_b)
    assert a.ndim == 2 and a.shape == b.shape
    n_lists = a.shape[0]
    unit = unit_of_list(unit_end, n_lists) if n_lists else []
    a, b = a.tolist(), b.tolist()
    out = np.zeros((n_perm, 2, len(SLOTS)), dtype=np.int64)
    for i in range(n_perm):
        bits = {}
        x, y = [], []
        for q in range(n_lists):
            u = unit[q]
            if u not in bits:
                bits[u] = swap_bit(seed, p0 + i, u)
            x.append(b[q] if bits[u] else a[q])
            y.append(a[q] if bits[u] else b[q])
        out[i, 0] = moments(*counts(x, n_gallery, gt_begin, gt_end))
        out[i, 1] = moments(*counts(y, n_gallery, gt_begin, gt_end))
    return out


# ---- the figures of a side, and the summary ------------------------------------------------------------------------------------------
def skewness(m, G):
    """float(c) / (float(a) sqrt(float(a))) with a = G S2 - S1^2, c = G^2 S3 - 3 G S1 S2 + 2 S1^3 in Python ints; 0.0 when a = 0."""
    S1, S2, S3 = int(m[0]), int(m[1]), int(m[2])
    a = G * S2 - S1 * S1
    c = G * G * S3 - 3 * G * S1 * S2 + 2 * S1 * S1 * S1
    return float(c) / (float(a) * math.sqrt(float(a))) if a else 0.0


def ratios(m, G):
    """{metric: (numerator, denominator > 0)} of the six rational figures of a non-empty side (S1 > 0)."""
    m = [int(v) for v in m]
    return {"anti_hub_pct": (100 * m[3], G), "hub_pct": (100 * m[4], G), "bad_hub_pct": (100 * m[6], G),
            "hub_occurrence_pct": (100 * m[5], m[0]), "good_occurrence_pct": (100 * m[7], m[0]), "max_occurrence": (m[8], 1)}


def figures(m, G):
    """Every figure of a non-empty side in fp64."""
    out = {"skewness": skewness(m, G)}
    out.update({name: (n / d if name != "max_occurrence" else n) for name, (n, d) in ratios(m, G).items()})
    return out


def summary(stats, moments_a, moments_b, n_gallery, seed=0, only=METRICS):
    """The summary of A minus B from stats [n_perm, 2, 9] and the integers of the un-permuted A and B (both non-empty).  The six
    rational figures are compared on cross-multiplied Python ints; skewness on the fp64 values of the stated formula.  only: the
    metrics wanted (the calibration asks for one or two)."""
    G = int(n_gallery)
    rows = np.asarray(stats).tolist()
    kept = [r for r in rows if r[0][0] > 0 and r[1][0] > 0]
    out = {"n_perm": len(rows), "n_empty": len(rows) - len(kept), "kept": len(kept), "seed": seed}
    n = 1 + len(kept)
    if "skewness" in only:
        d0 = skewness(moments_a, G) - skewness(moments_b, G)
        two = ge = le = 0
        for x, y in kept:
            d = skewness(x, G) - skewness(y, G)
            two += abs(d) >= abs(d0)
            ge += d >= d0
            le += d <= d0
        out["skewness"] = {"diff": d0, "p_two": (1 + two) / n, "p_ge": (1 + ge) / n, "p_le": (1 + le) / n}
    ra, rb = ratios(moments_a, G), ratios(moments_b, G)
    for name in RATIONAL:
        if name not in only:
            continue
        n0, m0 = ra[name][0] * rb[name][1] - rb[name][0] * ra[name][1], ra[name][1] * rb[name][1]
        two = ge = le = 0
        for x, y in kept:
            (xn, xd), (yn, yd) = ratios(x, G)[name], ratios(y, G)[name]
            left, right = (xn * yd - yn * xd) * m0, n0 * (xd * yd)
            two += abs(left) >= abs(right)
            ge += left >= right
            le += left <= right
        out[name] = {"diff": n0 / m0, "p_two": (1 + two) / n, "p_ge": (1 + ge) / n, "p_le": (1 + le) / n}
    return out


# ---- all permutations at once, for units of exactly one list each (the calibration runs on it) --------------------------------------
def swap_matrix(seed, p0, n_perm, U):
    """s(p, u) for p in [p0, p0 + n_perm), u in [0, U): bool [n_perm, U], uint64 wrap-around in NumPy."""
    c = (np.arange(p0, p0 + n_perm, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(U, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        z = np.uint64((int(seed) & MASK) ^ SALT) + (c + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(63)) == np.uint64(1)


def single_list_stats(idx_a, idx_b, n_gallery, seed=0, p0=0, n_perm=1000):
    """hubness_stats [n_perm, 2, 9] for units of one list each whose ground truth is [q, q + 1), every index in [0, n_gallery), the
    lists without repeats and U <= n_gallery: membership matrices and matrix products instead of loops (the products are taken in
    fp64, where integers of this size are exact, and go back to int64)."""
    a, b = np.asarray(idx_a, dtype=np.int64), np.asarray(idx_b, dtype=np.int64)
    U, G = a.shape[0], int(n_gallery)
    assert U <= G and 0 <= min(a.min(), b.min()) and max(a.max(), b.max()) < G
    ma, mb = np.zeros((U, G)), np.zeros((U, G))
    np.put_along_axis(ma, a, 1.0, axis=1)
    np.put_along_axis(mb, b, 1.0, axis=1)
    own = np.zeros((U, G))
    own[np.arange(U), np.arange(U)] = 1.0
    s = swap_matrix(seed, p0, n_perm, U).astype(np.float64)
    sides = []
    for first, second in ((ma, mb), (mb, ma)):                                   # X takes `second` where the bit is set
        N = np.rint(first.sum(0)[None, :] + s @ (second - first)).astype(np.int64)
        GN = np.rint((first * own).sum(0)[None, :] + s @ ((second - first) * own)).astype(np.int64)
        S1 = N.sum(1)
        hub = N * G > 2 * S1[:, None]
        sides.append(np.stack([S1, (N ** 2).sum(1), (N ** 3).sum(1), (N == 0).sum(1), hub.sum(1), (N * hub).sum(1),
                               (hub & (N - GN > GN)).sum(1), GN.sum(1), N.max(1)], axis=1))
    return np.stack(sides, axis=1).astype(np.int64)
