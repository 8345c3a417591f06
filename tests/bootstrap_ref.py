"""NumPy restatement of the bootstrap of rank statistics (DESIGN.md "Bootstrap confidence intervals"), the yardstick of
nr_bootstrap_rank_stats: draws with uint64 wrap-around, concatenate the drawn units' entries, sort, count."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MIX1 = np.uint64(0xBF58476D1CE4E5B9)
MIX2 = np.uint64(0x94D049BB133111EB)
DEFAULT_CUTS = (1, 5, 10, 50)


def sm64(seed, c):
    """SM64(seed, c): the (c + 1)-th output of SplitMix64 seeded with `seed`; c an integer or an array of counters (uint64)."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) % (1 << 64)) + (np.asarray(c, dtype=np.uint64) + np.uint64(1)) * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * MIX1
        z = (z ^ (z >> np.uint64(27))) * MIX2
        return z ^ (z >> np.uint64(31))


def draws(seed, b, U):
    """u(b, t) for t in [0, U): int64 [U]."""
    c = (np.uint64(int(b)) << np.uint64(32)) | np.arange(U, dtype=np.uint64)
    return (((sm64(seed, c) >> np.uint64(32)) * np.uint64(U)) >> np.uint64(32)).astype(np.int64)


def _units(ranks, unit_end):
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    end = np.asarray(unit_end, dtype=np.int64).reshape(-1) + 1
    begin = np.concatenate(([0], end[:-1]))
    assert (end >= begin).all() and end[-1] == len(ranks)
    return ranks, begin, end


def entry_stats(r, cuts=DEFAULT_CUTS):
    """[4 + K] int64 of a multiset of ranks: n, sum, med_lo, med_hi, hits."""
    r = np.sort(np.asarray(r, dtype=np.int64))
    n = len(r)
    med = [int(r[(n - 1) // 2]), int(r[n // 2])] if n else [-1, -1]
    return np.asarray([n, int(r.sum())] + med + [int((r < c).sum()) for c in cuts], dtype=np.int64)


def rank_stats(ranks_a, unit_end_a, ranks_b=None, unit_end_b=None, cuts=DEFAULT_CUTS, seed=0, b0=0, n_boot=1000):
    """int64 [n_boot, V, 4 + K]: the statistics of resamples b0 .. b0 + n_boot - 1."""
    rankings = [_units(ranks_a, unit_end_a)]
    if ranks_b is not None:
        rankings.append(_units(ranks_b, unit_end_b))
    U = len(rankings[0][1])
    assert all(len(b) == U for _, b, _ in rankings)
    out = np.zeros((n_boot, len(rankings), 4 + len(cuts)), dtype=np.int64)
    for i in range(n_boot):
        u = draws(seed, b0 + i, U)
        for v, (ranks, begin, end) in enumerate(rankings):
            size = end[u] - begin[u]
            # entry e of the resample: offset e - first[e's unit] inside the drawn unit
            idx = np.repeat(begin[u], size) + (np.arange(int(size.sum())) - np.repeat(np.cumsum(size) - size, size))
            out[i, v] = entry_stats(ranks[idx], cuts)
    return out


def draws_matrix(seed, b0, n_boot, U):
    """u(b, t) for b in [b0, b0 + n_boot), t in [0, U): int64 [n_boot, U], all resamples at once."""
    c = (np.arange(b0, b0 + n_boot, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(U, dtype=np.uint64)[None, :]
    return (((sm64(seed, c) >> np.uint64(32)) * np.uint64(U)) >> np.uint64(32)).astype(np.int64)


def single_entry_stats(ranks, cuts=DEFAULT_CUTS, seed=0, b0=0, n_boot=1000):
    """rank_stats [n_boot, 4 + K] (V = 1) for units of exactly one entry each, vectorised over the resamples."""
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    U = len(ranks)
    r = np.sort(ranks[draws_matrix(seed, b0, n_boot, U)], axis=1)
    cols = [np.full(n_boot, U), r.sum(1), r[:, (U - 1) // 2], r[:, U // 2]] + [(r < c).sum(1) for c in cuts]
    return np.stack(cols, axis=1).astype(np.int64)
