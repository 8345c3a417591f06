"""NumPy restatement of local scaling (DESIGN.md "Local scaling": CSLS, NICDM, LS).  The reference has no code for it, so this
file stands in for it: the lists of hubness_ref.topk_lists, a float32 sum taken in a plain loop, and the three formulas written
out once in float32 (every operation rounded once, as the kernel computes them) and once in fp64.

S [rows = texts / sentences, cols = videos] is on the cosine scale, d = 1 - s the distance.  A text's neighbourhood is its
top-k videos (a row list), a video's its top-k texts (a column list); with a querybank the row lists come from Qv = sim(test
texts, bank videos) and the column lists from Qt = sim(bank texts, test videos)."""
import numpy as np

import hubness_ref as H

EPS = np.float32(2.0 ** -20)
MODES = ("csls", "nicdm", "ls")
F = np.float32


def line_stats(idx, val):
    """(mean, kth) float32 [n] of the lists idx / val [n, k]: the present entries (idx >= 0) summed one by one in list order
    starting from the first, divided by their count; the last present value.  No present entry: NaN."""
    idx, val = np.asarray(idx), np.asarray(val, dtype=F)
    n = idx.shape[0]
    mean, kth = np.full(n, np.nan, dtype=F), np.full(n, np.nan, dtype=F)
    with np.errstate(all="ignore"):
        for i in range(n):
            present = val[i][idx[i] >= 0]
            if len(present) == 0:
                continue
            total = F(present[0])
            for x in present[1:]:
                total = F(total + F(x))
            mean[i] = F(total / F(len(present)))
            kth[i] = present[-1]
    return mean, kth


def neighbourhood_stats(S, k, Qt=None, Qv=None):
    """((mean_row, kth_row) [n_rows], (mean_col, kth_col) [n_cols]) float32.  Without a querybank both come from S."""
    S = np.asarray(S, dtype=F)
    Qv = S if Qv is None else np.asarray(Qv, dtype=F)
    Qt = S if Qt is None else np.asarray(Qt, dtype=F)
    return line_stats(*H.topk_lists(Qv, k)), line_stats(*H.topk_lists(Qt.T, k))


def _nanmax(x, lo):
    return np.maximum(x, lo)                                 # np.maximum keeps a NaN


def scores(S, mode, row_stat, col_stat, dtype=np.float32):
    """T of `mode` from S and the statistics its formula takes (means for csls / nicdm, k-th values for ls).  dtype float32:
    every operation rounded to float32 once, the kernel's arithmetic; float64: the formulas in fp64 on the same float32 inputs."""
    t = np.dtype(dtype).type
    s = np.asarray(S, dtype=F).astype(dtype)
    r = np.asarray(row_stat, dtype=F).astype(dtype)[:, None]
    c = np.asarray(col_stat, dtype=F).astype(dtype)[None, :]
    with np.errstate(all="ignore"):
        if mode == "csls":
            return ((t(2) * s - r).astype(dtype) - c).astype(dtype)
        d = _nanmax((t(1) - s).astype(dtype), t(0))
        a = _nanmax((t(1) - r).astype(dtype), t(EPS))
        b = _nanmax((t(1) - c).astype(dtype), t(EPS))
        ab = (a * b).astype(dtype)
        if mode == "nicdm":
            return -(d / np.sqrt(ab).astype(dtype)).astype(dtype)
        if mode == "ls":
            return -((d * d).astype(dtype) / ab).astype(dtype)
    raise ValueError(mode)


def pick(mode, stats):
    """The statistic `mode` takes out of (mean, kth)."""
    return stats[1] if mode == "ls" else stats[0]


def local_scale(S, mode, k, Qt=None, Qv=None, dtype=np.float32):
    """T of the whole matrix S."""
    rows, cols = neighbourhood_stats(S, k, Qt, Qv)
    return scores(S, mode, pick(mode, rows), pick(mode, cols), dtype)
