"""NumPy / torch-CPU restatement of mutual proximity (DESIGN.md "Mutual proximity": emp, gauss).  The reference has no code for
it, so this file stands in for it: brute-force counts, moments in fp64, and the two formulas written out once in float32 (every
operation rounded once, as the kernels compute them; float32 erfc is torch.special.erfc on CPU tensors) and once in fp64.

S [rows = texts / sentences, cols = videos].  Row i's reference line is Qv[i, :], column j's is Qt[:, j]; without a querybank
both are S itself (the score is part of both of its lines), with one Qv = sim(test texts, bank videos) and Qt = sim(bank texts,
test videos).  Both modes are the independent form MP_I = P_row P_col."""
import numpy as np
import torch

EPS = np.float32(2.0 ** -20)
MODES = ("emp", "gauss")
F = np.float32


def _sources(S, Qt, Qv):
    S = np.asarray(S, dtype=F)
    Qv = S if Qv is None else np.asarray(Qv, dtype=F)
    Qt = S if Qt is None else np.asarray(Qt, dtype=F)
    assert Qv.shape[0] == S.shape[0] and Qt.shape[1] == S.shape[1]
    return S, Qt, Qv


def r2(s, X):
    """r2[a, b] = 2 #{x in X[a, :] : x < s[a, b]} + #{x in X[a, :] : x == s[a, b]}, int64; IEEE compares (a NaN is neither less
    nor equal, -0 == +0).  s [A, B], X [A, C]."""
    s, X = np.asarray(s, dtype=F), np.asarray(X, dtype=F)
    out = np.zeros(s.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for a in range(s.shape[0]):
            out[a] = 2 * (X[a][None, :] < s[a][:, None]).sum(1) + (X[a][None, :] == s[a][:, None]).sum(1)
    return out


def line_counts(X, axis):
    """The number of non-NaN entries of every line of X along `axis`, int64."""
    return (~np.isnan(np.asarray(X, dtype=F))).sum(axis).astype(np.int64)


def counts(S, Qt=None, Qv=None):
    """(r2_row [n, L], r2_col [n, L], row_cnt [n], col_cnt [L]) int64: the doubled rank of every score in its row's line and in its
    column's line, and the lines' non-NaN counts."""
    S, Qt, Qv = _sources(S, Qt, Qv)
    return r2(S, Qv), r2(S.T, Qt.T).T, line_counts(Qv, 1), line_counts(Qt, 0)


def emp_scores(S, r2_row, r2_col, row_cnt, col_cnt, dtype=np.float32):
    """T = fl(fl(r2_row / 2 row_cnt) fl(r2_col / 2 col_cnt)) in `dtype`; c = 0: 0 / 0 = NaN; a NaN score gives NaN."""
    S = np.asarray(S, dtype=F)
    with np.errstate(all="ignore"):
        p = (np.asarray(r2_row).astype(dtype) / (2 * np.asarray(row_cnt)).astype(dtype)[:, None]).astype(dtype)
        q = (np.asarray(r2_col).astype(dtype) / (2 * np.asarray(col_cnt)).astype(dtype)[None, :]).astype(dtype)
        T = (p * q).astype(dtype)
    T[np.isnan(S)] = np.nan
    return T


def emp(S, Qt=None, Qv=None, dtype=np.float32):
    """T of the whole matrix S, mode emp."""
    return emp_scores(S, *counts(S, Qt, Qv), dtype=dtype)


def moments(X, axis):
    """(mean, sd) float32 of every line of X along `axis` over its non-NaN entries: sums in fp64, the population standard
    deviation (divide by c) from the squared distances to the mean, rounded to float32 once.  c = 0: both NaN; c = 1: sd = 0; an
    infinity follows IEEE (sd NaN)."""
    X = np.asarray(X, dtype=F).astype(np.float64)
    if axis == 0:
        X = X.T
    ok = ~np.isnan(X)
    c = ok.sum(1).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = np.where(ok, X, 0.0).sum(1) / c
        d = np.where(ok, X - mean[:, None], 0.0)
        sd = np.sqrt((d * d).sum(1) / c)
    return mean.astype(F), sd.astype(F)


def _erfc(x):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def tail(s, mean, sd, dtype=np.float32):
    """Q = 0.5 erfc(z / sqrt 2), z = (s - mean) / max(sd, EPS): the probability that the line's normal exceeds s.  float32: every
    operation rounded once, z times fl(1 / sqrt 2); float64: the formula in fp64 on the same float32 inputs."""
    t = np.dtype(dtype).type
    s, mean, sd = (np.asarray(a, dtype=F).astype(dtype) for a in (s, mean, sd))
    with np.errstate(all="ignore"):
        z = ((s - mean).astype(dtype) / np.maximum(sd, t(EPS))).astype(dtype)         # np.maximum keeps a NaN
        u = (z * F(np.sqrt(0.5))).astype(dtype) if dtype == np.float32 else z / np.sqrt(2.0)
        return (t(0.5) * _erfc(u)).astype(dtype)


def gauss_scores(S, row_mean, row_sd, col_mean, col_sd, dtype=np.float32):
    """T = -((Q_r + Q_c) - Q_r Q_c) = MP_I - 1 from S and the lines' moments."""
    S = np.asarray(S, dtype=F)
    a = tail(S, np.asarray(row_mean)[:, None], np.asarray(row_sd)[:, None], dtype)
    b = tail(S, np.asarray(col_mean)[None, :], np.asarray(col_sd)[None, :], dtype)
    with np.errstate(all="ignore"):
        return -((a + b).astype(dtype) - (a * b).astype(dtype)).astype(dtype)


def line_moments(S, Qt=None, Qv=None):
    """((row_mean, row_sd) [n], (col_mean, col_sd) [L]) float32 of the reference lines."""
    S, Qt, Qv = _sources(S, Qt, Qv)
    return moments(Qv, 1), moments(Qt, 0)


def gauss(S, Qt=None, Qv=None, dtype=np.float32):
    """T of the whole matrix S, mode gauss."""
    rows, cols = line_moments(S, Qt, Qv)
    return gauss_scores(S, *rows, *cols, dtype=dtype)


def mutual_proximity(S, mode, Qt=None, Qv=None, dtype=np.float32):
    if mode == "emp":
        return emp(S, Qt, Qv, dtype)
    if mode == "gauss":
        return gauss(S, Qt, Qv, dtype)
    raise ValueError(mode)


def rel_distance(got, want):
    """The largest |got - want| / |want| over the entries with a finite, non-zero `want` (0 when there is none)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.isfinite(want) & (want != 0)
    return float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max()) if ok.any() else 0.0
