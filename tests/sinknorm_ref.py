"""NumPy restatement of the test-time Sinkhorn normalisation (DESIGN.md "Test-time Sinkhorn normalisation"): the reference's
log-domain Sinkhorn (until_module.py:223-266, restated in oracle/nr_oracle.py sinkhorn_targets) applied to a test similarity.
Written out plainly from the definition.  fp64 by default; dtype=np.float32 follows the definition's roundings (every
intermediate a float32: the sums inside the LSE in NumPy's own order).

S [rows = texts / sentences, columns = videos].  a = fl(beta S) in float32 in both modes.  u = v = 0; n_iter times
u[i] = log_mu[i] - LSE_j(a[i,j] + v[j]), then v[j] = log_nu[j] - LSE_i(a[i,j] + u[i]); T = (a + u[:, None]) + v[None, :].
NaN entries carry no mass and stay NaN; a line whose LSE is not finite keeps potential 0."""
import numpy as np

import hubness_ref as H
import hubnorm_ref as R

# rank / recall / group helpers and hubness: the ones of the one-shot corrections
single_ranks, group_ranks, group_max, recall, is_scores = R.single_ranks, R.group_ranks, R.group_max, R.recall, R.is_scores
hubness = H.hubness


def beta_s(S, beta, dtype=np.float64):
    """a = fl(beta * s) in float32, carried in `dtype`."""
    return (np.float32(beta) * np.asarray(S, dtype=np.float32)).astype(dtype)


def lse(X, axis):
    """Log-sum-exp of X along `axis` over its non-NaN entries, in X's dtype: max + log(sum exp(x - max)), an entry equal to the
    max adding exactly 1; -inf when no entry is left."""
    X = np.asarray(X)
    dt = X.dtype.type
    ok = ~np.isnan(X)
    m = np.max(np.where(ok, X, dt(-np.inf)), axis=axis, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(X == m, dt(0), X - m)
        s = np.sum(np.where(ok, np.exp(d), dt(0)), axis=axis, dtype=X.dtype)
    m = np.squeeze(m, axis=axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, m + np.log(np.where(s > 0, s, dt(1))), dt(-np.inf)).astype(X.dtype)


def marginals(n_rows, n_cols, cut_off_points=None, dtype=np.float64):
    """(log_mu [n_rows], log_nu [n_cols]).  Every row -log n_rows.  Columns: -log n_cols, or with cut_off_points (index of the
    LAST sentence of every video) log(g_j / n_rows), g_j = the number of sentences of video j."""
    log_mu = np.full(n_rows, -np.log(float(n_rows)))
    if cut_off_points is None:
        log_nu = np.full(n_cols, -np.log(float(n_cols)))
    else:
        ends = np.asarray(cut_off_points, dtype=np.int64) + 1
        g = np.diff(np.concatenate(([0], ends))).astype(np.float64)
        assert len(g) == n_cols and ends[-1] == n_rows and (g > 0).all()
        log_nu = np.log(g / float(n_rows))
    return log_mu.astype(np.float32).astype(dtype), log_nu.astype(np.float32).astype(dtype)    # the fp32 vectors the kernels get


def _half(A, shift, log_m, axis):
    """One half-step: log_m - LSE along `axis` of A + shift, 0 where the LSE is not finite."""
    with np.errstate(invalid="ignore"):
        l = lse(A + (shift[None, :] if axis == 1 else shift[:, None]), axis)
        fin = np.isfinite(l)
        return np.where(fin, log_m - np.where(fin, l, 0), 0).astype(A.dtype)


def potentials(S, beta, n_iter, log_mu=None, log_nu=None, dtype=np.float64, history=False):
    """(u [n], v [L]) after n_iter iterations; history: the list of (u, v) after every iteration instead.  log_mu / log_nu:
    the log marginals, used as given (default: marginals(n, L), the uniform ones as the fp32 vectors the kernels get)."""
    A = beta_s(S, beta, dtype)
    n, L = A.shape
    mu, nu = marginals(n, L, None, dtype)
    log_mu = mu if log_mu is None else np.asarray(log_mu).astype(dtype)
    log_nu = nu if log_nu is None else np.asarray(log_nu).astype(dtype)
    u, v = np.zeros(n, dtype), np.zeros(L, dtype)
    steps = []
    for _ in range(int(n_iter)):
        u = _half(A, v, log_mu, 1)
        v = _half(A, u, log_nu, 0)
        steps.append((u, v))
    return steps if history else (u, v)


def plan(S, beta, u, v, dtype=np.float64):
    """T = (a + u[:, None]) + v[None, :] in `dtype`, the two additions in this order."""
    A = beta_s(S, beta, dtype)
    with np.errstate(invalid="ignore"):
        return ((A + np.asarray(u, dtype)[:, None]).astype(dtype) + np.asarray(v, dtype)[None, :]).astype(dtype)


def row_masses(T, log_mu):
    """exp(LSE_j T[i, j] - log_mu[i]) of every row (1 = balanced), NaN for a row that takes no part."""
    l = lse(np.asarray(T), 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isfinite(l), np.exp(l - log_mu), np.nan)


def col_masses(T, log_nu):
    l = lse(np.asarray(T), 0)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isfinite(l), np.exp(l - log_nu), np.nan)


def marginal_err(T, log_mu):
    """max_i |exp(LSE_j T[i, j] - log_mu[i]) - 1| over the rows that take part; 0 when none does."""
    m = row_masses(T, log_mu)
    m = m[~np.isnan(m)]
    return float(np.max(np.abs(m - 1))) if m.size else 0.0


def sinkhorn(S, beta, n_iter, cut_off_points=None, dtype=np.float64):
    """(T, u, v, marginal_err) of the whole matrix S with the marginals of the definition."""
    S = np.asarray(S, dtype=np.float32)
    log_mu, log_nu = marginals(S.shape[0], S.shape[1], cut_off_points, dtype)
    u, v = potentials(S, beta, n_iter, log_mu, log_nu, dtype)
    T = plan(S, beta, u, v, dtype)
    return T, u, v, marginal_err(T, log_mu)


def qbsinkhorn(S, Qt, Qv, beta, n_iter, dtype=np.float64, v_t=None, u_v=None):
    """(T, V, v_t, u_v): the querybank form.  Qt = sim(bank texts, test videos) [M, L], Qv = sim(test texts, bank videos)
    [n, M]; v_t = the column potentials of Qt, u_v = the row potentials of Qv (uniform marginals); T = fl(beta S) + v_t[None, :],
    V = fl(beta S) + u_v[:, None] -- hubnorm_ref.is_scores with the normalisers -v_t / -u_v (float32, bit for bit).  v_t / u_v
    override the potentials (e.g. with the GPU's own)."""
    if v_t is None:
        v_t = potentials(Qt, beta, n_iter, dtype=dtype)[1]
    if u_v is None:
        u_v = potentials(Qv, beta, n_iter, dtype=dtype)[0]
    T = R.is_scores(S, beta, -np.asarray(v_t, dtype=np.float32), 0)
    V = R.is_scores(S, beta, -np.asarray(u_v, dtype=np.float32), 1)
    return T, V, v_t, u_v
