"""CPU: the NumPy restatement of the test-time Sinkhorn normalisation (sinknorm_ref) against the oracle's log-Sinkhorn, its
marginals, its non-finite cases, the querybank form, a planted hub, the host-side refusals of the nr_sinknorm_* entry points
and the command-line flags."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import hubness_ref as H
import hubnorm_ref as R
import sinknorm_ref as K
from neighborretr_amd import hip
from oracle.nr_oracle import sinkhorn_targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA = 20.0


def _bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


# ---- the reference's Sinkhorn -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n_iter", [1, 5, 50])
def test_restatement_equals_the_oracles_log_sinkhorn(seed, n_iter):
    N = 24 + 7 * seed
    G = np.random.default_rng(seed).standard_normal((N, N)).astype(np.float32) * 2
    both = np.full(N, -np.log(2.0 * N))                     # the reference's `norm` (until_module.py:241), on both sides
    u, v = K.potentials(G, 1.0, n_iter, both, both)
    T = K.plan(G, 1.0, u, v)
    Q = sinkhorn_targets(torch.from_numpy(G).double(), 1.0, n_iter).numpy()      # beta = 1: the plan itself
    assert np.abs(T + np.log(2.0 * N) - np.log(Q)).max() <= 1e-12
    one = np.full(N, -np.log(float(N)))                     # this project's marginals: a constant away
    d = K.plan(G, 1.0, *K.potentials(G, 1.0, n_iter, one, one)) - T
    assert d.max() - d.min() <= 1e-12


# ---- marginals ----------------------------------------------------------------------------------------------------------------
def _hub_matrix(n, L, seed, hub=3, own=None):
    rng = np.random.default_rng(seed)
    S = (rng.standard_normal((n, L)) * 0.1).astype(np.float32)
    own = np.arange(n) % L if own is None else own
    S[np.arange(n), own] += 0.35
    S[:, hub] += 0.25
    return S


def _cut(sizes):
    return (np.cumsum(sizes) - 1).tolist()


SIZES = [5, 1, 9, 2, 7, 3, 4, 8, 6, 1, 2, 5, 7, 3, 9, 4, 6, 8, 2, 4]      # 96 sentences over 20 videos


@pytest.mark.parametrize("shape,cut", [((60, 60), None), ((96, 20), _cut(SIZES)), ((45, 80), None)])
def test_columns_are_exact_after_every_iteration_and_the_rows_converge(shape, cut):
    n, L = shape
    S = _hub_matrix(n, L, 11)
    log_mu, log_nu = K.marginals(n, L, cut)
    if cut is not None:
        g = np.asarray(SIZES, dtype=np.float64)
        assert np.allclose(np.exp(log_nu), g / n, rtol=1e-7) and abs(np.exp(log_nu).sum() - 1) < 1e-6
    errs = []
    for u, v in K.potentials(S, BETA, 30, log_mu, log_nu, history=True):
        T = K.plan(S, BETA, u, v)
        assert np.abs(K.col_masses(T, log_nu) - 1).max() <= 1e-12
        errs.append(K.marginal_err(T, log_mu))
    assert errs[4] < errs[0] and errs[29] < errs[4], errs    # falling with n_iter
    assert K.sinkhorn(S, BETA, 30, cut)[3] == errs[29]


def test_non_finite_entries_follow_the_definition():
    S = _hub_matrix(12, 9, 5)
    S[0, :] = np.nan                                        # a row with no entry
    S[:, 4] = np.nan                                        # a column with no entry
    S[2, 1] = np.nan
    S[3, :] = -np.inf                                       # a row with no mass
    S[5, 2] = -np.inf
    for dtype in (np.float64, np.float32):
        T, u, v, err = K.sinkhorn(S, BETA, 20, dtype=dtype)
        assert T.dtype == dtype and u.dtype == dtype
        assert u[0] == 0 and u[3] == 0 and v[4] == 0        # lines without a finite LSE keep potential 0
        assert np.array_equal(np.isnan(T), np.isnan(S))     # NaN stays NaN, nothing else becomes NaN
        assert np.all(T[3, ~np.isnan(S[3])] == -np.inf) and T[5, 2] == -np.inf
        log_mu, log_nu = K.marginals(12, 9, None, dtype)
        cols = K.col_masses(T, log_nu)
        assert np.isnan(cols[4]) and np.abs(np.delete(cols, 4) - 1).max() <= (1e-12 if dtype == np.float64 else 2e-5)
        rows = K.row_masses(T, log_mu)
        assert np.isnan(rows[0]) and np.isnan(rows[3]) and np.isfinite(np.delete(rows, [0, 3])).all()
        assert err == np.abs(np.delete(rows, [0, 3]) - 1).max()
        # the NaN entry carries no mass: the same potentials as with that entry at -inf
        S2 = S.copy()
        S2[2, 1] = -np.inf
        _, u2, v2, _ = K.sinkhorn(S2, BETA, 20, dtype=dtype)
        assert np.array_equal(u, u2) and np.array_equal(v, v2)
    # nothing at all
    T, u, v, err = K.sinkhorn(np.full((3, 4), np.nan, np.float32), BETA, 3)
    assert not u.any() and not v.any() and err == 0.0 and np.isnan(T).all()


def test_float32_mode_stays_close_to_fp64_with_the_same_ranks():
    S = _hub_matrix(200, 200, 3)
    T64, u64, v64, _ = K.sinkhorn(S, BETA, 50)
    T32, u32, v32, _ = K.sinkhorn(S, BETA, 50, dtype=np.float32)
    assert T32.dtype == np.float32
    assert np.abs(T32 - T64).max() < 1e-4                   # values up to about 25: a few units in the last place
    assert np.array_equal(K.single_ranks(T32), K.single_ranks(T64))


# ---- the querybank form ---------------------------------------------------------------------------------------------------------
def test_qbsinkhorn_is_the_is_apply_with_the_banks_potentials():
    S = _hub_matrix(30, 30, 8)
    Qt = _hub_matrix(17, 30, 9)                             # bank texts x test videos: they share the hub
    Qv = _hub_matrix(30, 13, 10, hub=1)                     # test texts x bank videos
    for dtype in (np.float32, np.float64):
        T, V, v_t, u_v = K.qbsinkhorn(S, Qt, Qv, BETA, 10, dtype=dtype)
        assert np.array_equal(v_t, K.potentials(Qt, BETA, 10, dtype=dtype)[1])
        assert np.array_equal(u_v, K.potentials(Qv, BETA, 10, dtype=dtype)[0])
        assert T.dtype == np.float32 and V.dtype == np.float32
        assert _bits(T, R.is_scores(S, BETA, -v_t.astype(np.float32), 0))
        assert _bits(V, R.is_scores(S, BETA, -u_v.astype(np.float32), 1))
    v32 = K.potentials(Qt, BETA, 10, dtype=np.float32)[1]
    want = (np.float32(BETA) * S + v32[None, :]).astype(np.float32)          # fl(fl(beta s) + v_t[j]), the definition's form
    assert _bits(K.qbsinkhorn(S, Qt, Qv, BETA, 10, dtype=np.float32)[0], want)


def test_qbsinkhorn_with_the_test_set_as_its_own_bank_ranks_the_rows_like_sinkhorn():
    S = _hub_matrix(40, 40, 21)
    T, _, _, _ = K.sinkhorn(S, BETA, 25)
    Tq, _, v_t, _ = K.qbsinkhorn(S, S, S, BETA, 25)
    # a row of sinkhorn's T is the row of the querybank form shifted by its own u[i]: the same order, row by row
    assert np.array_equal(np.argsort(-T, axis=1, kind="stable"), np.argsort(-Tq.astype(np.float64), axis=1, kind="stable"))
    assert np.array_equal(K.single_ranks(T), K.single_ranks(Tq))


# ---- what it is for -------------------------------------------------------------------------------------------------------------
def test_a_planted_hub_loses_its_surplus_top1_hits_square():
    hub = 3
    S = _hub_matrix(300, 300, 4, hub=hub)
    raw_hits = int(np.sum(S.argmax(1) == hub))
    assert raw_hits > 30
    T, _, _, err = K.sinkhorn(S, BETA, 50)
    assert int(np.sum(T.argmax(1) == hub)) < raw_hits
    assert int(np.sum(T.argmax(1) == hub)) <= 3
    raw_h, bal_h = H.hubness(S, 10)[0]["summary"], H.hubness(T.astype(np.float32), 10)[0]["summary"]
    assert bal_h["skewness"] < raw_h["skewness"]
    assert K.recall(K.single_ranks(T), 1) >= K.recall(K.single_ranks(S), 1)
    assert K.recall(K.single_ranks(T.T), 1) >= K.recall(K.single_ranks(S.T), 1)


def test_a_planted_hub_video_keeps_no_more_top1_sentences_than_it_owns_rectangular():
    hub = 0                                                 # owns SIZES[0] = 5 of the 96 sentences
    cut = _cut(SIZES)
    group = np.searchsorted(np.asarray(cut) + 1, np.arange(96), side="right")
    S = _hub_matrix(96, 20, 6, hub=hub, own=group)
    assert int(np.sum(S.argmax(1) == hub)) > 2 * SIZES[hub]
    T, _, _, _ = K.sinkhorn(S, BETA, 50, cut)
    assert int(np.sum(T.argmax(1) == hub)) <= SIZES[hub]
    # the group helpers take T as they take the one-shot corrections' outputs
    assert len(K.group_ranks(T, cut)) == 96 and K.group_max(T, cut).shape == (20, 20)


# ---- entry points -----------------------------------------------------------------------------------------------------------------
NAMES = ("nr_sinknorm_row", "nr_sinknorm_col_stats", "nr_sinknorm_finish_cols", "nr_sinknorm_apply", "nr_sinknorm_row_err")


def test_sinknorm_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header and name in hip.exported_symbols()
        assert hasattr(hip.lib(), name)
    assert "until_module.py:223-266" in header[header.index("Test-time Sinkhorn"):header.index("int nr_sinknorm_row(")]
    assert hip.ABI_VERSION == 5 and hip.version() == 5


def test_sinknorm_entry_points_refuse_bad_arguments_before_any_launch():
    lib = hip.lib()                                            # host-side checks: no device needed
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    for beta in (0.0, -1.0, float("inf"), float("nan"), -float("inf")):
        assert lib.nr_sinknorm_row(p, 4, 8, beta, p, p, p, None) == EINVAL
        assert lib.nr_sinknorm_col_stats(p, 4, 8, beta, p, p, p, None) == EINVAL
        assert lib.nr_sinknorm_apply(p, 4, 8, beta, p, p, p, None) == EINVAL
        assert lib.nr_sinknorm_row_err(p, 4, 8, beta, p, p, p, p, None) == EINVAL
    # null pointers, one argument at a time
    for k in (0, 4, 5, 6):
        a = [p, 4, 8, 20.0, p, p, p, None]
        a[k] = None
        assert lib.nr_sinknorm_row(*a) == EINVAL
        assert lib.nr_sinknorm_apply(*a) == EINVAL
    for k in (0, 4, 5):                                        # stats (6) may be null: the pairs stay in the workspace
        a = [p, 4, 8, 20.0, p, p, p, None]
        a[k] = None
        assert lib.nr_sinknorm_col_stats(*a) == EINVAL
    assert lib.nr_sinknorm_col_stats(None, 0, 8, 20.0, None, None, None, None) == EINVAL       # n = 0 and nothing to write
    for k in (0, 4, 5, 6, 7):
        a = [p, 4, 8, 20.0, p, p, p, p, None]
        a[k] = None
        assert lib.nr_sinknorm_row_err(*a) == EINVAL
    assert lib.nr_sinknorm_finish_cols(2, None, 8, p, p, None) == EINVAL
    assert lib.nr_sinknorm_finish_cols(2, p, 8, None, p, None) == EINVAL
    assert lib.nr_sinknorm_finish_cols(2, p, 8, p, None, None) == EINVAL
    # negative extents
    for n, L in ((-1, 8), (4, -8)):
        assert lib.nr_sinknorm_row(p, n, L, 20.0, p, p, p, None) == EINVAL
        assert lib.nr_sinknorm_col_stats(p, n, L, 20.0, p, p, p, None) == EINVAL
        assert lib.nr_sinknorm_apply(p, n, L, 20.0, p, p, p, None) == EINVAL
        assert lib.nr_sinknorm_row_err(p, n, L, 20.0, p, p, p, p, None) == EINVAL
    assert lib.nr_sinknorm_finish_cols(-1, p, 8, p, p, None) == EINVAL
    assert lib.nr_sinknorm_finish_cols(2, p, -8, p, p, None) == EINVAL
    # the one-shot apply still takes IS and DSL only
    assert lib.nr_hubnorm_apply(p, 4, 8, 20.0, 2, p, None, p, p, None, p, None) == EINVAL


def test_evaluator_knows_the_modes_and_refuses_bad_iteration_counts():
    from neighborretr_amd import evaluator
    assert evaluator.TEST_NORM_MODES[-2:] == ("sinkhorn", "qbsinkhorn")
    assert evaluator.test_norm_label("sinkhorn", 20.0, 50) == "[Sinkhorn b=20 it=50]"
    assert evaluator.test_norm_label("qbsinkhorn", 12.5, 7) == "[QB-Sinkhorn b=12.5 it=7]"
    assert evaluator.test_norm_label("is", 20.0) == "[IS b=20]"
    for mode in ("sinkhorn", "qbsinkhorn"):
        assert evaluator._check_test_norm(mode, 20.0, 1, 5) == (20.0, 1, 5)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            evaluator._check_n_iter(bad)
    assert evaluator._check_n_iter(50) == 50
    e, em = torch.empty((0, 0, 0)), torch.empty((0, 0))
    model = type("M", (), dict(mb_feat_t=e, mb_feat_v=e, mb_mask_t=em, mb_mask_v=em))()
    z = torch.zeros((4, 2, 8))
    with pytest.raises(ValueError, match="load_memory_bank"):      # an empty bank fails before any scoring
        evaluator.sharded_normalised_metrics(model, z, z, z[..., 0], z[..., 0], None, "qbsinkhorn")
    # the marginals the kernels get: uniform, or the share of the sentences a video owns
    mu, nu = evaluator._log_marginals(96, 20, np.cumsum(SIZES), "cpu")
    want_mu, want_nu = K.marginals(96, 20, _cut(SIZES), np.float32)
    assert _bits(mu.numpy(), want_mu) and _bits(nu.numpy(), want_nu)
    mu, nu = evaluator._log_marginals(7, 7, None, "cpu")
    assert _bits(mu.numpy(), K.marginals(7, 7, None, np.float32)[0]) and _bits(nu.numpy(), mu.numpy())


def _parse(argv, monkeypatch):
    sys.path.insert(0, ROOT)
    import main_retrieval
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
    return main_retrieval.get_args()


def test_main_retrieval_accepts_the_sinkhorn_flags(monkeypatch):
    a = _parse([], monkeypatch)
    assert a.test_norm == "none" and a.test_norm_iters == 50
    a = _parse(["--test_norm", "sinkhorn", "--test_norm_iters", "7"], monkeypatch)
    assert a.test_norm == "sinkhorn" and a.test_norm_iters == 7
    assert _parse(["--test_norm", "qbsinkhorn"], monkeypatch).test_norm == "qbsinkhorn"
    with pytest.raises(SystemExit):
        _parse(["--test_norm", "sinkhorn", "--test_norm_iters", "0"], monkeypatch)
