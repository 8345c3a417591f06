"""CPU: the NumPy restatement of local scaling (localscale_ref) on a hand-worked case per mode, the host-side refusals of the
nr_localscale_* entry points, the evaluator's argument checks and the command-line flags."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import hubness_ref as H
import localscale_ref as LS
from neighborretr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
nan, inf = np.nan, np.inf


def _bits(a, b):
    """NaN in the same places (its sign and payload are not part of the definition), the same bits everywhere else."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- a hand-worked case --------------------------------------------------------------------------------------------------------
# k = 2.  Row 2 and column 2 have one entry only (fewer than k), row 1 holds a +inf, (0, 2) is a NaN inside a populated row.
S = np.array([[0.5, 0.25, nan, 0.0],
              [0.75, inf, 0.5, -0.25],
              [nan, 0.5, nan, nan]], dtype=F)
K = 2
#            lists (values)            mean      kth
# row 0      0.5, 0.25                 0.375     0.25
# row 1      inf, 0.75                 inf       0.75
# row 2      0.5                       0.5       0.5
# col 0      0.75, 0.5                 0.625     0.5
# col 1      inf, 0.5                  inf       0.5
# col 2      0.5                       0.5       0.5
# col 3      0.0, -0.25                -0.125    -0.25
ROW_MEAN, ROW_KTH = [0.375, inf, 0.5], [0.25, 0.75, 0.5]
COL_MEAN, COL_KTH = [0.625, inf, 0.5, -0.125], [0.5, 0.5, 0.5, -0.25]


def test_hand_worked_statistics():
    (rm, rk), (cm, ck) = LS.neighbourhood_stats(S, K)
    assert _bits(rm, ROW_MEAN) and _bits(rk, ROW_KTH)
    assert _bits(cm, COL_MEAN) and _bits(ck, COL_KTH)
    # the lists behind them: score descending, NaN never selected, padded with -1 / -inf
    idx, val = H.topk_lists(S, K)
    assert idx.tolist() == [[0, 1], [1, 0], [1, -1]] and val[2].tolist() == [0.5, -inf]
    # a list with no entry at all: both statistics NaN; an absent slot's value is never read
    m, k = LS.line_stats(np.array([[-1, -1], [3, -1]]), np.array([[-inf, -inf], [0.25, 7.0]], dtype=F))
    assert np.isnan(m[0]) and np.isnan(k[0]) and m[1] == 0.25 and k[1] == 0.25
    # the sum is taken one by one in list order, in float32
    vals = np.array([[1.0, 2.0 ** -24, 2.0 ** -24]], dtype=F)
    m, k = LS.line_stats(np.array([[0, 1, 2]]), vals)
    assert m[0] == F(F(1.0) / F(3.0)) and k[0] == F(2.0 ** -24)       # (1 + 2^-24) + 2^-24 rounds to 1 twice


def test_hand_worked_csls():
    # T = (2 s - mean_row) - mean_col
    want = [[0.0, -inf, nan, -0.25],               # 1 - .375 - .625;  .5 - .375 - inf;  NaN;  0 - .375 + .125
            [-inf, nan, -inf, -inf],               # the row's mean is +inf: -inf, but inf - inf = NaN where s = +inf
            [nan, -inf, nan, nan]]                 # 1 - .5 - inf
    assert _bits(LS.local_scale(S, "csls", K), want)
    assert _bits(LS.local_scale(S, "csls", K, dtype=np.float64).astype(F), want)


def test_hand_worked_nicdm():
    # d = max(1 - s, 0);  a = max(1 - mean_row, EPS) = .625, EPS, .5;  b = max(1 - mean_col, EPS) = .375, EPS, .5, 1.125
    e = LS.EPS
    assert e == F(2.0 ** -20)

    def q(d, a, b):
        return -F(F(d) / F(np.sqrt(F(F(a) * F(b)))))
    want = [[q(.5, .625, .375), q(.75, .625, e), nan, q(1.0, .625, 1.125)],
            [q(.25, e, .375), -0.0, q(.5, e, .5), q(1.25, e, 1.125)],           # s = +inf: d = max(-inf, 0) = 0
            [nan, q(.5, .5, e), nan, nan]]
    got = LS.local_scale(S, "nicdm", K)
    assert _bits(got, want)
    assert got[0, 1] == -F(0.75) / F(np.sqrt(F(0.625 * 2.0 ** -20))) and np.signbit(got[1, 1]) and got[1, 1] == 0
    np.testing.assert_allclose(LS.local_scale(S, "nicdm", K, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=3e-7)


def test_hand_worked_ls():
    # a = max(1 - kth_row, EPS) = .75, .25, .5;  b = max(1 - kth_col, EPS) = .5, .5, .5, 1.25;  T = -d^2 / (a b)
    want = [[-F(F(.25) / F(.375)), -1.5, nan, -F(F(1.0) / F(.9375))],
            [-0.5, -0.0, -2.0, -5.0],              # .0625 / .125;  0 / .125;  .25 / .125;  1.5625 / .3125
            [nan, -1.0, nan, nan]]                 # .25 / .25
    assert _bits(LS.local_scale(S, "ls", K), want)
    np.testing.assert_allclose(LS.local_scale(S, "ls", K, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=1e-7)


def test_a_nan_statistic_makes_its_line_nan_and_the_floor_is_eps():
    M = np.array([[0.5, nan, 1.0], [0.25, nan, 1.0]], dtype=F)       # column 1 has no entry: its statistics are NaN
    for mode in LS.MODES:
        T = LS.local_scale(M, mode, 1)
        assert np.isnan(T[:, 1]).all() and np.isfinite(T[:, [0, 2]]).all(), mode
    # row 0's nearest neighbour is at distance 0: a = EPS, not 0;  column 0: kth = .5 -> b = .5;  d = .5
    a = F(2.0 ** -20)
    assert LS.local_scale(M, "ls", 1)[0, 0] == -F(F(0.25) / F(a * F(0.5)))


def test_querybank_neighbourhoods_come_from_the_bank():
    rng = np.random.default_rng(3)
    M = rng.uniform(-1, 1, (6, 6)).astype(F)
    Qt = rng.uniform(-1, 1, (4, 6)).astype(F)              # bank texts x test videos: the videos' neighbourhoods
    Qv = rng.uniform(-1, 1, (6, 5)).astype(F)              # test texts x bank videos: the texts' neighbourhoods
    (rm, _), (cm, _) = LS.neighbourhood_stats(M, 3, Qt, Qv)
    assert _bits(rm, LS.line_stats(*H.topk_lists(Qv, 3))[0]) and _bits(cm, LS.line_stats(*H.topk_lists(Qt.T, 3))[0])
    assert _bits(LS.local_scale(M, "csls", 3, Qt, Qv), (F(2) * M - rm[:, None]) - cm[None, :])


# ---- entry points ----------------------------------------------------------------------------------------------------------------
NAMES = ("nr_localscale_stats", "nr_localscale_apply")


def test_localscale_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header and name in hip.exported_symbols()
        assert hasattr(hip.lib(), name)
    comment = header[header.index("/* Local scaling"):header.index("int nr_localscale_stats(")]
    for word in ("csls", "nicdm", "ls:", "EPS = 2^-20", "NR_EINVAL"):
        assert word in comment, word
    assert hip.ABI_VERSION == 5 and hip.version() == 5
    assert (hip.LOCALSCALE_CSLS, hip.LOCALSCALE_NICDM, hip.LOCALSCALE_LS) == (0, 1, 2)


def test_localscale_entry_points_refuse_bad_arguments_before_any_launch():
    lib = hip.lib()                                            # host-side checks: no device needed
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    # null pointers, one argument at a time
    for at in (0, 1, 4, 5):
        a = [p, p, 4, 8, p, p, None]
        a[at] = None
        assert lib.nr_localscale_stats(*a) == EINVAL
    for at in (0, 4, 5, 6):
        a = [p, 4, 8, 0, p, p, p, None]
        a[at] = None
        assert lib.nr_localscale_apply(*a) == EINVAL
    # negative extents, k outside [1, 128], unknown modes
    assert lib.nr_localscale_stats(p, p, -1, 8, p, p, None) == EINVAL
    for k in (0, -1, 129):
        assert lib.nr_localscale_stats(p, p, 4, k, p, p, None) == EINVAL
    for n, L in ((-1, 8), (4, -8)):
        assert lib.nr_localscale_apply(p, n, L, 0, p, p, p, None) == EINVAL
    for mode in (-1, 3, 7):
        assert lib.nr_localscale_apply(p, 4, 8, mode, p, p, p, None) == EINVAL
        assert lib.nr_localscale_apply(p, 0, 8, mode, p, p, p, None) == EINVAL
    # nothing to do: NR_OK without a launch
    assert lib.nr_localscale_stats(p, p, 0, 8, p, p, None) == 0
    for mode in (0, 1, 2):
        assert lib.nr_localscale_apply(p, 0, 8, mode, p, p, p, None) == 0
        assert lib.nr_localscale_apply(p, 4, 0, mode, p, p, p, None) == 0
    # the one-shot apply of the softmax family still takes IS and DSL only
    assert lib.nr_hubnorm_apply(p, 4, 8, 20.0, 2, p, None, p, p, None, p, None) == EINVAL


# ---- the evaluator's checks --------------------------------------------------------------------------------------------------------
def test_evaluator_knows_the_modes_and_refuses_bad_arguments():
    from neighborretr_amd import evaluator, ops
    assert evaluator.LOCAL_SCALING_MODES == ("csls", "nicdm", "ls")
    assert evaluator.TEST_NORM_MODES == ("is", "dsl", "qbnorm", "sinkhorn", "qbsinkhorn")       # its own tuple: not touched
    assert not set(evaluator.LOCAL_SCALING_MODES) & set(evaluator.TEST_NORM_LABELS)
    assert evaluator.local_scaling_label("csls", 10, False) == "[CSLS k=10]"
    assert evaluator.local_scaling_label("nicdm", 10, True) == "[QB-NICDM k=10]"
    assert evaluator.local_scaling_label("ls", 3, False) == "[LS k=3]"
    assert set(ops.LOCALSCALE_MODES) == set(evaluator.LOCAL_SCALING_MODES)
    for mode in evaluator.LOCAL_SCALING_MODES:
        assert evaluator._check_local_scaling(mode, 10, 5) == (10, 5)
        assert evaluator._check_local_scaling(mode, 128) == (128, 0)
    for bad_mode in ("is", "mp", "", None):
        with pytest.raises(ValueError):
            evaluator._check_local_scaling(bad_mode, 10)
    for bad_k in (0, 129, True, -1, 2.5):
        with pytest.raises(ValueError):
            evaluator._check_local_scaling("csls", bad_k)
    with pytest.raises(ValueError):
        evaluator._check_local_scaling("csls", 10, 129)
    e, em = torch.empty((0, 0, 0)), torch.empty((0, 0))
    model = type("M", (), dict(mb_feat_t=e, mb_feat_v=e, mb_mask_t=em, mb_mask_v=em))()
    z = torch.zeros((4, 2, 8))
    for fn in (evaluator.sharded_local_scaled_slab, evaluator.sharded_local_scaled_metrics,
               evaluator.sharded_metrics_with_local_scaling):
        with pytest.raises(ValueError, match="load_memory_bank"):  # an empty bank fails before any scoring
            fn(model, z, z, z[..., 0], z[..., 0], None, "csls", bank=True)


def test_training_eval_epoch_refuses_local_scaling_with_test_norm_before_any_work():
    from types import SimpleNamespace
    from neighborretr_amd import training
    args = SimpleNamespace(local_scaling="csls", test_norm="is")
    with pytest.raises(ValueError, match="local_scaling"):
        training.eval_epoch(args, None, None, "cpu")           # no model, no loader: nothing may be touched


# ---- the command line --------------------------------------------------------------------------------------------------------------
def _parse(argv, monkeypatch):
    sys.path.insert(0, ROOT)
    import main_retrieval
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
    return main_retrieval.get_args()


def test_main_retrieval_accepts_the_local_scaling_flags(monkeypatch):
    a = _parse([], monkeypatch)
    assert (a.local_scaling, a.local_scaling_k, a.local_scaling_bank) == ("none", 10, 0)
    for mode in ("csls", "nicdm", "ls"):
        a = _parse(["--local_scaling", mode, "--local_scaling_k", "7", "--local_scaling_bank", "1"], monkeypatch)
        assert (a.local_scaling, a.local_scaling_k, a.local_scaling_bank) == (mode, 7, 1)
        assert a.test_norm == "none"


def test_main_retrieval_refuses_local_scaling_with_test_norm_and_as_a_test_norm_mode(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(["--local_scaling", "csls", "--test_norm", "is"], monkeypatch)
    with pytest.raises(SystemExit):
        _parse(["--test_norm", "csls"], monkeypatch)
    with pytest.raises(SystemExit):
        _parse(["--local_scaling", "mp"], monkeypatch)
    for bad in ("0", "129"):
        with pytest.raises(SystemExit):
            _parse(["--local_scaling", "csls", "--local_scaling_k", bad], monkeypatch)
    with pytest.raises(SystemExit):
        _parse(["--local_scaling", "csls", "--local_scaling_bank", "2"], monkeypatch)
