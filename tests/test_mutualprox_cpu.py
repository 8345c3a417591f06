"""CPU: the restatement of mutual proximity (mutualprox_ref) on a hand-worked case, the pinned properties of the definition, the
host-side refusals of the nr_mp_* entry points, the evaluator's argument checks and the command-line flags."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import mutualprox_ref as MP
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
# (2, 0) is a NaN inside a populated row, (1, 1) a +inf, row 0 holds a tie (0.25 twice), column 2 has no entry at all.
S = np.array([[0.5, 0.25, nan, 0.25],
              [0.75, inf, nan, -0.25],
              [nan, 0.5, nan, 0.0]], dtype=F)
# r2 = 2 #{x < s} + #{x == s} in the score's own line; a NaN score counts 0
#            line (non-NaN)        c     r2 of its scores
# row 0      .5, .25, .25          3     .5: 2*2 + 1 = 5;  .25: 0 + 2 = 2 (the tie: each half of two);  .25: 2
# row 1      .75, inf, -.25        3     .75: 2 + 1 = 3;  inf: 4 + 1 = 5;  -.25: 1
# row 2      .5, 0                 2     .5: 2 + 1 = 3;  0: 1
# col 0      .5, .75               2     .5: 1;  .75: 3
# col 1      .25, inf, .5          3     .25: 1;  inf: 5;  .5: 3
# col 2      -                     0     -
# col 3      .25, -.25, 0          3     .25: 5;  -.25: 1;  0: 3
R2_ROW = [[5, 2, 0, 2], [3, 5, 0, 1], [0, 3, 0, 1]]
R2_COL = [[1, 1, 0, 5], [3, 5, 0, 1], [0, 3, 0, 3]]
ROW_CNT, COL_CNT = [3, 3, 2], [2, 3, 0, 3]


def test_hand_worked_counts():
    r2, c2, rc, cc = MP.counts(S)
    assert r2.tolist() == R2_ROW and c2.tolist() == R2_COL
    assert rc.tolist() == ROW_CNT and cc.tolist() == COL_CNT


def test_hand_worked_emp():
    def p(a, b):
        return F(F(a) / F(b))
    # T = fl(fl(r2_row / 2 c_row) fl(r2_col / 2 c_col));  column 2: 0 / 0;  (2, 0): a NaN score
    want = [[p(5, 6) * p(1, 4), p(2, 6) * p(1, 6), nan, p(2, 6) * p(5, 6)],
            [p(3, 6) * p(3, 4), p(5, 6) * p(5, 6), nan, p(1, 6) * p(1, 6)],
            [nan, p(3, 4) * p(3, 6), nan, p(1, 4) * p(3, 6)]]
    got = MP.emp(S)
    assert got.dtype == np.float32 and _bits(got, np.asarray(want, dtype=F))
    assert got[1, 0] == F(0.375) and got[2, 3] == F(0.125)            # 1/2 * 3/4;  1/4 * 1/2
    np.testing.assert_allclose(MP.emp(S, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=2e-7)
    assert _bits(MP.mutual_proximity(S, "emp"), got)


def test_hand_worked_gauss():
    # line        mean     population sd
    # row 0       1/3      sqrt(((1/6)^2 + 2 (1/12)^2) / 3) = sqrt(1/72) = 0.11785113
    # row 1       inf      NaN (inf - inf)
    # row 2       0.25     0.25
    # col 0       0.625    0.125
    # col 1       inf      NaN
    # col 2       NaN      NaN (no entry)
    # col 3       0        sqrt(2 * 0.0625 / 3) = sqrt(1/24) = 0.20412415
    (rm, rs), (cm, cs) = MP.line_moments(S)
    assert _bits(rm, [F(1 / 3), inf, 0.25]) and _bits(rs, [F(np.sqrt(1 / 72)), nan, 0.25])
    assert _bits(cm, [0.625, inf, nan, 0.0]) and _bits(cs, [0.125, nan, nan, F(np.sqrt(1 / 24))])
    # Q(z) = 0.5 erfc(z / sqrt 2), T = -(Q_r + Q_c - Q_r Q_c); finite only where both lines are and the score is not NaN
    # (0, 0): z_r = (1/6) / sqrt(1/72) = sqrt 2, Q_r = 0.0786496035;  z_c = -1, Q_c = 0.8413447461;  T = -0.8538229189
    # (0, 3): z_r = -(1/12) / sqrt(1/72) = -0.70710678, Q_r = 0.7602499389;  z_c = .25 / sqrt(1/24) = 1.22474487,
    #         Q_c = 0.1103356980;  T = -0.7867029252
    # (2, 3): z_r = -1, Q_r = 0.8413447461;  z_c = 0, Q_c = 0.5;  T = -0.9206723730
    want = np.full((3, 4), nan)
    want[0, 0], want[0, 3], want[2, 3] = -0.8538229188874329, -0.7867029251574551, -0.9206723730342714
    got64 = MP.gauss(S, dtype=np.float64)
    assert np.array_equal(np.isnan(got64), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got64[ok], want[ok], rtol=1e-6)        # the moments are delivered as float32
    got32 = MP.gauss(S)
    assert got32.dtype == np.float32 and np.array_equal(np.isnan(got32), np.isnan(want))
    np.testing.assert_allclose(got32[ok].astype(np.float64), want[ok], rtol=2e-6)


# ---- pinned properties of the definition -------------------------------------------------------------------------------------------
def test_a_line_without_entries_is_nan_and_a_nan_score_stays_nan():
    M = np.array([[0.5, nan, 1.0], [0.25, nan, nan], [nan, nan, nan]], dtype=F)       # column 1 and row 2 have no entry
    for mode in MP.MODES:
        T = MP.mutual_proximity(M, mode)
        assert np.isnan(T[:, 1]).all() and np.isnan(T[2]).all(), mode
        assert np.isnan(T[np.isnan(M)]).all() and np.isfinite(T[0, 0]) and np.isfinite(T[0, 2]), mode
    assert MP.counts(M)[2].tolist() == [2, 1, 0] and MP.counts(M)[3].tolist() == [2, 0, 1]
    # one entry: sd = 0, floored to EPS; the score is its line's mean: z = 0, Q = 1/2
    (rm, rs), _ = MP.line_moments(M)
    assert rs[1] == 0 and rm[1] == F(0.25) and np.isnan(rm[2]) and np.isnan(rs[2])


def test_signed_zeros_are_equal():
    M = np.array([[0.0, -0.0]], dtype=F)
    r2, c2, rc, cc = MP.counts(M)
    assert r2.tolist() == [[2, 2]] and c2.tolist() == [[1, 1]] and rc.tolist() == [2] and cc.tolist() == [1, 1]
    assert _bits(MP.emp(M), [[0.25, 0.25]])                         # 2/4 * 1/2
    # infinities compare as they do: -inf below everything, +inf above
    r2 = MP.r2(np.array([[-inf, inf, 0.0]], dtype=F), np.array([[-inf, inf, 0.0, nan]], dtype=F))
    assert r2.tolist() == [[1, 5, 3]]


def test_the_gauss_floor_is_eps():
    assert MP.EPS == F(2.0 ** -20)
    # both lines constant at 0.5: sd = 0 -> EPS;  s = 0.5 + 2^-20: z = 1 in both, Q = 0.5 erfc(1 / sqrt 2) = 0.15865525
    s = np.array([[0.5 + 2.0 ** -20]], dtype=F)
    Qv, Qt = np.full((1, 3), 0.5, dtype=F), np.full((2, 1), 0.5, dtype=F)
    q = 0.15865525393145707
    np.testing.assert_allclose(MP.gauss(s, Qt, Qv, dtype=np.float64), [[-(2 * q - q * q)]], rtol=1e-12)
    np.testing.assert_allclose(MP.gauss(s, Qt, Qv).astype(np.float64), [[-(2 * q - q * q)]], rtol=1e-6)
    assert MP.tail(F(0.5), F(0.5), F(0.0)) == F(0.5)                # z = 0 / EPS = 0
    assert np.isnan(MP.tail(F(0.5), F(0.5), F(nan)))                # the max keeps a NaN sd


def test_best_matches_at_six_and_seven_sigma_stay_distinct():
    # every line has mean 0 and sd 1; the two scores sit 6 and 7 standard deviations above both of their lines
    s = np.array([[6.0, 7.0]], dtype=F)
    Qv = np.array([[1.0, -1.0]], dtype=F)
    Qt = np.array([[1.0, 1.0], [-1.0, -1.0]], dtype=F)
    T = MP.gauss(s, Qt, Qv)
    assert T.dtype == np.float32 and T[0, 0] < T[0, 1] < 0          # distinct, the better match ranks higher
    np.testing.assert_allclose(T.astype(np.float64), MP.gauss(s, Qt, Qv, dtype=np.float64), rtol=1e-5)
    # the reason for the upper-tail form: in float32 the lower tail Phi = 1 - Q is 1 for both
    Q = MP.tail(s, F(0), F(1))
    assert (Q > 0).all() and (F(1) - Q == F(1)).all()


# ---- querybank -----------------------------------------------------------------------------------------------------------------------
def test_querybank_lines_come_from_the_bank():
    rng = np.random.default_rng(3)
    M = (np.round(rng.uniform(-1, 1, (6, 6)) * 16) / 16).astype(F)
    Qt = (np.round(rng.uniform(-1, 1, (4, 6)) * 16) / 16).astype(F)   # bank texts x test videos: the videos' lines
    Qv = (np.round(rng.uniform(-1, 1, (6, 5)) * 16) / 16).astype(F)   # test texts x bank videos: the texts' lines
    r2, c2, rc, cc = MP.counts(M, Qt, Qv)
    assert rc.tolist() == [5] * 6 and cc.tolist() == [4] * 6
    for i in range(6):
        for j in range(6):
            assert r2[i, j] == 2 * (Qv[i] < M[i, j]).sum() + (Qv[i] == M[i, j]).sum()
            assert c2[i, j] == 2 * (Qt[:, j] < M[i, j]).sum() + (Qt[:, j] == M[i, j]).sum()
    assert _bits(MP.emp(M, Qt, Qv), (r2.astype(F) / F(10)) * (c2.astype(F) / F(8)))
    assert not _bits(MP.emp(M, Qt, Qv), MP.emp(M))
    (rm, rs), (cm, cs) = MP.line_moments(M, Qt, Qv)
    np.testing.assert_allclose(rm, Qv.astype(np.float64).mean(1), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cs, Qt.astype(np.float64).std(0), rtol=1e-6)
    assert _bits(MP.gauss(M, Qt, Qv), MP.gauss_scores(M, rm, rs, cm, cs))


# ---- entry points ----------------------------------------------------------------------------------------------------------------
NAMES = ("nr_mp_row_counts", "nr_mp_col_counts", "nr_mp_line_counts", "nr_mp_emp_apply", "nr_mp_row_moments", "nr_mp_col_moments",
         "nr_mp_moments_combine", "nr_mp_gauss_apply")


def test_mutual_proximity_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header and name in hip.exported_symbols()
        assert hasattr(hip.lib(), name)
    comment = header[header.index("/* Mutual proximity"):header.index("int nr_mp_row_counts(")]
    for word in ("emp:", "gauss:", "EPS = 2^-20", "NR_EINVAL", "2^24", "erfc", "accumulate"):
        assert word in comment, word
    assert hip.ABI_VERSION == 5 and hip.version() == 5
    assert hip.MP_LINE_MAX == 1 << 23


def test_mutual_proximity_entry_points_refuse_bad_arguments_before_any_launch():
    lib = hip.lib()                                            # host-side checks: no device needed
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    calls = {          # a valid argument list, the positions of its pointers and of its extents
        "nr_mp_row_counts": ([p, 4, 8, p, 8, p, None], (0, 3, 5), (1, 2, 4)),
        "nr_mp_col_counts": ([p, 4, 8, p, 6, p, 0, None], (0, 3, 5), (1, 2, 4)),
        "nr_mp_line_counts": ([p, 4, 8, p, p, 6, 8, p, None], (0, 4), (1, 2, 5, 6)),
        "nr_mp_emp_apply": ([p, 4, 8, p, p, p, p, p, None], (0, 3, 4, 5, 6, 7), (1, 2)),
        "nr_mp_row_moments": ([p, 4, 8, p, p, None], (0, 3, 4), (1, 2)),
        "nr_mp_col_moments": ([p, 6, 8, p, None], (0, 3), (1, 2)),
        "nr_mp_moments_combine": ([2, p, 8, p, p, None], (1, 3, 4), (0, 2)),
        "nr_mp_gauss_apply": ([p, 4, 8, p, p, p, p, p, None], (0, 3, 4, 5, 6, 7), (1, 2)),
    }
    assert set(calls) == set(NAMES)
    for name, (args, pointers, extents) in calls.items():
        fn = getattr(lib, name)
        for at in pointers:                                    # null pointers, one argument at a time
            a = list(args)
            a[at] = None
            assert fn(*a) == EINVAL, (name, at)
        for at in extents:                                     # negative extents
            a = list(args)
            a[at] = -1
            assert fn(*a) == EINVAL, (name, at)
    # nr_mp_line_counts: either output may be null, not both
    assert lib.nr_mp_line_counts(p, 4, 8, None, p, 6, 8, None, None) == EINVAL
    # accumulate outside {0, 1}
    for acc in (-1, 2, 7):
        assert lib.nr_mp_col_counts(p, 4, 8, p, 6, p, acc, None) == EINVAL
        assert lib.nr_mp_col_counts(p, 0, 8, p, 6, p, acc, None) == EINVAL
    # a line too long for exact counts: 2 c must stay below 2^24
    assert lib.nr_mp_row_counts(p, 4, 8, p, 1 << 23, p, None) == EINVAL
    assert lib.nr_mp_col_counts(p, 4, 8, p, 1 << 23, p, 0, None) == EINVAL
    assert lib.nr_mp_col_counts(p, 4, 8, p, 1 << 23, p, 1, None) == EINVAL
    # nothing to do: NR_OK without a launch
    assert lib.nr_mp_row_counts(p, 0, 8, p, 8, p, None) == 0 and lib.nr_mp_row_counts(p, 4, 0, p, 8, p, None) == 0
    assert lib.nr_mp_col_counts(p, 0, 8, p, 6, p, 0, None) == 0 and lib.nr_mp_col_counts(p, 4, 0, p, 6, p, 1, None) == 0
    assert lib.nr_mp_col_counts(p, 4, 8, None, 0, p, 1, None) == 0              # no reference row to add
    assert lib.nr_mp_line_counts(p, 0, 8, p, p, 6, 0, p, None) == 0
    assert lib.nr_mp_emp_apply(p, 0, 8, p, p, p, p, p, None) == 0 and lib.nr_mp_emp_apply(p, 4, 0, p, p, p, p, p, None) == 0
    assert lib.nr_mp_row_moments(p, 0, 8, p, p, None) == 0
    assert lib.nr_mp_col_moments(p, 6, 0, p, None) == 0
    assert lib.nr_mp_moments_combine(2, p, 0, p, p, None) == 0
    assert lib.nr_mp_gauss_apply(p, 0, 8, p, p, p, p, p, None) == 0 and lib.nr_mp_gauss_apply(p, 4, 0, p, p, p, p, p, None) == 0


# ---- the evaluator's checks --------------------------------------------------------------------------------------------------------
def test_evaluator_knows_the_modes_and_refuses_bad_arguments():
    from neighborretr_amd import evaluator
    assert evaluator.MUTUAL_PROXIMITY_MODES == ("emp", "gauss") == MP.MODES
    assert evaluator.TEST_NORM_MODES == ("is", "dsl", "qbnorm", "sinkhorn", "qbsinkhorn")       # the two existing tuples: not touched
    assert evaluator.LOCAL_SCALING_MODES == ("csls", "nicdm", "ls")
    for mode in ("emp", "gauss", "mp"):
        assert mode not in evaluator.TEST_NORM_MODES and mode not in evaluator.TEST_NORM_LABELS
        assert mode not in evaluator.LOCAL_SCALING_MODES and mode not in evaluator.LOCAL_SCALING_LABELS
    assert evaluator.mutual_proximity_label("emp", False) == "[MP-emp]"
    assert evaluator.mutual_proximity_label("gauss", False) == "[MP-gauss]"
    assert evaluator.mutual_proximity_label("emp", True) == "[QB-MP-emp]"
    assert evaluator.mutual_proximity_label("gauss", True) == "[QB-MP-gauss]"
    for mode in evaluator.MUTUAL_PROXIMITY_MODES:
        assert evaluator._check_mutual_proximity(mode, 5) == 5 and evaluator._check_mutual_proximity(mode, 0) == 0
        assert evaluator._check_mutual_proximity(mode, None) == 0
    for bad_mode in ("is", "csls", "mp", "", None, "none"):
        with pytest.raises(ValueError, match="mutual_proximity"):
            evaluator._check_mutual_proximity(bad_mode, 0)
        with pytest.raises(ValueError):
            evaluator.mutual_proximity_label(bad_mode, False)
    with pytest.raises(ValueError):
        evaluator._check_mutual_proximity("emp", 129)
    e, em = torch.empty((0, 0, 0)), torch.empty((0, 0))
    model = type("M", (), dict(mb_feat_t=e, mb_feat_v=e, mb_mask_t=em, mb_mask_v=em))()
    z = torch.zeros((4, 2, 8))
    for fn in (evaluator.sharded_mutual_proximity_slab, evaluator.sharded_mutual_proximity_metrics,
               evaluator.sharded_metrics_with_mutual_proximity):
        for mode in evaluator.MUTUAL_PROXIMITY_MODES:
            with pytest.raises(ValueError, match="load_memory_bank"):  # an empty bank fails before any scoring
                fn(model, z, z, z[..., 0], z[..., 0], None, mode, bank=True)
        with pytest.raises(ValueError, match="mutual_proximity"):
            fn(model, z, z, z[..., 0], z[..., 0], None, "csls")


def test_training_eval_epoch_refuses_mutual_proximity_with_another_correction_before_any_work():
    from types import SimpleNamespace
    from neighborretr_amd import training
    for other in (dict(test_norm="is"), dict(local_scaling="csls"), dict(test_norm="sinkhorn", local_scaling="ls")):
        for mode in ("emp", "gauss"):
            args = SimpleNamespace(mutual_proximity=mode, **other)
            with pytest.raises(ValueError, match="mutual_proximity"):
                training.eval_epoch(args, None, None, "cpu")   # no model, no loader: nothing may be touched


# ---- the command line --------------------------------------------------------------------------------------------------------------
def _parse(argv, monkeypatch):
    sys.path.insert(0, ROOT)
    import main_retrieval
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
    return main_retrieval.get_args()


def test_main_retrieval_accepts_the_mutual_proximity_flags(monkeypatch):
    a = _parse([], monkeypatch)
    assert (a.mutual_proximity, a.mutual_proximity_bank) == ("none", 0)
    assert (a.test_norm, a.local_scaling) == ("none", "none")
    for mode in ("emp", "gauss"):
        for bank in (0, 1):
            a = _parse(["--mutual_proximity", mode, "--mutual_proximity_bank", str(bank)], monkeypatch)
            assert (a.mutual_proximity, a.mutual_proximity_bank) == (mode, bank)
            assert a.test_norm == "none" and a.local_scaling == "none"
    a = _parse(["--mutual_proximity", "emp", "--hubness_k", "5"], monkeypatch)
    assert a.hubness_k == 5


def _refused(argv, monkeypatch, capsys):
    """The parser's error message for argv (it must refuse it)."""
    capsys.readouterr()
    with pytest.raises(SystemExit):
        _parse(argv, monkeypatch)
    return capsys.readouterr().err


def test_main_retrieval_refuses_the_combinations_and_the_modes_under_another_flag(monkeypatch, capsys):
    # the three exclusions: refused as combinations, not as unknown flags or values
    for other in (["--test_norm", "is"], ["--local_scaling", "csls"], ["--test_norm", "dsl", "--local_scaling", "ls"]):
        for mode in ("emp", "gauss"):
            err = _refused(["--mutual_proximity", mode] + other, monkeypatch, capsys)
            assert "separate corrections" in err and "unrecognized" not in err and "invalid choice" not in err, err
            if len(other) == 2:
                assert "--mutual_proximity" in err and other[0] in err, err
    # the modes belong to this flag alone
    err = _refused(["--test_norm", "emp"], monkeypatch, capsys)
    assert "argument --test_norm: invalid choice: 'emp'" in err
    err = _refused(["--local_scaling", "gauss"], monkeypatch, capsys)
    assert "argument --local_scaling: invalid choice: 'gauss'" in err
    err = _refused(["--mutual_proximity", "mp"], monkeypatch, capsys)
    assert "argument --mutual_proximity: invalid choice: 'mp'" in err
    err = _refused(["--mutual_proximity", "emp", "--mutual_proximity_bank", "2"], monkeypatch, capsys)
    assert "argument --mutual_proximity_bank: invalid choice: 2" in err
