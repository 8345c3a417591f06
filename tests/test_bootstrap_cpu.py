"""CPU: the restatement of the bootstrap of rank statistics (bootstrap_ref) on the definition's check values and a worked example,
the host summaries (RetrievalMetrics.bootstrap_summary / paired_bootstrap_summary) on hand-made statistics, the coverage of the
percentile interval, the host-side refusals of nr_bootstrap_rank_stats, the evaluator's argument checks and the command-line flags."""
import ctypes
import logging
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bootstrap_ref as B
from neighborretr_amd import hip
from neighborretr_amd.metrics import RetrievalMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the worked example of the definition ------------------------------------------------------------------------------------------
# ranking a: unit 2 is empty, unit 1 holds a tie, one rank (70000) needs a second digit of the select
RANKS_A, END_A = [0, 3, 3, 70000, 1, 0, 12], [0, 2, 2, 3, 6]
RANKS_B, END_B = [0, 0, 5, 2, 9], [0, 1, 2, 3, 4]
WORKED = [[[7, 70012, 3, 3, 2, 6, 6, 6], [5, 2, 0, 0, 4, 5, 5, 5]],
          [[8, 70026, 1, 1, 3, 5, 5, 7], [5, 25, 5, 5, 1, 2, 5, 5]],
          [[6, 70012, 3, 3, 1, 5, 5, 5], [5, 7, 0, 0, 3, 4, 5, 5]]]


def test_splitmix64_check_values():
    want = [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
    assert [int(B.sm64(1234567, c)) for c in range(5)] == want
    assert [int(x) for x in B.sm64(1234567, np.arange(5))] == want
    # all arithmetic is modulo 2^64: the largest seed wraps
    assert int(B.sm64((1 << 64) - 1, 0)) == int(B.sm64(-1, 0))


def test_draws_check_values():
    assert [B.draws(42, b, 5).tolist() for b in range(3)] == [[3, 0, 1, 1, 0], [3, 0, 2, 4, 4], [0, 3, 1, 2, 1]]
    assert B.draws_matrix(42, 0, 3, 5).tolist() == [[3, 0, 1, 1, 0], [3, 0, 2, 4, 4], [0, 3, 1, 2, 1]]
    assert B.draws_matrix(42, 1, 2, 5).tolist() == [[3, 0, 2, 4, 4], [0, 3, 1, 2, 1]]        # resample b, whatever b0
    u = B.draws(7, 3, 1 << 16)
    assert u.min() >= 0 and (1 << 16) - 64 <= u.max() < 1 << 16                 # the whole range is reached, never U itself


def test_worked_example():
    got = B.rank_stats(RANKS_A, END_A, RANKS_B, END_B, cuts=(1, 5, 10, 50), seed=42, b0=0, n_boot=3)
    assert got.dtype == np.int64 and got.tolist() == WORKED
    # by hand, resample 0 draws units [3 0 1 1 0]: a = {70000, 0, 3, 3, 3, 3, 0}: sorted 0 0 3 3 3 3 70000
    assert got[0, 0].tolist() == [7, 70012, 3, 3, 2, 6, 6, 6]
    # V = 2 is two V = 1 calls with the seed, and a later b0 is the tail of the same sequence
    assert np.array_equal(B.rank_stats(RANKS_B, END_B, seed=42, n_boot=3)[:, 0], got[:, 1])
    assert np.array_equal(B.rank_stats(RANKS_A, END_A, seed=42, b0=1, n_boot=2)[:, 0], got[1:, 0])


def test_single_entry_shortcut_is_the_restatement():
    rng = np.random.default_rng(5)
    ranks = rng.integers(0, 60, 37)
    want = B.rank_stats(ranks, np.arange(37), cuts=(1, 10), seed=9, b0=2, n_boot=6)[:, 0]
    assert np.array_equal(B.single_entry_stats(ranks, (1, 10), seed=9, b0=2, n_boot=6), want)


# ---- the summaries on hand-made statistics ---------------------------------------------------------------------------------------
CUTS2 = (1, 5)
#         n  sum lo  hi  <1  <5        R1   R5   MeanR  MedianR mid / low
STATS = [[4, 10, 1, 3, 1, 3],      # 25   75   3.5    3 / 2
         [0, 0, -1, -1, 0, 0],     # empty: dropped
         [2, 4, 2, 2, 0, 2],       # 0    100  3      3 / 3
         [5, 5, 0, 1, 3, 5],       # 60   100  2      1.5 / 1
         [4, 0, 0, 0, 4, 4]]       # 100  100  1      1 / 1
ENTRIES = [0, 0, 3, 7]             # the point: R1 50, R5 75, MeanR 3.5, MedianR 2.5 / 1


def test_bootstrap_summary_by_hand():
    s = RetrievalMetrics.bootstrap_summary(np.asarray(STATS), CUTS2, ENTRIES, level=0.5)
    assert (s["n_boot"], s["n_empty"], s["level"], s["median"]) == (5, 1, 0.5, "mid")
    assert set(s) == {"n_boot", "n_empty", "level", "median", "R1", "R5", "MedianR", "MeanR"}
    assert s["R1"]["point"] == 50.0 and s["R5"]["point"] == 75.0 and s["MeanR"]["point"] == 3.5 and s["MedianR"]["point"] == 2.5
    # R1 over the four kept resamples: 0 25 60 100; np.percentile's linear interpolation at positions 0.75 and 2.25
    assert s["R1"]["lo"] == pytest.approx(18.75, abs=1e-12) and s["R1"]["hi"] == pytest.approx(70.0, abs=1e-12)
    assert s["R1"]["se"] == pytest.approx(np.sqrt(1417.1875), rel=1e-14)          # the population standard deviation
    wide = RetrievalMetrics.bootstrap_summary(torch.tensor(STATS), CUTS2, ENTRIES)         # the default level, a tensor
    assert wide["level"] == 0.95
    assert wide["R1"]["lo"] == pytest.approx(1.875, abs=1e-12) and wide["R1"]["hi"] == pytest.approx(97.0, abs=1e-12)
    # MedianR: 3 3 1.5 1 (mid), 2 3 1 1 (low)
    assert s["MedianR"]["lo"] == pytest.approx(1.375) and s["MedianR"]["hi"] == pytest.approx(3.0)
    low = RetrievalMetrics.bootstrap_summary(np.asarray(STATS), CUTS2, ENTRIES, level=0.5, median="low")
    assert low["MedianR"]["point"] == 1.0 and low["MedianR"]["lo"] == pytest.approx(1.0) and low["MedianR"]["hi"] == pytest.approx(2.25)
    assert low["R1"] == s["R1"] and low["MeanR"] == s["MeanR"]
    assert s["MeanR"]["se"] == pytest.approx(np.std([3.5, 3, 2, 1]), rel=1e-14)


def test_bootstrap_summary_edge_cases():
    none = RetrievalMetrics.bootstrap_summary(np.asarray([STATS[1]] * 3), CUTS2, ENTRIES)
    assert none["n_empty"] == 3 and np.isnan(none["R1"]["se"]) and np.isnan(none["R1"]["lo"]) and none["R1"]["point"] == 50.0
    for bad in (0, 1, -0.5, 1.5):
        with pytest.raises(ValueError, match="level"):
            RetrievalMetrics.bootstrap_summary(np.asarray(STATS), CUTS2, ENTRIES, level=bad)
    with pytest.raises(ValueError, match="median"):
        RetrievalMetrics.bootstrap_summary(np.asarray(STATS), CUTS2, ENTRIES, median="high")
    with pytest.raises(ValueError, match="stats"):
        RetrievalMetrics.bootstrap_summary(np.asarray(STATS), (1, 5, 10), ENTRIES)


def test_paired_bootstrap_summary_by_hand():
    raw = [[4, 12, 2, 4, 0, 2],        # R1 0    MeanR 4
           [3, 3, 1, 1, 1, 3],         # the corrected ranking's resample is empty: dropped
           [2, 2, 1, 1, 0, 2],         # R1 0    MeanR 2
           [0, 0, -1, -1, 0, 0],       # empty: dropped
           [4, 4, 1, 1, 2, 4]]         # R1 50   MeanR 2
    p = RetrievalMetrics.paired_bootstrap_summary(np.asarray(STATS), np.asarray(raw), CUTS2, ENTRIES, [1, 1, 2, 8], level=0.5)
    assert (p["n_boot"], p["n_empty"]) == (5, 2)
    # R1 differences 25 0 50; MeanR differences -0.5 1 -1
    assert p["R1"]["point"] == 50.0 and p["MeanR"]["point"] == 3.5 - 4.0
    assert p["R1"]["frac_le0"] == pytest.approx(1 / 3) and p["R1"]["frac_ge0"] == 1.0
    assert p["MeanR"]["frac_le0"] == pytest.approx(2 / 3) and p["MeanR"]["frac_ge0"] == pytest.approx(1 / 3)
    assert p["R1"]["lo"] == pytest.approx(12.5) and p["R1"]["hi"] == pytest.approx(37.5)
    assert p["R1"]["se"] == pytest.approx(np.std([25, 0, 50]))
    with pytest.raises(ValueError, match="one call"):
        RetrievalMetrics.paired_bootstrap_summary(np.asarray(STATS), np.asarray(raw[:3]), CUTS2, ENTRIES, ENTRIES)


def test_format_and_log_bootstrap():
    s = RetrievalMetrics.bootstrap_summary(B.single_entry_stats(np.arange(40) % 13, seed=1, n_boot=50), B.DEFAULT_CUTS, np.arange(40) % 13)
    line = RetrievalMetrics.format_bootstrap(s, prefix="Text-to-Video: ")
    assert line.startswith("Text-to-Video: R@1: ") and "Median R: " in line and "Mean R: " in line
    assert line.endswith("(95% bootstrap, 50 resamples)") and line.count("[") == 5
    two = B.rank_stats(np.arange(40) % 13, np.arange(40), np.arange(40) % 7, np.arange(40), seed=1, n_boot=50)
    p = RetrievalMetrics.paired_bootstrap_summary(two[:, 1], two[:, 0], B.DEFAULT_CUTS, np.arange(40) % 7, np.arange(40) % 13)
    line = RetrievalMetrics.format_bootstrap(p, prefix="x - raw: ")
    assert "frac<=0" in line and "paired bootstrap vs raw" in line and "R@1: +" in line
    RetrievalMetrics(logger=None).log_bootstrap(s)                             # silent without a logger
    seen = []
    handler = logging.Handler()
    handler.emit = lambda rec: seen.append(rec.getMessage())
    lg = logging.getLogger("test_bootstrap_cpu")
    lg.addHandler(handler)
    lg.setLevel(logging.INFO)
    try:
        RetrievalMetrics(logger=lg).log_bootstrap(s, prefix="p ")
    finally:
        lg.removeHandler(handler)
    assert seen == [RetrievalMetrics.format_bootstrap(s, prefix="p ")]


# ---- the definition itself: the percentile interval covers ------------------------------------------------------------------------------
def test_percentile_interval_of_recall_covers_the_truth():
    """200 independent samples of U = 400 queries that hit (rank 0) with probability 0.4 and miss (rank 7) otherwise; the 95 %
    interval of R@1 from 400 resamples must cover 40 % in 90 % to 99 % of them: 95 % -+ three binomial standard deviations
    (sqrt(.95 * .05 / 200) = 1.54 points)."""
    U, n_boot, trials, p = 400, 400, 200, 0.4
    covered, ratio = 0, []
    for s in range(trials):
        ranks = np.where(np.random.default_rng(s).random(U) < p, 0, 7)
        stats = B.single_entry_stats(ranks, (1,), seed=1000 + s, n_boot=n_boot)
        m = RetrievalMetrics.bootstrap_summary(stats, (1,), ranks)["R1"]
        covered += m["lo"] <= 100 * p <= m["hi"]
        ratio.append(m["se"] / (100 * np.sqrt(p * (1 - p) / U)))
    print(f"coverage {covered / trials:.3f}, bootstrap se / binomial se: mean {np.mean(ratio):.3f}")
    assert 0.90 <= covered / trials <= 0.99
    assert 0.95 <= np.mean(ratio) <= 1.05                  # the se is the binomial's: the plug-in p and 400 resamples move it by ~1 %


# ---- the entry point ----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    assert "int nr_bootstrap_rank_stats(" in header and "nr_bootstrap_rank_stats" in hip.exported_symbols()
    assert hasattr(hip.lib(), "nr_bootstrap_rank_stats")
    comment = header[header.index("/* Bootstrap of rank statistics"):header.index("int nr_bootstrap_rank_stats(")]
    for word in ("SplitMix64", "0x9E3779B97F4A7C15", "unit_end", "med_lo", "(n-1)/2", "NR_EINVAL", "2^24", "2^30", "NR_OK", "HOST"):
        assert word in comment, word
    assert hip.ABI_VERSION == 5 and hip.version() == 5
    assert (hip.BOOT_MAX_UNITS, hip.BOOT_MAX_CUTS, hip.BOOT_RANK_LIMIT) == (1 << 24, 8, 1 << 30)
    args, res = hip._SIGNATURES["nr_bootstrap_rank_stats"]
    assert len(args) == 14 and args[9] is ctypes.c_uint64 and res is ctypes.c_int


def test_entry_point_refuses_bad_arguments_before_any_launch():
    fn = hip.lib().nr_bootstrap_rank_stats                    # host-side checks: no device needed
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    cuts = (ctypes.c_int32 * 8)(1, 5, 10, 50, 60, 70, 80, 90)
    #       ranks_a end_a E_a ranks_b end_b E_b U  cuts  K  seed b0 n_boot out stream
    good = [p, p, 4, p, p, 4, 3, cuts, 4, 42, 0, 5, p, None]

    def call(**over):
        names = ("ranks_a", "end_a", "E_a", "ranks_b", "end_b", "E_b", "U", "cuts", "K", "seed", "b0", "n_boot", "out", "stream")
        a = list(good)
        for k, v in over.items():
            a[names.index(k)] = v
        return fn(*a)
    for name in ("ranks_a", "end_a", "end_b", "cuts", "out"):                      # a null required pointer
        assert call(**{name: None}) == EINVAL, name
    for U in (0, -1, (1 << 24) + 1):
        assert call(U=U) == EINVAL, U
    for K in (0, -1, 9):
        assert call(K=K) == EINVAL, K
    assert call(E_a=-1) == EINVAL and call(E_b=-1) == EINVAL
    assert call(b0=-1) == EINVAL and call(n_boot=-1) == EINVAL
    assert call(b0=(1 << 31) - 5, n_boot=5) == EINVAL and call(b0=(1 << 31) - 1, n_boot=1) == EINVAL
    for bad in ((0, 5, 10, 50), (1, 5, 5, 50), (5, 1, 10, 50), (-1, 5, 10, 50)):   # cut-offs: positive and strictly increasing
        assert call(cuts=(ctypes.c_int32 * 4)(*bad)) == EINVAL, bad
    # nothing to do: NR_OK without a launch; ranks_b NULL is V = 1 and its other arguments are ignored
    assert call(n_boot=0) == 0 and call(n_boot=0, b0=(1 << 31) - 1) == 0
    assert call(n_boot=0, ranks_b=None, end_b=None, E_b=-7) == 0
    assert call(n_boot=0, U=1 << 24, K=8) == 0 and call(n_boot=0, U=1, K=1, E_a=0) == 0
    assert call(n_boot=0, K=4, cuts=(ctypes.c_int32 * 4)(0, 5, 10, 50)) == EINVAL  # arguments are checked even then


# ---- the evaluator's checks and units --------------------------------------------------------------------------------------------------
def test_evaluator_checks_the_bootstrap_arguments():
    from neighborretr_amd import evaluator
    assert evaluator._check_bootstrap(0) is None and evaluator._check_bootstrap(0, 5, 0.5) is None
    assert evaluator._check_bootstrap(200, 3, 0.9) == (200, 3, 0.9) and evaluator._check_bootstrap(1 << 20) == (1 << 20, 0, 0.95)
    for bad in (-1, (1 << 20) + 1, 2.5, "10", None, True):
        with pytest.raises(ValueError, match="bootstrap must"):
            evaluator._check_bootstrap(bad)
    for bad in (-1, (1 << 64) - 1, 0.5, None):
        with pytest.raises(ValueError, match="bootstrap_seed"):
            evaluator._check_bootstrap(10, bad)
    for bad in (0, 1, 0.0, 1.0, -0.1, 95, "0.9", None):
        with pytest.raises(ValueError, match="bootstrap_level"):
            evaluator._check_bootstrap(10, 0, bad)
    z = torch.zeros((4, 2, 8))
    for fn, extra in ((evaluator.sharded_metrics, ()), (evaluator.sharded_multi_sentence_metrics, ([0, 1, 2, 3],)),
                      (evaluator.sharded_metrics_with_hubness, (5,)), (evaluator.sharded_metrics_with_test_norm, ("is",)),
                      (evaluator.sharded_metrics_with_local_scaling, ("csls",)),
                      (evaluator.sharded_metrics_with_mutual_proximity, ("emp",))):
        head = (None, z, z, z[..., 0], z[..., 0])
        pos = head + extra + (None,) if fn is evaluator.sharded_multi_sentence_metrics else head + (None,) + extra
        with pytest.raises(ValueError, match="bootstrap must"):               # before any scoring: there is no model
            fn(*pos, bootstrap=-3)
        with pytest.raises(ValueError, match="bootstrap_level"):
            fn(*pos, bootstrap=10, bootstrap_level=1.0)


def test_evaluator_units():
    from neighborretr_amd import evaluator
    # single-sentence: query i owns its equal[i] consecutive entries
    entries, end, median = evaluator._query_units([4, 0, 2], [1, 3, 2])
    assert entries.tolist() == [4, 0, 1, 2, 2, 3] and end.tolist() == [0, 3, 5] and median == "mid"
    # multi-sentence: videos of 2, 1, 3 sentences; the second video's only sentence is not ranked: an empty unit
    ranks = torch.tensor([3, 0, -1, 5, -1, 1], dtype=torch.int32)
    entries, end, median = evaluator._video_units(ranks, np.asarray([2, 3, 6]))
    assert entries.tolist() == [3, 0, 5, 1] and end.tolist() == [1, 1, 3] and median == "low"
    entries, end, _ = evaluator._video_units(torch.tensor([-1, 2], dtype=torch.int32), np.asarray([1, 2]))
    assert entries.tolist() == [2] and end.tolist() == [-1, 0]                  # the first video is empty: it ends at -1


def test_training_eval_epoch_refuses_bad_bootstrap_arguments_before_any_work():
    from neighborretr_amd import training
    for bad in (-1, (1 << 20) + 1, 2.5, "many"):
        with pytest.raises(ValueError, match="bootstrap must"):
            training.eval_epoch(SimpleNamespace(bootstrap=bad), None, None, "cpu")   # no model, no loader: nothing may be touched
    for bad in (0.0, 1.0, 1.5, -0.2, "wide"):
        with pytest.raises(ValueError, match="bootstrap_level"):
            training.eval_epoch(SimpleNamespace(bootstrap=100, bootstrap_level=bad), None, None, "cpu")
    with pytest.raises(ValueError, match="bootstrap_seed"):
        training.eval_epoch(SimpleNamespace(bootstrap=100, bootstrap_seed=-4), None, None, "cpu")


# ---- the command line --------------------------------------------------------------------------------------------------------------
def _parse(argv, monkeypatch):
    sys.path.insert(0, ROOT)
    import main_retrieval
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
    return main_retrieval.get_args()


def test_main_retrieval_accepts_the_bootstrap_flags(monkeypatch, capsys):
    a = _parse([], monkeypatch)
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_level) == (0, 0, 0.95)
    a = _parse(["--bootstrap", "200", "--bootstrap_seed", "7", "--bootstrap_level", "0.9", "--mutual_proximity", "emp"], monkeypatch)
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_level, a.mutual_proximity) == (200, 7, 0.9, "emp")
    for argv, word in ((["--bootstrap", "-1"], "--bootstrap must"), (["--bootstrap", str((1 << 20) + 1)], "--bootstrap must"),
                       (["--bootstrap", "10", "--bootstrap_level", "1"], "--bootstrap_level"),
                       (["--bootstrap", "10", "--bootstrap_seed", "-1"], "--bootstrap_seed")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            _parse(argv, monkeypatch)
        assert word in capsys.readouterr().err
